// Log-probabilities over a row of bf16 logits: the chosen token's and the
// LP_TOP most likely alternatives', for the rows of a step that ask for them.
// The logits come from the store-epilogue GEMM, as the truncated sampler's do
// (sample_truncate_kernels.h, whose row walk and key helpers this reuses);
// rows that do not ask keep their path and pay nothing.
//
// The contract, for one row l[0..V) with chosen token t (ops/sampling.py:
// logprob_reference is the numpy twin in float64, logprob_bound the bound on
// |device - twin|):
//
//   layout     row stride ld, ld % 8 == 0, rows 16-byte aligned; columns V..ld
//              are padding and never read as data
//   candidates the columns with a finite logit; +0 and -0 are one value.  A
//              NaN or infinite logit is never a candidate
//   normaliser m = the largest candidate value, Z = sum exp(l[n] - m) over the
//              candidates, lp(n) = (l[n] - m) - log Z: log_softmax at
//              temperature 1, before any truncation
//   token      lp(t); -inf if t is outside [0, V) or not a candidate
//   top        the LP_TOP = 5 candidates with the largest value, ties to the
//              lower column, in that order, each with its lp; unused places
//              (fewer than 5 candidates, or none) hold id -1 and -inf
//   pure       the order of the additions is fixed by (V, thread count) alone
//              and there are no float atomics: a row gives the same bits
//              whatever launch, row index or neighbours it has
//   one lp     lp_value() below is the only formula: where t is one of the
//              alternatives its two values are bitwise equal
//   outputs    float32 [R][1 + LP_TOP] (token first, then the alternatives),
//              int32 [R][LP_TOP]
//
// How: one 256-thread block a row (grid-stride over rows), two passes.
//   1. every thread keeps the best LP_TOP of its columns as sorted 64-bit
//      words (key + 1 in the high half, ~column in the low: a larger word is a
//      larger value or, among equal values, a lower column).  LP_TOP rounds of
//      a block-wide maximum over the threads' heads then pick the
//      alternatives; the owner of a round's winner moves on to its next.  The
//      first winner's value is m.
//   2. every thread sums expf(l - m) over its columns in ascending column
//      order (st_row's order), the 64 lanes of a wave add in a xor shuffle
//      tree, and the 4 wave sums add as (w0 + w1) + (w2 + w3).
// The second pass re-reads the row (256 KB at V = 128,256) from L2.
//
// expf and logf are the device library's accurate ones (at most 1 ulp each by
// the HIP math API's table), not the __expf / __logf intrinsics, and this file
// must not be built with fast-math.
//
// Error bound, against the twin in exact arithmetic on the same bf16 values,
// with u = 2^-24, for columns with |l - m| <= span (the twin's
// logprob_bound(V, span) is this sum):
//   d = fl(l - m)      |d - (l - m)| <= span * u.  In a term of Z this is a
//                      relative error |d| u; weighted by the term's share
//                      p(n) = exp(d) / Z it sums to at most u * E_p|d| =
//                      u * (H(p) - log Z) <= u * log V
//   expf               1 ulp: a relative 2u a term (a term below 2^-126 is a
//                      denormal or 0: at most V * 2^-126 in all, against
//                      Z >= 1; nothing at this scale)
//   the sum            terms are >= 0, so each addition adds at most u
//                      relative.  The longest chain is a thread's
//                      8 * ceil(V / 2048) columns, then 6 shuffle levels and 2
//                      for the waves: depth(V) = 8 * ceil(V / 2048) + 8
//   so                 |Z' / Z - 1| <= rho = (log V + 2 + depth) u, taken as
//                      expm1((log V + 2 + depth) * log1p(u)) for the second
//                      order, and |log Z' - log Z| <= -log1p(-rho)
//   logf               1 ulp of a value in [0, log V + rho]: 2u (log V + rho)
//   lp = fl(d - logZ)  |lp| <= span + log V + 1: (span + log V + 1) u, plus
//                      d's own span * u from above
// At V = 128,256 (depth 512) and span = 128 this is 4.9e-5 nats, of which the
// sum is 3.1e-5.
//
// LDS is 48 bytes a block, so the register file sets the occupancy: with the
// 8 loads of 16 bytes st_row keeps in flight and the five 64-bit words the
// kernel takes 88 VGPRs, 5 waves a SIMD, so at least 4 blocks (16 waves)
// share a CU.  LP_MAX_BLOCKS is 4 blocks on each of 256 CUs: a step's rows (about a
// thousand at most) each get a block of their own in a single wave of blocks,
// and anything beyond takes the grid-stride loop.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sample_truncate_kernels.h"

namespace llmq {

constexpr int LP_TOP = 5;
constexpr int LP_THREADS = ST_THREADS;               // (st_row walks a row with ST_THREADS threads)
constexpr int LP_MAX_BLOCKS = 1024;                  // 4 blocks a CU (above)

// the one formula of a log-probability: v a candidate's value, m the row's maximum
__device__ __forceinline__ float lp_value(float v, float m, float logz) { return (v - m) - logz; }

// key and column as one word: larger = larger value, then lower column; 0: none
__device__ __forceinline__ uint64_t lp_pack(int key, int col) {
  return ((uint64_t)(uint32_t)(key + 1) << 32) | (uint32_t)~(uint32_t)col;
}

// block-wide max of a 64-bit word (every thread gets it); red: 4 words of LDS
__device__ __forceinline__ uint64_t lp_block_max(uint64_t v, uint64_t* red) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = (uint64_t)__shfl_xor((unsigned long long)v, o);
    v = w > v ? w : v;
  }
  __syncthreads();                                   // (red's previous readers are done)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint64_t a = red[0] > red[1] ? red[0] : red[1];
  const uint64_t b = red[2] > red[3] ? red[2] : red[3];
  return a > b ? a : b;
}

__global__ void __launch_bounds__(LP_THREADS)
logprob_kernel(const uint16_t* __restrict__ logits, int R, int V, int ld, const int32_t* __restrict__ tok,
               float* __restrict__ out_lp, int32_t* __restrict__ out_id) {
  __shared__ uint64_t red[4];
  __shared__ float redf[4];
  const int t = threadIdx.x;

  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* row = logits + (size_t)r * ld;
    float* olp = out_lp + (size_t)r * (1 + LP_TOP);
    int32_t* oid = out_id + (size_t)r * LP_TOP;

    // 1. my best LP_TOP columns, descending
    uint64_t best[LP_TOP];
#pragma unroll
    for (int i = 0; i < LP_TOP; ++i) best[i] = 0;
    st_row(row, V, [&](uint32_t b, int n) {
      const int k = st_key(b);
      uint64_t p = k < 0 ? 0 : lp_pack(k, n);
      if (p > best[LP_TOP - 1]) {
#pragma unroll
        for (int i = 0; i < LP_TOP; ++i)
          if (p > best[i]) {
            const uint64_t q = best[i];
            best[i] = p;
            p = q;
          }
      }
    });
    // the block's: LP_TOP rounds over the threads' heads
    uint64_t top[LP_TOP];
#pragma unroll
    for (int i = 0; i < LP_TOP; ++i) {
      top[i] = lp_block_max(best[0], red);
      if (top[i] != 0 && best[0] == top[i]) {        // (columns are distinct: one owner)
#pragma unroll
        for (int j = 0; j + 1 < LP_TOP; ++j) best[j] = best[j + 1];
        best[LP_TOP - 1] = 0;
      }
    }
    if (top[0] == 0) {                               // no finite logit
      if (t <= LP_TOP) olp[t] = -INFINITY;
      if (t < LP_TOP) oid[t] = -1;
      continue;
    }
    const float m = st_value((int)(top[0] >> 32) - 1);

    // 2. Z = sum exp(l - m), a fixed order of additions
    float z = 0.f;
    st_row(row, V, [&](uint32_t b, int) {
      const int k = st_key(b);
      if (k >= 0) z += expf(st_value(k) - m);
    });
    for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
    __syncthreads();                                 // (redf's previous readers are done)
    if ((t & 63) == 0) redf[t >> 6] = z;
    __syncthreads();
    const float logz = logf((redf[0] + redf[1]) + (redf[2] + redf[3]));

    if (t == 0) {
      const int c = tok[r];
      float lt = -INFINITY;
      if (c >= 0 && c < V) {
        const int k = st_key(row[c]);
        if (k >= 0) lt = lp_value(st_value(k), m, logz);
      }
      olp[0] = lt;
#pragma unroll
      for (int i = 0; i < LP_TOP; ++i) {
        const bool has = top[i] != 0;
        olp[1 + i] = has ? lp_value(st_value((int)(top[i] >> 32) - 1), m, logz) : -INFINITY;
        oid[i] = has ? (int32_t)~(uint32_t)top[i] : -1;
      }
    }
  }
}

}  // namespace llmq
