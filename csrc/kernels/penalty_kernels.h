// Presence, frequency and repetition penalties over a row of bf16 logits, the
// greedy pick over an edited row, and the device-side token history both read.
// Rows that ask for a penalty take this path (logits from the store-epilogue
// GEMM, as the truncated and the log-probability rows); every other row keeps
// the fused LM head.
//
// The edit, for one row (ops/sampling.py: penalise_reference is the numpy
// twin, bit for bit):
//
//   inputs     bf16 logits l[0..V) of a row of leading dimension ld (ld % 8 ==
//              0), edited in place; a history h[0..n) of int32 token ids, the
//              first n_p of them prompt tokens, the rest generated; fp32 pp
//              (presence), fp (frequency), rp (repetition)
//   columns    every distinct id t of h with 0 <= t < V, once.  Any other id
//              is ignored.  c_all = the count of t in h, c_gen = its count in
//              h[n_p..n), x = float(l[t])
//   1.         if rp != 1:  x = x > 0 ? x / rp : x * rp   (the Hugging Face
//              rule, over prompt and generated tokens; __fdiv_rn, the
//              correctly rounded fp32 quotient, and __fmul_rn)
//   2.         x = fma(-fp, float(c_gen), x), one rounding (__fmaf_rn)
//   3.         if c_gen > 0:  x = x - pp   (__fsub_rn; 2. and 3. count
//              generated tokens only, vLLM's rule)
//   4.         l[t] = bf16(x), round to nearest even; NaN stays NaN (written as
//              0x7fc0), an infinity or an overflow is an infinity (no
//              candidate downstream)
//   untouched  every column not in h, and the padding [V, ld), keep their bits
//   pure       a function of the row, h and the three parameters: counts are
//              integers, every column has one writer, no atomics, nothing
//              depends on thread count or scan order
//
// How: one 256-thread block a row (grid-stride over rows).  h goes into LDS;
// entry i is owned by thread i % 256, which scans h (every lane of a wave
// reads the same LDS word: a broadcast) for the counts of its id and edits
// the column only if no earlier entry holds the same id, so columns are
// distinct without atomics or scratch.  n^2 / 256 LDS reads a thread: 64 K at
// the cap, 1.4 at the benchmark's 19 tokens.
//
// Where h lives: a table int32 [slots][stride] indexed by absolute position
// (history_record_kernel writes it with the tokens every forward consumes);
// a row names its window by span = (slot, from, split, end): h = table[slot]
// [from..end), n_p = split - from.  A span outside the table is clamped, a
// slot outside it makes the row a no-op: no index leaves the table.
//
// The greedy pick over an edited row (penalised_argmax_kernel; twin
// penalised_pick_reference): argmax over the finite columns < V, ties to the
// lower column, token 0 for a row with none -- the candidates and the tie
// rule of sample_truncate_kernels.h.  A row with inv_temp > 0 is skipped (it
// is drawn by sample_truncated_kernel over the same edited logits).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace llmq {

constexpr int PEN_THREADS = 256;
constexpr int PEN_HIST_MAX = 4096;                   // history entries a row (16 KiB of LDS)
constexpr int PEN_MAX_BLOCKS = 1024;                 // grid-stride above this many rows

__device__ __forceinline__ uint16_t pen_bf16(float x) {        // round to nearest even
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;                    // NaN stays NaN (the canonical one)
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);                        // (overflow carries into inf)
}

// the contract's steps 1 to 4 for one column
__device__ __forceinline__ uint16_t pen_edit(uint16_t b, int c_gen, float pp, float fp, float rp) {
#pragma clang fp contract(off)                       // (every step below rounds once, on its own)
  float x = __uint_as_float((uint32_t)b << 16);
  if (rp != 1.0f) x = x > 0.0f ? __fdiv_rn(x, rp) : __fmul_rn(x, rp);
  x = __fmaf_rn(-fp, (float)c_gen, x);
  if (c_gen > 0) x = __fsub_rn(x, pp);
  return pen_bf16(x);
}

// spans int32 [R][4] = (slot, from, split, end), params fp32 [R][3] = (pp, fp, rp)
__global__ void __launch_bounds__(PEN_THREADS)
penalise_kernel(uint16_t* __restrict__ logits, int R, int V, int ld, const int32_t* __restrict__ hist, int n_slots,
                int stride, const int32_t* __restrict__ spans, const float* __restrict__ params) {
  __shared__ int32_t h[PEN_HIST_MAX];
  const int t = threadIdx.x;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int slot = spans[4 * r];
    if (slot < 0 || slot >= n_slots) continue;       // (uniform over the block)
    const int cap = min(stride, PEN_HIST_MAX);
    const int from = min(max(spans[4 * r + 1], 0), stride);
    const int end = min(min(max(spans[4 * r + 3], from), stride), from + cap);
    const int split = min(max(spans[4 * r + 2], from), end);
    const int n = end - from, n_p = split - from;
    const float pp = params[3 * r], fp = params[3 * r + 1], rp = params[3 * r + 2];
    const int32_t* src = hist + (size_t)slot * stride + from;
    __syncthreads();                                 // (the previous row's readers are done)
    for (int i = t; i < n; i += PEN_THREADS) h[i] = src[i];
    __syncthreads();
    uint16_t* row = logits + (size_t)r * ld;
    for (int i = t; i < n; i += PEN_THREADS) {
      const int32_t id = h[i];
      if (id < 0 || id >= V) continue;
      bool first = true;
      int c_gen = 0;
      for (int j = 0; j < n; ++j) {
        if (h[j] == id) {
          if (j < i) {
            first = false;
            break;
          }
          c_gen += j >= n_p;
        }
      }
      if (first) row[id] = pen_edit(row[id], c_gen, pp, fp, rp);
    }
  }
}

// out[r] = argmax over the finite columns < V of row r (ties to the lower
// column, 0 for none), for the rows with inv_temp[r] <= 0 (inv_temp null: all)
__global__ void __launch_bounds__(PEN_THREADS)
penalised_argmax_kernel(const uint16_t* __restrict__ logits, int R, int V, int ld,
                        const float* __restrict__ inv_temp, int32_t* __restrict__ out) {
  __shared__ float redv[4];
  __shared__ int redc[4];
  const int t = threadIdx.x;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    if (inv_temp != nullptr && inv_temp[r] > 0.0f) continue;
    const uint16_t* row = logits + (size_t)r * ld;
    float bv = -INFINITY;
    int bc = 0x7fffffff;
    for (int n = t * 8; n < V; n += PEN_THREADS * 8) {           // (ld % 8 == 0: the vector stays in the row)
      const uint4 q = *reinterpret_cast<const uint4*>(row + n);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t b = (w[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        const float v = __uint_as_float(b << 16);
        if (n + e < V && (b & 0x7f80u) != 0x7f80u && (v > bv || bc == 0x7fffffff)) {   // (columns ascend: a tie keeps the lower)
          bv = v;
          bc = n + e;
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oc = __shfl_xor(bc, o);
      if (oc != 0x7fffffff && (bc == 0x7fffffff || ov > bv || (ov == bv && oc < bc))) {
        bv = ov;
        bc = oc;
      }
    }
    __syncthreads();                                 // (the previous row's reader is done)
    if ((t & 63) == 0) {
      redv[t >> 6] = bv;
      redc[t >> 6] = bc;
    }
    __syncthreads();
    if (t == 0) {
      for (int i = 1; i < 4; ++i)
        if (redc[i] != 0x7fffffff && (bc == 0x7fffffff || redv[i] > bv || (redv[i] == bv && redc[i] < bc))) {
          bv = redv[i];
          bc = redc[i];
        }
      out[r] = bc == 0x7fffffff ? 0 : bc;
    }
  }
}

// hist[slot[t]][pos[t]] = tok[t] for the Q token rows t = rows[0..Q) of a
// forward of T tokens (int64 ids, int32 pos / slot).  A row, slot or position
// outside its range writes nothing.
__global__ void __launch_bounds__(PEN_THREADS)
history_record_kernel(int32_t* __restrict__ hist, int n_slots, int stride, const int64_t* __restrict__ tok,
                      const int32_t* __restrict__ pos, const int32_t* __restrict__ slot, int T,
                      const int32_t* __restrict__ rows, int Q) {
  for (int i = blockIdx.x * PEN_THREADS + threadIdx.x; i < Q; i += gridDim.x * PEN_THREADS) {
    const int t = rows[i];
    if (t < 0 || t >= T) continue;
    const int s = slot[t], p = pos[t];
    if (s < 0 || s >= n_slots || p < 0 || p >= stride) continue;
    hist[(size_t)s * stride + p] = (int32_t)tok[t];
  }
}

}  // namespace llmq
