// Top-k / top-p (nucleus) / min-p sampling over a row of bf16 logits: the
// selection and the draw in one kernel, under the noise contract of sample_noise.h.
// Rows that ask for truncation take this path (logits from the store-epilogue
// GEMM); every other row keeps the fused LM head (GM_EPI_SAMPLE), which needs
// no logits tensor but cannot know a per-row threshold in its single pass.
//
// The contract, for one row (ops/sampling.py: truncation_keep and
// sample_truncated_reference are the numpy twin, in float64):
//
//   inputs     bf16 logits l[0..V), inv_temp (fp32, > 0), the row key (k0, k1),
//              top_k (int, 0 = off), top_p (fp32, >= 1 = off), log_min_p (fp32,
//              the host's float32(log(min_p)); -inf, or no array at all = off)
//   order      temperature, then top-k, then top-p, then min-p, then the draw
//   candidates the columns with a finite logit.  A NaN (or infinite) logit is
//              never kept; a row with no finite logit yields token 0
//   groups     selection works on values, not positions: the distinct values
//              of the candidates in descending order, each one group with its
//              count (+0 and -0 are one value).  Ties stay together, so the
//              kept set depends on neither scan order nor thread count
//   top-k      keep the shortest prefix of groups whose cumulative count is
//              >= top_k: a group is kept iff the count of all groups before it
//              is < top_k.  Every column tied with the k-th largest is kept
//   top-p      over what top-k kept: group mass = count * exp((value - max) *
//              inv_temp); keep the shortest prefix whose cumulative mass is >=
//              top_p * (total mass of the groups top-k kept): a group is kept
//              iff the mass of all groups before it is < that target
//   min-p      over what top-k and top-p kept: a column of value v is kept
//              iff fl(fl(v - max) * inv_temp) >= log_min_p, each operation
//              rounded once in fp32 (__fsub_rn, __fmul_rn; the twin does the
//              same in np.float32, so the rule is exact for any input).  The
//              maximum passes every earlier rule, so this is a pure threshold
//              on values and commutes with renormalisation; log_min_p = 0
//              (min_p = 1) keeps exactly the group of the maximum.  Off, the
//              test is not evaluated and the results are what they are without
//              the argument
//   first      the first group (the maximum) is always kept by top-k and
//              top-p (and by min-p for any log_min_p <= 0)
//   pick       argmax over kept columns n of float(l[n]) * inv_temp +
//              G(k0, k1, n), G the Gumbel of sample_noise.h; ties to the lower
//              column: an exact draw from the renormalised truncated softmax
//   pure       the kept set is a pure function of the row: counts are
//              integers (LDS integer atomics), masses are fp32 sums over
//              (count, value) in a fixed order (below), no float atomics
//
// How: a bf16 value is one of 65,536 ordered 16-bit keys, so the row's whole
// distribution is a count histogram over keys and the select is exact.  One
// 256-thread block a row (grid-stride over rows):
//   1. one pass for the largest candidate key;
//   2. an LDS count histogram of the window of ST_WIN = 32,768 keys below and
//      including the maximum (128 KiB; the second window, the remaining keys,
//      only if the first cannot decide: at most two.  Top-k stops at the
//      window that holds the k-th largest; top-p without top-k needs the mass
//      of both and builds the second first, so that the first is the one in
//      LDS when the prefix is scanned);
//   3. a descending scan: thread t owns the 128 consecutive keys [128 t, 128 t
//      + 128) below the window's top and sums their counts / masses in
//      descending key order; the 256 partials are added in thread order.
//      First the top-k threshold key and the kept mass, then the top-p
//      threshold key;
//   4. one pass that evaluates the noise for kept columns only (key >=
//      threshold, and the min-p test) and reduces the argmax.
// A row without top-k / top-p (top_k == 0, top_p >= 1) skips 2 and 3, with or
// without min-p.
// Thread t's 128 counters are 129 dwords apart (one pad dword a chunk), so the
// 64 lanes of a wave walk 64 different banks.  Counters are 32 bits: a row of
// any length whose columns share one value cannot overflow them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sample_noise.h"

namespace llmq {

constexpr int ST_THREADS = 256;
constexpr int ST_WIN = 32768;                        // keys a window
constexpr int ST_CHUNK = ST_WIN / ST_THREADS;        // keys a thread scans
constexpr int ST_HIST = ST_WIN + ST_THREADS;         // counters + one pad dword a chunk
constexpr int ST_MAX_BLOCKS = 256;                   // one block a CU (the histogram fills most of its LDS)
// histogram, then [256] count partials, [256] mass partials, [8] wave reduce slots (x2 words)
constexpr size_t ST_LDS_BYTES = 4 * ((size_t)ST_HIST + 2 * ST_THREADS + 16);

// bf16 bits -> key, ascending with the value; -1: not a candidate (NaN, inf)
__device__ __forceinline__ int st_key(uint32_t b) {
  if ((b & 0x7f80u) == 0x7f80u) return -1;
  const uint32_t neg = (uint32_t)((int32_t)(b << 16) >> 31);        // all ones for a negative value
  const uint32_t k = (b ^ (neg | 0x8000u)) & 0xffffu;               // ~b for a negative value, b | 0x8000 else
  return k == 0x7fffu ? 0x8000 : (int)k;                             // -0 is +0
}

__device__ __forceinline__ float st_value(int key) {
  const uint32_t b = (key & 0x8000) ? (uint32_t)(key & 0x7fff) : (~(uint32_t)key & 0xffffu);
  return __uint_as_float(b << 16);
}

__device__ __forceinline__ int st_slot(int j) { return j + (j >> 7); }     // counter of window offset j (padded)

// block-wide max of an int (every thread gets it); red: >= 4 ints of LDS
__device__ __forceinline__ int st_block_max(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  __syncthreads();                                   // (red's previous readers are done)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

// f(bits, column) for every column < V of the row, each thread its columns in
// ascending order: 16-byte loads of 8 bf16, ST_UNROLL of them in flight a
// thread (one block a CU hides the memory latency only by what each thread
// keeps in flight); the tail V..ld of the last vector is masked
constexpr int ST_UNROLL = 8;

template <bool MASK, typename F>
__device__ __forceinline__ void st_each8(const uint4& q, int n, int V, F& f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (!MASK || n + e < V) f((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu, n + e);
}

template <typename F>
__device__ __forceinline__ void st_row(const uint16_t* __restrict__ row, int V, F f) {
  constexpr int STRIDE = ST_THREADS * 8;
  int n = threadIdx.x * 8;
  for (; n + (ST_UNROLL - 1) * STRIDE + 8 <= V; n += ST_UNROLL * STRIDE) {     // whole vectors: no mask
    uint4 q[ST_UNROLL];
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) q[u] = *reinterpret_cast<const uint4*>(row + n + u * STRIDE);
#pragma unroll
    for (int u = 0; u < ST_UNROLL; ++u) st_each8<false>(q[u], n + u * STRIDE, V, f);
  }
  for (; n < V; n += STRIDE) st_each8<true>(*reinterpret_cast<const uint4*>(row + n), n, V, f);
}

// The window whose top key is ``hi``: counts of the row's candidate keys in
// (hi - ST_WIN, hi] into hist (slot of key k: st_slot(hi - k)).
__device__ __forceinline__ void st_build(const uint16_t* __restrict__ row, int V, int hi, uint32_t* hist) {
  __syncthreads();                                   // (the previous window's readers are done)
  for (int i = threadIdx.x; i < ST_HIST / 4; i += ST_THREADS) reinterpret_cast<uint4*>(hist)[i] = uint4{0, 0, 0, 0};
  __syncthreads();
  st_row(row, V, [&](uint32_t b, int) {
    const int k = st_key(b);
    const int j = hi - k;
    if (k >= 0 && j >= 0 && j < ST_WIN) atomicAdd(&hist[st_slot(j)], 1u);
  });
  __syncthreads();
}

// exclusive prefix of the 256 partials in thread order (the same sequence of
// additions for every thread) and their total
template <typename T>
__device__ __forceinline__ void st_prefix(T mine, T* part, T& before, T& total) {
  __syncthreads();
  part[threadIdx.x] = mine;
  __syncthreads();
  T run = 0, b = 0;
  for (int i = 0; i < ST_THREADS; ++i) {
    if (i == (int)threadIdx.x) b = run;
    run += part[i];
  }
  before = b;
  total = run;
}

// the mass of my chunk's groups with key >= low_key, in descending key order
__device__ __forceinline__ float st_mass(const uint32_t* hist, int hi, int low_key, float vmax, float it) {
  float m = 0.f;
  for (int i = 0; i < ST_CHUNK; ++i) {
    const int j = threadIdx.x * ST_CHUNK + i;
    const uint32_t n = hist[st_slot(j)];
    if (n && hi - j >= low_key) m += (float)n * __expf((st_value(hi - j) - vmax) * it);
  }
  return m;
}

__global__ void __launch_bounds__(ST_THREADS)
sample_truncated_kernel(const uint16_t* __restrict__ logits, int R, int V, int ld,
                        const float* __restrict__ inv_temp, const uint32_t* __restrict__ keys,
                        const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                        const float* __restrict__ log_min_p, int32_t* __restrict__ out) {
  extern __shared__ __align__(16) uint32_t st_lds[];
  uint32_t* hist = st_lds;
  uint32_t* part_c = st_lds + ST_HIST;
  float* part_m = reinterpret_cast<float*>(part_c + ST_THREADS);
  int* red = reinterpret_cast<int*>(part_m + ST_THREADS);
  float* redf = reinterpret_cast<float*>(red + 8);
  const int t = threadIdx.x;

  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const uint16_t* row = logits + (size_t)r * ld;
    const float it = inv_temp[r];
    const uint32_t k0 = keys[2 * r], k1 = keys[2 * r + 1];
    const int tk = top_k[r];
    const float tp = top_p[r];
    const float lmp = log_min_p != nullptr ? log_min_p[r] : -INFINITY;
    const bool by_m = !(lmp == -INFINITY);

    // 1. the largest candidate key
    float fmx = -INFINITY;                           // (a candidate is finite: -inf is "none")
    st_row(row, V, [&](uint32_t b, int) {
      if ((b & 0x7f80u) != 0x7f80u) fmx = fmaxf(fmx, __uint_as_float(b << 16));
    });
    int kmax = fmx == -INFINITY ? -1 : st_key(__float_as_uint(fmx) >> 16);
    kmax = st_block_max(kmax, red);
    if (kmax < 0) {                                  // no finite logit
      if (t == 0) out[r] = 0;
      continue;
    }
    const float vmax = st_value(kmax);

    // 2. + 3. the threshold key: columns with key >= thr are kept
    int thr = 0;
    const bool by_k = tk > 0, by_p = tp < 1.f;
    if (by_k || by_p) {
      // top-k: the lowest key it keeps and the mass Z of what it keeps
      int thr_k = kmax, cur = -1;
      uint32_t c_before = 0;                         // candidates in the windows above
      float Z = 0.f;
      if (!by_k) {
        // top-k keeps every candidate.  The second window first, so that the
        // first, where the top-p prefix nearly always ends, stays in LDS
        thr_k = 0;
        float z1 = 0.f, unused;
        if (kmax >= ST_WIN) {
          st_build(row, V, kmax - ST_WIN, hist);
          st_prefix(st_mass(hist, kmax - ST_WIN, 0, vmax, it), part_m, unused, z1);
        }
        st_build(row, V, kmax, hist);
        cur = 0;
        st_prefix(st_mass(hist, kmax, 0, vmax, it), part_m, unused, Z);
        Z += z1;
      }
      for (int w = 0; by_k && w < 2; ++w) {
        const int hi = kmax - w * ST_WIN;
        if (hi < 0) break;
        st_build(row, V, hi, hist);
        cur = w;
        uint32_t mine = 0;
        for (int i = 0; i < ST_CHUNK; ++i) mine += hist[st_slot(t * ST_CHUNK + i)];
        uint32_t before, total;
        st_prefix(mine, part_c, before, total);
        uint32_t c = c_before + before;
        float m = 0.f;
        int low = -1;                                // lowest kept window offset of my chunk
        for (int i = 0; i < ST_CHUNK; ++i) {
          const int j = t * ST_CHUNK + i;
          const uint32_t n = hist[st_slot(j)];
          if (n && c < (uint32_t)tk) {
            m += (float)n * __expf((st_value(hi - j) - vmax) * it);
            low = j;
          }
          c += n;
        }
        float m_before, m_total;
        st_prefix(m, part_m, m_before, m_total);
        Z += m_total;
        low = st_block_max(low, red);
        if (low >= 0) thr_k = hi - low;
        c_before += total;
        if (by_k && c_before >= (uint32_t)tk) break; // the k-th largest lies in this window
      }
      thr = thr_k;
      if (by_p) {
        // top-p over keys >= thr_k: kept iff the mass before the group < tp * Z
        const float target = tp * Z;
        int thr_p = kmax;
        float m_above = 0.f;
        for (int w = 0; w < 2; ++w) {
          const int hi = kmax - w * ST_WIN;
          if (hi < thr_k) break;
          if (cur != w) {
            st_build(row, V, hi, hist);
            cur = w;
          }
          float m_before, m_total;
          st_prefix(st_mass(hist, hi, thr_k, vmax, it), part_m, m_before, m_total);
          float run = m_above + m_before;
          int low = -1;
          for (int i = 0; i < ST_CHUNK; ++i) {
            const int j = t * ST_CHUNK + i;
            const uint32_t n = hist[st_slot(j)];
            if (n && hi - j >= thr_k) {
              if (run < target) low = j;
              run += (float)n * __expf((st_value(hi - j) - vmax) * it);
            }
          }
          low = st_block_max(low, red);
          if (low >= 0) thr_p = hi - low;
          m_above += m_total;
          if (!(m_above < target)) break;            // the prefix ends in this window
        }
        thr = thr_p;
      }
      thr = min(thr, kmax);                          // the first group is always kept
    }

    // 4. the draw over kept columns
    float bv = -INFINITY;
    int bc = 0x7fffffff;
    st_row(row, V, [&](uint32_t b, int n) {
      const int k = st_key(b);
      if (k >= thr && k >= 0 && (!by_m || __fmul_rn(__fsub_rn(__uint_as_float(b << 16), vmax), it) >= lmp)) {
        const float s = __uint_as_float(b << 16) * it + sn_gumbel(k0, k1, (uint32_t)n);
        if (s > bv) {                                // (columns ascend within a thread: a tie keeps the lower)
          bv = s;
          bc = n;
        }
      }
    });
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oc = __shfl_xor(bc, o);
      if (ov > bv || (ov == bv && oc < bc)) {
        bv = ov;
        bc = oc;
      }
    }
    __syncthreads();
    if ((t & 63) == 0) {
      redf[t >> 6] = bv;
      red[4 + (t >> 6)] = bc;
    }
    __syncthreads();
    if (t == 0) {
      for (int i = 1; i < 4; ++i)
        if (redf[i] > bv || (redf[i] == bv && red[4 + i] < bc)) {
          bv = redf[i];
          bc = red[4 + i];
        }
      out[r] = bc == 0x7fffffff ? 0 : bc;
    }
  }
}

}  // namespace llmq
