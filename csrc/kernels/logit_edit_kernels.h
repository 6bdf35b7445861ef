// An allow-list and additive biases over a row of bf16 logits: the in-place
// edit behind `allowed_token_ids` and `logit_bias`.  Rows that ask for either
// take the edited-row path of penalty_kernels.h (logits from the
// store-epilogue GEMM, penalise_kernel first, this edit second, then
// penalised_argmax_kernel or sample_truncated_kernel); every other row keeps
// the fused LM head.
//
// The edit, for one row (ops/sampling.py: logit_edit_reference is the numpy
// twin, bit for bit):
//
//   inputs     bf16 logits l[0..V) of a row of leading dimension ld (ld % 8 ==
//              0, the row 16-byte aligned), edited in place; an allow list
//              a[0..n_allow) of int32 token ids; bias entries (id_i, b_i), i in
//              [0, n_bias), int32 and fp32
//   1. allow   if n_allow > 0: every column n < V that is not in a becomes
//              0xff80 (-inf: no candidate downstream); a column in a keeps its
//              bits.  An id outside [0, V) is ignored, a duplicate is harmless.
//              A list with no id in [0, V) masks the whole row
//   2. bias    for each entry i with 0 <= id_i < V, only if no earlier entry
//              of the row holds the same id:  x = float(l[id_i]);  x = x + b_i
//              (__fadd_rn, one rounding);  l[id_i] = bf16(x), round to nearest
//              even (pen_bf16: NaN is written as 0x7fc0, an overflow is an
//              infinity).  -inf plus a finite bias is -inf: a bias on a column
//              that is not allowed has no effect
//   untouched  the padding [V, ld) of every row; with n_allow == 0 every
//              column without a bias entry; a row with both counts 0 is a
//              no-op
//   pure       a function of the row and its two lists: no atomics, nothing
//              depends on grid size, thread count or scan order.  A column has
//              one writer in each of the three phases below, and the phases
//              are strictly ordered by block barriers
//
// Where the lists live: one flat int32 array ids[0..N) and one fp32 array
// vals[0..N) of the same length; a row names its lists by span = (allow_off,
// n_allow, bias_off, n_bias): a = ids[allow_off .. allow_off + n_allow), (id_i,
// b_i) = (ids[bias_off + i], vals[bias_off + i]).  An offset is clamped into
// [0, N], a count into [0, min(LE_MAX, N - offset)]: no index leaves a buffer.
//
// How: one 256-thread block a row (grid-stride over rows).  Membership is
// tested against the <= 64 ids staged in LDS -- per list entry, not per
// column, so the allow pass reads nothing of the row but the allowed columns:
//   a. entry i (thread i) reads the bits of its allowed column into LDS; an
//      entry whose id is out of range, or that an earlier entry repeats, owns
//      nothing;                                                     barrier
//   b. the block sweeps [0, V) with 16-byte stores of eight 0xff80 (the last,
//      partial vector of a row is written column by column, so nothing spills
//      into [V, ld));                                               barrier
//   c. the owners write their saved bits back;                      barrier
//   d. bias entry i (thread i), if it owns its id, edits its column.
// The row's cost is one write of 2 V bytes and at most 128 scattered
// accesses.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "penalty_kernels.h"

namespace llmq {

constexpr int LE_THREADS = 256;
constexpr int LE_MAX = 64;                           // entries a list (LE_MAX <= LE_THREADS: thread i owns entry i)
constexpr int LE_MAX_BLOCKS = 1024;                  // grid-stride above this many rows

// x + b, rounded once, as bf16 (the contract's step 2 for one column)
__device__ __forceinline__ uint16_t le_bias(uint16_t b, float bias) {
  return pen_bf16(__fadd_rn(__uint_as_float((uint32_t)b << 16), bias));
}

// does entry i of list[0..n) own its id: in [0, V) and in no earlier entry
__device__ __forceinline__ bool le_owner(const int32_t* list, int i, int V) {
  const int32_t id = list[i];
  if (id < 0 || id >= V) return false;
  for (int j = 0; j < i; ++j)
    if (list[j] == id) return false;
  return true;
}

// ids int32 [N], vals fp32 [N], spans int32 [R][4] = (allow_off, n_allow, bias_off, n_bias)
__global__ void __launch_bounds__(LE_THREADS)
logit_edit_kernel(uint16_t* __restrict__ logits, int R, int V, int ld, const int32_t* __restrict__ ids,
                  const float* __restrict__ vals, int N, const int32_t* __restrict__ spans) {
  __shared__ int32_t al[LE_MAX];                     // the allow list
  __shared__ int32_t bi[LE_MAX];                     // the bias ids
  __shared__ uint16_t keep[LE_MAX];                  // the allowed columns' bits
  const int t = threadIdx.x;
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int a_off = min(max(spans[4 * r], 0), N);
    const int n_a = min(min(max(spans[4 * r + 1], 0), LE_MAX), N - a_off);
    const int b_off = min(max(spans[4 * r + 2], 0), N);
    const int n_b = min(min(max(spans[4 * r + 3], 0), LE_MAX), N - b_off);
    if (n_a == 0 && n_b == 0) continue;              // (uniform over the block)
    uint16_t* row = logits + (size_t)r * ld;
    __syncthreads();                                 // (the previous row's readers are done)
    if (t < n_a) al[t] = ids[a_off + t];
    if (t < n_b) bi[t] = ids[b_off + t];
    __syncthreads();
    if (n_a > 0) {
      const bool own = t < n_a && le_owner(al, t, V);
      if (own) keep[t] = row[al[t]];
      __syncthreads();                               // a. before b.: every allowed column is read before it is masked
      const uint32_t m = 0xff80ff80u;
      const int whole = V & ~7;
      for (int n = t * 8; n < whole; n += LE_THREADS * 8) *reinterpret_cast<uint4*>(row + n) = uint4{m, m, m, m};
      if (t < V - whole) row[whole + t] = (uint16_t)0xff80u;
      __syncthreads();                               // b. before c.
      if (own) row[al[t]] = keep[t];
      __syncthreads();                               // c. before d.
    }
    if (t < n_b && le_owner(bi, t, V)) row[bi[t]] = le_bias(row[bi[t]], vals[b_off + t]);
  }
}

}  // namespace llmq
