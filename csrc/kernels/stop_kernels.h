// Stop tokens and stop sequences: does the tail of what a request has
// generated, the token just chosen included, equal one of its stop entries.
// Nothing here changes a token: the kernel reads the step's final ids and the
// device-side token history (penalty_kernels.h: history_record_kernel) and
// writes one int32 a row; the engine acts on it when the step is reaped.
//
// The decision, for one row (ops/sampling.py: stop_match_reference is the
// numpy twin; everything is integer, so the twin is exact):
//
//   inputs     t0, the token finally chosen for the row in this step (int32,
//              read after every overwrite path of the head); a row record
//              int32 [6] = (slot, gen_from, end, min_tokens, ent_off, n_ent);
//              the history table hist int32 [n_slots][stride]; the packed
//              entry table ent int32 [N][1 + STOP_LEN] = (length, the entry's
//              tokens, oldest first, padded)
//   window     w = hist[slot][gen_from..end) + [t0]: the tokens this attempt
//              has generated, g = end - gen_from of them before this step.
//              gen_from is clamped into [0, stride], end into [gen_from,
//              stride]; a slot outside [0, n_slots) makes g = 0, so only t0 is
//              compared.  No index leaves the table, and nothing before
//              gen_from is read
//   entries    ent[ent_off .. ent_off + n_ent): ent_off is clamped into [0,
//              N], n_ent into [0, min(STOP_ENTRIES, N - ent_off)].  An entry
//              whose length is outside 1..STOP_LEN is ignored
//   output     the lowest k whose entry, of length l <= g + 1, equals the last
//              l tokens of w, provided g + 1 >= min_tokens; else -1
//   reads      a row whose entries all have length 1 reads no history word
//              (the engine passes slot -1 for it, as the penalty spans do)
//
// How: one wave64 a row.  Lane 8 k + j compares position j from the end of
// entry k with the token j back: j = 0 is t0, j >= 1 the history word at end -
// j.  A lane with j >= l votes true, a lane with j > g false (the entry is
// longer than the window), a lane of an entry that is absent or ignored
// false.  One 64-bit __ballot decides the row: entry k matches iff byte k of
// the mask is 0xff.  256-thread blocks hold four rows each, grid-stride above
// STOP_MAX_BLOCKS blocks.  No LDS, no atomics; lane 0 stores the result.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace llmq {

constexpr int STOP_THREADS = 256;
constexpr int STOP_ENTRIES = 8;                      // entries a row (stop tokens, then sequences)
constexpr int STOP_LEN = 8;                          // tokens an entry
constexpr int STOP_ROW_WORDS = 6;                    // (slot, gen_from, end, min_tokens, ent_off, n_ent)
constexpr int STOP_ENT_WORDS = 1 + STOP_LEN;         // (length, tokens oldest first)
constexpr int STOP_MAX_BLOCKS = 1024;                // grid-stride above this many blocks (4 rows each)

static_assert(STOP_ENTRIES * STOP_LEN == 64, "one lane per (entry, position): a wave64 a row");

// tok int32 [R], rows int32 [R][STOP_ROW_WORDS], ent int32 [N][STOP_ENT_WORDS], out int32 [R]
__global__ void __launch_bounds__(STOP_THREADS)
stop_match_kernel(const int32_t* __restrict__ tok, int R, const int32_t* __restrict__ hist, int n_slots, int stride,
                  const int32_t* __restrict__ rows, const int32_t* __restrict__ ent, int N,
                  int32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int k = lane >> 3, j = lane & 7;
  constexpr int per = STOP_THREADS / 64;
  for (int r = blockIdx.x * per + (threadIdx.x >> 6); r < R; r += gridDim.x * per) {      // (uniform over the wave)
    const int32_t* rw = rows + (size_t)r * STOP_ROW_WORDS;
    const int slot = rw[0];
    const bool in_table = hist != nullptr && slot >= 0 && slot < n_slots;
    const int from = min(max(rw[1], 0), stride);
    const int end = min(max(rw[2], from), stride);
    const int g = in_table ? end - from : 0;
    const int e_off = min(max(rw[4], 0), N);
    const int n_e = min(min(max(rw[5], 0), STOP_ENTRIES), N - e_off);
    bool vote = false;
    if (k < n_e) {
      const int32_t* e = ent + (size_t)(e_off + k) * STOP_ENT_WORDS;
      const int l = e[0];
      if (l >= 1 && l <= STOP_LEN) {
        if (j >= l) {
          vote = true;
        } else if (j <= g) {                         // (j >= 1 here implies in_table and end - j >= from >= 0)
          const int32_t have = j == 0 ? tok[r] : hist[(size_t)slot * stride + (end - j)];
          vote = e[1 + (l - 1 - j)] == have;
        }
      }
    }
    const unsigned long long mask = __ballot(vote);
    if (lane == 0) {
      int hit = -1;
      if ((long long)g + 1 >= (long long)rw[3]) {
        for (int q = STOP_ENTRIES - 1; q >= 0; --q)
          if (((mask >> (8 * q)) & 0xffull) == 0xffull) hit = q;
      }
      out[r] = hit;
    }
  }
}

}  // namespace llmq
