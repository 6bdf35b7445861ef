// Hand-written gfx950 bf16 GEMM of the backend model: C = A · Wᵀ with
// A [M][K] and W [N][K] both K-contiguous (the layout F.linear feeds
// hipBLASLt), fp32 accumulation on v_mfma_f32_16x16x32_bf16.  One function,
// gemm_tile<EPI, DIAG, FP8>, is the body of every kernel here:
// gemm_bf16_kernel<EPI> with nine epilogues, and gemm_fp8w_kernel<EPI>, the
// same tile over FP8 weights (W8A16; "The FP8 weight format" below) with
// three of them (host entry points in hipops.hip):
//
//   GM_EPI_STORE      C[M][N] = A·Wᵀ (bf16)                           gemm_bf16, gemm_fp8w
//   GM_EPI_SWIGLU     H[M][N/2] = silu(A·Wgᵀ) * (A·Wuᵀ)               gemm_bf16, gemm_fp8w
//   GM_EPI_ROPE       qkv projection + RoPE + K/V cache write         gemm_qkv_rope
//   GM_EPI_ARGMAX     LM head + greedy argmax, no logits tensor       gemm_argmax
//   GM_EPI_SAMPLE     LM head + per-row temperature sampling          gemm_sample
//   GM_EPI_RESID      C[M][N] += A·Wᵀ, residual through registers     gemm_bf16 (A/B)
//   GM_EPI_RESID_LDS  ... residual tile staged into LDS by DMA        gemm_bf16 (default), gemm_fp8w
//   GM_EPI_RESID_PRE  ... its first quarter fetched at kernel start   gemm_bf16 (A/B)
//   GM_EPI_RESID_RMS  GM_EPI_RESID_LDS + the RMSNorm row scales       gemm_residual_rms
//
// The residual forms read and write bf16 C with one rounding of the fp32 sum,
// as hipBLASLt's beta = 1: the o / down projections into the residual stream.
// STORE, SWIGLU and ROPE take optional per-row scales (the folded RMSNorm);
// STORE, SWIGLU, ROPE and RESID_LDS can run their last tiles split-K (GmSplit).
//
// The SwiGLU form removes the separate silu_mul pass and the HBM round trip
// of the [M][2F] gate/up product (profiles/r1_gemm_experiments.md): W rows are
// pre-permuted (`swiglu_permute` in ops/gemm.py) so that each wave's 64
// output columns are 32 gate features followed by the same 32 up features,
// i.e. every lane holds g and u of one (row, feature) in the same register
// slot of two accumulators -- the epilogue is pure register math.
//
// Layout of this file: gm_tile_coords (block -> tile), gm_split_join (split-K
// hand-over), then gemm_tile, which calls them around the main loop and ends
// in one `if constexpr` branch per epilogue family.
//
// Structure (cdna_hip_programming.md §5, "the 256² 8-phase template"):
//   * 256x256 output tile, BK = 64, 512 threads = 8 waves as 2 (M) x 4 (N),
//     128x64 outputs per wave = 32 16x16 fp32 accumulators (128 AGPR/VGPR).
//   * LDS 128 KiB = 2 K-tile buffers x {A0, A1, B0, B1} half-tiles of 128
//     rows x 128 B.  A half h holds the rows of m-half h of BOTH wave rows,
//     B half h the columns of n-half h of all four wave columns, so each
//     half-tile is consumed in exactly one quadrant phase and can be
//     restaged as soon as that phase's reads retire.
//   * Staging by buffer_load_dwordx4 ... lds (16 B per lane, lane-linear LDS
//     image; fixed per-lane VGPR offset + scalar K offset, no VALU per load); the bank swizzle p = c ^ ((row >> 1) & 7) on the 16-B chunk is
//     applied to the per-lane SOURCE address and to the ds_read address
//     (rule 21), which makes the 16 x b128 fragment reads conflict-free
//     across the ds_read_b128 lane groups of the 128-B-row image.
//   * 8 phases per 2 K-tiles: each phase reads one operand half, issues one
//     half-tile prefetch (2 glds per lane), barrier, 16 MFMAs (one quadrant x
//     K = 64), barrier.  The prefetch runs 3 half-tiles ahead; a counted
//     `s_waitcnt vmcnt(6)` in every phase (never 0 in the steady state)
//     retires exactly the buffer the next phase reads, and raw s_barrier is
//     used throughout so no wait drains the DMA queue early.
//   * XCD-aware block order: blocks that the dispatcher puts on one XCD take
//     a contiguous run of tiles, grouped 8 M-tiles x N so concurrently
//     running tiles share A and W panels in that XCD's L2.
//   * M need not be a multiple of 256: A rows are clamped on load, rows >= M
//     are not stored.  K % 128 == 0 and N % 256 == 0 are checked by the host.
//
// The FP8 weight format (gemm_tile<EPI, GM_DIAG_NONE, true>, EPI in STORE /
// SWIGLU / RESID_LDS): C (+)= (A · decode(Wq)ᵀ) * cs[n] * rs[m] with Wq [N][K]
// uint8 e4m3fn codes (K-contiguous, the tensor the skinny FP8 kernel reads) and
// one fp32 scale a weight row, cs [N] (ops/quant.py holds the contract).  For
// the micro-forwards that carry prefill (more than 64 rows), where the skinny
// kernel's 128-row chunks re-read and re-decode their weights a chunk.  Every
// k enters the MFMA step (K-tile, kk) and operand slot (lane fq, element) it
// enters in the bf16 form, so with power-of-two scales the result is bit-equal
// to gemm_bf16_kernel over the decoded weights.  Everything above holds; what
// differs sits behind `if constexpr (FP8)` in gemm_tile:
//   * A B half-tile is 128 columns x 64 codes = 8 KiB of 64-byte rows: ONE
//     16-byte buffer_load ... lds a lane (wave w: rows 16w .. 16w + 15, four
//     lanes a row).  LDS row lr holds column (lr / 32) * 64 + h * 32 + lr % 32
//     of the tile, as the bf16 image.  Operand LDS: 2 x (2 x 16 + 2 x 8) =
//     96 KiB; the launch still asks for 128 KiB, which the store and residual
//     epilogues use (8 waves x 16 KiB).
//   * Swizzle of the B image: the 16-byte chunk c of row r sits in slot
//     c ^ ((r >> 2) & 3), applied to the per-lane SOURCE address and to the
//     read address.  A B fragment is 8 bytes a lane (ds_read_b64: two 32-lane
//     groups, bank = (addr / 4) % 64, i.e. addr % 256).  A group is 16 rows fr
//     x two lanes fq (2g, 2g + 1) that read the two 8-byte halves of source
//     chunk g + 2 kk: address % 256 = (fr & 3) * 64 + ((g + 2 kk) ^ (fr >> 2))
//     * 16 + (fq & 1) * 8.  fr & 3 picks the 64-byte quarter, fr >> 2 (four
//     values, xor with a constant is a bijection) the 16-byte slot in it,
//     fq & 1 the half: 32 lanes, 32 distinct 8-byte bank pairs -- no conflict.
//     (Unswizzled, rows r and r + 4 would share their banks: 4-way.)
//   * The codes are decoded to bf16 in registers after the fragment read, right
//     before the MFMAs that use them (sk_fp8x8_bf16: 4 VALU ops a fragment,
//     16 a phase beside its 16 MFMAs); the raw fragments are 2 VGPRs each.
//   * The counted waits follow the DMAs a half-tile (the table at kFlyA in
//     gemm_tile).
//   * The column scale multiplies the fp32 accumulators after the split-K
//     join, before the row scale and any epilogue math: a lane owns columns
//     tn * 256 + wc * 64 + nh * 32 + n * 16 + fr (under SwiGLU gate and up of
//     a feature carry different scales; cs follows the permuted row order).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fp8_decode.h"
#include "sample_noise.h"

namespace llmq {

typedef __attribute__((ext_vector_type(8))) short gm_bf16x8;
typedef __attribute__((ext_vector_type(4))) float gm_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int gm_u32x4;

constexpr int GM_BM = 256, GM_BN = 256, GM_BK = 64, GM_THREADS = 512;
constexpr int GM_HALF_BYTES = 128 * GM_BK * 2;     // 16 KiB
constexpr int GM_BUF_BYTES = 4 * GM_HALF_BYTES;    // A0 A1 B0 B1
constexpr int GM_LDS_BYTES = 2 * GM_BUF_BYTES;     // 128 KiB
constexpr int GM_GROUP_M = 8;                    // default M-tiles per block-order group

enum { GM_EPI_STORE = 0, GM_EPI_SWIGLU = 2, GM_EPI_ROPE = 3, GM_EPI_ARGMAX = 4, GM_EPI_RESID = 5,
       GM_EPI_RESID_LDS = 6, GM_EPI_RESID_PRE = 7, GM_EPI_RESID_RMS = 8, GM_EPI_SAMPLE = 9 };
// GM_EPI_RESID_PRE: GM_EPI_RESID_LDS whose first quarter of the residual tile
// (rows 0-31 of every wave's 128 x 64 block) is fetched into the 32 KiB of
// LDS gfx950 has beyond the operand buffers at kernel start, so it is in LDS
// long before the epilogue; the launch asks for 160 KiB.
constexpr int GM_LDS_SPARE = 32768;
template <int EPI>
constexpr int gm_lds_bytes() { return EPI == GM_EPI_RESID_PRE ? GM_LDS_BYTES + GM_LDS_SPARE : GM_LDS_BYTES; }

// Power / energy DIAGNOSTICS of the main loop (bench/gemm_energy_diag.hip, the
// evidence behind the README's power-cap claim; never launched by the
// library).  Each drops one kind of work from the steady-state K loop while
// keeping every MFMA, so all but GM_DIAG_CLOCK compute WRONG numbers:
enum {
  GM_DIAG_NONE = 0,          // production
  GM_DIAG_SKIP_A2 = 1,       // no A fragment reads in phases 3 / 7: one third fewer LDS read bytes,
                             // what a 128x128 wave tile would read
  GM_DIAG_NO_LDS_READ = 2,   // no fragment read in the loop
  GM_DIAG_NO_DMA = 3,        // no staging DMA in the loop (no L2 / HBM traffic in steady state)
  GM_DIAG_CLOCK = 4,         // production + shader-clock stamps (gm_diag_stamp)
  GM_DIAG_CLOCK_NO_DMA = 5,  // GM_DIAG_NO_DMA + the stamps
  GM_DIAG_L2_PANELS = 6      // every block stages the panels of tile (0, 0): staging served from L2
};

// Epilogue side outputs.
// GM_EPI_ARGMAX: the LM head's greedy sampling as the epilogue -- no [M][N]
// logits tensor.  Each tile writes, per row, the max over its 256 columns and
// the (global) column of its first occurrence into pv / pi [M][N / 256];
// gemm_argmax_reduce_kernel picks the first maximum over the tiles (ties go
// to the lower column, as torch.argmax does).  Values are the fp32
// accumulators (not bf16-rounded logits).
// GM_EPI_RESID_RMS (GM_EPI_RESID_LDS plus): the
// RMSNorm row scale of the updated residual rows, fused into the epilogue --
// each block's per-row sums of squares of the bf16 values it stores (rpart
// [tiles_m][tiles_n][256], written through to memory), and the last of a
// row tile's tiles_n blocks (rticket[tiles_m], zero at launch, re-zeroed)
// adds them in column-tile order and writes 1 / sqrt(sum / N + reps) to
// rscale[tm * 256 + row]: what row_rms_kernel computes, in a fixed order,
// without the 33 MB re-read of the rows by a separate launch.
// GM_EPI_SAMPLE: GM_EPI_ARGMAX over score = acc * inv_temp[row] + G(key[row],
// column) -- per-request temperature sampling by the Gumbel-max identity,
// the noise a pure function of (row key, column) (sample_noise.h).  A row
// with inv_temp == 0 is greedy: its score is the raw accumulator, so its
// result is GM_EPI_ARGMAX's, ties included.  inv_temp [ceil(M / 256) * 256]
// and key [ceil(M / 256) * 256][2] (k0, k1) hold whole row tiles, like the
// row scales; they share the storage of the GM_EPI_RESID_RMS pointers (no
// epilogue uses both), so the other kernels' argument layout is unchanged.
struct GmSide {
  float* pv;
  int32_t* pi;
  union {
    float* rpart;
    const float* inv_temp;
  };
  union {
    int* rticket;
    const uint32_t* key;
  };
  float* rscale;
  float reps;
};

// GM_EPI_ROPE: the fused qkv projection's epilogue = the rope_kv kernel
// (llama_kernels.h): RoPE (rotate-half) on q and k, q to ``q``, k / v into
// this layer's cache at (slot[row], pos[row]); W rows are the plain
// [q heads | k heads | v heads] order (N = (Hq + 2 Hkv) * 128).
struct GmRope {
  const int32_t* pos;
  const int32_t* slot;
  const float* cos_t;                              // [max_ctx][64]
  const float* sin_t;
  uint16_t* q;                                     // [M][Hq * 128]
  uint16_t* kc;                                    // [n_slots][Hkv][max_ctx][128]
  uint16_t* vc;
  int Hq, Hkv, max_ctx, n_slots;
};
enum { GM_A0 = 0, GM_A1 = 1, GM_B0 = 2, GM_B1 = 3 };

__device__ __forceinline__ uint16_t gm_f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);                 // round to nearest even (finite inputs)
  return (uint16_t)(u >> 16);
}

// Per-row scales of this lane's 32 accumulator rows (row0 + mh*64 + m*16 +
// fq*4 + j): eight 16-B loads issued together, one branch for the whole set
// (a per-element load under a runtime condition makes hipcc wait for each
// load in turn).  rs must hold ceil(M / 256) * 256 floats (ops/gemm.py pads).
__device__ __forceinline__ void gm_load_row_scales(const float* __restrict__ rs, int row0, int fq,
                                                   gm_f32x4 (&sc)[2][4]) {
  if (rs) {
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int m = 0; m < 4; ++m)
        sc[mh][m] = *reinterpret_cast<const gm_f32x4*>(rs + row0 + mh * 64 + m * 16 + fq * 4);
  } else {
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int m = 0; m < 4; ++m) sc[mh][m] = gm_f32x4{1.f, 1.f, 1.f, 1.f};
  }
}

// Split-K for the last partial wave of tiles (GM_EPI_ROPE): with 384 tiles on
// 256 CUs the second wave would run half empty.  Tiles [full, nwg) run as two
// blocks each over one half of K; the first to finish publishes its fp32
// accumulators (agent-scope release), the second adds them (acquire) and runs
// the epilogue -- cdna_hip_programming.md §5 "Projection GEMM" item 2.
#define GM_CPOL_SC1 16   // cache-policy bit: agent-scope coherent access

struct GmSplit {
  int full;       // tiles [0, full) run whole
  float* ws;      // [nwg - full][GM_THREADS * 128] fp32 accumulator slabs (nullptr: no split)
  int* cnt;       // [nwg - full][2]: ticket, ready -- zero at launch; the second half re-zeroes them
};

typedef __attribute__((address_space(3))) void* gm_lds_ptr;
typedef gm_f32x4 gm_acc_t[2][4][2][2];             // a wave's 128 x 64 outputs: [mh][m][nh][n]

// One half-tile (128 rows x 64 bf16) global -> LDS: 2 buffer_load ... lds per
// lane.  The per-lane row/chunk offset is a fixed VGPR, the K-tile offset a
// scalar (soffset), so the K-loop spends no VALU on staging addresses.
__device__ __forceinline__ void gm_stage(__amdgpu_buffer_rsrc_t rs, uint32_t v0, uint32_t v1, uint32_t soff,
                                         uint8_t* smem, uint32_t dst0, uint32_t dst1) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (gm_lds_ptr)(smem + dst0), 16, v0, soff, 0, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (gm_lds_ptr)(smem + dst1), 16, v1, soff, 0, 0);
}

#define GM_LGKM(N) asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory")
#define GM_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")   // N: a constant expression
#define GM_FENCE() __builtin_amdgcn_sched_barrier(0)
#define GM_BARRIER()                  \
  do {                                \
    GM_FENCE();                       \
    __builtin_amdgcn_s_barrier();     \
    GM_FENCE();                       \
  } while (0)

// One 8-byte LDS read that stays a ds_read_b64 (the FP8 form's B fragments).
// Left to the compiler, the n = 0 / n = 1 fragments (1 KiB apart) pair into
// ds_read2st64_b64, which takes twice the LDS cycles and banks by 16-lane
// groups modulo 32 (a 2-way conflict on this image).  The compiler does not
// count this read in lgkmcnt: GM_PHASE_END waits lgkmcnt(0) and fences before
// the first use.
typedef __attribute__((ext_vector_type(2))) unsigned int gf_u32x2;
template <int OFF>
__device__ __forceinline__ gf_u32x2 gf_lds_read_b64(uint32_t addr) {
  gf_u32x2 r;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}

// XCD-contiguous remap (bijective for any count): the dispatcher puts block
// b of PER * count blocks on XCD b % 8; the XCDs take contiguous runs of the
// blocks' work items, and this is where the run of b's XCD starts (b is item
// b / 8 of that run).  PER, the blocks per tile, is a template parameter and
// the caller adds b >> 3 because the optimiser simplifies this function
// before it inlines it: both keep the compiler's output what it was with the
// formula written out per caller (docs/development.md, "two-tree comparison").
template <int PER>
__device__ __forceinline__ int gm_xcd_run_start(int b, int count) {
  const int n = PER * count;
  const int xcd = b & 7, q8 = n >> 3, r8 = n & 7;
  return xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
}

struct GmTile {
  int tm, tn;     // output tile
  int pid;        // its index in the launch's tile order
  int khalf;      // -1: the whole K; 0 / 1: this block's K-half of a split tile
};

// Block ``bid`` of the launch's block order -> its tile: the whole tiles
// [0, full) by the XCD-contiguous remap, then 8-M-tile grouping; split tiles
// take two consecutive blocks.
__device__ __forceinline__ GmTile gm_tile_coords(int bid, int tiles_m, int tiles_n, int nwg, int full,
                                                 int group_m) {
  GmTile t;
  t.khalf = -1;
  if (bid < full) {
    t.pid = gm_xcd_run_start<1>(bid, full) + (bid >> 3);
  } else {
    // split tiles: the same XCD-contiguous remap over the tail's blocks, so
    // an XCD runs both K-halves of a contiguous run of tiles (their A / B
    // panels share its L2) instead of one half of every 4th tile
    const int b = bid - full;
    const int j = gm_xcd_run_start<2>(b, nwg - full) + (b >> 3);
    t.pid = full + (j >> 1);
    t.khalf = j & 1;
  }
  const int group = t.pid / (group_m * tiles_n);
  const int first_m = group * group_m;
  const int gsize = min(tiles_m - first_m, group_m);
  t.tm = first_m + (t.pid % (group_m * tiles_n)) % gsize;
  t.tn = (t.pid % (group_m * tiles_n)) / gsize;
  return t;
}

// ------------------------------------------------------------ split-K hand-over
// Split tile ``tix``: the first K-half to finish hands its accumulators over
// and returns true (the block is done); the second adds them to its own and
// returns false (it runs the epilogue).
__device__ __forceinline__ bool gm_split_join(uint8_t* __restrict__ smem, gm_acc_t& acc, const GmSplit& sp,
                                              int tix) {
  const int tid = threadIdx.x;
  int* cnt = sp.cnt + 2 * tix;
  if (tid == 0) *reinterpret_cast<int*>(smem) =
      __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const int ticket = *reinterpret_cast<volatile int*>(smem);
  __syncthreads();
  // The slab moves with agent-scope (sc1) stores / loads -- written through
  // and read past this XCD's L2 (the halves run on different XCDs) -- so
  // neither side needs the whole-L2 write-back / invalidate of an
  // agent-scope fence (measured: 156 vs 160 us at T=4041, fences cost L2
  // hits for every block on the XCD).  Order: all slab stores acknowledged
  // (vmcnt 0) -> barrier -> ready flag; the reader sees the flag before
  // its barrier and then loads.
  float* slab = sp.ws + (size_t)tix * GM_THREADS * 128;
  const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(slab, 0, GM_THREADS * 32 * 16, 0x00020000);
  if (ticket == 0) {                             // first: publish, then leave
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int d = 0; d < 2; ++d)
          {
            const int i = ((a * 4 + b) * 4 + c * 2 + d) * GM_THREADS + tid;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gm_u32x4, acc[a][b][c][d]), srs, i * 16,
                                                   0, GM_CPOL_SC1);
          }
    GM_VMCNT(0);
    __syncthreads();
    if (tid == 0) __hip_atomic_store(cnt + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
  }
  if (tid == 0) {                                // second: wait for the slab (bounded)
    for (int spin = 0; spin < (1 << 24); ++spin) {
      if (__hip_atomic_load(cnt + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
      __builtin_amdgcn_s_sleep(2);
    }
    GM_VMCNT(0);
    // both halves are done with the counters: leave them zeroed for the next launch
    __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cnt + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < 2; ++d)
        {
          const int i = ((a * 4 + b) * 4 + c * 2 + d) * GM_THREADS + tid;
          acc[a][b][c][d] += __builtin_bit_cast(gm_f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                 srs, i * 16, 0, GM_CPOL_SC1));
        }
  return false;
}


// ------------------------------------------------------------ the tile
// One output tile (or one K-half of a split tile): block ``bid`` of the
// launch's block order.  In order: tile coordinates (gm_tile_coords), the
// main loop (operand addresses, prologue, steady 8-phase loop, drain), the
// split-K join (gm_split_join), then one `if constexpr` branch per epilogue
// family.  The main loop and the epilogues stay in this one function on
// purpose: hoisting either into a function of its own changes the kernels'
// register allocation (profiles/gemm_refactor.md).  The weight format is a
// parameter for the same reason: FP8 = true (W: uint8 codes, cs: their column
// scales; the file header) differs in `if constexpr (FP8)` branches in place,
// which leave the bf16 kernels' instructions what they were
// (profiles/gemm_fp8w_merge.md).
template <int EPI, int DIAG, bool FP8 = false>
__device__ __forceinline__ void gemm_tile(
    uint8_t* __restrict__ smem, const uint16_t* __restrict__ A, const void* __restrict__ W,
    const float* __restrict__ cs, uint16_t* __restrict__ C, int M, int N, int K, int group_m,
    const float* __restrict__ rs, const GmRope& rp, const GmSplit& sp, const GmSide& am, const int bid) {
  static_assert(!FP8 || (DIAG == GM_DIAG_NONE &&
                         (EPI == GM_EPI_STORE || EPI == GM_EPI_SWIGLU || EPI == GM_EPI_RESID_LDS)),
                "the FP8 form: STORE, SWIGLU and RESID_LDS, no diagnostics");
  // a B half-tile (128 columns x BK): 16 KiB of bf16 or 8 KiB of codes; a K-tile buffer A0 A1 B0 B1
  constexpr int kBHalf = 128 * GM_BK * (FP8 ? 1 : 2);
  constexpr int kBuf = 2 * GM_HALF_BYTES + 2 * kBHalf;   // 64 KiB / 48 KiB
  static_assert(2 * kBuf <= GM_LDS_BYTES, "operand buffers inside the launch's LDS");
  constexpr bool kStamp = DIAG == GM_DIAG_CLOCK || DIAG == GM_DIAG_CLOCK_NO_DMA;
  const int tiles_m = (M + GM_BM - 1) / GM_BM;
  const int tiles_n = N / GM_BN;
  const int nwg = tiles_m * tiles_n;
  const int full = sp.ws ? sp.full : nwg;          // tiles [full, nwg) run split-K
  const GmTile tile = gm_tile_coords(bid, tiles_m, tiles_n, nwg, full, group_m);
  const int pid = tile.pid, khalf = tile.khalf, tm = tile.tm, tn = tile.tn;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // GM_DIAG_CLOCK*: shader-clock and 100 MHz reference stamps at
  // entry and exit, written by thread 0 to am.pv as 4 x u64 per block --
  // the in-kernel clock = d(memtime) / d(memrealtime) x 100 MHz, unprofiled
  // (MI355X_MICROARCH.md 'DVFS give-back' item 6)
  uint64_t st_t0 = 0, st_r0 = 0;
  if constexpr (kStamp) {
    st_t0 = __builtin_amdgcn_s_memtime();
    st_r0 = __builtin_amdgcn_s_memrealtime();
  }
  const int wr = w >> 2, wc = w & 3;

  // ---- staging sources: half h, instruction i -> LDS local row lr = i*64 + w*8 + lane/8
  // (FP8, B: half h, its one instruction -> LDS row w*16 + lane/4, slot lane%4)
  const int srow = w * 8 + (lane >> 3);            // 0..63
  const int schunk = (lane & 7) ^ ((srow >> 1) & 7);   // source chunk for LDS slot lane&7
  const int brow = w * 16 + (lane >> 2);           // 0..127
  const int bchunk = (lane & 3) ^ ((brow >> 2) & 3);   // source chunk for LDS slot lane&3
  const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsw =
      __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, N * K * (FP8 ? 1 : 2), 0x00020000);
  uint32_t va[2][2], vb[2][FP8 ? 1 : 2];           // byte offsets (row, chunk) of K-tile 0
  // (GM_DIAG_L2_PANELS: the panels of tile (0, 0), so nearly every staging read hits the XCD's L2)
  const int ltm = DIAG == GM_DIAG_L2_PANELS ? 0 : tm, ltn = DIAG == GM_DIAG_L2_PANELS ? 0 : tn;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int row = ltm * GM_BM + i * 128 + h * 64 + srow;
      row = row < M ? row : M - 1;
      va[h][i] = (uint32_t)row * (uint32_t)K * 2u + (uint32_t)schunk * 16u;
      if constexpr (!FP8) {
        const int col = ltn * GM_BN + (2 * i + (w >> 2)) * 64 + h * 32 + (w & 3) * 8 + (lane >> 3);
        vb[h][i] = (uint32_t)col * (uint32_t)K * 2u + (uint32_t)schunk * 16u;
      }
    }
    if constexpr (FP8) {
      const int col = ltn * GM_BN + (brow >> 5) * 64 + h * 32 + (brow & 31);
      vb[h][0] = (uint32_t)col * (uint32_t)K + (uint32_t)bchunk * 16u;
    }
  }
  // LDS destination (wave-uniform) of instruction i inside a half-tile
  const uint32_t dst_i0 = (uint32_t)(w * 8) * 128u;
  const uint32_t dst_i1 = (uint32_t)(64 + w * 8) * 128u;
  const uint32_t dst_b = (uint32_t)(w * 16) * 64u;   // FP8: of the one B instruction

  // ---- fragment read offsets (bytes inside buffer 0), per k-step kk
  const uint32_t sbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;   // LDS address
  const int fr = lane & 15, fq = lane >> 4;
  uint32_t aoff[2][2], boff[2][2];                 // [buffer][kk]; buffer 1 = + kBuf (beyond ds offset:)
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int c = fq + 4 * kk;                     // 8 k of the K-tile: 16 B of A and bf16 B, 8 B of codes
    aoff[0][kk] = (uint32_t)(wr * 64 + fr) * 128u + (uint32_t)((c ^ ((fr >> 1) & 7)) * 16);
    if constexpr (FP8)
      boff[0][kk] = (uint32_t)(2 * GM_HALF_BYTES) + (uint32_t)(wc * 32 + fr) * 64u +
                    (uint32_t)(((c >> 1) ^ ((fr >> 2) & 3)) * 16 + (c & 1) * 8);
    else
      boff[0][kk] = (uint32_t)(wc * 32 + fr) * 128u + (uint32_t)((c ^ ((fr >> 1) & 7)) * 16) + 2 * GM_HALF_BYTES;
    aoff[1][kk] = aoff[0][kk] + kBuf;
    boff[1][kk] = boff[0][kk] + kBuf;
  }

  gm_acc_t acc;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < 2; ++d) acc[a][b][c][d] = gm_f32x4{0.f, 0.f, 0.f, 0.f};

  gm_bf16x8 af[4][2];                              // one m-half: [m][kk]
  using gm_bfrag = std::conditional_t<FP8, gf_u32x2, gm_bf16x8>;   // a B fragment: 8 codes or 8 bf16
  gm_bfrag bfr[2][2][2];                           // both n-halves: [nh][n][kk]
  gm_bfrag b0y[2][2];                              // buffer 1's B0 fragments ([nh = 0] of bfr: buffer 0's)
  // K-tiles of this block: all, or one half for a split tile (host: nt % 4 == 0)
  const int nt = khalf < 0 ? K / GM_BK : K / GM_BK / 2;
  const int kt0 = khalf > 0 ? nt : 0;

  // ---- the phase macros (every name they use is declared above)
  // FP8: a B half is one 16-byte DMA a lane, its K-tile step GM_BK bytes
#define GM_STAGE(BUF, HALF, KT)                                                               \
  do {                                                                                        \
    if constexpr (FP8 && (HALF) >= 2) {                                                       \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(                                               \
          rsw, (gm_lds_ptr)(smem + (uint32_t)(BUF) * kBuf + 2 * GM_HALF_BYTES + (uint32_t)((HALF)-2) * kBHalf + dst_b), \
          16, vb[(HALF)-2][0], (uint32_t)((KT) + kt0) * GM_BK, 0, 0);                         \
    } else {                                                                                  \
      const uint32_t _ko = (uint32_t)((KT) + kt0) * (GM_BK * 2);                              \
      const uint32_t _b = (uint32_t)(BUF) * kBuf + (uint32_t)(HALF) * GM_HALF_BYTES;          \
      if constexpr ((HALF) < 2)                                                               \
        gm_stage(rsa, va[(HALF)][0], va[(HALF)][1], _ko, smem, _b + dst_i0, _b + dst_i1);     \
      else                                                                                    \
        gm_stage(rsw, vb[(HALF)-2][0], vb[(HALF)-2][1], _ko, smem, _b + dst_i0, _b + dst_i1); \
    }                                                                                         \
  } while (0)

#define GM_READ_A(BUF, MH)                                                                     \
  do {                                                                                         \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                              \
      _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                         \
        af[m][kk] = *reinterpret_cast<const gm_bf16x8*>(smem + aoff[BUF][kk] + (MH) * GM_HALF_BYTES + m * 2048); \
  } while (0)

// the B fragments of n-half NH of buffer BUF (16 rows apart: 2 KiB, FP8 1 KiB) into DST[n][kk]
#define GM_READ_B_INTO(BUF, NH, DST)                                                           \
  do {                                                                                         \
    if constexpr (FP8) {                                                                       \
      _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                       \
        DST[0][kk] = gf_lds_read_b64<(NH) * kBHalf>(sbase + boff[BUF][kk]);                    \
        DST[1][kk] = gf_lds_read_b64<(NH) * kBHalf + 1024>(sbase + boff[BUF][kk]);             \
      }                                                                                        \
    } else {                                                                                   \
      _Pragma("unroll") for (int n = 0; n < 2; ++n)                                            \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                       \
          DST[n][kk] = *reinterpret_cast<const gm_bf16x8*>(smem + boff[BUF][kk] + (NH) * kBHalf + n * 2048); \
    }                                                                                          \
  } while (0)
#define GM_READ_B(BUF, NH) GM_READ_B_INTO(BUF, NH, bfr[NH])
// B0 fragments into an explicit register set, MFMA with it
#define GM_READ_B0_INTO(BUF, DST) GM_READ_B_INTO(BUF, 0, DST)

// (FP8: the codes of BREG decoded in front of the MFMAs that use them)
#define GM_MFMA_WITH(MH, NH, BREG)                                                             \
  do {                                                                                         \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                         \
      gm_bf16x8 _b[2];                                                                         \
      _Pragma("unroll") for (int n = 0; n < 2; ++n) {                                          \
        if constexpr (FP8) _b[n] = sk_fp8x8_bf16(BREG[n][kk].x, BREG[n][kk].y);                \
        else _b[n] = BREG[n][kk];                                                              \
      }                                                                                        \
      _Pragma("unroll") for (int m = 0; m < 4; ++m)                                            \
        _Pragma("unroll") for (int n = 0; n < 2; ++n)                                          \
          acc[MH][m][NH][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m][kk], _b[n],        \
                                                                      acc[MH][m][NH][n], 0, 0, 0); \
    }                                                                                          \
  } while (0)

// (FP8: the fence keeps the decode behind the wait -- the asm fragment reads
// are not in the compiler's lgkmcnt count, gf_lds_read_b64)
#define GM_PHASE_END(MH, NH, BREG)   \
  do {                               \
    GM_BARRIER();                    \
    GM_LGKM(0);                      \
    if constexpr (FP8) GM_FENCE();   \
    GM_MFMA_WITH(MH, NH, BREG);      \
    GM_BARRIER();                    \
  } while (0)

  // Counted waits.  A stage is kDmaA or kDmaB buffer_load ... lds a lane, and
  // every phase must leave exactly the last three staged half-tiles in flight:
  //     stage of the phase   in flight after it       s_waitcnt (bf16 / FP8)
  //     A0 or A1             A, B, A                  kFlyA: vmcnt(6) / vmcnt(5)
  //     B0 or B1             B, A, B                  kFlyB: vmcnt(6) / vmcnt(4)
  //     prologue (7 halves)  B1, A0, B0 of buffer 1   kFlyB
  //     drain phases 1-4     A1 B1 A0 / A1 B1 / A1 / -    6, 4, 2, 0 / 5, 3, 2, 0
  constexpr int kDmaA = 2, kDmaB = FP8 ? 1 : 2;
  constexpr int kFlyA = 2 * kDmaA + kDmaB, kFlyB = kDmaA + 2 * kDmaB;

  // ---- main loop: prologue
  // Wave priority: one static s_setprio 1 for wave row 1 (the
  // later-dispatched half, cdna_hip_programming.md T5 static form), no
  // per-cluster flips -- 1.7 % faster than s_setprio 1 around every MFMA
  // cluster at T = 4041; the static priority on wave row 0, or none, lost too
  // (profiles/r2_gemm_prio_ab.jsonl).
  if (wr == 1) __builtin_amdgcn_s_setprio(1);
  // Balanced schedule: every phase retires the half-tile staged 3 phases
  // earlier (vmcnt(6) each phase), so the NEXT buffer's B0 fragments can be
  // read one phase early (phases 4 and 8, which otherwise read nothing):
  // 8/4/8/4 fragment reads per phase instead of 12/4/8/0.  Stage order per
  // buffer is B0, A0, B1, A1; every restage is >= 2 phases after the
  // half-tile's last read (safe with the wave-row stagger).
  if constexpr (EPI == GM_EPI_RESID_PRE) {
    // the residual rows 0-31 of this wave's output block -> spare LDS; the
    // prologue's counted vmcnt waits retire them with the first half-tiles
    const int col0p = tn * GM_BN + wc * 64, row0p = tm * GM_BM + wr * 128;
    const __amdgpu_buffer_rsrc_t rsp =
        __builtin_amdgcn_make_buffer_rsrc((void*)C, 0, (uint32_t)M * (uint32_t)N * 2u, 0x00020000);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = i * 8 + (lane >> 3), c = lane & 7;
      const uint32_t vo = ((uint32_t)(row0p + r) * (uint32_t)N + (uint32_t)(col0p + c * 8)) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsp, (gm_lds_ptr)(smem + GM_LDS_BYTES + w * 4096 + i * 1024), 16,
                                               vo, 0, 0, 0);
    }
  }
  GM_STAGE(0, GM_B0, 0);
  GM_STAGE(0, GM_A0, 0);
  GM_STAGE(0, GM_B1, 0);
  GM_STAGE(0, GM_A1, 0);
  GM_STAGE(1, GM_B0, 1);
  GM_STAGE(1, GM_A0, 1);
  GM_STAGE(1, GM_B1, 1);
  GM_VMCNT(kFlyB);
  GM_BARRIER();
  GM_READ_B0_INTO(0, bfr[0]);
  if constexpr (DIAG >= GM_DIAG_SKIP_A2 && DIAG <= GM_DIAG_NO_DMA) {   // every fragment register defined
    GM_READ_A(0, 0);
    GM_READ_B(0, 1);
    GM_READ_B0_INTO(1, b0y);
  }
  // wave-row 1 runs half a phase behind wave-row 0: on every SIMD (one wave
  // of each row) one wave's fragment reads + DMA issue overlap the other's
  // MFMA cluster.  One extra barrier here, balanced after the loop.
  if (wr == 1) GM_BARRIER();

  // ---- main loop: steady state, two K-tiles = eight phases per trip.  The
  // GM_D_* forms are the diagnostics' switches (GM_DIAG_*): which fragment
  // reads and staging DMAs the steady loop issues
  int t = 0;
  constexpr bool kRdA = DIAG != GM_DIAG_NO_LDS_READ;
  constexpr bool kRdA2 = DIAG != GM_DIAG_SKIP_A2 && DIAG != GM_DIAG_NO_LDS_READ;
  constexpr bool kRdB = DIAG != GM_DIAG_NO_LDS_READ;
  constexpr bool kDma = DIAG != GM_DIAG_NO_DMA && DIAG != GM_DIAG_CLOCK_NO_DMA;
#define GM_D_READ_A(ON, B, H) do { if constexpr (ON) GM_READ_A(B, H); } while (0)
#define GM_D_READ_B(B, H) do { if constexpr (kRdB) GM_READ_B(B, H); } while (0)
#define GM_D_READ_B0(B, D) do { if constexpr (kRdB) GM_READ_B0_INTO(B, D); } while (0)
#define GM_D_STAGE(B, H, K) do { if constexpr (kDma) GM_STAGE(B, H, K); } while (0)
  for (; t < nt - 2; t += 2) {
    {
      GM_D_READ_A(kRdA, 0, 0); GM_D_STAGE(1, GM_A1, t + 1); GM_VMCNT(kFlyA); GM_PHASE_END(0, 0, bfr[0]);
      GM_D_READ_B(0, 1); GM_D_STAGE(0, GM_B0, t + 2); GM_VMCNT(kFlyB); GM_PHASE_END(0, 1, bfr[1]);
      GM_D_READ_A(kRdA2, 0, 1); GM_D_STAGE(0, GM_A0, t + 2); GM_VMCNT(kFlyA); GM_PHASE_END(1, 1, bfr[1]);
      GM_D_READ_B0(1, b0y); GM_D_STAGE(0, GM_B1, t + 2); GM_VMCNT(kFlyB); GM_PHASE_END(1, 0, bfr[0]);
      GM_D_READ_A(kRdA, 1, 0); GM_D_STAGE(0, GM_A1, t + 2); GM_VMCNT(kFlyA); GM_PHASE_END(0, 0, b0y);
      GM_D_READ_B(1, 1); GM_D_STAGE(1, GM_B0, t + 3); GM_VMCNT(kFlyB); GM_PHASE_END(0, 1, bfr[1]);
      GM_D_READ_A(kRdA2, 1, 1); GM_D_STAGE(1, GM_A0, t + 3); GM_VMCNT(kFlyA); GM_PHASE_END(1, 1, bfr[1]);
      GM_D_READ_B0(0, bfr[0]); GM_D_STAGE(1, GM_B1, t + 3); GM_VMCNT(kFlyB); GM_PHASE_END(1, 0, b0y);
    }
  }
  {                                              // ---- main loop: drain, the last two K-tiles
      GM_READ_A(0, 0); GM_STAGE(1, GM_A1, t + 1); GM_VMCNT(kFlyA); GM_PHASE_END(0, 0, bfr[0]);
      GM_READ_B(0, 1); GM_VMCNT(kDmaA + kDmaB); GM_PHASE_END(0, 1, bfr[1]);
      GM_READ_A(0, 1); GM_VMCNT(kDmaA); GM_PHASE_END(1, 1, bfr[1]);
      GM_READ_B0_INTO(1, b0y); GM_VMCNT(0); GM_PHASE_END(1, 0, bfr[0]);
      GM_READ_A(1, 0); GM_PHASE_END(0, 0, b0y);
      GM_READ_B(1, 1); GM_PHASE_END(0, 1, bfr[1]);
      GM_READ_A(1, 1); GM_PHASE_END(1, 1, bfr[1]);
      GM_PHASE_END(1, 0, b0y);
  }
  __builtin_amdgcn_s_setprio(0);
  if (wr == 0) GM_BARRIER();                       // balances the stagger's extra barrier
#undef GM_D_READ_A
#undef GM_D_READ_B
#undef GM_D_READ_B0
#undef GM_D_STAGE
#undef GM_PHASE_END
#undef GM_MFMA_WITH
#undef GM_READ_B0_INTO
#undef GM_READ_B
#undef GM_READ_B_INTO
#undef GM_READ_A
#undef GM_STAGE

  // ---- split tile: the first K-half to finish hands its accumulators over
  if (khalf >= 0 && gm_split_join(smem, acc, sp, pid - full)) return;

  // ---- FP8: the column scales of this lane's four columns, on the joined sums
  if constexpr (FP8) {
    const float* csp = cs + tn * GM_BN + wc * 64 + fr;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float s = csp[nh * 32 + n * 16];
#pragma unroll
        for (int mh = 0; mh < 2; ++mh)
#pragma unroll
          for (int m = 0; m < 4; ++m) acc[mh][m][nh][n] *= s;
      }
  }

  // ---- epilogue through LDS (the staging buffers are free after the last barrier)
  const int row0 = tm * GM_BM + wr * 128;          // first output row of this wave
  if constexpr (EPI == GM_EPI_ARGMAX || EPI == GM_EPI_SAMPLE) {
    if constexpr (EPI == GM_EPI_SAMPLE) {
      // score = acc / T + Gumbel(key[row], column) in place; the row inputs
      // of this lane's 32 rows come as whole-tile vector loads (padded
      // arrays: rows >= M read the padding, inv_temp 0, and are not stored)
      const uint32_t col = (uint32_t)(tn * GM_BN + wc * 64 + fr);
#pragma unroll
      for (int mh = 0; mh < 2; ++mh)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int r4 = row0 + mh * 64 + m * 16 + fq * 4;
          const gm_f32x4 it = *reinterpret_cast<const gm_f32x4*>(am.inv_temp + r4);
          const gm_u32x4 ka = *reinterpret_cast<const gm_u32x4*>(am.key + 2 * r4);
          const gm_u32x4 kb = *reinterpret_cast<const gm_u32x4*>(am.key + 2 * r4 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t k0 = j < 2 ? ka[2 * j] : kb[2 * j - 4];
            const uint32_t k1 = j < 2 ? ka[2 * j + 1] : kb[2 * j - 3];
            if (it[j] != 0.f) {                    // (a greedy row keeps its accumulators)
#pragma unroll
              for (int nh = 0; nh < 2; ++nh)
#pragma unroll
                for (int n = 0; n < 2; ++n)
                  acc[mh][m][nh][n][j] = acc[mh][m][nh][n][j] * it[j] + sn_gumbel(k0, k1, col + nh * 32 + n * 16);
            }
          }
        }
    }
    // per (row, wave): max over the wave's 64 columns -- 4 per lane, then the
    // 16 lanes of a row group (xor butterfly; ties keep the lower column)
    float* lv = reinterpret_cast<float*>(smem);                    // [256 rows][4 wave cols]
    int* lc = reinterpret_cast<int*>(smem + GM_BM * 4 * 4);
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[mh][m][0][0][j];
          int c = fr;
#pragma unroll
          for (int nh = 0; nh < 2; ++nh)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
              const float x = acc[mh][m][nh][n][j];
              if (x > v) { v = x; c = nh * 32 + n * 16 + fr; }
            }
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) {
            const float ov = __shfl_xor(v, off, 64);
            const int oc = __shfl_xor(c, off, 64);
            if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
          }
          if (fr == 0) {
            const int r = wr * 128 + mh * 64 + m * 16 + fq * 4 + j;
            lv[r * 4 + wc] = v;
            lc[r * 4 + wc] = wc * 64 + c;
          }
        }
    __syncthreads();
    if (tid < GM_BM) {                             // one thread per tile row: the 4 wave columns
      const int grow = tm * GM_BM + tid;
      float v = lv[tid * 4];
      int c = lc[tid * 4];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (lv[tid * 4 + k] > v) { v = lv[tid * 4 + k]; c = lc[tid * 4 + k]; }
      if (grow < M) {
        am.pv[(int64_t)grow * tiles_n + tn] = v;
        am.pi[(int64_t)grow * tiles_n + tn] = tn * GM_BN + c;
      }
    }
  } else if constexpr (EPI == GM_EPI_RESID) {
    // fp32 through LDS in four passes of 32 rows (8.5 KiB per wave, row
    // stride 68 floats: the four fq row groups of a write land on distinct
    // banks), then coalesced: 16 B of fp32 + 8 B of the bf16 residual per
    // lane, one rounding of the sum
    float* o = reinterpret_cast<float*>(smem + w * (32 * 68 * 4));
    const int col0 = tn * GM_BN + wc * 64;
    // every residual chunk of this lane loaded up front (64 VGPRs): after the
    // first store the compiler cannot move a load of C above a store to C, so
    // loads interleaved with the passes would wait out one round trip each
    uint2 cres[2][2][8];
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int mp = 0; mp < 2; ++mp)
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int qd = it * 64 + lane;
          const int grow = row0 + mh * 64 + mp * 32 + (qd >> 4);
          cres[mh][mp][it] = grow < M ? *reinterpret_cast<const uint2*>(C + (int64_t)grow * N + col0 + (qd & 15) * 4)
                                      : make_uint2(0u, 0u);
        }
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int mp = 0; mp < 2; ++mp) {
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
          for (int nh = 0; nh < 2; ++nh)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
              for (int j = 0; j < 4; ++j)
                o[(mm * 16 + fq * 4 + j) * 68 + nh * 32 + n * 16 + fr] = acc[mh][mp * 2 + mm][nh][n][j];
        GM_LGKM(0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < 8; ++it) {
          const int qd = it * 64 + lane;           // row qd/16, 4-float chunk qd%16
          const int r = qd >> 4, c4 = qd & 15;
          const int grow = row0 + mh * 64 + mp * 32 + r;
          const gm_f32x4 v = *reinterpret_cast<const gm_f32x4*>(o + r * 68 + c4 * 4);
          if (grow < M) {
            uint2* cp = reinterpret_cast<uint2*>(C + (int64_t)grow * N + col0 + c4 * 4);
            const uint2 cr = cres[mh][mp][it];
            const float r0 = __uint_as_float(cr.x << 16) + v[0], r1 = __uint_as_float(cr.x & 0xffff0000u) + v[1];
            const float r2 = __uint_as_float(cr.y << 16) + v[2], r3 = __uint_as_float(cr.y & 0xffff0000u) + v[3];
            *cp = make_uint2((uint32_t)gm_f2bf(r0) | ((uint32_t)gm_f2bf(r1) << 16),
                             (uint32_t)gm_f2bf(r2) | ((uint32_t)gm_f2bf(r3) << 16));
          }
        }
        GM_LGKM(0);
        __builtin_amdgcn_wave_barrier();
      }
  } else if constexpr (EPI == GM_EPI_RESID_LDS || EPI == GM_EPI_RESID_PRE || EPI == GM_EPI_RESID_RMS) {
    // The residual tile staged by DMA instead of through registers: the
    // wave's 128 x 64 bf16 block of C lands in its 16 KiB of LDS (16
    // buffer_load ... lds of 16 B per lane, row-major, the plain epilogue's
    // layout; rows >= M read 0 off the buffer descriptor), each lane adds its
    // fp32 accumulators in place (one rounding of the sum) and the block
    // leaves with the plain epilogue's 16-B coalesced stores.  Against the
    // four-pass fp32 staging (GM_EPI_RESID): half the global instructions
    // (16-B instead of 8-B loads and stores), no fp32 LDS round trip, one
    // wave barrier instead of eight.
    // (GM_EPI_RESID_PRE: rows 0-31 are already in the spare LDS, loaded at
    // kernel start; rows r < 32 are exactly mh = 0, m < 2 / it < 4 below)
    constexpr int kPre = EPI == GM_EPI_RESID_PRE ? 4 : 0;
    uint8_t* cw = smem + w * 16384;
    uint8_t* cpre = smem + GM_LDS_BYTES + w * 4096;
    auto rowp = [&](int r) -> uint8_t* { return (kPre && r < 32) ? cpre + r * 128 : cw + r * 128; };
    const int col0 = tn * GM_BN + wc * 64;
    const __amdgpu_buffer_rsrc_t rsc =
        __builtin_amdgcn_make_buffer_rsrc((void*)C, 0, (uint32_t)M * (uint32_t)N * 2u, 0x00020000);
#pragma unroll
    for (int i = kPre; i < 16; ++i) {              // LDS bytes [i KiB, i+1 KiB): rows 8i .. 8i+7
      const int r = i * 8 + (lane >> 3), c = lane & 7;
      const uint32_t vo = ((uint32_t)(row0 + r) * (uint32_t)N + (uint32_t)(col0 + c * 8)) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsc, (gm_lds_ptr)(cw + i * 1024), 16, vo, 0, 0, 0);
    }
    GM_VMCNT(0);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
          for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int r = mh * 64 + m * 16 + fq * 4 + j;
              uint16_t* e = reinterpret_cast<uint16_t*>(rowp(r) + (nh * 32 + n * 16 + fr) * 2);
              *e = gm_f2bf(__uint_as_float((uint32_t)*e << 16) + acc[mh][m][nh][n][j]);
            }
    GM_LGKM(0);
    __builtin_amdgcn_wave_barrier();
    constexpr bool rms = EPI == GM_EPI_RESID_RMS;   // + the RMSNorm row scales (GmSide.r*)
    float ssq[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int qd = it * 64 + lane;               // row qd/8, chunk qd%8
      const int r = qd >> 3, cb = qd & 7;
      const int grow = row0 + r;
      const gm_u32x4 v = *reinterpret_cast<const gm_u32x4*>(rowp(r) + cb * 16);
      if (grow < M) *reinterpret_cast<gm_u32x4*>(C + (int64_t)grow * N + col0 + cb * 8) = v;
      if constexpr (rms) {                         // squares of the 8 stored bf16 values
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xFFFF0000u);
          q += lo * lo + hi * hi;
        }
        ssq[it] = q;
      }
    }
    if constexpr (rms) {
      // row r = it * 8 + lane / 8 of this wave's 128: its 8 chunk lanes meet
      // by three xor-shuffles; the wave's 128 partials go to the start of its
      // own (now unused) 16 KiB of LDS, the block's 4 column waves of a row
      // half are added in wc order, written through to rpart, and the last
      // block of the row tile (ticket) finishes the scale
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        float q = ssq[it];
        q += __shfl_xor(q, 1, 64);
        q += __shfl_xor(q, 2, 64);
        q += __shfl_xor(q, 4, 64);
        ssq[it] = q;
      }
      GM_LGKM(0);
      __builtin_amdgcn_wave_barrier();
      float* wp = reinterpret_cast<float*>(cw);
      if ((lane & 7) == 0) {
#pragma unroll
        for (int it = 0; it < 16; ++it) wp[it * 8 + (lane >> 3)] = ssq[it];
      }
      __syncthreads();
      const int tiles_n_ = N / GM_BN;
      if (tid < 256) {                             // block row tid: wave row tid / 128, row tid % 128
        const int hw = tid >> 7, rr = tid & 127;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) sum += reinterpret_cast<const float*>(smem + (hw * 4 + c) * 16384)[rr];
        const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
            am.rpart + (size_t)(tm * tiles_n_ + tn) * 256, 0, 256 * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(sum), prs, tid * 4, 0, GM_CPOL_SC1);
      }
      GM_VMCNT(0);
      __syncthreads();
      if (tid == 0)
        *reinterpret_cast<int*>(smem) = __hip_atomic_fetch_add(am.rticket + tm, 1, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const int done = *reinterpret_cast<volatile int*>(smem);
      if (done == tiles_n_ - 1 && tid < 256) {     // the row tile's last block: finish its 256 scales
        float sum = 0.f;
        for (int t2 = 0; t2 < tiles_n_; ++t2) {
          const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(
              am.rpart + (size_t)(tm * tiles_n_ + t2) * 256, 0, 256 * 4, 0x00020000);
          sum += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(prs, tid * 4, 0, GM_CPOL_SC1));
        }
        am.rscale[tm * 256 + tid] = rsqrtf(sum / (float)N + am.reps);
        if (tid == 0) __hip_atomic_store(am.rticket + tm, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else if constexpr (EPI == GM_EPI_SWIGLU) {
    // wave w: 128 rows x 32 features bf16 = 8 KiB at w * 8 KiB
    uint16_t* o = reinterpret_cast<uint16_t*>(smem + w * 8192);
    gm_f32x4 sc[2][4];
    gm_load_row_scales(rs, row0, fq, sc);
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float g = acc[mh][m][0][n][j] * sc[mh][m][j];
            const float u = acc[mh][m][1][n][j] * sc[mh][m][j];
            const float s = g / (1.0f + __expf(-g));
            o[(mh * 64 + m * 16 + fq * 4 + j) * 32 + n * 16 + fr] = gm_f2bf(s * u);
          }
    GM_LGKM(0);
    __builtin_amdgcn_wave_barrier();
    const int F = N >> 1;
    const int col0 = tn * (GM_BN / 2) + wc * 32;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int qd = it * 64 + lane;               // 16-B chunk: row qd/4, chunk qd%4
      const int r = qd >> 2, cb = qd & 3;
      const int grow = row0 + r;
      const gm_u32x4 v = *reinterpret_cast<const gm_u32x4*>(smem + w * 8192 + r * 64 + cb * 16);
      if (grow < M) *reinterpret_cast<gm_u32x4*>(C + (int64_t)grow * F + col0 + cb * 8) = v;
    }
  } else {
    // wave w: 128 rows x 64 columns bf16 = 16 KiB at w * 16 KiB
    uint16_t* o = reinterpret_cast<uint16_t*>(smem + w * 16384);
    gm_f32x4 sc[2][4];
    gm_load_row_scales(rs, row0, fq, sc);
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
          for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              o[(mh * 64 + m * 16 + fq * 4 + j) * 64 + nh * 32 + n * 16 + fr] =
                  gm_f2bf(acc[mh][m][nh][n][j] * sc[mh][m][j]);
    if constexpr (EPI == GM_EPI_STORE) {
      GM_LGKM(0);
      __builtin_amdgcn_wave_barrier();
      const int col0 = tn * GM_BN + wc * 64;
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        const int qd = it * 64 + lane;               // row qd/8, chunk qd%8
        const int r = qd >> 3, cb = qd & 7;
        const int grow = row0 + r;
        const gm_u32x4 v = *reinterpret_cast<const gm_u32x4*>(smem + w * 16384 + r * 128 + cb * 16);
        if (grow < M) *reinterpret_cast<gm_u32x4*>(C + (int64_t)grow * N + col0 + cb * 8) = v;
      }
    } else {                                       // GM_EPI_ROPE
      __syncthreads();                             // the rotary partner (d + 64) is another wave's column
      // (tile row r, tile column c) -> byte offset of the bf16 element in LDS
      auto at = [&](int r, int c) -> const uint8_t* {
        return smem + ((r >> 7) * 4 + (c >> 6)) * 16384 + (r & 127) * 128 + (c & 63) * 2;
      };
      const int nq = rp.Hq / 2, nk = rp.Hkv / 2;   // 256-column tiles of q / of k heads
      // Every thread keeps one (head, 8-dim chunk) and walks rows r0 + stride*k:
      // all row metadata and rotary factors are loaded up front (independent
      // loads in flight together, not one dependent round trip per row).
      if (tn < nq + nk) {
        const int hh = (tid >> 3) & 1, j = tid & 7, r0 = tid >> 4;   // rows r0 + 32k, k < 8
        int pk[8], sk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int grow = min(tm * GM_BM + r0 + 32 * k, M - 1);
          pk[k] = rp.pos[grow];
          sk[k] = rp.slot[grow];
        }
        float4 c0[8], c1[8], s0[8], s1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int64_t o = (int64_t)min(max(pk[k], 0), rp.max_ctx - 1) * 64 + 8 * j;
          c0[k] = *reinterpret_cast<const float4*>(rp.cos_t + o);
          c1[k] = *reinterpret_cast<const float4*>(rp.cos_t + o + 4);
          s0[k] = *reinterpret_cast<const float4*>(rp.sin_t + o);
          s1[k] = *reinterpret_cast<const float4*>(rp.sin_t + o + 4);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int r = r0 + 32 * k;
          const int grow = tm * GM_BM + r;
          const int p = pk[k], sl = sk[k];
          if (grow >= M || (unsigned)sl >= (unsigned)rp.n_slots || (unsigned)p >= (unsigned)rp.max_ctx) continue;
          const gm_u32x4 lo = *reinterpret_cast<const gm_u32x4*>(at(r, hh * 128 + 8 * j));
          const gm_u32x4 hi = *reinterpret_cast<const gm_u32x4*>(at(r, hh * 128 + 64 + 8 * j));
          const float cc[8] = {c0[k].x, c0[k].y, c0[k].z, c0[k].w, c1[k].x, c1[k].y, c1[k].z, c1[k].w};
          const float ss[8] = {s0[k].x, s0[k].y, s0[k].z, s0[k].w, s1[k].x, s1[k].y, s1[k].z, s1[k].w};
          gm_u32x4 olo, ohi;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float a0 = __uint_as_float(lo[e] << 16), a1 = __uint_as_float(lo[e] & 0xffff0000u);
            const float b0 = __uint_as_float(hi[e] << 16), b1 = __uint_as_float(hi[e] & 0xffff0000u);
            const float c_0 = cc[2 * e], c_1 = cc[2 * e + 1], s_0 = ss[2 * e], s_1 = ss[2 * e + 1];
            olo[e] = (uint32_t)gm_f2bf(a0 * c_0 - b0 * s_0) | ((uint32_t)gm_f2bf(a1 * c_1 - b1 * s_1) << 16);
            ohi[e] = (uint32_t)gm_f2bf(b0 * c_0 + a0 * s_0) | ((uint32_t)gm_f2bf(b1 * c_1 + a1 * s_1) << 16);
          }
          uint16_t* dst;
          if (tn < nq) {
            dst = rp.q + (int64_t)grow * rp.Hq * 128 + (2 * tn + hh) * 128;
          } else {
            const int kvh = 2 * (tn - nq) + hh;
            dst = rp.kc + (((int64_t)sl * rp.Hkv + kvh) * rp.max_ctx + p) * 128;
          }
          *reinterpret_cast<gm_u32x4*>(dst + 8 * j) = olo;
          *reinterpret_cast<gm_u32x4*>(dst + 64 + 8 * j) = ohi;
        }
      } else {
        const int hh = (tid >> 4) & 1, cb = tid & 15, r0 = tid >> 5;  // rows r0 + 16k, k < 16
        int pk[16], sk[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int grow = min(tm * GM_BM + r0 + 16 * k, M - 1);
          pk[k] = rp.pos[grow];
          sk[k] = rp.slot[grow];
        }
        const int kvh = 2 * (tn - nq - nk) + hh;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int r = r0 + 16 * k;
          const int grow = tm * GM_BM + r;
          const int p = pk[k], sl = sk[k];
          if (grow >= M || (unsigned)sl >= (unsigned)rp.n_slots || (unsigned)p >= (unsigned)rp.max_ctx) continue;
          uint16_t* dst = rp.vc + (((int64_t)sl * rp.Hkv + kvh) * rp.max_ctx + p) * 128;
          *reinterpret_cast<gm_u32x4*>(dst + 8 * cb) = *reinterpret_cast<const gm_u32x4*>(at(r, hh * 128 + 8 * cb));
        }
      }
    }
  }
  if constexpr (kStamp) {
    const uint64_t st_t1 = __builtin_amdgcn_s_memtime(), st_r1 = __builtin_amdgcn_s_memrealtime();
    if (tid == 0 && am.pv != nullptr) {
      uint64_t* dbg = reinterpret_cast<uint64_t*>(am.pv) + (size_t)bid * 4;
      dbg[0] = st_t0;
      dbg[1] = st_t1;
      dbg[2] = st_r0;
      dbg[3] = st_r1;
    }
  }
}

// DIAG != GM_DIAG_NONE only from bench/gemm_energy_diag.hip
template <int EPI, int DIAG = GM_DIAG_NONE>
__global__ __launch_bounds__(GM_THREADS) void gemm_bf16_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ W, uint16_t* __restrict__ C,
    int M, int N, int K, int group_m, const float* __restrict__ rs, const GmRope rp, const GmSplit sp,
    const GmSide am) {
  extern __shared__ __align__(16) uint8_t smem[];
  gemm_tile<EPI, DIAG>(smem, A, W, nullptr, C, M, N, K, group_m, rs, rp, sp, am, (int)blockIdx.x);
}

// The tile over FP8 weights (the file header): EPI in GM_EPI_STORE /
// GM_EPI_SWIGLU / GM_EPI_RESID_LDS; Wq [N][K] e4m3 codes, cs [N] their scales
template <int EPI>
__global__ __launch_bounds__(GM_THREADS) void gemm_fp8w_kernel(
    const uint16_t* __restrict__ A, const uint8_t* __restrict__ Wq, const float* __restrict__ cs,
    uint16_t* __restrict__ C, int M, int N, int K, int group_m, const float* __restrict__ rs, const GmSplit sp) {
  extern __shared__ __align__(16) uint8_t smem[];
  gemm_tile<EPI, GM_DIAG_NONE, true>(smem, A, Wq, cs, C, M, N, K, group_m, rs, GmRope{}, sp, GmSide{},
                                     (int)blockIdx.x);
}

// out[row] = column of the first maximum over the tiles' partials (one wave per row)
__global__ __launch_bounds__(256) void gemm_argmax_reduce_kernel(const float* __restrict__ pv,
                                                                 const int32_t* __restrict__ pi, int M, int tiles,
                                                                 int32_t* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  float v = -__builtin_inff();
  int c = 0x7fffffff;
  for (int t = lane; t < tiles; t += 64) {         // ascending tiles: a later equal value never wins
    const float x = pv[(int64_t)row * tiles + t];
    if (x > v) { v = x; c = pi[(int64_t)row * tiles + t]; }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oc = __shfl_xor(c, off, 64);
    if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
  }
  if (lane == 0) out[row] = c == 0x7fffffff ? 0 : c;   // all-NaN row: token 0
}

// out[k][i] = the noise bits of column n0 + i under key k (sample_noise.h):
// lets a test compare the device generator with the numpy twin directly
__global__ __launch_bounds__(256) void sample_bits_kernel(const uint32_t* __restrict__ keys, uint32_t n0, int count,
                                                          uint32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (i < count) out[(int64_t)k * count + i] = sn_bits(keys[2 * k], keys[2 * k + 1], n0 + (uint32_t)i);
}

#undef GM_LGKM
#undef GM_VMCNT
#undef GM_BARRIER
#undef GM_FENCE

}  // namespace llmq
