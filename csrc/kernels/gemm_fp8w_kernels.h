// The 256x256-tile GEMM of gemm_kernels.h over FP8 weights (W8A16):
// C (+)= (A · decode(Wq)ᵀ) * cs[n] * rs[m] with A [M][K] bf16, Wq [N][K] uint8
// e4m3fn codes (K-contiguous, the tensor the skinny FP8 kernel reads) and one
// fp32 scale a weight row, cs [N] (ops/quant.py holds the contract).  For the
// micro-forwards that carry prefill (more than 64 rows), where the skinny
// kernel's 128-row chunks re-read and re-decode their weights a chunk.
//
// gemm_fp8w_kernel<EPI>, EPI in GM_EPI_STORE / GM_EPI_SWIGLU /
// GM_EPI_RESID_LDS (host entry point gemm_fp8w in hipops.hip).  A sibling of
// gemm_tile, not a parameter of it: the bf16 kernels' instructions stay what
// they were (docs/development.md, "two-tree comparison").
//
// Same as gemm_bf16_kernel: the 256x256 tile, BK = 64, 8 waves as 2 (M) x 4
// (N), the A half-tiles (image, swizzle, two DMAs a lane), gm_tile_coords,
// gm_split_join, the 8-phase loop with its wave-row stagger, stage order B0,
// A0, B1, A1 three half-tiles ahead, and the three epilogues.  Every k enters
// the MFMA step (K-tile, kk) and operand slot (lane fq, element) it enters
// there, so with power-of-two scales the result is bit-equal to
// gemm_bf16_kernel over the decoded weights.
//
// What differs:
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
//   * Counted waits.  A stage is 2 DMAs (A) or 1 (B), and every phase must
//     leave exactly the last three staged half-tiles in flight:
//         stage of the phase   in flight after it     s_waitcnt
//         A0 or A1             A, B, A  (2 + 1 + 2)   vmcnt(5)
//         B0 or B1             B, A, B  (1 + 2 + 1)   vmcnt(4)
//         prologue (7 halves)  B1, A0, B0 of buffer 1 vmcnt(4)
//         drain phases 1-4     A1 B1 A0 / A1 B1 / A1 / -   5, 3, 2, 0
//   * The column scale multiplies the fp32 accumulators after the split-K
//     join, before the row scale and any epilogue math: a lane owns columns
//     tn * 256 + wc * 64 + nh * 32 + n * 16 + fr (under SwiGLU gate and up of
//     a feature carry different scales; cs follows the permuted row order).
#pragma once

#include "gemm_kernels.h"
#include "skinny_kernels.h"

namespace llmq {

constexpr int GF_BHALF_BYTES = 128 * GM_BK;                              // 8 KiB
constexpr int GF_BUF_BYTES = 2 * GM_HALF_BYTES + 2 * GF_BHALF_BYTES;     // A0 A1 B0 B1: 48 KiB
constexpr int GF_B_BASE = 2 * GM_HALF_BYTES;                             // B0 inside a buffer
static_assert(2 * GF_BUF_BYTES <= GM_LDS_BYTES, "operand buffers inside the launch's LDS");

#define GF_LGKM(N) asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory")
#define GF_VMCNT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
#define GF_FENCE() __builtin_amdgcn_sched_barrier(0)
#define GF_BARRIER()                  \
  do {                                \
    GF_FENCE();                       \
    __builtin_amdgcn_s_barrier();     \
    GF_FENCE();                       \
  } while (0)

// One 8-byte LDS read that stays a ds_read_b64.  Left to the compiler, the
// n = 0 / n = 1 fragments (1 KiB apart) pair into ds_read2st64_b64, which
// takes twice the LDS cycles and banks by 16-lane groups modulo 32 (a 2-way
// conflict on this image).  The compiler does not count this read in lgkmcnt:
// GF_PHASE_END waits lgkmcnt(0) and fences before the first use.
typedef __attribute__((ext_vector_type(2))) unsigned int gf_u32x2;
template <int OFF>
__device__ __forceinline__ gf_u32x2 gf_lds_read_b64(uint32_t addr) {
  gf_u32x2 r;
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
  return r;
}

template <int EPI>
__device__ __forceinline__ void gemm_fp8w_tile(
    uint8_t* __restrict__ smem, const uint16_t* __restrict__ A, const uint8_t* __restrict__ Wq,
    const float* __restrict__ cs, uint16_t* __restrict__ C, int M, int N, int K, int group_m,
    const float* __restrict__ rs, const GmSplit& sp, const int bid) {
  static_assert(EPI == GM_EPI_STORE || EPI == GM_EPI_SWIGLU || EPI == GM_EPI_RESID_LDS, "epilogue");
  const int tiles_m = (M + GM_BM - 1) / GM_BM;
  const int tiles_n = N / GM_BN;
  const int nwg = tiles_m * tiles_n;
  const int full = sp.ws ? sp.full : nwg;          // tiles [full, nwg) run split-K
  const GmTile tile = gm_tile_coords(bid, tiles_m, tiles_n, nwg, full, group_m);
  const int pid = tile.pid, khalf = tile.khalf, tm = tile.tm, tn = tile.tn;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;

  // ---- staging sources.  A: as gemm_tile (half h, instruction i -> LDS row
  // i*64 + w*8 + lane/8).  B: half h -> LDS row w*16 + lane/4, slot lane%4
  const int srow = w * 8 + (lane >> 3);
  const int schunk = (lane & 7) ^ ((srow >> 1) & 7);
  const int brow = w * 16 + (lane >> 2);           // 0..127
  const int bchunk = (lane & 3) ^ ((brow >> 2) & 3);   // source chunk for LDS slot lane&3
  const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc((void*)A, 0, M * K * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)Wq, 0, N * K, 0x00020000);
  uint32_t va[2][2], vb[2];                        // byte offsets (row, chunk) of K-tile 0
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int row = tm * GM_BM + i * 128 + h * 64 + srow;
      row = row < M ? row : M - 1;
      va[h][i] = (uint32_t)row * (uint32_t)K * 2u + (uint32_t)schunk * 16u;
    }
    const int col = tn * GM_BN + (brow >> 5) * 64 + h * 32 + (brow & 31);
    vb[h] = (uint32_t)col * (uint32_t)K + (uint32_t)bchunk * 16u;
  }
  // LDS destinations (wave-uniform) inside a half-tile
  const uint32_t dst_i0 = (uint32_t)(w * 8) * 128u;
  const uint32_t dst_i1 = (uint32_t)(64 + w * 8) * 128u;
  const uint32_t dst_b = (uint32_t)(w * 16) * 64u;

  // ---- fragment read offsets (bytes inside buffer 0), per k-step kk
  const uint32_t sbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem;   // LDS address
  const int fr = lane & 15, fq = lane >> 4;
  uint32_t aoff[2][2], boff[2][2];                 // [buffer][kk]
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int c = fq + 4 * kk;                     // 8 k of the K-tile: 16 B of A, 8 B of B
    aoff[0][kk] = (uint32_t)(wr * 64 + fr) * 128u + (uint32_t)((c ^ ((fr >> 1) & 7)) * 16);
    boff[0][kk] = (uint32_t)GF_B_BASE + (uint32_t)(wc * 32 + fr) * 64u +
                  (uint32_t)(((c >> 1) ^ ((fr >> 2) & 3)) * 16 + (c & 1) * 8);
    aoff[1][kk] = aoff[0][kk] + GF_BUF_BYTES;
    boff[1][kk] = boff[0][kk] + GF_BUF_BYTES;
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
  gf_u32x2 bfr[2][2][2];                             // both n-halves, codes: [nh][n][kk]
  gf_u32x2 b0y[2][2];                              // buffer 1's B0 fragments ([nh = 0] of bfr: buffer 0's)
  const int nt = khalf < 0 ? K / GM_BK : K / GM_BK / 2;
  const int kt0 = khalf > 0 ? nt : 0;

#define GF_STAGE_A(BUF, H, KT)                                                                 \
  do {                                                                                         \
    const uint32_t _b = (uint32_t)(BUF) * GF_BUF_BYTES + (uint32_t)(H) * GM_HALF_BYTES;        \
    gm_stage(rsa, va[(H)][0], va[(H)][1], (uint32_t)((KT) + kt0) * (GM_BK * 2), smem, _b + dst_i0, _b + dst_i1); \
  } while (0)

#define GF_STAGE_B(BUF, H, KT)                                                                 \
  __builtin_amdgcn_raw_ptr_buffer_load_lds(                                                    \
      rsw, (gm_lds_ptr)(smem + (uint32_t)(BUF) * GF_BUF_BYTES + GF_B_BASE + (uint32_t)(H) * GF_BHALF_BYTES + dst_b), \
      16, vb[(H)], (uint32_t)((KT) + kt0) * GM_BK, 0, 0)

#define GF_READ_A(BUF, MH)                                                                     \
  do {                                                                                         \
    _Pragma("unroll") for (int m = 0; m < 4; ++m)                                              \
      _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                         \
        af[m][kk] = *reinterpret_cast<const gm_bf16x8*>(smem + aoff[BUF][kk] + (MH) * GM_HALF_BYTES + m * 2048); \
  } while (0)

// the B fragments of n-half NH of buffer BUF (16 rows = 1 KiB apart) into DST[n][kk]
#define GF_READ_B_INTO(BUF, NH, DST)                                                           \
  do {                                                                                         \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                         \
      DST[0][kk] = gf_lds_read_b64<(NH) * GF_BHALF_BYTES>(sbase + boff[BUF][kk]);              \
      DST[1][kk] = gf_lds_read_b64<(NH) * GF_BHALF_BYTES + 1024>(sbase + boff[BUF][kk]);       \
    }                                                                                          \
  } while (0)

#define GF_PHASE_END(MH, NH, BREG)                                                             \
  do {                                                                                         \
    GF_BARRIER();                                                                              \
    GF_LGKM(0);                                                                                \
    GF_FENCE();                                                                                \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                         \
      const gm_bf16x8 _b0 = sk_fp8x8_bf16(BREG[0][kk].x, BREG[0][kk].y);                       \
      const gm_bf16x8 _b1 = sk_fp8x8_bf16(BREG[1][kk].x, BREG[1][kk].y);                       \
      _Pragma("unroll") for (int m = 0; m < 4; ++m) {                                          \
        acc[MH][m][NH][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m][kk], _b0, acc[MH][m][NH][0], 0, 0, 0); \
        acc[MH][m][NH][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m][kk], _b1, acc[MH][m][NH][1], 0, 0, 0); \
      }                                                                                        \
    }                                                                                          \
    GF_BARRIER();                                                                              \
  } while (0)

  // ---- main loop: prologue (the schedule of gemm_tile; the waits: header)
  if (wr == 1) __builtin_amdgcn_s_setprio(1);
  GF_STAGE_B(0, 0, 0);
  GF_STAGE_A(0, 0, 0);
  GF_STAGE_B(0, 1, 0);
  GF_STAGE_A(0, 1, 0);
  GF_STAGE_B(1, 0, 1);
  GF_STAGE_A(1, 0, 1);
  GF_STAGE_B(1, 1, 1);
  GF_VMCNT(4);
  GF_BARRIER();
  GF_READ_B_INTO(0, 0, bfr[0]);
  if (wr == 1) GF_BARRIER();                       // wave row 1 half a phase behind (balanced below)

  // ---- main loop: steady state, two K-tiles = eight phases per trip
  int t = 0;
  for (; t < nt - 2; t += 2) {
    GF_READ_A(0, 0); GF_STAGE_A(1, 1, t + 1); GF_VMCNT(5); GF_PHASE_END(0, 0, bfr[0]);
    GF_READ_B_INTO(0, 1, bfr[1]); GF_STAGE_B(0, 0, t + 2); GF_VMCNT(4); GF_PHASE_END(0, 1, bfr[1]);
    GF_READ_A(0, 1); GF_STAGE_A(0, 0, t + 2); GF_VMCNT(5); GF_PHASE_END(1, 1, bfr[1]);
    GF_READ_B_INTO(1, 0, b0y); GF_STAGE_B(0, 1, t + 2); GF_VMCNT(4); GF_PHASE_END(1, 0, bfr[0]);
    GF_READ_A(1, 0); GF_STAGE_A(0, 1, t + 2); GF_VMCNT(5); GF_PHASE_END(0, 0, b0y);
    GF_READ_B_INTO(1, 1, bfr[1]); GF_STAGE_B(1, 0, t + 3); GF_VMCNT(4); GF_PHASE_END(0, 1, bfr[1]);
    GF_READ_A(1, 1); GF_STAGE_A(1, 0, t + 3); GF_VMCNT(5); GF_PHASE_END(1, 1, bfr[1]);
    GF_READ_B_INTO(0, 0, bfr[0]); GF_STAGE_B(1, 1, t + 3); GF_VMCNT(4); GF_PHASE_END(1, 0, b0y);
  }
  {                                                // ---- main loop: drain, the last two K-tiles
    GF_READ_A(0, 0); GF_STAGE_A(1, 1, t + 1); GF_VMCNT(5); GF_PHASE_END(0, 0, bfr[0]);
    GF_READ_B_INTO(0, 1, bfr[1]); GF_VMCNT(3); GF_PHASE_END(0, 1, bfr[1]);
    GF_READ_A(0, 1); GF_VMCNT(2); GF_PHASE_END(1, 1, bfr[1]);
    GF_READ_B_INTO(1, 0, b0y); GF_VMCNT(0); GF_PHASE_END(1, 0, bfr[0]);
    GF_READ_A(1, 0); GF_PHASE_END(0, 0, b0y);
    GF_READ_B_INTO(1, 1, bfr[1]); GF_PHASE_END(0, 1, bfr[1]);
    GF_READ_A(1, 1); GF_PHASE_END(1, 1, bfr[1]);
    GF_PHASE_END(1, 0, b0y);
  }
  __builtin_amdgcn_s_setprio(0);
  if (wr == 0) GF_BARRIER();                       // balances the stagger's extra barrier
#undef GF_PHASE_END
#undef GF_READ_B_INTO
#undef GF_READ_A
#undef GF_STAGE_B
#undef GF_STAGE_A

  // ---- split tile: the first K-half to finish hands its accumulators over
  if (khalf >= 0 && gm_split_join(smem, acc, sp, pid - full)) return;

  // ---- the column scales of this lane's four columns, on the joined sums
  {
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

  // ---- epilogue through LDS: gemm_tile's, for the three forms
  const int row0 = tm * GM_BM + wr * 128;          // first output row of this wave
  if constexpr (EPI == GM_EPI_RESID_LDS) {
    uint8_t* cw = smem + w * 16384;
    const int col0 = tn * GM_BN + wc * 64;
    const __amdgpu_buffer_rsrc_t rsc =
        __builtin_amdgcn_make_buffer_rsrc((void*)C, 0, (uint32_t)M * (uint32_t)N * 2u, 0x00020000);
#pragma unroll
    for (int i = 0; i < 16; ++i) {                 // LDS bytes [i KiB, i+1 KiB): rows 8i .. 8i+7
      const int r = i * 8 + (lane >> 3), c = lane & 7;
      const uint32_t vo = ((uint32_t)(row0 + r) * (uint32_t)N + (uint32_t)(col0 + c * 8)) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsc, (gm_lds_ptr)(cw + i * 1024), 16, vo, 0, 0, 0);
    }
    GF_VMCNT(0);
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
              uint16_t* e = reinterpret_cast<uint16_t*>(cw + r * 128 + (nh * 32 + n * 16 + fr) * 2);
              *e = gm_f2bf(__uint_as_float((uint32_t)*e << 16) + acc[mh][m][nh][n][j]);
            }
    GF_LGKM(0);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int qd = it * 64 + lane;               // row qd/8, chunk qd%8
      const int r = qd >> 3, cb = qd & 7;
      const int grow = row0 + r;
      const gm_u32x4 v = *reinterpret_cast<const gm_u32x4*>(cw + r * 128 + cb * 16);
      if (grow < M) *reinterpret_cast<gm_u32x4*>(C + (int64_t)grow * N + col0 + cb * 8) = v;
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
    GF_LGKM(0);
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
    GF_LGKM(0);
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
  }
}

template <int EPI>
__global__ __launch_bounds__(GM_THREADS) void gemm_fp8w_kernel(
    const uint16_t* __restrict__ A, const uint8_t* __restrict__ Wq, const float* __restrict__ cs,
    uint16_t* __restrict__ C, int M, int N, int K, int group_m, const float* __restrict__ rs, const GmSplit sp) {
  extern __shared__ __align__(16) uint8_t smem[];
  gemm_fp8w_tile<EPI>(smem, A, Wq, cs, C, M, N, K, group_m, rs, sp, (int)blockIdx.x);
}

#undef GF_LGKM
#undef GF_VMCNT
#undef GF_BARRIER
#undef GF_FENCE

}  // namespace llmq
