// Skinny GEMMs for small steps (M <= 64 rows, up to 1024 in 128-row chunks):
// C = A[M][K] . W[N][K]^T with the realtime micro-forwards' epilogues (store,
// residual add, SwiGLU over the permuted gate/up weight, optional per-row
// RMSNorm scale).  One partial kernel, two weight formats: bf16, or FP8 (e4m3)
// codes with one fp32 scale a weight row (W8A16; ops/quant.py holds the
// contract); A is bf16 in both.
//
// Why a second GEMM: at M <= 64 the 256x256-tile kernel (gemm_kernels.h)
// computes 4x the useful MFMA work per tile and a 16-tile N = 4096 product
// leaves most CUs of even a 32-CU partition idle, so a micro-forward ran at
// ~0.42 TB/s of weight traffic (profiles/r6_realtime_modes.md).  A small step
// is a stream over the weights: this kernel reads every weight byte once in
// contiguous runs, keeps a chunk's whole M in one block (MT 16-row MFMA
// fragments), keeps 256 bytes a lane a fragment of weight loads in flight
// behind the step it computes, and splits K when the column blocks alone
// cannot fill the CUs.
//
// Layout.  A block = 4 waves = 128 output columns x a K range; wave w owns
// columns [32w, 32w + 32) as two 16-column fragments.  K is walked 128 at a
// time in a PERMUTED order: MFMA step s4 of lane (fr, fq) takes the K chunk
// (fq * 4 + s4) * 8 for BOTH operands, so each lane's weight read for the
// 128-deep step is one contiguous run of 32 elements and the sum over K is
// unchanged (the same permutation on both sides).  A[0:M][k:k+128] is staged
// in LDS (double buffered, rows padded by 16 B) and read as MFMA A fragments;
// the weight fragments come straight from global memory into a ring of
// register stages (SkW):
//   bf16: 64-byte runs (256 B a weight row per four lanes), three stages of
//         4 x 16 B, two steps of loads behind the one computed: 96 registers;
//   fp8:  32-byte runs (a weight row's 128 bytes = one cache line per four
//         lanes), half the bf16 ones, so five stages of 2 x 16 B, four steps
//         behind: the same 256 bytes in flight in 80 registers.  The codes
//         are decoded to bf16 in registers right before the bf16 MFMA (every
//         finite code is exactly a bf16 number), so the arithmetic is the
//         bf16 kernel's on the decoded weights and the row's scale waits for
//         the finalize kernel.
//
// Split-K partials are written to ws[S][M][N] fp32 and summed in split
// order by the finalize kernel (deterministic: no atomics), which applies
// the column scale (fp8), the row scale and the epilogue and writes bf16.
//
// The end of the file is the quantiser that makes the codes and the decode
// the tests use.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fp8_decode.h"   // sk_fp8x8_bf16, sk_bf16x8, sk_u32x4

namespace llmq {

typedef __attribute__((ext_vector_type(4))) float sk_f32x4;

constexpr int SK_NB = 128;          // output columns per block
constexpr int SK_KS = 128;          // K per pipeline step
constexpr int SK_LDA = SK_KS + 8;   // LDS row stride of the A tile (elements)

enum { SK_EPI_STORE = 0, SK_EPI_RESID = 1, SK_EPI_SWIGLU = 2 };

// M > 64 (up to SK_MAX_M): blockIdx.x also selects one of nm 128-row chunks
// of A (MT = 8; a chunk's A rows staged in two 64-row groups).  Every chunk re-reads its column block's weights, so the nm
// chunks of a column block run on one XCD back to back (block b -> XCD b % 8:
// chunk fastest within the XCD's share) and the repeats come from its L2.
constexpr int SK_MAX_M = 1024;           // up to 8 chunks (o / down at mid-size steps)

// The weight format of skinny_partial_kernel: the element type, the register
// stages ST of the ring and the 16-byte loads NV of a stage (a lane's run of a
// 128-deep step), for two fragments.  ST * NV * 16 = 256 bytes (the header).
template <bool FP8>
struct SkW {
  using elem = std::conditional_t<FP8, uint8_t, uint16_t>;
  static constexpr int ST = FP8 ? 5 : 3;
  static constexpr int NV = FP8 ? 2 : 4;
};

template <int MT, bool FP8>
__global__ void __launch_bounds__(256)
skinny_partial_kernel(const uint16_t* __restrict__ A, const typename SkW<FP8>::elem* __restrict__ W,
                      float* __restrict__ ws, int M, int N, int K, int kc, int nm) {
  using elem = typename SkW<FP8>::elem;
  constexpr int ST = SkW<FP8>::ST, NV = SkW<FP8>::NV;
  __shared__ __align__(16) uint16_t As[2][MT * 16][SK_LDA];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int ncb = N / SK_NB;
  int cb = blockIdx.x, mc = 0;
  if (nm > 1) {
    if ((ncb & 7) == 0) {
      const int b = blockIdx.x, idx = b >> 3;
      cb = (idx / nm) * 8 + (b & 7);
      mc = idx % nm;
    } else {
      cb = blockIdx.x / nm;
      mc = blockIdx.x % nm;
    }
  }
  const int m0 = mc * (MT * 16);
  const int Ml = min(M - m0, MT * 16);             // rows of this chunk
  const int n0 = cb * SK_NB + w * 32;
  const int kb = blockIdx.y * kc;
  const int nsteps = kc / SK_KS;
  // weight rows of this lane's two fragments; K offset of its 32-element run
  const elem* wp0 = W + (size_t)(n0 + fr) * K + kb + fq * 32;
  const elem* wp1 = wp0 + (size_t)16 * K;
  // A staging: thread t -> row g * 64 + t / 4 of each 64-row group g,
  // chunks (t % 4) * 4 .. + 3 (16 B each)
  constexpr int RG = (MT * 16 + 63) / 64;
  const int arow = tid >> 2, acb = (tid & 3) * 4;
  bool a_on[RG], a_live[RG];
  const uint16_t* ap[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int r = g * 64 + arow;
    a_on[g] = r < MT * 16;
    a_live[g] = a_on[g] && r < Ml;
    ap[g] = A + (size_t)(m0 + (a_live[g] ? r : 0)) * K + kb + acb * 8;
  }

  sk_f32x4 acc[MT][2];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc[m][0] = sk_f32x4{0.f, 0.f, 0.f, 0.f};
    acc[m][1] = sk_f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // weight fragments in a ring of ST register stages: step k computes from
  // stage k % ST while steps k + 1 .. k + ST - 1 are in flight (256 B a lane
  // a fragment: enough bytes outstanding per CU to stream the weights at the
  // partition's bandwidth); the stage index is compile-time below
  sk_u32x4 wb[ST][2][NV];
  sk_u32x4 ab[RG][4];
  auto load_w = [&](auto stc, int step) {
    constexpr int S = decltype(stc)::value, EV = 16 / sizeof(elem);   // elements a 16-byte load
    const int ko = step * SK_KS;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      wb[S][0][i] = *reinterpret_cast<const sk_u32x4*>(wp0 + ko + EV * i);
      wb[S][1][i] = *reinterpret_cast<const sk_u32x4*>(wp1 + ko + EV * i);
    }
  };
  auto load_a = [&](int step) {
    const int ko = step * SK_KS;
#pragma unroll
    for (int g = 0; g < RG; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        ab[g][i] = a_live[g] ? *reinterpret_cast<const sk_u32x4*>(ap[g] + ko + 8 * i) : sk_u32x4{0u, 0u, 0u, 0u};
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int g = 0; g < RG; ++g) {
      if (a_on[g]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<sk_u32x4*>(&As[buf][g * 64 + arow][(acb + i) * 8]) = ab[g][i];
      }
    }
  };
  // one 128-deep step from register stage CUR (= step % ST) and A buffer
  // step % 2; the weights of step + ST - 1 and the A tile of step + 1 load
  // meanwhile
  auto run_step = [&](auto curc, int step) {
    constexpr int CUR = decltype(curc)::value;
    if (step + ST - 1 < nsteps) load_w(std::integral_constant<int, (CUR + ST - 1) % ST>{}, step + ST - 1);
    const bool more = step + 1 < nsteps;
    if (more) load_a(step + 1);
    const int abuf = step & 1;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      sk_bf16x8 b0, b1;
      if constexpr (FP8) {   // K chunk s4 of the run: bytes 8 s4 .. 8 s4 + 7
        b0 = sk_fp8x8_bf16(wb[CUR][0][s4 >> 1][(s4 & 1) * 2], wb[CUR][0][s4 >> 1][(s4 & 1) * 2 + 1]);
        b1 = sk_fp8x8_bf16(wb[CUR][1][s4 >> 1][(s4 & 1) * 2], wb[CUR][1][s4 >> 1][(s4 & 1) * 2 + 1]);
      } else {
        b0 = __builtin_bit_cast(sk_bf16x8, wb[CUR][0][s4]);
        b1 = __builtin_bit_cast(sk_bf16x8, wb[CUR][1][s4]);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const sk_bf16x8 a = *reinterpret_cast<const sk_bf16x8*>(&As[abuf][m * 16 + fr][(fq * 4 + s4) * 8]);
        acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[m][1], 0, 0, 0);
      }
    }
    if (more) store_a(abuf ^ 1);
    __syncthreads();
  };

  load_a(0);
  load_w(std::integral_constant<int, 0>{}, 0);
  if (nsteps > 1) load_w(std::integral_constant<int, 1>{}, 1);
  if constexpr (ST > 3) {
    if (nsteps > 2) load_w(std::integral_constant<int, 2>{}, 2);
    if (nsteps > 3) load_w(std::integral_constant<int, 3>{}, 3);
  }
  store_a(0);
  __syncthreads();
  // (written out, not folded over the stages: a generic unroll changed the
  // instructions of every instantiation -- profiles/skinny_merge.md)
  for (int step = 0; step < nsteps; step += ST) {
    run_step(std::integral_constant<int, 0>{}, step);
    if (step + 1 < nsteps) run_step(std::integral_constant<int, 1>{}, step + 1);
    if (step + 2 < nsteps) run_step(std::integral_constant<int, 2>{}, step + 2);
    if constexpr (ST > 3) {
      if (step + 3 < nsteps) run_step(std::integral_constant<int, 3>{}, step + 3);
      if (step + 4 < nsteps) run_step(std::integral_constant<int, 4>{}, step + 4);
    }
  }
  // partials: lane -> column n0 + j * 16 + fr, rows m * 16 + fq * 4 + e
  float* out = ws + (size_t)blockIdx.y * M * N;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = m * 16 + fq * 4 + e;
        if (row < Ml) out[(size_t)(m0 + row) * N + n0 + j * 16 + fr] = acc[m][j][e];
      }
}

__device__ __forceinline__ uint16_t sk_f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// One thread = 4 consecutive output columns of one row: the S split partials
// summed in split order, times the row scale, then the epilogue.
//   STORE:  C[row][c]  = sum                          (C: [M][N])
//   RESID:  C[row][c] += sum, one bf16 rounding       (C: [M][N])
//   SWIGLU: C[row][f]  = silu(g) * u over the swiglu-permuted columns of W
//           (gate f at 256 t + 64 wc + c, up 32 columns later; C: [M][N / 2])
//
// COLS (the fp8-weight GEMM): the sum of column n is first multiplied by
// cs[n], the fp32 dequantisation scale of weight row n -- under SWIGLU the
// gate and the up column each by its own entry (cs is indexed like the
// permuted weight's rows).  The bf16 kernel instantiates COLS = false only.
template <int EPI, bool COLS>
__device__ __forceinline__ void sk_finalize(const float* __restrict__ ws, int S, int M, int N,
                                            const float* __restrict__ rs, const float* __restrict__ cs,
                                            uint16_t* __restrict__ C) {
  const int Nout = EPI == SK_EPI_SWIGLU ? N / 2 : N;
  const int per_row = Nout / 4;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= M * per_row) return;
  const int row = gid / per_row, c4 = (gid % per_row) * 4;
  const float scale = rs ? rs[row] : 1.f;
  if constexpr (EPI == SK_EPI_SWIGLU) {
    const int t = c4 / 128, wc = (c4 % 128) / 32, c = c4 % 32;
    const int gcol = t * 256 + wc * 64 + c;
    sk_f32x4 g = sk_f32x4{0.f, 0.f, 0.f, 0.f}, u = g;
    for (int s = 0; s < S; ++s) {
      const float* p = ws + ((size_t)s * M + row) * N;
      g += *reinterpret_cast<const sk_f32x4*>(p + gcol);
      u += *reinterpret_cast<const sk_f32x4*>(p + gcol + 32);
    }
    if constexpr (COLS) {
      g *= *reinterpret_cast<const sk_f32x4*>(cs + gcol);
      u *= *reinterpret_cast<const sk_f32x4*>(cs + gcol + 32);
    }
    uint16_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float ge = g[e] * scale, ue = u[e] * scale;
      o[e] = sk_f2bf(ge / (1.f + __expf(-ge)) * ue);
    }
    *reinterpret_cast<uint2*>(C + (size_t)row * Nout + c4) =
        make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
  } else {
    sk_f32x4 v = sk_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) v += *reinterpret_cast<const sk_f32x4*>(ws + ((size_t)s * M + row) * N + c4);
    if constexpr (COLS) v *= *reinterpret_cast<const sk_f32x4*>(cs + c4);
    uint2* cp = reinterpret_cast<uint2*>(C + (size_t)row * N + c4);
    float r[4] = {v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale};
    if constexpr (EPI == SK_EPI_RESID) {
      const uint2 cr = *cp;
      r[0] += __uint_as_float(cr.x << 16);
      r[1] += __uint_as_float(cr.x & 0xffff0000u);
      r[2] += __uint_as_float(cr.y << 16);
      r[3] += __uint_as_float(cr.y & 0xffff0000u);
    }
    *cp = make_uint2((uint32_t)sk_f2bf(r[0]) | ((uint32_t)sk_f2bf(r[1]) << 16),
                     (uint32_t)sk_f2bf(r[2]) | ((uint32_t)sk_f2bf(r[3]) << 16));
  }
}

template <int EPI>
__global__ void __launch_bounds__(256)
skinny_finalize_kernel(const float* __restrict__ ws, int S, int M, int N, const float* __restrict__ rs,
                       uint16_t* __restrict__ C) {
  sk_finalize<EPI, false>(ws, S, M, N, rs, nullptr, C);
}

template <int EPI>
__global__ void __launch_bounds__(256)
skinny_finalize_cs_kernel(const float* __restrict__ ws, int S, int M, int N, const float* __restrict__ rs,
                          const float* __restrict__ cs, uint16_t* __restrict__ C) {
  sk_finalize<EPI, true>(ws, S, M, N, rs, cs, C);
}

// out[i] = bf16 bits of the code in byte i % 4 of in[i / 4]: the GEMM's decode, for tests
__global__ void __launch_bounds__(256) fp8_decode_kernel(const uint32_t* __restrict__ in, int n,
                                                         uint16_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t w = in[i >> 2];
  const uint32_t p = (i & 2) ? sk_fp8x2_bf16<true>(w) : sk_fp8x2_bf16<false>(w);
  out[i] = (uint16_t)((i & 1) ? p >> 16 : p);
}

// Rows of bf16 weights -> e4m3 codes + one power-of-two scale a row, bit for
// bit ops/quant.py's quantize_rows_e4m3: one block a row; absmax over the
// bf16 magnitudes (as integers), scale 2^e = the smallest power of two with
// absmax / 2^e <= 448 (e >= -126; an all-zero row: scale 1, codes 0), then
// round-to-nearest-even of w / 2^e to e4m3 -- the normal range by rounding
// the fp32 mantissa to 3 bits, below 2^-6 by the fp32 add of 2^14 (whose ulp
// is the subnormal step 2^-9).  |w / 2^e| <= 448 by construction: no NaN code.
__device__ __forceinline__ uint32_t sk_e4m3_rne(float x) {
  const uint32_t b = __float_as_uint(x), sign = (b >> 24) & 0x80u;
  uint32_t u = b & 0x7fffffffu;
  if (u >= 0x3c800000u) {                            // >= 2^-6: normal in e4m3
    u += 0x7ffffu + ((u >> 20) & 1u);
    return sign | ((u >> 20) - (120u << 3));
  }
  const float f = __uint_as_float(u) + 16384.f;      // 2^14: the add rounds to multiples of 2^-9
  return sign | (__float_as_uint(f) - 0x46800000u);
}

__global__ void __launch_bounds__(256)
quant_rows_e4m3_kernel(const uint16_t* __restrict__ W, int K, uint8_t* __restrict__ codes, float* __restrict__ scale) {
  __shared__ uint32_t red[4];
  const uint16_t* wr = W + (size_t)blockIdx.x * K;
  uint8_t* cr = codes + (size_t)blockIdx.x * K;
  const int nv = K / 8;
  uint32_t amax = 0;
  for (int v = threadIdx.x; v < nv; v += 256) {
    const sk_u32x4 x = *reinterpret_cast<const sk_u32x4*>(wr + v * 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) amax = max(amax, max(x[i] & 0x7fffu, (x[i] >> 16) & 0x7fffu));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  amax = max(max(red[0], red[1]), max(red[2], red[3]));
  if (amax == 0) {                                   // (uniform over the block)
    for (int v = threadIdx.x; v < nv; v += 256) *reinterpret_cast<uint2*>(cr + v * 8) = make_uint2(0u, 0u);
    if (threadIdx.x == 0) scale[blockIdx.x] = 1.f;
    return;
  }
  // absmax = 1.m * 2^(E - 127): <= 1.75 * 2^(e + 8) <=> e = E - 135 (+ 1 when 1.m > 1.75)
  const int E = (int)(amax >> 7);
  int e = E - 135 + ((amax & 0x7fu) > 0x60u ? 1 : 0);
  if (E == 0 || e < -126) e = -126;
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
  if (threadIdx.x == 0) scale[blockIdx.x] = __uint_as_float((uint32_t)(127 + e) << 23);
  for (int v = threadIdx.x; v < nv; v += 256) {
    const sk_u32x4 x = *reinterpret_cast<const sk_u32x4*>(wr + v * 8);
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t c0 = sk_e4m3_rne(__uint_as_float(x[i] << 16) * inv);
      const uint32_t c1 = sk_e4m3_rne(__uint_as_float(x[i] & 0xffff0000u) * inv);
      o[i >> 1] |= (c0 | (c1 << 8)) << ((i & 1) * 16);
    }
    *reinterpret_cast<uint2*>(cr + v * 8) = make_uint2(o[0], o[1]);
  }
}

}  // namespace llmq
