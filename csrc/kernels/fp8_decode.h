// The FP8 (e4m3) -> bf16 decode in registers that both W8A16 GEMMs run right
// before their bf16 MFMAs: the skinny kernel (skinny_kernels.h) and the FP8
// form of the 256x256 tile (gemm_kernels.h).  Every finite code is exactly a
// bf16 number (ops/quant.py holds the contract).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace llmq {

typedef __attribute__((ext_vector_type(8))) short sk_bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int sk_u32x4;

// fp8 (e4m3) -> bf16: bytes 2 HI, 2 HI + 1 of w -> two bf16 (low half first): the scaled pack
// conversion with scale 1, one VALU op a pair.  (v_cvt_pk_f32_fp8 + packing
// the two high halves measured 0-7 % slower per GEMM: profiles/skinny_fp8.md.)
template <bool HI>
__device__ __forceinline__ uint32_t sk_fp8x2_bf16(uint32_t w) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}

__device__ __forceinline__ sk_bf16x8 sk_fp8x8_bf16(uint32_t lo, uint32_t hi) {
  const sk_u32x4 r = {sk_fp8x2_bf16<false>(lo), sk_fp8x2_bf16<true>(lo), sk_fp8x2_bf16<false>(hi),
                      sk_fp8x2_bf16<true>(hi)};
  return __builtin_bit_cast(sk_bf16x8, r);
}

}  // namespace llmq
