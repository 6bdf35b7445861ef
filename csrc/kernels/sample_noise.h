// The sampling-noise contract of the LM head (GM_EPI_SAMPLE, gemm_kernels.h).
//
// Temperature sampling is argmax_n(logit_n / T + G_n) with i.i.d. standard
// Gumbel G_n (the Gumbel-max identity: an exact draw from softmax(logits / T)).
// G_n is a pure function of (request seed, index of the generated token,
// vocabulary column), so a request's tokens do not depend on the step, row,
// batch or GPU that computed them.  ops/sampling.py is the numpy twin; the
// integer part (row key, bits) agrees with it bit for bit.
//
//   row key (host only)   z = splitmix64(seed + 0x9E3779B97F4A7C15 * (gidx + 1))
//                         k0 = low 32 bits of z, k1 = high 32 bits
//   bits                  m = fmix32(fmix32(n ^ k0) + k1)       n = global column
//   exponential           v = (m + 0.5) * 2^-32
//                         E = -log1p(-v) = v + v*v/2 + v*v*v/3  v <  2^-12
//                                        = -log(1 - v)          otherwise
//   Gumbel                G = -log(E)
//
// Small E is large G is small v, where a float built from the 32-bit integer
// keeps full relative precision: the winners of an argmax over 128k columns
// sit in that tail.  G is finite for every m (max ~22.9 at m = 0, min ~-3.1
// at m = 2^32 - 1).  The series branch is exact to float32 rounding (v*v/2
// alone would be off by v^3/3, 2^-24/3 relative at the switch; with the cubic
// term the two branches meet to 4e-12 there); the other has relative error <= ~2^-12 in
// E (1 - v rounds to 2^-25 absolute against v >= 2^-12), ~2.4e-4 absolute in
// G.  1 - v is built from ~m ((~m + 0.5) * 2^-32, the same real number) so
// that it cannot round to 0 for m near 2^32.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SN_HD __host__ __device__ __forceinline__
#else
#define SN_HD inline
#endif

namespace llmq {

SN_HD uint32_t sn_fmix32(uint32_t h) {             // the murmur3 finaliser
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

SN_HD uint64_t sn_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// (k0, k1) of generated token ``gidx`` of a request with ``seed``
SN_HD void sn_row_key(uint64_t seed, uint64_t gidx, uint32_t& k0, uint32_t& k1) {
  const uint64_t z = sn_splitmix64(seed + 0x9E3779B97F4A7C15ull * (gidx + 1));
  k0 = (uint32_t)z;
  k1 = (uint32_t)(z >> 32);
}

SN_HD uint32_t sn_bits(uint32_t k0, uint32_t k1, uint32_t n) { return sn_fmix32(sn_fmix32(n ^ k0) + k1); }

SN_HD float sn_log(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __logf(x);                                // v_log_f32 * ln 2
#else
  return std::log(x);
#endif
}

SN_HD float sn_gumbel_from_bits(uint32_t m) {
  const float v = ((float)m + 0.5f) * 0x1p-32f;    // exact below 2^-12 (m < 2^20)
  const float u = ((float)~m + 0.5f) * 0x1p-32f;   // 1 - v, >= 2^-33
  const float e = v < 0x1p-12f ? v * (1.f + v * (0.5f + v * (1.f / 3.f))) : -sn_log(u);
  return -sn_log(e);
}

SN_HD float sn_gumbel(uint32_t k0, uint32_t k1, uint32_t n) { return sn_gumbel_from_bits(sn_bits(k0, k1, n)); }

}  // namespace llmq

#undef SN_HD
