"""Host twin of the FP8 weight quantisation (``csrc/kernels/skinny_kernels.h``:
``quant_rows_e4m3_kernel``, the decode of ``skinny_partial_kernel<MT, true>``).

Contract.  A weight matrix ``w`` [N][K] becomes one byte an element plus one
float32 scale a row (= an output channel of ``x . wᵀ``):

* codes are OCP ``e4m3fn`` (1 sign, 4 exponent, 3 mantissa bits, bias 7, no
  infinities, ``0x7f`` / ``0xff`` = NaN, largest finite value 448) -- the fp8
  of gfx950, not the ``fnuz`` flavour of gfx942;
* the scale of a row is a power of two: the smallest ``2^e`` with
  ``absmax(row) / 2^e <= 448``, never below ``2^-126`` (a normal float32).
  An all-zero row has scale 1 and codes 0;
* ``code = round-to-nearest-even(w / scale)``.  The quotient is exact (a
  power-of-two scale) and at most 448 in magnitude, so no NaN code is ever
  produced.  Non-finite weights are refused;
* ``dequantize``: ``TABLE[code] * scale``.  Every finite e4m3 value has 4
  significant bits, so its product with a power of two is exactly a bfloat16
  number: the fp8 GEMM ``(A . codesᵀ) * scale[n] * row_scale[m]`` is the bf16
  GEMM over ``dequantize(codes, scale)`` up to the place of the scale in the
  fp32 epilogue, and the bf16 kernels and fp32 references are its oracles.
  (The GEMM kernel itself takes arbitrary float32 column scales.)

The integer arithmetic below is the device kernel's, step for step; the tests
hold both to ``torch``'s CPU ``float8_e4m3fn`` cast.
"""
from __future__ import annotations

import numpy as np
import torch

E4M3_MAX = 448.0
MIN_EXP = -126                     # the smallest scale exponent


def _decode_table() -> np.ndarray:
    c = np.arange(256, dtype=np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    mag = np.where((c & 0x7F) == 0x7F, np.nan, mag)
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


TABLE = _decode_table()            # float32 [256]: the value of every code (NaN at 0x7f / 0xff)


def scale_exponents(absmax) -> np.ndarray:
    """int32 ``e`` per row: the smallest ``e >= MIN_EXP`` with ``absmax <=
    448 * 2^e`` (0 for a zero row), from the float32 bits as the kernel
    does: ``absmax = 1.m * 2^(E - 127) <= 1.75 * 2^(e + 8)``."""
    bits = np.ascontiguousarray(absmax, dtype=np.float32).view(np.uint32).astype(np.int64)
    E, man = bits >> 23, bits & 0x7FFFFF
    e = E - 135 + (man > 0x600000)
    e = np.where((E == 0) | (e < MIN_EXP), MIN_EXP, e)
    return np.where(bits == 0, 0, e).astype(np.int32)


def e4m3_rne(x) -> np.ndarray:
    """uint8 codes of float32 ``x`` (``|x| <= 448``), round-to-nearest-even:
    from ``2^-6`` up the float32 mantissa rounded to 3 bits and the exponent
    re-biased; below, the float32 sum ``|x| + 2^14``, whose ulp is e4m3's
    subnormal step ``2^-9`` (the sum's low bits are the code)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    sign = (b >> np.uint32(24)) & np.uint32(0x80)
    u = b & np.uint32(0x7FFFFFFF)
    normal = u >= np.uint32(0x3C800000)
    un = u.astype(np.uint64)
    un = ((un + 0x7FFFF + ((un >> 20) & 1)) >> 20) - (120 << 3)
    with np.errstate(invalid="ignore"):
        f = (np.where(normal, np.uint32(0), u).view(np.float32) + np.float32(16384.0)).astype(np.float32)
    sub = f.view(np.uint32).astype(np.uint64) - 0x46800000
    return (sign.astype(np.uint64) | np.where(normal, un, sub)).astype(np.uint8)


def quantize_rows_e4m3(w: torch.Tensor):
    """``w`` [N][K] (bfloat16 or float32, CPU) -> (codes uint8 [N][K], scale
    float32 [N]) by the contract above."""
    if w.dim() != 2:
        raise ValueError("quantize_rows_e4m3: w must be [N][K]")
    x = w.detach().to("cpu", torch.float32).contiguous().numpy()
    if not np.isfinite(x).all():
        raise ValueError("quantize_rows_e4m3: non-finite weight")
    absmax = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    e = scale_exponents(absmax)
    scale = np.ldexp(np.float32(1.0), e).astype(np.float32)
    q = x * np.ldexp(np.float32(1.0), -e).astype(np.float32)[:, None]
    codes = e4m3_rne(q)
    codes[absmax == 0] = 0
    return torch.from_numpy(codes), torch.from_numpy(scale)


def dequantize(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """bfloat16 [N][K] = ``TABLE[codes] * scale[:, None]`` (exact for
    power-of-two scales), on the tensors' device."""
    if codes.dtype != torch.uint8 or scale.dtype != torch.float32 or codes.dim() != 2 \
            or scale.shape != (codes.shape[0],):
        raise ValueError("dequantize: codes uint8 [N][K], scale float32 [N]")
    table = torch.from_numpy(TABLE).to(codes.device)
    return (table[codes.long()] * scale[:, None]).to(torch.bfloat16)


def requantized(w: torch.Tensor) -> torch.Tensor:
    """``dequantize(quantize(w))`` in ``w``'s dtype, on its device: the
    weight the fp8 path computes with."""
    codes, scale = quantize_rows_e4m3(w)
    return dequantize(codes, scale).to(device=w.device, dtype=w.dtype)
