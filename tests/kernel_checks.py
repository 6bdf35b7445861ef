"""What the kernel tests share when they compare a bf16 result with a float64
reference: distances in bf16 steps, the bf16 spacing, the sentinel pattern of
memory no kernel may write, and the rotate-half reference with its derived
bound.  Plain torch; nothing here needs a GPU."""
import torch

SENTINEL = 0x5A5A
BF16_MIN_NORMAL = 2.0 ** -126


def _bf16(x):
    return x.to(torch.bfloat16)


def _ordered(t):
    """bf16 bit patterns as integers in value order (ulp distances)."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_distance(y, ref64):
    """Largest distance, in bf16 steps, between y and the correctly rounded reference."""
    return int((_ordered(y.cpu()) - _ordered(_bf16(ref64.float()))).abs().max())


def _bf16_ulp(r):
    """Spacing of bf16 at |r| (float64 tensor)."""
    e = torch.floor(torch.log2(r.abs().clamp(min=BF16_MIN_NORMAL)))
    return torch.exp2(e - 7)


def sentinel(shape, device="cpu"):
    """bf16 tensor whose every element is the SENTINEL bit pattern."""
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=device).view(torch.bfloat16)


def _rope_ref(x64, cos64, sin64):
    """x [T, H, 128], cos / sin [T, 64] -> rotate-half result, its bound
    (1 bf16 ulp + the fp32 rounding of two products and a sum: an FMA or a
    plain multiply-add both fit) in float64."""
    a, b = x64[..., :64], x64[..., 64:]
    c, s = cos64[:, None, :], sin64[:, None, :]
    ref = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=-1)
    return ref, _bf16_ulp(ref) + 2.0 ** -22 * mag
