"""Exact-arithmetic cases for the 256x256-tile bf16 GEMM (the GPU tests in
test_gpu_gemm_tile.py and the construction checks in test_gemm_cases_cpu.py).

``x`` and ``w`` hold -1, 0 and 1 (and one planted 16 a residual case),
residuals are small integers and row
scales powers of two, so every product and every partial sum is an integer far
below 2^24: fp32 accumulation is exact in any order -- on the MFMA, across the
split-K hand-over and in the epilogue -- and wherever the final value is a bf16
number the kernel's output is fixed bit for bit.  Every builder asserts that
precondition on its float64 reference.  Only SwiGLU and the q / k rotation
round; their inputs are exact, so the error is the epilogue's own and the
bounds are the ones derived for the same formulas in test_gpu_llama_ops.py.
Plain torch on the CPU; nothing here touches a GPU unless a caller passes a
device to the buffer builders."""
import functools
from types import SimpleNamespace

import torch

from kernel_checks import BF16_MIN_NORMAL, SENTINEL, _rope_ref, sentinel, ulp_distance
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops.llama_ops import rope_tables

# M: the wave-row (128) and tile-row (256) boundaries of the 2 x 4 wave layout, one row, a third M-tile.
# (N, K): K = 128 is prologue + drain only, 256 one trip of the 8-phase loop, 384 an odd number of
# K-tile pairs; 512 and 768 can run split-K (two and three pairs a half)
STORE_M = (1, 127, 128, 129, 255, 256, 257, 300)
STORE_NK = ((256, 128), (256, 256), (512, 384), (512, 512), (768, 768))
RMS_M = (1, 129, 257, 300)
RMS_NK = ((256, 128), (768, 128), (1024, 512))
SWIGLU_M = (1, 129, 257, 300)
SWIGLU_NK = ((256, 128), (512, 512), (768, 768))
ROPE_HEADS = ((2, 2), (4, 2), (6, 4))          # one, two, three q tiles: N = 768, 1024, 1792
ROPE_K = (128, 512)
ROPE_M = (7, 300)
ORDER_CASES = ((513, 768), (1281, 256))         # 3 x 3 tiles with one row in the last M-tile; 6 x 1
ROPE_SLOTS, ROPE_CTX = 3, 128
# rows of the dropped-token case and their out-of-range (slot, pos)
ROPE_BAD = {1: (ROPE_SLOTS, 5), 3: (-1, 5), 5: (1, ROPE_CTX), 6: (1, -1), 8: (0, ROPE_CTX + 3), 9: (2, -8)}
RMS_EPS = 1e-5


def splits(K):
    """The split_cus values a K takes: whole, and every tile split where the
    kernel can halve K (K % 256 == 0, K >= 512)."""
    return (0, 64) if K % 256 == 0 and K >= 512 else (0,)


def roundtrips(t64):
    """Every value of the float64 tensor is a bf16 number."""
    return torch.equal(t64.to(torch.bfloat16).double(), t64)


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(y, ref64):
    """The bf16 tensor ``y`` is, bit for bit, the float64 reference rounded to
    bf16 (for an exact case: the reference itself)."""
    return torch.equal(bits(y.cpu()), bits(ref64.to(torch.bfloat16)))


def _tri(shape, g, density):
    """float64 values in {-1, 0, 1}, non-zero with probability ``density``."""
    u = torch.rand(shape, generator=g, dtype=torch.float64)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return torch.where(u < density, sign, torch.zeros((), dtype=torch.float64))


def _pow2_scales(M, g):
    """[row_scale_len(M)] fp32: 0.5, 1, 2 or 4 per row, NaN in the padding the
    kernel reads by design and must never store."""
    rs = torch.full((G.row_scale_len(M),), float("nan"), dtype=torch.float32)
    rs[:M] = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, (M,), generator=g)]
    return rs


@functools.lru_cache(maxsize=None)
def int_case(M, N, K, seed, row_scale=False, resid=False, density=2 / 3, res_max=64):
    """``x`` [M][K], ``w`` [N][K] bf16 over {-1, 0, 1}; ``row_scale`` (powers
    of two, NaN padding) and ``res`` [M][N] (integers in [-res_max, res_max],
    and one -256 against a planted product of 257) on request; ``prod`` the
    float64 product and ``ref`` what the kernel must store: ``prod * row_scale
    + res``, asserted to be bf16 numbers."""
    g = torch.Generator().manual_seed(seed)
    x, w = _tri((M, K), g, density), _tri((N, K), g, density)
    if resid:
        # one product that is no bf16 number, 16 * 16 + 1 = 257 in the last row, against a residual
        # of -256: the sum is 1 unless the product was rounded on its way to the add (256: then 0)
        x[M - 1], w[N - 3] = 0.0, 0.0
        x[M - 1, :2], w[N - 3, :2] = torch.tensor([16.0, 1.0]), torch.tensor([16.0, 1.0])
    prod = x @ w.t()
    c = SimpleNamespace(M=M, N=N, K=K, x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), prod=prod, res=None,
                        row_scale=None)
    ref = prod
    if row_scale:
        c.row_scale = _pow2_scales(M, g)
        ref = ref * c.row_scale[:M, None].double()
    if resid:
        res = torch.randint(-res_max, res_max + 1, (M, N), generator=g).double()
        res[M - 1, N - 3] = -256.0
        assert roundtrips(res) and prod[M - 1, N - 3] == 257 and not roundtrips(prod[M - 1])
        c.res = res.to(torch.bfloat16)
        ref = ref + res
    c.ref = ref
    assert torch.equal(c.x.double(), x) and torch.equal(c.w.double(), w)
    assert prod.abs().max() <= 512 and torch.equal(prod, prod.round())       # integers the fp32 sums hold exactly
    assert roundtrips(ref), f"M={M} N={N} K={K} seed={seed}: the exact result is not a bf16 number"
    return c


def rms_case(M, N, K, seed):
    """A residual case whose updated rows stay inside [-64, 64]: every square
    and every partial sum of squares of a row (N <= 1024) is then an integer
    below 1024 * 64^2 = 2^22, exact in fp32 in any order.  ``scale`` is the
    float64 ``1 / sqrt(sum / N + eps)``."""
    c = int_case(M, N, K, seed, resid=True, density=0.4, res_max=8)
    assert c.ref.abs().max() <= 64 and N * 64 * 64 < 2 ** 24
    c.scale = 1.0 / torch.sqrt((c.ref * c.ref).sum(-1) / N + RMS_EPS)
    return c


# The fused scale is rsqrtf(sum / (float)N + eps) over an exact fp32 ``sum``: the division (or a
# reciprocal and a product: 1.5 * 2^-23), the add (2^-24) and eps as an fp32 number (2^-25 of eps)
# give the argument a relative error of at most 2^-22, which the -1/2 power halves; rsqrtf itself
# is good to 2 ulp = 2^-22.  Together under 2^-22 + 2^-23 < 2^-21.
RMS_REL_BOUND = 2.0 ** -21


# ----------------------------------------------------------------------------- guarded buffers
def x_guarded(x, rows=16, device="cpu"):
    """``x`` as the first M rows of a buffer whose other ``rows`` rows are NaN:
    the kernel clamps its row loads to M - 1, so a NaN in any output means it
    read past the rows it was given."""
    M, K = x.shape
    buf = torch.full((M + rows, K), float("nan"), dtype=torch.bfloat16, device=device)
    buf[:M] = x.to(device)
    return buf[:M]


class Guarded:
    """``out`` [M][cols], a view into a buffer of the SENTINEL pattern with
    ``rows`` rows in front, ``rows`` rows and ``tail`` elements behind."""

    def __init__(self, M, cols, rows, tail, device):
        self.lo = rows * cols
        self.hi = self.lo + M * cols
        self.buf = sentinel((self.hi + rows * cols + tail,), device)
        self.out = self.buf[self.lo:self.hi].view(M, cols)

    def intact(self):
        """Everything around ``out`` still holds the sentinel (compared as int16)."""
        b = bits(self.buf).cpu()
        return bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.hi:] == SENTINEL).all())


def out_guarded(M, cols, rows=8, tail=256, device="cpu"):
    assert cols % 8 == 0                                      # ``out`` stays 16-byte aligned
    return Guarded(M, cols, rows, tail, device)


def exact(g, ref, what):
    """The guarded output holds no NaN (a read past x's rows or of the row
    scales' padding), is the reference bit for bit, and nothing around it changed."""
    y = g.out.cpu()
    assert not torch.isnan(y.float()).any(), f"{what}: NaN"
    bad = (bits(y) != bits(ref.to(torch.bfloat16))).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} wrong elements, first at {bad[0].tolist()}"
    assert same_bits(y, ref)
    assert g.intact(), f"{what}: wrote outside its [M][N]"


# ----------------------------------------------------------------------------- SwiGLU
@functools.lru_cache(maxsize=None)
def swiglu_case(M, N, K, seed, row_scale=False):
    """An :func:`int_case` whose ``w`` is the [gate; up] weight (F = N / 2 rows
    each): ``w_perm`` for the kernel and the float64 ``silu(g) * u`` of the
    exact, scaled integers g, u."""
    c = int_case(M, N, K, seed, row_scale=row_scale)
    F = N // 2
    s = c.row_scale[:M, None].double() if row_scale else 1.0
    g, u = c.prod[:, :F] * s, c.prod[:, F:] * s
    return SimpleNamespace(M=M, N=N, K=K, F=F, x=c.x, w_gu=c.w, w_perm=G.swiglu_permute(c.w), row_scale=c.row_scale,
                           g=g, u=u, ref=g / (1.0 + torch.exp(-g)) * u)


# exp(-g) leaves fp32 above ln(FLT_MAX) = 88.7228; __expf forms -g * log2(e) in fp32 first, whose
# rounding moves that edge by under 1e-5.  The scaled gates are multiples of 1/2.
EXP_OVERFLOW_GATE = -88.7


def swiglu_check(y, c):
    """``y`` is finite and within one bf16 rounding of the float64 ``c.ref``
    (2^-9 relative, and as much again for the fp32 exp, division and product
    in front of it: ``2^-8 |ref| + BF16_MIN_NORMAL``, the bound of
    test_silu_mul_vs_fp64 -- below the smallest normal a result may lose every
    bit).

    One correction to that derivation, from the fp32 format and the documented
    formula ``g / (1 + exp(-g))`` alone: for g < -88.7228 exp(-g) is above
    FLT_MAX, the quotient is a signed zero and so is the product, while the
    true |silu(g) u| is still a normal number down to g of about -100 (at
    g = -90 and u = 100 it is 7e-36).  test_silu_mul_vs_fp64 has no gate
    between -88 and -100 and never met this; integer gates times a row scale
    of 4 do.  Where g < EXP_OVERFLOW_GATE the bound is therefore |ref| at
    least -- a zero passes -- which is under 88.73 / FLT_MAX * |u| = 2.7e-37
    |u|, nothing a bf16 consumer of the MLP can see.  A NaN (inf / inf, 0 * inf)
    still fails.  Returns the worst distance in bf16 steps over the normal
    results outside that range."""
    y, ref = y.cpu(), c.ref
    assert torch.isfinite(y.float()).all(), "a non-finite SwiGLU output (exp(-g) overflows fp32: inf, never NaN)"
    err = (y.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + BF16_MIN_NORMAL
    over = c.g < EXP_OVERFLOW_GATE
    bound = torch.where(over, torch.maximum(bound, ref.abs()), bound)
    assert (err <= bound).all(), (err - bound).max().item()
    normal = (ref.abs() >= 2 * BF16_MIN_NORMAL) & ~over
    return ulp_distance(y[normal], ref[normal]) if normal.any() else 0


def swiglu_overflow_zeros(y, c):
    """How many results pass :func:`swiglu_check` only by its overflow clause
    (a zero where the reference is a normal number): reported, not asserted."""
    err = (y.cpu().double() - c.ref).abs()
    return int(((c.g < EXP_OVERFLOW_GATE) & (err > 2.0 ** -8 * c.ref.abs() + BF16_MIN_NORMAL)).sum())


# ----------------------------------------------------------------------------- qkv + RoPE
@functools.lru_cache(maxsize=None)
def rope_case(Hq, Hkv, M, K, seed, front=0, back=0, row_scale=False, drop=False):
    """An integer qkv projection (``proj`` float64 [M][(Hq + 2 Hkv) * 128],
    row scale applied, bf16 numbers), distinct (slot, pos) cells for the valid
    tokens -- one at pos 0, one at the last position -- and with ``drop`` the
    out-of-range tokens of ROPE_BAD (``valid`` marks the others).  ``front``
    / ``back``: guard slots, and 8 guard table rows each, around what the
    kernel is told about; :func:`rope_buffers` builds them."""
    N = (Hq + 2 * Hkv) * 128
    c = int_case(M, N, K, seed, row_scale=row_scale)
    g = torch.Generator().manual_seed(seed + 1)
    forced = [1 * ROPE_CTX + 0, 2 * ROPE_CTX + ROPE_CTX - 1]
    cells = [v for v in torch.randperm(ROPE_SLOTS * ROPE_CTX, generator=g).tolist() if v not in forced][:M]
    cells[0] = forced[0]
    cells[M - 1] = forced[1] if M > 1 else forced[0]
    slot, pos = [v // ROPE_CTX for v in cells], [v % ROPE_CTX for v in cells]
    valid = [True] * M
    if drop:
        assert M > max(ROPE_BAD)
        for r, (s, p) in ROPE_BAD.items():
            slot[r], pos[r], valid[r] = s, p, False
    live = [(s, p) for s, p, v in zip(slot, pos, valid) if v]
    assert len(set(live)) == len(live) and any(p == 0 for _, p in live)
    # the table proper (pos 0: cos 1, sin 0) between guard rows of NaN, which no clamped position reads
    nan_rows = [torch.full((8 * n, 64), float("nan")) for n in (front, back)]
    cos, sin = (torch.cat([nan_rows[0], t, nan_rows[1]]) for t in rope_tables(ROPE_CTX))
    return SimpleNamespace(Hq=Hq, Hkv=Hkv, M=M, N=N, K=K, front=front, back=back, x=c.x, w=c.w, row_scale=c.row_scale,
                           proj=c.ref, slot=torch.tensor(slot, dtype=torch.int32),
                           pos=torch.tensor(pos, dtype=torch.int32), valid=valid, cos=cos, sin=sin)


def rope_buffers(c, device="cpu"):
    """The operands of one launch on ``device``: sentinel-filled ``kfull`` /
    ``vfull`` with their ``kc`` / ``vc`` views behind ``front`` guard slots,
    the tables from row 8 * front on, and a guarded ``q``."""
    n = ROPE_SLOTS + c.front + c.back
    kfull, vfull = (sentinel((n, c.Hkv, ROPE_CTX, 128), device) for _ in range(2))
    cos, sin = c.cos.to(device), c.sin.to(device)
    return SimpleNamespace(kfull=kfull, vfull=vfull, kc=kfull[c.front:c.front + ROPE_SLOTS],
                           vc=vfull[c.front:c.front + ROPE_SLOTS], cos=cos, sin=sin, cos_v=cos[8 * c.front:],
                           sin_v=sin[8 * c.front:], q=out_guarded(c.M, c.Hq * 128, device=device),
                           pos=c.pos.to(device), slot=c.slot.to(device))


def rope_check(c, b):
    """After the launch: q rows and K rows of the valid tokens within
    ``_rope_ref``'s bound (1 bf16 ulp + 2^-22 (|a c| + |b s|): the fp32
    roundings of two products and a sum) of the float64 rotation of the exact
    projection, bit-exact at pos 0 (cos 1, sin 0); V rows bit-equal to the
    projection; every ``kc`` and ``vc`` cell no valid token addresses, the q
    rows of dropped tokens, the guard slots and the memory around q still the
    sentinel.  Returns the worst distance in bf16 steps."""
    M, Hq, Hkv = c.M, c.Hq, c.Hkv
    x = c.proj.view(M, Hq + 2 * Hkv, 128)
    row = torch.tensor([8 * c.front + int(p) if v else 0 for p, v in zip(c.pos, c.valid)])
    qref, qb = _rope_ref(x[:, :Hq], c.cos[row].double(), c.sin[row].double())
    kref, kb = _rope_ref(x[:, Hq:Hq + Hkv], c.cos[row].double(), c.sin[row].double())
    q = b.q.out.cpu().view(M, Hq, 128)
    kf, vf = b.kfull.cpu(), b.vfull.cpu()
    touched = torch.zeros(kf.shape[0], ROPE_CTX, dtype=torch.bool)
    worst = 0
    for t in range(M):
        if not c.valid[t]:
            assert (bits(q[t]) == SENTINEL).all(), f"dropped token {t} wrote q"
            continue
        s, p = c.front + int(c.slot[t]), int(c.pos[t])
        touched[s, p] = True
        k = kf[s, :, p]
        assert ((q[t].double() - qref[t]).abs() <= qb[t]).all(), f"q of token {t}"
        assert ((k.double() - kref[t]).abs() <= kb[t]).all(), f"k of token {t}"
        assert same_bits(vf[s, :, p], x[t, Hq + Hkv:]), f"v of token {t}"
        if p == 0:
            assert same_bits(q[t], x[t, :Hq]) and same_bits(k, x[t, Hq:Hq + Hkv]), f"token {t} at pos 0"
        worst = max(worst, ulp_distance(q[t], qref[t]), ulp_distance(k, kref[t]))
    rest = ~touched[:, None, :].expand(-1, Hkv, -1)
    assert (bits(kf)[rest] == SENTINEL).all(), "a K row that no token addresses changed"
    assert (bits(vf)[rest] == SENTINEL).all(), "a V row that no token addresses changed"
    assert b.q.intact(), "memory around q changed"
    return worst


# ----------------------------------------------------------------------------- LM head
@functools.lru_cache(maxsize=None)
def needle_case():
    """x = I_512, w [512][512] integers in [-3, 3] with a diagonal of 4: row m
    of the logits is column m of ``w``, its only maximum at column m, so every
    one of the 256 column positions of both tiles wins once."""
    g = torch.Generator().manual_seed(11)
    w = torch.randint(-3, 4, (512, 512), generator=g).double()
    w.fill_diagonal_(4.0)
    x = torch.eye(512, dtype=torch.float64)
    assert torch.equal((x @ w.t()).argmax(1), torch.arange(512))
    return SimpleNamespace(x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), want=torch.arange(512, dtype=torch.int32))


# (lower column, higher column) of two equal maxima.  A lane holds columns c, c + 16, c + 32 and
# c + 48 of its wave's 64; the 16 lanes of a row group hold neighbouring columns; the 4 wave
# columns hold 64 each; a tile 256.
TIES = ((0, 16), (5, 37), (15, 63), (70, 86), (300, 332),            # inside one lane
        (0, 1), (14, 15), (200, 201), (3, 12),                       # two lanes of one wave
        (0, 64), (9, 201), (63, 64), (257, 449), (130, 131 + 64),    # two wave columns
        (0, 256), (255, 256), (77, 333), (255, 511))                 # two tiles


@functools.lru_cache(maxsize=None)
def tie_case():
    """N = 512, K = 128.  Row r of ``x`` is the unit vector e_r, so its logits
    are column r of ``w``: small integers with two equal maxima (TIES: the
    lower column must win), then a row of negative logits with one maximum and
    an all-zero row (every logit ties at 0: column 0)."""
    g = torch.Generator().manual_seed(12)
    R = len(TIES) + 2
    logits = torch.randint(-3, 3, (R, 512), generator=g).double()
    want = []
    for r, (lo, hi) in enumerate(TIES):
        logits[r, lo] = logits[r, hi] = 5.0
        want.append(lo)
    logits[R - 2] = -3.0
    logits[R - 2, 389] = -1.0
    want.append(389)
    x = torch.zeros(R, 128, dtype=torch.float64)
    x[torch.arange(R - 1), torch.arange(R - 1)] = 1.0            # the last row stays zero
    want.append(0)
    w = torch.zeros(512, 128, dtype=torch.float64)
    w[:, :R - 1] = logits[:R - 1].t()
    w[:, R - 1:] = 2.0                                           # (columns no row of x selects)
    got = x @ w.t()
    assert torch.equal(got[:R - 1], logits[:R - 1]) and (got[R - 1] == 0).all()
    assert got.argmax(1).tolist() == want                        # torch.argmax: the first maximum
    return SimpleNamespace(x=x.to(torch.bfloat16), w=w.to(torch.bfloat16), logits=got,
                           want=torch.tensor(want, dtype=torch.int32))
