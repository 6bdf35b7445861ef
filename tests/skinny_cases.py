"""Exact-arithmetic cases for the skinny GEMM, bf16 and FP8 weights (the GPU
tests in test_gpu_skinny.py and the construction checks in
test_skinny_cases_cpu.py).

``x`` holds -2 .. 2 and the weight the 16 values of ALPHABET, each of them an
e4m3 code and a bf16 number, so every product and every partial sum is a
multiple of 1/4 below 1024 in magnitude: 12 bits.  Row scales (0.5 .. 4) and
the "pow2" column scales (2^-3 .. 2^2) move that to multiples of 2^-6 below
2^14, 20 bits, and an integer residual up to 256 adds none.  fp32 holds all of
it, so accumulation is exact in any order -- across MFMA steps, ring stages
and split partials -- and so are the scalings and the residual add.  Unlike
gemm_cases.int_case the result is NOT a bf16 number everywhere: what the
kernel must store is the one round-to-nearest-even of an exactly known fp32
value, which puts ``sk_f2bf`` under test, with two planted ties (257 -> 256,
259 -> 260).  Every builder asserts its preconditions on the float64 product.

With arbitrary ("any") column scales ``sum * cs`` rounds; the expected value
is then the float32 twin of the documented order ``bf16(fl32(fl32(sum * cs) *
rs) + res)``: the row scale is a power of two, so only the first product and
the add round, and a contracted multiply-add gives the same bits.

Reference zeros are +0: the kernel's accumulators start at +0, a sum of -0
products onto +0 is +0, an exact cancellation is +0 under round-to-nearest,
the scales are positive and no residual is -0.  The comparisons are on bits,
and float64 matmul may return -0 for a column of -0 products.

Plain torch / numpy on the CPU; nothing here touches a GPU."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import gemm_cases as GC
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import quant as Q

BF = torch.bfloat16
X_VALUES = torch.tensor([-2.0, -1.0, 0.0, 0.0, 1.0, 2.0], dtype=torch.float64)
ALPHABET = torch.tensor([0.0, -0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0],
                        dtype=torch.float64)
NEG_ZERO_CODE = 0x80
TABLE = torch.from_numpy(Q.TABLE)                     # float32 [256]


def _alphabet_codes():
    """The e4m3 code of every ALPHABET value, looked up in ops.quant.TABLE (value and sign)."""
    codes = []
    for v in ALPHABET.tolist():
        hit = [c for c in range(256) if Q.TABLE[c] == v and bool(np.signbit(Q.TABLE[c])) == bool(np.signbit(v))]
        assert len(hit) == 1, (v, hit)
        codes.append(hit[0])
    return torch.tensor(codes, dtype=torch.uint8)


CODES = _alphabet_codes()
MAX_SUM = 1024.0                                      # bound asserted on |x . w|

# ----------------------------------------------------------------------------- the shapes of test_gpu_skinny.py
# pipeline: K = 128 n, one split.  The bf16 ring (3 stages) wraps at n = 4, the FP8 ring (5) at 6 and 11
PIPE_M, PIPE_N, PIPE_STEPS = (5, 128), (128, 256), (1, 2, 3, 4, 5, 6, 7, 11)
# MT = 1 .. 8 fragments of 16 rows, both sides of each edge and of the 64-row staging group
FRAG_M = (1, 15, 16, 17, 33, 48, 63, 64, 65, 81, 97, 113, 127, 128)
FRAG_N, FRAG_KS = 256, ((384, 1), (768, 2))
# more than one 128-row chunk: N = 384 takes the plain block mapping (3 column blocks), 1024 the XCD-grouped one
CHUNK_M, CHUNK_N, CHUNK_KS = (129, 192, 193, 256, 257, 300), (384, 1024), ((256, 1), (768, 3))
CHUNK_ONCE = ((1024, 2048, 128, 1), (1024, 128, 256, 2), (300, 2048, 256, 1))     # (M, N, K, S)
SPLIT_M, SPLIT_N = 17, 256
SPLIT_KS = ((256, 2), (768, 2), (768, 3), (768, 6), (896, 7), (1792, 7), (2048, 16))
SPLIT_AUTO_K, SPLIT_AUTO_CUS = 2048, (8, 32, 256)
ANY_M, ANY_N, ANY_K, ANY_S = (17, 129), (256, 384), 768, (1, 3)
PROBE_STEPS = (1, 2, 3, 4, 5, 6)
SWIGLU_M, SWIGLU_N, SWIGLU_KS = (1, 17, 64, 128, 129, 300), (256, 512, 1024), ((128, 1), (768, 1), (768, 3))
ROW_SCALE_PAD = 8


def seed_of(M, N, K):
    return M + N + K


def store_shapes():
    """Every (M, N, K) a STORE / RESID test of the GPU file launches."""
    s = {(M, N, 128 * n) for M in PIPE_M for N in PIPE_N for n in PIPE_STEPS}
    s |= {(M, FRAG_N, K) for M in FRAG_M for K, _ in FRAG_KS}
    s |= {(M, N, K) for M in CHUNK_M for N in CHUNK_N for K, _ in CHUNK_KS}
    s |= {(M, N, K) for M, N, K, _ in CHUNK_ONCE}
    s |= {(SPLIT_M, SPLIT_N, K) for K, _ in SPLIT_KS} | {(SPLIT_M, SPLIT_N, SPLIT_AUTO_K)}
    s |= {(M, N, ANY_K) for M in ANY_M for N in ANY_N}
    return sorted(s)


def swiglu_shapes():
    return sorted({(M, N, K) for M in SWIGLU_M for N in SWIGLU_N for K, _ in SWIGLU_KS})


# ----------------------------------------------------------------------------- data
def row_scales(M, g):
    """[M + ROW_SCALE_PAD] fp32: 0.5, 1, 2 or 4 a row, NaN behind the M entries
    the kernel may read."""
    rs = torch.full((M + ROW_SCALE_PAD,), float("nan"), dtype=torch.float32)
    rs[:M] = torch.tensor([0.5, 1.0, 2.0, 4.0])[torch.randint(0, 4, (M,), generator=g)]
    return rs


def pow2_col_scales(N):
    """2^-3 .. 2^2 by column, exponent (n + n // 16) % 6 - 3: columns 1, 16
    and 32 apart differ by 1 or 2, 5 and 4 modulo 6 -- a neighbour's scale,
    the other fragment's and (under SwiGLU) the gate's for the up column are
    all wrong ones."""
    n = torch.arange(N)
    return torch.exp2(((n + n // 16) % 6 - 3).double()).float()


def any_col_scales(N, g):
    return (0.5 + 1.5 * torch.rand(N, generator=g, dtype=torch.float32)).contiguous()


def _bits32(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _data(M, N, K, seed):
    """x [M][K] over X_VALUES, the weight [N][K] over ALPHABET (float64, and as
    e4m3 codes), their float64 product and the asserted preconditions.  Weight
    rows N - 3 and N - 5 and the head of x's last row are planted: the products
    257 and 259, both halfway between two bf16 numbers."""
    assert K >= 128 and N >= 128
    g = torch.Generator().manual_seed(seed)
    x = X_VALUES[torch.randint(0, 6, (M, K), generator=g)]
    wi = torch.randint(0, 16, (N, K), generator=g)
    x[M - 1, :32], x[M - 1, 32] = 2.0, 1.0
    for row, last in ((N - 3, 6), (N - 5, 12)):               # 32 * (2 * 4) + 1 * 1 and + 1 * 3
        wi[row] = 0
        wi[row, :32], wi[row, 32] = 14, last
    w, codes = ALPHABET[wi], CODES[wi]
    assert bool((codes == NEG_ZERO_CODE).any()) and bool((wi == 0).any())
    # decoding the codes gives back the alphabet values, signs of zero included
    assert torch.equal(_bits32(TABLE[codes.long()]), _bits32(w.float()))
    xb, wb = x.to(BF), w.to(BF)
    assert torch.equal(xb.double(), x) and torch.equal(_bits32(wb.float()), _bits32(w.float()))
    prod = x @ w.t()
    assert torch.equal(prod * 4, (prod * 4).round()) and prod.abs().max() < MAX_SUM
    assert torch.equal(prod.float().double(), prod)                       # its own fp32 round trip
    assert torch.equal((x.float() @ w.float().t()).double(), prod)        # and the fp32 matmul
    assert prod[M - 1, N - 3] == 257 and prod[M - 1, N - 5] == 259
    odd = int((prod.to(BF).double() != prod).sum())
    assert odd >= 2                                                       # (the ties at least)
    return SimpleNamespace(x=xb, w=wb, codes=codes.contiguous(), prod=prod, not_bf16=odd / prod.numel())


def _plus_zero(t):
    return torch.where(t == 0, torch.zeros((), dtype=t.dtype), t)


@functools.lru_cache(maxsize=None)
def skinny_case(M, N, K, seed, fmt="bf16", row_scale=True, resid=False, col_scale=None):
    """One STORE (or, ``resid``, RESID) launch: ``x``, ``w`` bf16 [N][K] (the
    decoded weight) and for ``fmt="fp8"`` its ``codes`` and ``cs`` (``col_scale``
    "pow2" or "any"), ``row_scale`` [M + 8], ``res`` (integers in [-64, 64] and
    the planted -256 against the scaled 257), ``ref`` float64 and ``want``, the
    bf16 the kernel must store bit for bit."""
    fp8 = fmt == "fp8"
    assert fmt in ("bf16", "fp8") and (col_scale in ("pow2", "any")) == fp8 and (fp8 or col_scale is None)
    d = _data(M, N, K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    exact = col_scale != "any"
    c = SimpleNamespace(M=M, N=N, K=K, fmt=fmt, epi=G.SK_RESID if resid else G.SK_STORE, x=d.x, w=d.w,
                        codes=d.codes if fp8 else None, cs=None, row_scale=None, res=None, prod=d.prod, exact=exact,
                        not_bf16=d.not_bf16)
    rs = torch.ones(M, dtype=torch.float32)
    if row_scale:
        c.row_scale = row_scales(M, g)
        rs = c.row_scale[:M]
    cs = torch.ones(N, dtype=torch.float32)
    if fp8:
        c.cs = cs = pow2_col_scales(N) if col_scale == "pow2" else any_col_scales(N, g)
    res = None
    if resid:
        res = torch.randint(-64, 65, (M, N), generator=g).double()
        # against the planted 257: the sum is one scaled unit unless the product was rounded before the add
        res[M - 1, N - 3] = -256.0 * (float(rs[M - 1]) * float(cs[N - 3]) if exact else 1.0)
        c.res = res.to(BF)
        assert torch.equal(c.res.double(), res)
    if exact:
        ref = d.prod * cs.double()[None, :] * rs.double()[:, None]
        if resid:
            ref = ref + res
            assert ref[M - 1, N - 3] == float(rs[M - 1]) * float(cs[N - 3])
        assert torch.equal(ref.float().double(), ref)         # fp32 holds it: the only rounding is the bf16 one
    else:
        t = (d.prod.float().numpy() * cs.numpy()[None, :]).astype(np.float32)
        t = (t * rs.numpy()[:, None]).astype(np.float32)
        if resid:
            t = (t + res.float().numpy()).astype(np.float32)
        ref = torch.from_numpy(t).double()
    c.ref = _plus_zero(ref)
    c.want = c.ref.float().to(BF)
    return c


def swiglu_cols(F):
    """(gate, up) columns of feature f in the permuted weight's row order."""
    f = torch.arange(F)
    gcol = f // 128 * 256 + f % 128 // 32 * 64 + f % 32
    return gcol, gcol + 32


@functools.lru_cache(maxsize=None)
def swiglu_case(M, N, K, seed, fmt="bf16", row_scale=True):
    """The same data as the [gate; up] weight (F = N / 2 rows each): ``w`` /
    ``codes`` / ``cs`` in the permuted row order the kernel takes (FP8: the
    "pow2" pattern laid over the permuted order, so a gate and its up column
    differ), ``w_gu`` / ``cs_gu`` unpermuted, and the float64 ``silu(g) * u``
    of the exact scaled ``g``, ``u`` for gemm_cases.swiglu_check."""
    fp8 = fmt == "fp8"
    d = _data(M, N, K, seed)
    g = torch.Generator().manual_seed(seed + 1)
    F = N // 2
    idx = G.swiglu_perm_index(F)
    c = SimpleNamespace(M=M, N=N, K=K, F=F, fmt=fmt, epi=G.SK_SWIGLU, x=d.x, w_gu=d.w,
                        w=d.w.index_select(0, idx).contiguous(), codes=None, cs=None, cs_gu=None, row_scale=None,
                        res=None, exact=False)
    assert torch.equal(c.w, G.swiglu_permute(d.w))
    s = torch.ones(M, 1, dtype=torch.float64)
    if row_scale:
        c.row_scale = row_scales(M, g)
        s = c.row_scale[:M, None].double()
    cs_gu = torch.ones(N, dtype=torch.float32)
    if fp8:
        c.codes = d.codes.index_select(0, idx).contiguous()
        c.cs = pow2_col_scales(N)
        cs_gu = torch.empty(N, dtype=torch.float32)
        cs_gu.index_copy_(0, idx, c.cs)                        # cs_gu[idx[r]] = cs[r]
        c.cs_gu = cs_gu
        gcol, ucol = swiglu_cols(F)
        assert bool((c.cs[gcol] != c.cs[ucol]).all())
    c.g = d.prod[:, :F] * cs_gu.double()[None, :F] * s
    c.u = d.prod[:, F:] * cs_gu.double()[None, F:] * s
    assert torch.equal(c.g.float().double(), c.g) and torch.equal(c.u.float().double(), c.u)
    c.ref = c.g / (1.0 + torch.exp(-c.g)) * c.u
    return c


def probe_codes(K):
    """[256][K]: row n is a fixed permutation of the 254 finite codes and two
    zeros, rotated by n (and by another 101 every 256 k), so at every k the 256
    rows hold every finite code."""
    finite = np.array([c for c in range(256) if c & 0x7F != 0x7F] + [0, 0], dtype=np.int64)
    perm = finite[np.random.default_rng(7).permutation(256)]
    n, k = np.arange(256)[:, None], np.arange(K)[None, :]
    return torch.from_numpy(perm[(k + n + 101 * (k // 256)) % 256].astype(np.uint8)).contiguous()


@functools.lru_cache(maxsize=None)
def probe_case(steps, block):
    """FP8 identity probe, M = 128, N = 256, K = 128 * steps: x is the identity
    in K block ``block`` and zero elsewhere, so out[m][n] is one decode --
    codes[n][128 block + m] -- times one arbitrary column scale (one fp32
    rounding) times a power-of-two row scale, and one bf16 rounding.  Over the
    256 rows every finite code visits every byte of a lane's 32-byte run, both
    column fragments and, over ``block``, every ring stage."""
    M, N, K = 128, 256, 128 * steps
    assert 0 <= block < steps
    g = torch.Generator().manual_seed(100 * steps + block)
    codes = probe_codes(K)
    x = torch.zeros(M, K, dtype=torch.float64)
    x[torch.arange(M), 128 * block + torch.arange(M)] = 1.0
    cs, rs = any_col_scales(N, g), row_scales(M, g)
    dec = Q.TABLE[codes[:, 128 * block:128 * block + 128].numpy()]       # float32 [N][128], no NaN code
    assert np.isfinite(dec).all()
    t = (dec * cs.numpy()[:, None]).astype(np.float32).T
    t = (t * rs[:M].numpy()[:, None]).astype(np.float32)
    ref = _plus_zero(torch.from_numpy(np.ascontiguousarray(t)).double())
    return SimpleNamespace(M=M, N=N, K=K, fmt="fp8", epi=G.SK_STORE, x=x.to(BF), w=None, codes=codes, cs=cs,
                           row_scale=rs, res=None, exact=False, ref=ref, want=ref.float().to(BF))


# ----------------------------------------------------------------------------- the kernel's contract, emulated
FAULTS = {
    1: "an 8-element K chunk dropped", 2: "the last 128-deep step dropped",
    3: "a step from the previous step's weights",
    4: "one split partial dropped", 5: "one split partial counted twice", 6: "a partial left as the poisoned workspace",
    7: "the column scale of column n + 1", 8: "the column scale of column n + 16", 9: "the gate's scale used for up",
    10: "the row scale of row m + 1", 11: "the row scale applied after the residual add",
    12: "the product rounded to bf16 before the add", 13: "truncation instead of round-to-nearest-even",
    14: "the last row of a chunk's tail not written", 15: "chunks mc and mc + 1 swapped",
    16: "the two 16-column fragments of a wave swapped", 17: "gate and up swapped",
    18: "the two codes of a byte pair swapped in the decode", 19: "the 4-byte halves of an 8-code group swapped",
    20: "a written guard row behind out", 21: "-0 decoded as NaN",
}


def emulate(c, S, fault=None):
    """The kernel's contract in plain torch: fp32 partials per K split, summed
    in split order from +0, times the column scale, times the row scale, the
    epilogue, one round-to-nearest-even to bf16, into a guarded buffer (which
    it returns).  ``fault``: one key of FAULTS applied on the way."""
    assert fault is None or fault in FAULTS
    M, N, K = c.M, c.N, c.K
    assert K % (128 * S) == 0
    fp8 = c.fmt == "fp8"
    x = c.x.float()
    wd = TABLE[c.codes.long()].clone() if fp8 else c.w.float().clone()
    k = torch.arange(K)
    if fault == 1:
        wd[16:32, 40:48] = 0.0                                 # fragment 1 of wave 0, chunk 5 of step 0
    elif fault == 2:
        wd[:128, K - 128:] = 0.0
    elif fault == 3:
        assert K >= 256
        wd[:128, 128:256] = wd[:128, 0:128]
    elif fault == 18:
        wd = wd[:, k ^ 1]
    elif fault == 19:
        wd = wd[:, k ^ 4]
    elif fault == 21:
        wd[(c.codes == NEG_ZERO_CODE) if fp8 else (GC.bits(c.w) == -32768)] = float("nan")
    kc = K // S
    ws = torch.stack([x[:, s * kc:(s + 1) * kc] @ wd[:, s * kc:(s + 1) * kc].t() for s in range(S)])
    if fault == 6:
        ws[S - 1, :128, :128] = float("nan")
    elif fault == 14:
        ws[:, M - 1, :] = float("nan")
    elif fault == 15:
        assert M >= 256
        ws = torch.cat([ws[:, 128:256], ws[:, 0:128], ws[:, 256:]], dim=1)
    elif fault == 16:
        ws = torch.cat([ws[:, :, 16:32], ws[:, :, 0:16], ws[:, :, 32:]], dim=2)
    parts = list(ws)
    if fault == 4:
        assert S > 1
        parts = parts[1:]
    elif fault == 5:
        parts.append(parts[0])
    v = torch.zeros(M, N, dtype=torch.float32)
    for p in parts:
        v = v + p
    if c.cs is not None:
        cs = c.cs
        if fault == 7:
            cs = cs.roll(-1)
        elif fault == 8:
            cs = cs.roll(-16)
        elif fault == 9:
            gcol, ucol = swiglu_cols(N // 2)
            cs = cs.clone()
            cs[ucol] = c.cs[gcol]
        v = v * cs[None, :]
    rs = torch.ones(M, 1, dtype=torch.float32)
    if c.row_scale is not None:
        rs = (c.row_scale[1:M + 1] if fault == 10 else c.row_scale[:M])[:, None]
    if c.epi == G.SK_SWIGLU:
        gcol, ucol = swiglu_cols(N // 2)
        ge, ue = v[:, gcol] * rs, v[:, ucol] * rs
        if fault == 17:
            ge, ue = ue, ge
        r = ge / (1.0 + torch.exp(-ge)) * ue
    elif c.res is None:
        r = v * rs
    elif fault == 11:
        r = (v + c.res.float()) * rs
    elif fault == 12:
        r = (v * rs).to(BF).float() + c.res.float()
    else:
        r = v * rs + c.res.float()
    y = (_bits32(r) >> 16).to(torch.int16).view(BF) if fault == 13 else r.to(BF)
    g = GC.out_guarded(M, y.shape[1])
    g.out.copy_(y)
    if fault == 20:
        g.buf[g.hi + 5] = 1.0
    return g


def check(g, c, what=""):
    """The comparison of every launch: SwiGLU within gemm_cases.swiglu_check's
    derived bound (returns the worst distance in bf16 steps), everything else
    ``c.want`` bit for bit with no NaN; nothing around the output changed."""
    if c.epi == G.SK_SWIGLU:
        worst = GC.swiglu_check(g.out, c)
        assert g.intact(), f"{what}: wrote outside its [M][F]"
        return worst
    GC.exact(g, c.want, what)
    return 0


# ----------------------------------------------------------------------------- skinny_splits
SPLIT_CANDIDATES = (1, 2, 4, 7, 8, 14, 16)


def model_nk():
    """(N, K) of the four layer GEMMs of both model configs."""
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    out = set()
    for cfg in (LlamaConfig.tiny(), LlamaConfig.llama3_8b()):
        d, f = cfg.dim, cfg.ffn
        out |= {((cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, d), (d, d), (2 * f, d), (d, f)}
    return sorted(out)
