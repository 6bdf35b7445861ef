"""The skinny GEMM (``skinny_partial_kernel<MT, FP8>`` and its finalize
kernels, ops/gemm.py ``skinny`` / ``skinny_fp8``) on the exact-arithmetic cases
of tests/skinny_cases.py, at the smallest shapes where it can go wrong: every
length of the register ring's walk, every fragment count MT = 1 .. 8, 128-row
chunks under both block mappings, one-step splits, both weight formats, with
power-of-two and arbitrary column scales, and an identity probe of the FP8
byte selection.  STORE and RESID have zero tolerance -- the one rounding of an
exactly known fp32 value -- and SwiGLU the bound derived in gemm_cases.py.
Every ``x`` sits in front of NaN rows, every row scale carries NaN padding,
every output lies inside sentinel-filled memory and the split-K workspace is
NaN before every launch: a partial nobody wrote cannot be covered by what an
earlier launch left there."""
import pytest
import torch

import gemm_cases as GC
import skinny_cases as SC
from llm_message_queue_amd.ops import gemm as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FMTS = ("bf16", "fp8")


def _kw(fmt, col_scale="pow2", **kw):
    return dict(fmt="fp8", col_scale=col_scale, **kw) if fmt == "fp8" else dict(kw)


def _store(M, N, K, fmt, **kw):
    return SC.skinny_case(M, N, K, SC.seed_of(M, N, K), **_kw(fmt, **kw))


def _live():
    live, _ = G._scratch_entry(DEV, torch.cuda.current_stream(DEV).cuda_stream, "skinny")
    return live[0] if live else None


def _workspace(need):
    """The stream's skinny workspace (a first tiny launch allocates it), which
    must already hold ``need`` floats: a launch that grew it would get fresh,
    unpoisoned memory."""
    if _live() is None:
        z = torch.zeros(128, 128, dtype=torch.bfloat16, device=DEV)
        G.skinny(z[:1], z, torch.empty(1, 128, dtype=torch.bfloat16, device=DEV), G.SK_STORE, splits=1)
    ws = _live()
    assert ws is not None and ws.numel() >= need
    return ws


def _launch(c, S, cus=32):
    """One launch of case ``c`` with ``splits=S`` (0: the wrapper's own
    choice) behind a NaN workspace; returns the guarded output.  Exactly the
    [S][M][N] partials were written."""
    swiglu = c.epi == G.SK_SWIGLU
    used = S or G.skinny_splits(c.N, c.K, cus, c.M)
    x, rs = GC.x_guarded(c.x, device=DEV), c.row_scale.to(DEV)
    g = GC.out_guarded(c.M, c.N // 2 if swiglu else c.N, device=DEV)
    if c.res is not None:
        g.out.copy_(c.res.to(DEV))
    ws = _workspace(used * c.M * c.N)
    ws.fill_(float("nan"))
    if c.fmt == "fp8":
        G.skinny_fp8(x, c.codes.to(DEV), c.cs.to(DEV), g.out, c.epi, row_scale=rs, cus=cus, splits=S)
    else:
        G.skinny(x, c.w.to(DEV), g.out, c.epi, row_scale=rs, cus=cus, splits=S)
    torch.cuda.synchronize()
    n = used * c.M * c.N
    assert _live() is ws
    assert not torch.isnan(ws[:n]).any(), "a partial was never written (or a NaN was read)"
    assert torch.isnan(ws[n:]).all(), f"wrote the workspace past {used} partials"
    return g


def _run(c, S, what, cus=32):
    g = _launch(c, S, cus)
    SC.check(g, c, f"{what} M={c.M} N={c.N} K={c.K} S={S} {c.fmt} epi={c.epi}")
    return g


# ----------------------------------------------------------------------------- a. the register ring
@pytest.mark.parametrize("n", SC.PIPE_STEPS)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_walk_of_the_ring_is_exact(fmt, n):
    """K = 128 n in one split: the prologue alone, every partly filled ring and
    its wrap (bf16: three stages, n = 4; FP8: five, n = 6 and 11)."""
    for M in SC.PIPE_M:
        for N in SC.PIPE_N:
            _run(_store(M, N, 128 * n, fmt), 1, "ring")


# ----------------------------------------------------------------------------- b. fragment counts
@pytest.mark.parametrize("M", SC.FRAG_M)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_fragment_count_is_exact(fmt, M):
    """MT = 1 .. 8 on both sides of each 16-row edge and of the 64-row staging
    group, STORE and RESID, whole and in two splits (FP8: "pow2" column scales)."""
    for K, S in SC.FRAG_KS:
        for resid in (False, True):
            _run(_store(M, SC.FRAG_N, K, fmt, resid=resid), S, "fragments")


# ----------------------------------------------------------------------------- c. 128-row chunks
@pytest.mark.parametrize("N", SC.CHUNK_N)
@pytest.mark.parametrize("M", SC.CHUNK_M)
@pytest.mark.parametrize("fmt", FMTS)
def test_chunks_under_both_block_mappings_are_exact(fmt, M, N):
    """Two and three chunks with tails of 1, 44, 64, 65 and 128 rows; N = 384
    (3 column blocks) maps blocks by ``blockIdx.x / nm``, N = 1024 (8) by the
    XCD-grouped formula."""
    assert (N // 128) % 8 == (0 if N == 1024 else 3)
    for K, S in SC.CHUNK_KS:
        for resid in (False, True):
            _run(_store(M, N, K, fmt, resid=resid), S, "chunks")


@pytest.mark.parametrize("M,N,K,S", SC.CHUNK_ONCE)
@pytest.mark.parametrize("fmt", FMTS)
def test_eight_chunks_and_a_second_group_of_column_blocks(fmt, M, N, K, S):
    _run(_store(M, N, K, fmt), S, "chunks")


# ----------------------------------------------------------------------------- d. splits
@pytest.mark.parametrize("K,S", SC.SPLIT_KS)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_split_gives_the_bits_of_one(fmt, K, S):
    """Down to one 128-deep step a split, and S = 7 and 16 partials."""
    c = _store(SC.SPLIT_M, SC.SPLIT_N, K, fmt)
    one, many = _run(c, 1, "splits"), _run(c, S, "splits")
    assert torch.equal(GC.bits(one.out), GC.bits(many.out))


@pytest.mark.parametrize("cus", SC.SPLIT_AUTO_CUS)
@pytest.mark.parametrize("fmt", FMTS)
def test_the_wrappers_own_split_choice(fmt, cus):
    """``splits=0``: skinny_splits decides (4 here: the deepest split that
    keeps 512 of K), and the workspace shows that many partials were written."""
    c = _store(SC.SPLIT_M, SC.SPLIT_N, SC.SPLIT_AUTO_K, fmt)
    assert G.skinny_splits(c.N, c.K, cus, c.M) == 4
    auto, one = _run(c, 0, "auto", cus=cus), _run(c, 1, "auto")
    assert torch.equal(GC.bits(auto.out), GC.bits(one.out))


# ----------------------------------------------------------------------------- e. arbitrary column scales
@pytest.mark.parametrize("N", SC.ANY_N)
@pytest.mark.parametrize("M", SC.ANY_M)
def test_arbitrary_column_scales_match_the_float32_twin(M, N):
    """bf16(fl32(fl32(sum * cs) * rs) + res) in numpy float32, bit for bit."""
    for S in SC.ANY_S:
        for resid in (False, True):
            _run(_store(M, N, SC.ANY_K, "fp8", col_scale="any", resid=resid), S, "any")


# ----------------------------------------------------------------------------- f. FP8 identity probe
@pytest.mark.parametrize("steps", SC.PROBE_STEPS)
def test_identity_probe_of_the_fp8_byte_selection(steps):
    """x = I in one K block: out[m][n] is decode(codes[n][128 block + m]) times
    one scale.  Every finite code in every byte of a lane's 32-byte run, in
    both column fragments and, over the blocks, in every ring stage."""
    for block in range(steps):
        _run(SC.probe_case(steps, block), 1, f"probe block {block}")


# ----------------------------------------------------------------------------- g. SwiGLU
@pytest.mark.parametrize("N", SC.SWIGLU_N)
@pytest.mark.parametrize("M", SC.SWIGLU_M)
@pytest.mark.parametrize("fmt", FMTS)
def test_swiglu_within_one_rounding_of_fp64(fmt, M, N):
    """float64 silu(g) u of the exact scaled g, u (FP8: a gate and its up
    column carry different scales), gemm_cases.swiglu_check's bound unchanged."""
    for K, S in SC.SWIGLU_KS:
        c = SC.swiglu_case(M, N, K, SC.seed_of(M, N, K), fmt=fmt)
        g = _launch(c, S)
        worst = SC.check(g, c, "swiglu")
        print(f"SKINNY_ULP swiglu {fmt} M={M} N={N} K={K} S={S}: {worst} ulp, "
              f"{GC.swiglu_overflow_zeros(g.out, c)} zeros past the exp overflow")


# ----------------------------------------------------------------------------- h. refusals
def _refusal_ops(fp8):
    c = _store(5, 256, 256, "fp8" if fp8 else "bf16")
    o = dict(x=c.x.to(DEV), rs=c.row_scale.to(DEV), epi=G.SK_STORE, splits=1)
    if fp8:
        o.update(codes=c.codes.to(DEV), cs=c.cs.to(DEV))
    else:
        o.update(w=c.w.to(DEV))
    return c, o


def _call(o, out):
    if "codes" in o:
        return G.skinny_fp8(o["x"], o["codes"], o["cs"], out, o["epi"], row_scale=o["rs"], splits=o["splits"])
    return G.skinny(o["x"], o["w"], out, o["epi"], row_scale=o["rs"], splits=o["splits"])


def _misaligned(t):
    """``t``'s values one element into a fresh buffer: contiguous, not 16-byte aligned."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16
    return v


@pytest.mark.parametrize("fp8", [False, True])
def test_refusals_raise_before_any_launch(fp8):
    """Every bad argument is a ValueError from the wrapper or the launcher's
    own checks; the output it was given keeps its sentinels and the next good
    launch is exact."""
    c, o = _refusal_ops(fp8)
    M, N, K = c.M, c.N, c.K
    wk = "codes" if fp8 else "w"
    w = o[wk]
    bad = [
        ("K % 128", dict(x=o["x"][:, :192].contiguous(), **{wk: w[:, :192].contiguous()}), (M, N)),
        ("a split that does not divide K", dict(splits=3), (M, N)),
        ("M = 0", dict(x=o["x"][:0]), (0, N)),
        ("M = 1025", dict(x=torch.zeros(1025, K, dtype=torch.bfloat16, device=DEV),
                          rs=torch.ones(1033, device=DEV)), (1025, N)),
        ("a wider out", {}, (M, N + 128)),
        ("a taller out", {}, (M + 1, N)),
        ("SwiGLU with N = 128", dict(epi=G.SK_SWIGLU, **{wk: w[:128].contiguous()},
                                     **(dict(cs=o["cs"][:128].contiguous()) if fp8 else {})), (M, 64)),
        ("a short row_scale", dict(rs=o["rs"][:M - 1]), (M, N)),
        ("a float64 row_scale", dict(rs=o["rs"].double()), (M, N)),
        ("a non-contiguous w", {wk: w.t().contiguous().t()}, (M, N)),
        ("a misaligned w", {wk: _misaligned(w)}, (M, N)),
        ("w on the CPU", {wk: w.cpu()}, (M, N)),
        ("row_scale on the CPU", dict(rs=o["rs"].cpu()), (M, N)),
        ("x on the CPU", dict(x=o["x"].cpu()), (M, N)),
        ("out on the CPU", {}, "cpu"),
    ]
    if fp8:
        bad.append(("col_scale on the CPU", dict(cs=o["cs"].cpu()), (M, N)))
    for what, change, shape in bad:
        g = GC.out_guarded(M, N, device="cpu") if shape == "cpu" else GC.out_guarded(*shape, device=DEV)
        with pytest.raises(ValueError):
            _call({**o, **change}, g.out)
            pytest.fail(f"{what}: accepted")
        torch.cuda.synchronize()
        assert (GC.bits(g.buf) == GC.SENTINEL).all(), what
        _run(c, 1, f"after {what}")
    everything = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()}
    with pytest.raises(ValueError, match="x must be on a GPU"):
        _call(everything, GC.out_guarded(M, N).out)
    _run(c, 1, "after everything on the CPU")
