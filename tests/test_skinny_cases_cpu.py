"""Construction checks of the skinny-GEMM cases (tests/skinny_cases.py): the
preconditions hold at every shape test_gpu_skinny.py parametrises, a correct
emulation of the kernel's contract passes every comparison and each of 21
single faults fails the comparison meant to catch it; ``skinny_splits`` against
its stated rule; the wrappers' device checks, which need no GPU."""
import pytest
import torch

import gemm_cases as GC
import skinny_cases as SC
from llm_message_queue_amd.ops import gemm as G

BF = torch.bfloat16


# ----------------------------------------------------------------------------- preconditions
def test_alphabet_is_sixteen_e4m3_codes_with_minus_zero():
    assert len(set(SC.CODES.tolist())) == 16 and int(SC.CODES[1]) == SC.NEG_ZERO_CODE and int(SC.CODES[0]) == 0
    dec = SC.TABLE[SC.CODES.long()]
    assert torch.equal(dec.double(), SC.ALPHABET) and torch.signbit(dec[1]) and not torch.signbit(dec[0])
    assert set(SC.ALPHABET.abs().tolist()) == {0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0}


def test_pow2_column_scales_differ_1_16_and_32_columns_apart():
    cs = SC.pow2_col_scales(2048)
    assert set(cs.tolist()) == {2.0 ** e for e in range(-3, 3)}
    for d in (1, 16, 32):
        assert bool((cs[d:] != cs[:-d]).all())


def _check_case(c):
    M, N = c.M, c.N
    assert set(c.x.double().unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    r = c.row_scale
    assert r.numel() == M + 8 and torch.isnan(r[M:]).all() and set(r[:M].tolist()) <= {0.5, 1.0, 2.0, 4.0}
    assert not (c.ref == 0).logical_and(torch.signbit(c.ref)).any() and torch.isfinite(c.ref).all()
    assert c.want.dtype == BF and c.want.shape == (M, N)
    if c.res is not None:
        inner = c.res.double().clone()
        inner[M - 1, N - 3] = 0
        assert inner.abs().max() <= 64 and torch.equal(inner, inner.round())
    if c.fmt == "fp8":
        assert c.codes.dtype == torch.uint8 and bool((c.codes == SC.NEG_ZERO_CODE).any())
        assert torch.equal(SC.TABLE[c.codes.long()].to(BF).double(), c.w.double())
        assert c.cs.dtype == torch.float32 and c.cs.shape == (N,)
    # the single rounding under test does happen, ties included
    assert c.not_bf16 > 0 and int((c.want.double() != c.ref).sum()) >= 1
    S = 3 if c.K % 384 == 0 else 1
    SC.check(SC.emulate(c, S), c, "emulation")


@pytest.mark.parametrize("M,N,K", SC.store_shapes())
def test_store_and_residual_cases_hold_their_preconditions(M, N, K):
    seed = SC.seed_of(M, N, K)
    c = SC.skinny_case(M, N, K, seed)
    assert c.prod[M - 1, N - 3] == 257 and c.prod[M - 1, N - 5] == 259
    if c.row_scale[M - 1] == 1:                                # 257 -> 256 and 259 -> 260: both ties to even
        assert c.want[M - 1, N - 3] == 256 and c.want[M - 1, N - 5] == 260
    for kw in (dict(), dict(resid=True), dict(fmt="fp8", col_scale="pow2"),
               dict(fmt="fp8", col_scale="pow2", resid=True)):
        _check_case(SC.skinny_case(M, N, K, seed, **kw))
    if K == SC.ANY_K and M in SC.ANY_M and N in SC.ANY_N:
        for resid in (False, True):
            c = SC.skinny_case(M, N, K, seed, fmt="fp8", col_scale="any", resid=resid)
            assert 0.5 <= c.cs.min() and c.cs.max() < 2 and not c.exact
            _check_case(c)


def test_the_share_of_results_that_are_no_bf16_numbers():
    """Printed: 1.3 % at K = 128 to 36 % at K = 2048.  Beyond the two planted
    ties every shape has more results that round, so the rounding is under
    test everywhere."""
    shares = [(SC.skinny_case(M, N, K, SC.seed_of(M, N, K)).not_bf16, M * N) for M, N, K in SC.store_shapes()]
    print(f"not bf16 numbers: {min(s for s, _ in shares):.3%} .. {max(s for s, _ in shares):.3%}")
    assert all(s * n > 2 for s, n in shares)


@pytest.mark.parametrize("M,N,K", SC.swiglu_shapes())
def test_swiglu_cases(M, N, K):
    for fmt in ("bf16", "fp8"):
        c = SC.swiglu_case(M, N, K, SC.seed_of(M, N, K), fmt=fmt)
        assert c.ref.shape == (M, N // 2) and torch.isfinite(c.ref).all()
        assert torch.equal(G.swiglu_unpermute(c.w), c.w_gu)
        if fmt == "fp8":
            assert torch.equal(SC.TABLE[c.codes.long()].to(BF).double(), c.w.double())
            assert torch.equal(c.cs_gu.index_select(0, G.swiglu_perm_index(c.F)), c.cs)
        for S in {1, 3 if K % 384 == 0 else 1}:
            assert SC.check(SC.emulate(c, S), c) <= 1


@pytest.mark.parametrize("steps", SC.PROBE_STEPS)
def test_probe_cases_put_every_code_at_every_k(steps):
    finite = {c for c in range(256) if c & 0x7F != 0x7F}
    codes = SC.probe_codes(128 * steps)
    for k in range(128 * steps):
        assert set(codes[:, k].tolist()) == finite
    for block in range(steps):
        c = SC.probe_case(steps, block)
        assert c.x.shape == (128, 128 * steps) and int(c.x.double().sum()) == 128
        assert torch.equal(c.x[:, 128 * block:128 * block + 128].double(), torch.eye(128, dtype=torch.float64))
        assert not (c.ref == 0).logical_and(torch.signbit(c.ref)).any()
        SC.check(SC.emulate(c, 1), c, "emulation")
        for fault in (7, 18, 19) + ((3,) if block == 1 else ()):
            with pytest.raises(AssertionError):
                SC.check(SC.emulate(c, 1, fault), c)


# ----------------------------------------------------------------------------- sensitivity
def _store(M, N, K, **kw):
    return SC.skinny_case(M, N, K, SC.seed_of(M, N, K), **kw)


def _swiglu(M, N, K, **kw):
    return SC.swiglu_case(M, N, K, SC.seed_of(M, N, K), **kw)


FP8 = dict(fmt="fp8", col_scale="pow2")
# fault -> the (case, S) launches of the GPU file meant to catch it
FAULT_CASES = {
    1: [(_store, (17, 256, 384), {}, 1), (_store, (17, 256, 384), FP8, 1)],
    2: [(_store, (17, 256, 384), {}, 1), (_store, (5, 128, 256), FP8, 1)],
    3: [(_store, (5, 128, 512), {}, 1), (_store, (5, 128, 768), FP8, 1)],
    4: [(_store, (17, 256, 768), {}, 3), (_store, (17, 256, 1792), FP8, 7)],
    5: [(_store, (17, 256, 768), {}, 2), (_store, (17, 256, 768), FP8, 6)],
    6: [(_store, (17, 256, 768), {}, 3), (_store, (300, 384, 768), FP8, 3)],
    7: [(_store, (17, 256, 768), FP8, 1), (_store, (17, 256, 768), dict(fmt="fp8", col_scale="any"), 3)],
    8: [(_store, (17, 256, 768), FP8, 1), (_store, (129, 384, 768), dict(fmt="fp8", col_scale="any"), 1)],
    9: [(_swiglu, (17, 512, 768), dict(fmt="fp8"), 1), (_swiglu, (1, 256, 128), dict(fmt="fp8"), 1)],
    10: [(_store, (17, 256, 384), {}, 1), (_store, (1, 256, 384), FP8, 1)],
    11: [(_store, (17, 256, 384), dict(resid=True), 1), (_store, (129, 384, 256), dict(resid=True, **FP8), 1)],
    12: [(_store, (17, 256, 384), dict(resid=True), 1), (_store, (129, 384, 256), dict(resid=True, **FP8), 1)],
    13: [(_store, (17, 256, 384), {}, 1), (_store, (17, 256, 384), dict(resid=True, **FP8), 1)],
    14: [(_store, (300, 384, 256), {}, 1), (_store, (17, 256, 384), FP8, 1)],
    15: [(_store, (300, 384, 256), {}, 1), (_store, (257, 1024, 768), FP8, 3)],
    16: [(_store, (17, 256, 384), {}, 1), (_store, (17, 256, 384), FP8, 1)],
    17: [(_swiglu, (17, 512, 768), {}, 1), (_swiglu, (17, 512, 768), dict(fmt="fp8"), 3)],
    18: [(_store, (17, 256, 384), FP8, 1)],
    19: [(_store, (17, 256, 384), FP8, 1)],
    20: [(_store, (17, 256, 384), {}, 1), (_swiglu, (17, 512, 768), {}, 1)],
    21: [(_store, (17, 256, 384), FP8, 1), (_store, (17, 256, 384), {}, 1)],
}


def test_every_fault_has_a_case():
    assert sorted(FAULT_CASES) == sorted(SC.FAULTS) == list(range(1, 22))


@pytest.mark.parametrize("fault", sorted(SC.FAULTS))
def test_each_single_fault_fails_its_comparison(fault):
    for build, shape, kw, S in FAULT_CASES[fault]:
        c = build(*shape, **kw)
        SC.check(SC.emulate(c, S), c, "no fault")
        with pytest.raises(AssertionError):
            SC.check(SC.emulate(c, S, fault), c, SC.FAULTS[fault])


def test_the_planted_pair_alone_catches_a_rounded_product():
    """257 against -256: one scaled unit, or 0 when the product went through bf16 first."""
    c = _store(17, 256, 384, resid=True)
    good, bad = SC.emulate(c, 1).out, SC.emulate(c, 1, 12).out
    m, n = c.M - 1, c.N - 3
    assert good[m, n] == float(c.row_scale[m]) and bad[m, n] == 0


def test_every_split_of_the_emulation_gives_the_bits_of_one():
    for K, S in SC.SPLIT_KS:
        for kw in ({}, FP8):
            c = _store(SC.SPLIT_M, SC.SPLIT_N, K, **kw)
            assert torch.equal(GC.bits(SC.emulate(c, S).out), GC.bits(SC.emulate(c, 1).out))


# ----------------------------------------------------------------------------- skinny_splits
@pytest.mark.parametrize("cus", [8, 32, 64, 256])
@pytest.mark.parametrize("M", [1, 64, 129, 1024])
def test_skinny_splits_table(M, cus):
    """S divides K into 128-deep steps, leaves every split at least 512 deep
    (or is 1) and is the smallest candidate that reaches two blocks a CU when
    one exists."""
    nk = SC.model_nk()
    assert len(nk) >= 7
    for N, K in nk:
        S = G.skinny_splits(N, K, cus, M)
        assert S in SC.SPLIT_CANDIDATES and K % (128 * S) == 0 and (K // S >= 512 or S == 1)
        blocks = N // 128 * -(-M // 128)
        legal = [s for s in SC.SPLIT_CANDIDATES if K % (128 * s) == 0 and K // s >= 512]
        reach = [s for s in legal if blocks * s >= 2 * cus]
        if reach:
            assert S == min(reach)
        elif legal:
            assert S == max(legal)


def test_skinny_splits_is_one_for_a_short_k():
    for cus in (8, 32, 64, 256):
        for M in (1, 64, 129, 1024):
            assert G.skinny_splits(4096, 256, cus, M) == 1
            assert G.skinny_splits(128, 384, cus, M) == 1


def test_skinny_splits_of_the_gpu_file():
    for cus in SC.SPLIT_AUTO_CUS:
        assert G.skinny_splits(SC.SPLIT_N, SC.SPLIT_AUTO_K, cus, SC.SPLIT_M) == 4


# ----------------------------------------------------------------------------- wrapper guards that need no GPU
def _ops(fp8):
    c = _store(5, 256, 256, **(FP8 if fp8 else {}))
    g = GC.out_guarded(5, 256)
    return c, g, dict(x=c.x, w=c.w, codes=c.codes, cs=c.cs, out=g.out, row_scale=c.row_scale)


def _call(fp8, o):
    if fp8:
        return G.skinny_fp8(o["x"], o["codes"], o["cs"], o["out"], G.SK_STORE, row_scale=o["row_scale"], splits=1)
    return G.skinny(o["x"], o["w"], o["out"], G.SK_STORE, row_scale=o["row_scale"], splits=1)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("name", ["w", "out", "row_scale"])
def test_skinny_refuses_an_operand_on_another_device(name, fp8):
    """Checked before the native module is looked up, so nothing can launch."""
    c, g, o = _ops(fp8)
    names = ("codes", "cs") if fp8 and name == "w" else (name,)
    for n in names:
        bad = dict(o)
        bad[n] = torch.empty_like(o[n], device="meta")
        with pytest.raises(ValueError, match="on x's device"):
            _call(fp8, bad)
    assert g.intact() and (GC.bits(g.out) == GC.SENTINEL).all()


@pytest.mark.parametrize("fp8", [False, True])
def test_skinny_refuses_x_on_the_cpu(fp8):
    c, g, o = _ops(fp8)
    with pytest.raises(ValueError, match="x must be on a GPU"):
        _call(fp8, o)
    assert g.intact() and (GC.bits(g.out) == GC.SENTINEL).all()
