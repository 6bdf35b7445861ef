"""Construction checks of the tile-GEMM cases (tests/gemm_cases.py): the
inputs are exact in bf16 and the preconditions hold at every shape the GPU
file parametrises, the float64 references compute the documented operations
(RefOps, swiglu_reference), and each comparison passes a correct emulation of
the kernel (fp32 accumulate, the documented roundings, bf16) and fails each of
a list of single faults -- what shows test_gpu_gemm_tile.py would notice a
subtly wrong kernel."""
import pytest
import torch

import gemm_cases as GC
from kernel_checks import SENTINEL
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops.llama_ops import RefOps

BF = torch.bfloat16


def _fp32_product(x, w):
    return x.float() @ w.float().t()


# ----------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("N,K", GC.STORE_NK)
def test_int_cases_are_exact_at_every_store_and_residual_shape(N, K):
    for M in GC.STORE_M:
        for rs in (False, True):
            c = GC.int_case(M, N, K, seed=M + N + K, row_scale=rs)
            assert GC.roundtrips(c.ref) and c.x.shape == (M, K) and c.w.shape == (N, K)
            assert set(c.x.double().unique().tolist()) <= {-1.0, 0.0, 1.0}
            if rs:
                r = c.row_scale
                assert r.numel() == G.row_scale_len(M) and torch.isnan(r[M:]).all()
                assert set(r[:M].tolist()) <= {0.5, 1.0, 2.0, 4.0}
                assert torch.equal(c.ref, c.prod * r[:M, None].double())
        c = GC.int_case(M, N, K, seed=M + N + K, resid=True)
        assert GC.roundtrips(c.ref) and torch.equal(c.ref, c.prod + c.res.double())
        assert c.res.double().abs().max() <= 256
        # the fp32 sum the epilogue rounds is the float64 one: nothing is lost before the rounding
        assert torch.equal((c.res.float() + _fp32_product(c.x, c.w)).double(), c.ref)


def test_int_cases_of_the_tile_order_launches_are_exact():
    for M, N in GC.ORDER_CASES:
        assert GC.roundtrips(GC.int_case(M, N, 128, seed=M).ref)
    assert GC.roundtrips(GC.int_case(513, 768, 512, seed=513).ref)
    assert G.split_plan(513, 768, 512, 8) == 8 and G.split_all(513, 768, 512, 8) is None
    assert G._tiles(513, 768) == 9 and G._tiles(1281, 256) == 6


@pytest.mark.parametrize("N,K", GC.RMS_NK)
def test_rms_cases_keep_every_sum_of_squares_exact(N, K):
    for M in GC.RMS_M:
        c = GC.rms_case(M, N, K, seed=M + N)
        assert c.ref.abs().max() <= 64 and GC.roundtrips(c.ref)
        ssq = (c.ref * c.ref).sum(-1)
        assert ssq.max() < 2 ** 24 and torch.equal(ssq, ssq.round())
        # fp32 in two different orders gives the same sums: they are exact
        r32 = c.ref.float()
        assert torch.equal((r32 * r32).sum(-1).double(), ssq)
        assert torch.equal((r32 * r32).flip(-1).cumsum(-1)[:, -1].double(), ssq)
        # the reference is RefOps.row_rms of the updated rows
        ref = RefOps().row_rms(c.ref.to(BF), GC.RMS_EPS).double()
        assert ((ref - c.scale).abs() / c.scale).max() <= 2.0 ** -21
        # and a correct fp32 epilogue (division, add, rsqrt) is inside the bound
        emu = torch.rsqrt((r32 * r32).sum(-1) / float(N) + GC.RMS_EPS).double()
        assert ((emu - c.scale).abs() / c.scale).max() <= GC.RMS_REL_BOUND


def test_swiglu_reference_is_the_documented_op():
    overflow = False
    for N, K in GC.SWIGLU_NK:
        for M in GC.SWIGLU_M:
            for rs in (False, True):
                c = GC.swiglu_case(M, N, K, seed=M + N + K, row_scale=rs)
                assert c.ref.shape == (M, N // 2) and torch.isfinite(c.ref).all()
                assert torch.equal(G.swiglu_unpermute(c.w_perm), c.w_gu)
                overflow |= bool((c.g < -89).any())              # exp(-g) > fp32 max
                if rs:
                    want = RefOps().swiglu_rows(c.x, c.w_perm, c.row_scale[:M])
                else:
                    want = G.swiglu_reference(c.x, c.w_gu)
                # the fp32 references round once from fp32 math: inside the kernel's own bound
                GC.swiglu_check(want, c)
    assert overflow


def test_rope_cases_have_distinct_cells_and_exact_projections():
    for Hq, Hkv in GC.ROPE_HEADS:
        for K in GC.ROPE_K:
            for M in GC.ROPE_M:
                for rs in (False, True):
                    c = GC.rope_case(Hq, Hkv, M, K, seed=Hq + K + M, row_scale=rs)
                    assert c.N == (Hq + 2 * Hkv) * 128 and GC.roundtrips(c.proj) and all(c.valid)
                    cells = set(zip(c.slot.tolist(), c.pos.tolist()))
                    assert len(cells) == M and (1, 0) in cells
                    assert 0 <= c.slot.min() and c.slot.max() < GC.ROPE_SLOTS
                    assert 0 <= c.pos.min() and c.pos.max() < GC.ROPE_CTX
    c = GC.rope_case(4, 2, 11, 512, seed=5, front=1, back=1, drop=True)
    bad = [(int(s), int(p)) for s, p, v in zip(c.slot, c.pos, c.valid) if not v]
    assert sorted(bad) == sorted(GC.ROPE_BAD.values()) and sum(c.valid) == 5
    for s, p in bad:
        assert not (0 <= s < GC.ROPE_SLOTS and 0 <= p < GC.ROPE_CTX)
    assert {s for s, _ in bad} >= {-1, GC.ROPE_SLOTS} and {p for _, p in bad} >= {-1, -8, GC.ROPE_CTX, GC.ROPE_CTX + 3}
    b = GC.rope_buffers(c)
    assert b.kfull.shape[0] == GC.ROPE_SLOTS + 2 and b.kc.is_contiguous() and b.kc.shape[0] == GC.ROPE_SLOTS
    assert b.cos_v.shape[0] == GC.ROPE_CTX + 8 and b.kc.data_ptr() % 16 == 0 and b.cos_v.data_ptr() % 16 == 0


def test_head_cases():
    n = GC.needle_case()
    assert torch.equal(n.x.double(), torch.eye(512, dtype=torch.float64))
    assert _fp32_product(n.x, n.w).argmax(1).tolist() == list(range(512))
    t = GC.tie_case()
    lg = _fp32_product(t.x, t.w).double()
    assert torch.equal(lg, t.logits)
    for r, (lo, hi) in enumerate(GC.TIES):
        assert lo < hi and lg[r, lo] == lg[r, hi] == lg[r].max() and int((lg[r] == lg[r].max()).sum()) == 2
    kinds = {"lane": 0, "wave": 0, "wavecol": 0, "tile": 0}
    for lo, hi in GC.TIES:
        if lo // 256 != hi // 256:
            kinds["tile"] += 1
        elif lo // 64 != hi // 64:
            kinds["wavecol"] += 1
        elif lo % 16 == hi % 16:
            kinds["lane"] += 1
        else:
            kinds["wave"] += 1
    assert min(kinds.values()) >= 3
    assert {hi - lo for lo, hi in GC.TIES} >= {16, 32, 48, 1, 64, 192, 256}
    assert (lg[-2] < 0).all() and int((lg[-2] == lg[-2].max()).sum()) == 1 and (lg[-1] == 0).all()


# ----------------------------------------------------------------------------- sensitivity
def _emulate_store(c):
    """fp32 accumulate, the row scale in fp32, one rounding to bf16."""
    acc = _fp32_product(c.x, c.w)
    if c.row_scale is not None:
        acc = acc * c.row_scale[:c.M, None]
    if c.res is not None:
        acc = acc + c.res.float()
    return acc.to(BF)


@pytest.mark.parametrize("rs,resid", [(False, False), (True, False), (False, True)])
def test_exact_compare_passes_the_emulation_and_fails_single_faults(rs, resid):
    M, N, K = 129, 512, 384
    c = GC.int_case(M, N, K, seed=M + N + K, row_scale=rs, resid=resid)
    good = _emulate_store(c)
    assert GC.same_bits(good, c.ref)
    # one k dropped from one output element
    m, n = 77, 300
    k = int((c.x[m].float() * c.w[n].float()).abs().argmax())
    assert c.x[m, k] != 0 and c.w[n, k] != 0
    bad = good.clone()
    v = c.prod[m, n] - c.x[m, k].double() * c.w[n, k].double()
    if rs:
        v = v * c.row_scale[m].double()
    if resid:
        v = v + c.res[m, n].double()
    bad[m, n] = v.to(BF)
    assert not GC.same_bits(bad, c.ref)
    # two adjacent columns swapped
    diff = (good[:, 200] != good[:, 201]).nonzero()
    assert diff.numel()
    bad = good.clone()
    bad[:, [200, 201]] = good[:, [201, 200]]
    assert not GC.same_bits(bad, c.ref)
    # a whole K-tile pair (128 values of k) left out of one tile's accumulators
    bad = good.clone()
    part = _fp32_product(c.x[:, :K - 128], c.w[:256, :K - 128])
    if rs:
        part = part * c.row_scale[:M, None]
    if resid:
        part = part + c.res[:, :256].float()
    bad[:, :256] = part.to(BF)
    assert not GC.same_bits(bad, c.ref)


@pytest.mark.parametrize("M,N,K", [(1, 256, 128), (129, 512, 384), (300, 768, 768)])
def test_an_extra_bf16_rounding_before_the_residual_add_is_caught(M, N, K):
    """Every residual case plants one product that is no bf16 number (257)
    against a residual of -256: rounding the product before the add gives 0
    where the single rounding of the fp32 sum gives 1."""
    for c in (GC.int_case(M, N, K, seed=M + N + K, resid=True), GC.rms_case(M, 256, 128, seed=M + 256)):
        good = (c.res.float() + _fp32_product(c.x, c.w)).to(BF)
        assert GC.same_bits(good, c.ref) and c.ref[c.M - 1, c.N - 3] == 1
        bad = (c.res.float() + _fp32_product(c.x, c.w).to(BF).float()).to(BF)
        assert not GC.same_bits(bad, c.ref) and int((bad != good).sum()) == 1


def test_guard_compare_fails_one_padded_row_written():
    c = GC.int_case(129, 256, 128, seed=1)
    g = GC.out_guarded(129, 256)
    g.out.copy_(_emulate_store(c))
    assert g.intact() and GC.same_bits(g.out, c.ref)
    assert (GC.bits(g.buf)[:g.lo] == SENTINEL).all() and g.buf.numel() == (129 + 16) * 256 + 256
    for at in (g.hi, g.hi + 255, g.lo - 1, g.buf.numel() - 1):   # row M, row M - 1 of the front guard, the tail
        h = GC.out_guarded(129, 256)
        h.out.copy_(g.out)
        h.buf[at] = 1.0
        assert not h.intact()
    xg = GC.x_guarded(c.x)
    assert torch.equal(xg, c.x) and xg.is_contiguous() and xg.data_ptr() % 16 == 0
    assert torch.isnan(xg._base[129:].float()).all() and xg._base.shape == (129 + 16, 128)


def _emulate_swiglu(c):
    acc = _fp32_product(c.x, c.w_gu)
    if c.row_scale is not None:
        acc = acc * c.row_scale[:c.M, None]
    g, u = acc[:, :c.F], acc[:, c.F:]
    return (g / (1.0 + torch.exp(-g)) * u).to(BF)


def test_swiglu_compare_passes_the_emulation_and_fails_single_faults():
    c = GC.swiglu_case(129, 512, 512, seed=129 + 512 + 512, row_scale=True)
    good = _emulate_swiglu(c)
    assert GC.swiglu_check(good, c) <= 1
    # two adjacent features swapped
    bad = good.clone()
    bad[:, [40, 41]] = good[:, [41, 40]]
    with pytest.raises(AssertionError):
        GC.swiglu_check(bad, c)
    # one k dropped from one gate
    m, f = 5, 100
    k = int((c.x[m].float() * c.w_gu[f].float()).abs().argmax())
    acc = _fp32_product(c.x, c.w_gu)
    acc[m, f] -= c.x[m, k].float() * c.w_gu[f, k].float()
    acc = acc * c.row_scale[:c.M, None]
    g, u = acc[:, :c.F], acc[:, c.F:]
    assert u[m, f] != 0
    with pytest.raises(AssertionError):
        GC.swiglu_check((g / (1.0 + torch.exp(-g)) * u).to(BF), c)
    # an epilogue that forms inf / inf for an overflowing gate
    bad = good.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        GC.swiglu_check(bad, c)


def _emulate_rope(c, b, shift=0):
    """The epilogue on the CPU: the projection rounded to bf16, rotated in
    fp32 with the fp32 table row of ``pos + shift``, rounded to bf16; tokens
    out of range are dropped."""
    M, Hq, Hkv = c.M, c.Hq, c.Hkv
    acc = _fp32_product(c.x, c.w)
    if c.row_scale is not None:
        acc = acc * c.row_scale[:M, None]
    qkv = acc.to(BF).view(M, Hq + 2 * Hkv, 128)
    for t in range(M):
        s, p = int(c.slot[t]), int(c.pos[t])
        if not (0 <= s < GC.ROPE_SLOTS and 0 <= p < GC.ROPE_CTX):
            continue
        cs, sn = b.cos_v[p + shift][None], b.sin_v[p + shift][None]
        h = qkv[t].float()
        a, bb = h[:, :64], h[:, 64:]
        rot = torch.cat([a * cs - bb * sn, bb * cs + a * sn], dim=-1).to(BF)
        b.q.out[t] = rot[:Hq].reshape(-1)
        b.kc[s, :, p] = rot[Hq:Hq + Hkv]
        b.vc[s, :, p] = qkv[t, Hq + Hkv:]


@pytest.mark.parametrize("drop", [False, True])
def test_rope_compare_passes_the_emulation_and_fails_single_faults(drop):
    c = GC.rope_case(4, 2, 11, 512, seed=5, front=1, back=1, drop=drop, row_scale=True)
    b = GC.rope_buffers(c)
    _emulate_rope(c, b)
    assert GC.rope_check(c, b) <= 1
    # a rotation using pos + 1
    b2 = GC.rope_buffers(c)
    _emulate_rope(c, b2, shift=1)
    with pytest.raises(AssertionError):
        GC.rope_check(c, b2)
    # a V row written for a cell nobody addresses, in vc only
    b3 = GC.rope_buffers(c)
    _emulate_rope(c, b3)
    free = [(s, p) for s in range(GC.ROPE_SLOTS) for p in range(GC.ROPE_CTX)
            if (s, p) not in set(zip(c.slot.tolist(), c.pos.tolist()))][0]
    b3.vc[free[0], 1, free[1], 9] = 1.0
    with pytest.raises(AssertionError, match="V row"):
        GC.rope_check(c, b3)
    # a write into the guard slot behind the caches
    b4 = GC.rope_buffers(c)
    _emulate_rope(c, b4)
    b4.kfull[-1, 0, 5, 0] = 1.0
    with pytest.raises(AssertionError, match="K row"):
        GC.rope_check(c, b4)
    # a V row with two adjacent elements swapped
    b5 = GC.rope_buffers(c)
    _emulate_rope(c, b5)
    t = next(i for i, v in enumerate(c.valid) if v)
    row = b5.vc[int(c.slot[t]), 0, int(c.pos[t])]
    j = int((row[1:] != row[:-1]).nonzero()[0])
    row[[j, j + 1]] = row[[j + 1, j]]
    with pytest.raises(AssertionError, match="v of token"):
        GC.rope_check(c, b5)
    if drop:                                                     # a dropped token's q row written
        b6 = GC.rope_buffers(c)
        _emulate_rope(c, b6)
        b6.q.out[3, 0] = 1.0
        with pytest.raises(AssertionError, match="dropped token 3"):
            GC.rope_check(c, b6)


def test_tie_compare_fails_the_higher_column():
    t = GC.tie_case()
    lg = _fp32_product(t.x, t.w)
    first = lg.argmax(1).to(torch.int32)
    assert torch.equal(first, t.want)
    last = (511 - lg.flip(1).argmax(1)).to(torch.int32)          # every tie resolved to the higher column
    assert not torch.equal(last, t.want)
    assert [int(v) for v in last[:len(GC.TIES)]] == [hi for _, hi in GC.TIES]
    assert int(last[-2]) == int(t.want[-2])                      # a single maximum has no other answer


# ----------------------------------------------------------------------------- wrapper guards that need no GPU
@pytest.mark.parametrize("name", ["pos", "slot", "kc", "vc", "cos_t", "wqkv"])
def test_qkv_rope_refuses_an_operand_on_another_device(name):
    """Checked before the native module is even looked up, so nothing can launch."""
    c = GC.rope_case(2, 2, 7, 128, seed=2 + 128 + 7)
    b = GC.rope_buffers(c)
    ops = dict(x=c.x, wqkv=c.w, pos=b.pos, slot=b.slot, cos_t=b.cos_v, sin_t=b.sin_v, kc=b.kc, vc=b.vc)
    ops[name] = torch.empty_like(ops[name], device="meta")
    with pytest.raises(ValueError, match=f"{name} must be on x's device"):
        G.qkv_rope(ops["x"], ops["wqkv"], ops["pos"], ops["slot"], ops["cos_t"], ops["sin_t"], c.Hq, c.Hkv,
                   ops["kc"], ops["vc"], q_out=b.q.out)
    assert b.q.intact() and (GC.bits(b.q.out) == SENTINEL).all()
