"""Every epilogue of the 256x256-tile bf16 GEMM (``gemm_bf16_kernel<EPI>``,
ops/gemm.py) on the exact-arithmetic cases of tests/gemm_cases.py, at the
smallest shapes where it can go wrong: M on the wave-row and tile-row
boundaries, K of the prologue and drain alone, one loop trip and an odd number
of K-tile pairs, tile counts that are no power of two, every ``group_m``, whole
and split-K.  STORE, the four residual forms, the V rows of the RoPE epilogue
and the LM head have zero tolerance: a dropped, duplicated or misplaced k, row,
column, tile or K-half is a bit mismatch.  SwiGLU and the q / k rotation use
the bounds derived in gemm_cases.py.  Inputs sit in front of NaN rows, row
scales carry NaN padding and every output lies inside sentinel-filled memory."""
import pytest
import torch

import gemm_cases as GC
from kernel_checks import SENTINEL
from llm_message_queue_amd.ops import gemm as G

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(t):
    return None if t is None else t.to(DEV)


def _scratch(name):
    live, _ = G._scratch_entry(DEV, torch.cuda.current_stream(DEV).cuda_stream, name)
    return live


def _split_counters_are_zero():
    live = _scratch("split")
    return bool(live) and int(live[1].abs().sum()) == 0


def _exact(g, ref, what):
    torch.cuda.synchronize()
    GC.exact(g, ref, what)


# ----------------------------------------------------------------------------- a. STORE
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("N,K", GC.STORE_NK)
@pytest.mark.parametrize("M", GC.STORE_M)
def test_store_is_exact(M, N, K, rs):
    c = GC.int_case(M, N, K, seed=M + N + K, row_scale=rs)
    x, w, r = GC.x_guarded(c.x, device=DEV), c.w.to(DEV), _dev(c.row_scale)
    for split_cus in GC.splits(K):
        g = GC.out_guarded(M, N, device=DEV)
        G.gemm(x, w, out=g.out, row_scale=r, split_cus=split_cus)
        _exact(g, c.ref, f"split_cus={split_cus}")
        if split_cus:
            assert G.split_all(M, N, K, split_cus) == 0 and _split_counters_are_zero()


# ----------------------------------------------------------------------------- b. residual forms
def _residual_launch(c, launch):
    g = GC.out_guarded(c.M, c.N, device=DEV)
    g.out.copy_(c.res.to(DEV))
    launch(g.out)
    return g


@pytest.mark.parametrize("N,K", GC.STORE_NK)
@pytest.mark.parametrize("M", GC.STORE_M)
def test_residual_forms_are_exact(M, N, K):
    """bf16(res + x.wT), one rounding of the fp32 sum: every case holds one
    product (257) that an extra rounding on the way to the add would change."""
    c = GC.int_case(M, N, K, seed=M + N + K, resid=True)
    x, w = GC.x_guarded(c.x, device=DEV), c.w.to(DEV)
    forms = [(f"epi={e}", lambda out, e=e: G._launch(x, w, out, e))
             for e in (G.EPI_RESID, G.EPI_RESID_LDS, G.EPI_RESID_PRE)]
    if len(GC.splits(K)) > 1:
        assert G.RESID_EPI == G.EPI_RESID_LDS and G.split_all(M, N, K, 64) == 0
        forms.append(("gemm_residual split", lambda out: G.gemm_residual(x, w, out, split_cus=64)))
    for what, launch in forms:
        first = _residual_launch(c, launch)
        _exact(first, c.ref, what)
        again = _residual_launch(c, launch)
        _exact(again, c.ref, what + " again")
        assert torch.equal(GC.bits(first.out), GC.bits(again.out))
    if len(forms) == 4:
        assert _split_counters_are_zero()


# ----------------------------------------------------------------------------- c. residual + RMS
@pytest.mark.parametrize("N,K", GC.RMS_NK)
@pytest.mark.parametrize("M", GC.RMS_M)
def test_residual_rms_is_exact_and_its_scales_within_fp32_rounding(M, N, K):
    """``res`` as the plain LDS epilogue leaves it, bit for bit; the sums of
    squares are exact integers in fp32 (gemm_cases.rms_case), so the scales
    carry only the roundings of the division, the add and rsqrtf
    (gemm_cases.RMS_REL_BOUND, derived there).  Twice in a row: bit-equal
    scales, and the tickets are back at zero."""
    c = GC.rms_case(M, N, K, seed=M + N)
    x, w = GC.x_guarded(c.x, device=DEV), c.w.to(DEV)
    plain = _residual_launch(c, lambda out: G._launch(x, w, out, G.EPI_RESID_LDS))
    _exact(plain, c.ref, "plain")
    scales = []
    for it in range(2):
        box = []
        g = _residual_launch(c, lambda out: box.append(G.gemm_residual_rms(x, w, out, GC.RMS_EPS)))
        _exact(g, c.ref, f"rms launch {it}")
        assert torch.equal(GC.bits(g.out), GC.bits(plain.out))
        assert box[0].dtype == torch.float32 and box[0].numel() == G.row_scale_len(M)
        scales.append(box[0][:M].cpu())
        tickets = _scratch("rms")[1]
        assert int(tickets.abs().sum()) == 0
    assert torch.equal(scales[0].view(torch.int32), scales[1].view(torch.int32))
    rel = ((scales[0].double() - c.scale).abs() / c.scale).max().item()
    print(f"GEMM_TILE_ULP residual_rms M={M} N={N} K={K}: scale rel err {rel / 2 ** -24:.2f} * 2^-24")
    assert rel <= GC.RMS_REL_BOUND, rel


# ----------------------------------------------------------------------------- d. tile order
@pytest.mark.parametrize("group_m", [1, 2, 4, 8])
@pytest.mark.parametrize("M,N", GC.ORDER_CASES)
def test_tile_order_covers_every_tile_once(M, N, group_m):
    """9 and 6 tiles -- no multiple of 8, so the XCD runs of the block remap
    differ in length -- at every group size: a tile computed twice or never
    shows as wrong bits or as the sentinel."""
    c = GC.int_case(M, N, 128, seed=M)
    g = GC.out_guarded(M, N, device=DEV)
    G._launch(GC.x_guarded(c.x, device=DEV), c.w.to(DEV), g.out, G.EPI_STORE, group_m=group_m)
    _exact(g, c.ref, f"group_m={group_m}")


def test_tile_order_of_whole_and_split_tiles_mixed():
    """8 whole tiles and one split tile in one launch."""
    M, N, K = 513, 768, 512
    assert G.split_plan(M, N, K, 8) == 8 and G.split_all(M, N, K, 8) is None
    c = GC.int_case(M, N, K, seed=M)
    g = GC.out_guarded(M, N, device=DEV)
    G.gemm(GC.x_guarded(c.x, device=DEV), c.w.to(DEV), out=g.out, split_cus=8)
    _exact(g, c.ref, "mixed")
    assert _split_counters_are_zero()


# ----------------------------------------------------------------------------- e. SwiGLU
@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("N,K", GC.SWIGLU_NK)
@pytest.mark.parametrize("M", GC.SWIGLU_M)
def test_swiglu_within_one_rounding_of_fp64(M, N, K, rs):
    """float64 silu(g) u on the exact integers g, u (times the row scale):
    the only error is the epilogue's own.  The bound is ``2^-8 |ref| +
    BF16_MIN_NORMAL`` with one correction to its derivation
    (gemm_cases.swiglu_check): for a scaled gate below -88.72 fp32's exp(-g)
    is infinite, so ``g / (1 + exp(-g))`` is a signed zero while the true
    product, under 2.7e-37 |u|, can still be a normal number; there a zero is
    accepted too.  The line printed per case counts the results that needed
    that clause.  NaN is never accepted."""
    c = GC.swiglu_case(M, N, K, seed=M + N + K, row_scale=rs)
    x, w, r = GC.x_guarded(c.x, device=DEV), c.w_perm.to(DEV), _dev(c.row_scale)
    for split_cus in GC.splits(K):
        g = GC.out_guarded(M, c.F, device=DEV)
        G.gemm_swiglu(x, w, out=g.out, row_scale=r, split_cus=split_cus)
        torch.cuda.synchronize()
        worst = GC.swiglu_check(g.out, c)
        print(f"GEMM_TILE_ULP swiglu M={M} N={N} K={K} row_scale={rs} split_cus={split_cus}: {worst} ulp, "
              f"{GC.swiglu_overflow_zeros(g.out, c)} zeros past the exp overflow")
        assert g.intact()
        if split_cus:
            assert _split_counters_are_zero()


# ----------------------------------------------------------------------------- f. qkv + RoPE
def _rope_modes(c):
    """split=False; at K = 512 also every tile split and all but the last whole."""
    modes = [("whole", dict(split=False))]
    if c.K % 256 == 0 and c.K >= 512:
        tiles = G._tiles(c.M, c.N)
        modes += [("all split", dict(split=True, split_full=0)), ("mixed", dict(split=True, split_full=tiles - 1))]
    return modes


def _rope_run(c, what):
    x, w, r = GC.x_guarded(c.x, device=DEV), c.w.to(DEV), _dev(c.row_scale)
    for name, kw in _rope_modes(c):
        b = GC.rope_buffers(c, DEV)
        assert b.kc.is_contiguous() and b.kc.shape[0] == GC.ROPE_SLOTS
        q = G.qkv_rope(x, w, b.pos, b.slot, b.cos_v, b.sin_v, c.Hq, c.Hkv, b.kc, b.vc, q_out=b.q.out, row_scale=r, **kw)
        torch.cuda.synchronize()
        assert q.data_ptr() == b.q.out.data_ptr()
        worst = GC.rope_check(c, b)
        print(f"GEMM_TILE_ULP qkv_rope {what} {name}: {worst} ulp")
        if kw["split"]:
            assert _split_counters_are_zero()


@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("M", GC.ROPE_M)
@pytest.mark.parametrize("K", GC.ROPE_K)
@pytest.mark.parametrize("Hq,Hkv", GC.ROPE_HEADS)
def test_qkv_rope_vs_fp64(Hq, Hkv, K, M, rs):
    c = GC.rope_case(Hq, Hkv, M, K, seed=Hq + K + M, row_scale=rs)
    _rope_run(c, f"Hq={Hq} Hkv={Hkv} K={K} M={M} row_scale={rs}")


@pytest.mark.parametrize("rs", [False, True])
def test_qkv_rope_drops_out_of_range_tokens(rs):
    """One cache slot in front of and behind what the kernel is told about,
    8 table rows of NaN on each side: whatever a missing guard would touch
    belongs to this test, and a table row it would read shows as NaN."""
    c = GC.rope_case(4, 2, 11, 512, seed=5, front=1, back=1, row_scale=rs, drop=True)
    assert sum(c.valid) == 5
    _rope_run(c, f"dropped tokens row_scale={rs}")


# ----------------------------------------------------------------------------- g. LM head
def _greedy_sample(x, w, out=None):
    """lm_head_sample with every row greedy (inv_temp == 0): lm_head_argmax's ids."""
    M = x.shape[0]
    return G.lm_head_sample(x, w, torch.zeros(M, dtype=torch.float32, device=DEV),
                            torch.zeros(M, 2, dtype=torch.int32, device=DEV), out=out)


@pytest.mark.parametrize("head", [G.lm_head_argmax, _greedy_sample])
def test_lm_head_needle_every_column_wins_once(head):
    c = GC.needle_case()
    x, w = c.x.to(DEV), c.w.to(DEV)
    got = head(x, w)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c.want)
    M = 300                                                      # a partial second M-tile, into guarded memory
    buf = torch.full((M + 8,), -7, dtype=torch.int32, device=DEV)
    head(GC.x_guarded(c.x[:M], device=DEV), w, out=buf[:M])
    torch.cuda.synchronize()
    assert torch.equal(buf[:M].cpu(), c.want[:M]) and (buf[M:] == -7).all()


@pytest.mark.parametrize("head", [G.lm_head_argmax, _greedy_sample])
def test_lm_head_ties_pick_the_lower_column(head):
    """Two equal maxima inside one lane's four columns, in two lanes of a
    wave, in two wave columns and in two tiles (gemm_cases.TIES); negative
    logits with one maximum; an all-zero row."""
    c = GC.tie_case()
    got = head(c.x.to(DEV), c.w.to(DEV))
    torch.cuda.synchronize()
    assert got.cpu().tolist() == c.want.tolist()


# ----------------------------------------------------------------------------- h. refusals
def test_gemm_residual_rms_refuses_mismatched_operands():
    """A weight whose inner dimension is not x's (the larger one here, so even
    an unguarded launch would stay inside its allocations), an N or K the
    kernel does not tile, a ``res`` of another shape: ValueError before any
    launch, ``res`` untouched."""
    x = torch.ones(5, 128, dtype=torch.bfloat16, device=DEV)
    g = GC.out_guarded(5, 256, device=DEV)
    with pytest.raises(ValueError, match="inner dimensions"):
        G.gemm_residual_rms(x, torch.ones(256, 256, dtype=torch.bfloat16, device=DEV), g.out, 1e-5)
    with pytest.raises(ValueError, match="unsupported shape"):
        G.gemm_residual_rms(x[:, :64].contiguous(), torch.ones(256, 64, dtype=torch.bfloat16, device=DEV), g.out, 1e-5)
    g2 = GC.out_guarded(5, 200, device=DEV)
    with pytest.raises(ValueError, match="unsupported shape"):
        G.gemm_residual_rms(x, torch.ones(200, 128, dtype=torch.bfloat16, device=DEV), g2.out, 1e-5)
    with pytest.raises(ValueError, match="res shape"):
        G.gemm_residual_rms(x, torch.ones(256, 128, dtype=torch.bfloat16, device=DEV), g.buf[:6 * 256].view(6, 256), 1e-5)
    torch.cuda.synchronize()
    for buf in (g.buf, g2.buf):
        assert (GC.bits(buf) == SENTINEL).all()


def test_qkv_rope_refuses_mismatched_operands():
    """``wqkv`` [N][2K] and a ``q_out`` of another shape (both larger than
    what the kernel would address): ValueError before any launch; q and the
    caches keep their sentinels."""
    c = GC.rope_case(2, 2, 7, 128, seed=2 + 128 + 7)
    b = GC.rope_buffers(c, DEV)
    x, w = c.x.to(DEV), c.w.to(DEV)
    args = (b.pos, b.slot, b.cos_v, b.sin_v, c.Hq, c.Hkv, b.kc, b.vc)
    with pytest.raises(ValueError, match="inner dimensions"):
        G.qkv_rope(x, torch.cat([w, w], dim=1).contiguous(), *args, q_out=b.q.out)
    wide = GC.out_guarded(c.M, c.Hq * 128 + 128, device=DEV)
    tall = GC.out_guarded(c.M + 1, c.Hq * 128, device=DEV)
    for q in (wide, tall):
        with pytest.raises(ValueError, match="q_out shape"):
            G.qkv_rope(x, w, *args, q_out=q.out)
    torch.cuda.synchronize()
    for buf in (b.q.buf, wide.buf, tall.buf, b.kfull, b.vfull):
        assert (GC.bits(buf) == SENTINEL).all()
