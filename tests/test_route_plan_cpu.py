"""Properties of the trunk's route plan (``models.routes``) over every
input: the flags a constructor can produce, four CU counts, four
``small_cus`` values, ``quant`` where a model can run it, and the row counts
1..1100 thinned to every threshold +-2 plus a stride (the plan is pure
Python over small records, but the whole product is millions of calls).

What a constructor can produce: without the HIP ops, or without a CU count
(``fused_resid`` off), ``library_gemm`` is set; a ``quant`` plan is only ever
asked of a HIP model with ``fused_mlp``, ``fused_qkv`` and ``row_scale_norm``
(the constructor refuses fp8 weights otherwise, and the reference ops run a
quant forward as a bf16 one over the decoded weights).
"""
import itertools

import pytest

from llm_message_queue_amd.models import routes as R
from llm_message_queue_amd.ops import gemm as G

CUS = (0, 8, 64, 256)
SMALL_CUS = (0, 8, 32, 64)
DIMS = ((512, 768), (2048, 3072))                # (dim, qkv width): tiny enough that waves fill below 1,100 rows
MIN_FUSED = ((512, 2048), (48, 80))              # the defaults; the GPU route tests' library model
FP8_KINDS = {"skinny_fp8", "tile_fp8"}
SKINNY_KINDS = {"skinny", "skinny_fp8"}


def _rows():
    marks = {48, 80, G.SKINNY_MAX_M, G.SKINNY_PROJ_MAX_M, G.SKINNY_RESID_MAX_M, G.SKINNY_CHUNKED_MAX_M, 768,
             *G.FP8_TILE_MIN_M_SMALL.values(), *G.FP8_TILE_MIN_M_CHIP.values()}
    near = {m + d for m in marks for d in (-2, -1, 0, 1, 2)}
    return sorted(m for m in near | set(range(1, 1101, 37)) if 1 <= m <= 1100)


ROWS = _rows()


def _flags():
    for hip, fused_mlp, fused_qkv, rsn, fused_rms, lib, cus, (dim, nqkv), (mlp, qkv) in itertools.product(
            *[(False, True)] * 6, CUS, DIMS, MIN_FUSED):
        if (not hip or cus == 0) and not lib:
            continue
        yield R.RouteFlags(hip=hip, residual_in_gemm=True, split_qkv=False, fused_mlp=fused_mlp, fused_qkv=fused_qkv,
                           row_scale_norm=rsn, fused_rms=fused_rms, prune_last=True, library_gemm=lib,
                           min_fused_tokens=mlp, min_fused_qkv_tokens=qkv, cus=cus, dim=dim, n_qkv=nqkv)


def _cases():
    for f in _flags():
        for small_cus in SMALL_CUS:
            quants = (False, True) if f.hip and f.fused_mlp and f.fused_qkv and f.row_scale_norm else (False,)
            for quant in quants:
                yield f, small_cus, quant


def _check(f, M, small_cus, quant):
    if quant and M > G.SKINNY_CHUNKED_MAX_M:             # no such step: refused before anything runs
        with pytest.raises(ValueError, match="at most"):
            R.plan_qkv(f, M, small_cus, quant)
        return
    qkv = R.plan_qkv(f, M, small_cus, quant)
    blk = R.plan_block(f, M, small_cus, quant)
    tail = R.plan_block(f, M, small_cus, quant, last=True)
    small = small_cus > 0 and f.hip
    hand = small or (not f.library_gemm and f.cus > 0)
    resid = (blk.o, blk.down, tail.down)
    gemms = (qkv, blk.gu) + resid

    assert qkv.kind in R.QKV_KINDS and blk.gu.kind in R.GU_KINDS and all(p.kind in R.RESID_KINDS for p in resid)
    # the last layer's block differs in its down GEMM alone, which makes no scales
    assert (tail.o, tail.gu) == (blk.o, blk.gu) and not tail.down.makes_scale
    for p in gemms:
        assert p.makes_scale == (p.kind == "tile_rms")
        assert p.takes_scale == (p.kind in ("tile_rows", "tile_split", "rows"))

    if quant:
        # never a bf16 or library kind; the kernel is fp8_plan's; one cus convention
        for p, g in zip(gemms, ("qkv", "gu", "o", "down", "down")):
            assert p.kind == ("tile_fp8" if G.fp8_plan(M, g, small) == "tile" else "skinny_fp8")
            if p.kind == "tile_fp8":
                assert (p.cus, p.split_cus) == (0, small_cus or f.cus)
            else:
                assert (p.cus, p.split_cus) == (small_cus or f.cus or 32, 0)
        return
    assert not any(p.kind in FP8_KINDS for p in gemms)

    if small:
        # a micro-forward never names a library kernel -- where the model holds the weight in a
        # hand-written kernel's layout at all (fused_mlp / fused_qkv off: it is the library's)
        assert all(p.kind != "library" for p in resid)
        assert blk.gu.kind != "mlp_up" or not f.fused_mlp
        assert qkv.kind != "library" or not f.fused_qkv

    # skinny: only with the folded norms its row scale stands for, and only up to its row counts
    for p in resid + (blk.gu,):
        if p.kind == "skinny":
            assert f.row_scale_norm and f.fused_mlp and hand
            assert M <= (G.SKINNY_MAX_M if small else G.SKINNY_RESID_MAX_M)
            assert p.cus == (small_cus if small else f.cus)
    if blk.gu.kind == "skinny":
        assert M <= G.SKINNY_MAX_M
    if qkv.kind == "skinny":
        assert f.row_scale_norm and f.fused_mlp and f.fused_qkv and hand
        assert M <= (G.SKINNY_MAX_M if small else G.SKINNY_PROJ_MAX_M)
        assert qkv.cus == (small_cus if small else f.cus)

    # row scales out of a residual GEMM: fused_rms, a full wave, the LDS epilogue, no micro-forward
    tiles_ok = f.cus > 0 and G.residual_tiles_ok(M, f.dim, f.cus)
    for p in resid:
        if p.kind == "tile_rms":
            assert f.fused_rms and tiles_ok and G.RESID_EPI == G.EPI_RESID_LDS and not small
            assert f.row_scale_norm                      # and somebody to take them
        if p.kind == "tile":
            cus = small_cus if small else (f.cus if hand else 0)
            assert p.split_cus == (cus if (small or not tiles_ok) else 0)
    if blk.down.kind == "tile_rms":
        assert f.fused_qkv
    if blk.gu.kind == "tile_split":
        assert hand and blk.gu.split_cus == (small_cus if small else f.cus)

    # the tile qkv's split_all plan: only on the hand-written-everywhere routes
    if qkv.kind == "tile_rows":
        assert qkv.split_full == (G.split_all(M, f.n_qkv, f.dim, small_cus if small else f.cus) if hand else None)
    else:
        assert qkv.split_full is None

    if f.cus == 0 and not small:
        # no CU count (the reference ops; fused_resid off): the library's o / down, and a hand-written
        # kernel only through the ops object (qkv_rope_rows / swiglu_rows / mlp_up, which the
        # reference ops have too) -- but for row_scale_norm=False above the min_fused_* thresholds,
        # an A/B setting of the HIP model that calls ops.gemm itself
        assert all(p.kind == "library" for p in resid)
        assert blk.gu.kind in ({"rows", "mlp_up"} if f.row_scale_norm else {"tile_normed", "mlp_up"})
        assert qkv.kind in ({"tile_rows", "library"} if f.row_scale_norm else {"tile_normed", "library"})
        assert all((p.cus, p.split_cus) == (0, 0) for p in gemms)


def test_plan_properties_over_every_input():
    n = 0
    for f, small_cus, quant in _cases():
        for M in ROWS:
            _check(f, M, small_cus, quant)
            n += 1
    assert n > 100_000


def test_no_row_scales_from_the_register_epilogue(monkeypatch):
    """``RESID_EPI`` is read when the plan is made: with another residual
    epilogue than the LDS one no GEMM makes row scales, whatever the flags."""
    full = [M for M in ROWS if G.residual_tiles_ok(M, 512, 8)]
    f = next(f for f in _flags() if f.hip and f.fused_rms and f.fused_mlp and f.fused_qkv and f.row_scale_norm
             and not f.library_gemm and f.cus == 8 and f.dim == 512)
    assert full and all(R.plan_block(f, M, 0, False).o.kind == "tile_rms" for M in full)
    for epi in (G.EPI_RESID, G.EPI_RESID_PRE):
        monkeypatch.setattr(G, "RESID_EPI", epi)
        for g, small_cus, quant in _cases():
            for M in full:
                _check(g, M, small_cus, quant)
        assert all(R.plan_block(f, M, 0, False).o.kind == "tile" for M in full)


@pytest.mark.parametrize("residual_in_gemm,split_qkv,prune_last,library_gemm",
                         list(itertools.product((False, True), repeat=4)))
def test_step_plan(residual_in_gemm, split_qkv, prune_last, library_gemm):
    f = next(_flags())._replace(residual_in_gemm=residual_in_gemm, split_qkv=split_qkv, prune_last=prune_last,
                                library_gemm=library_gemm)
    for small_cus in SMALL_CUS:
        s = R.plan_step(f, small_cus)
        assert s.residual_norm == (not residual_in_gemm)
        assert s.prune == (prune_last and residual_in_gemm)
        assert s.head_min_rows == (1 if small_cus or not library_gemm else 256)


def test_the_plan_imports_no_torch():
    import ast
    import inspect
    names = {a.name for n in ast.walk(ast.parse(inspect.getsource(R))) if isinstance(n, (ast.Import, ast.ImportFrom))
             for a in n.names} | {n.module for n in ast.walk(ast.parse(inspect.getsource(R)))
                                  if isinstance(n, ast.ImportFrom)}
    assert not any(n and n.split(".")[0] == "torch" for n in names)
