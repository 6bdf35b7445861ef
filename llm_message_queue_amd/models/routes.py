"""Which kernel each GEMM of the Llama trunk takes: one pure plan.

A layer has four GEMMs -- qkv, o, gate/up, down -- and each has several
kernels (the skinny stream over the weights, the 256x256 tiles whole or
split-K, with or without the folded-RMSNorm row scale, the FP8-weight twins
of both, the library).  ``plan_qkv`` and ``plan_block`` say, for a row count,
which one a GEMM takes and with which launch arguments; ``LlamaStub`` only
dispatches on the answer.  This module is the only place where the model
compares a row count with a threshold.

The plans read ``RouteFlags`` (what the model was built with), the row
count, ``small_cus`` and ``quant``; they take no tensor and touch no device.
The thresholds and planners are ``ops.gemm``'s (``SKINNY_*_MAX_M``,
``fp8_plan``, ``split_all``, ``residual_tiles_ok``), and ``ops.gemm.RESID_EPI``
is read at every call: it is a module global an A/B run reassigns.

        kind          the call                                            carries
  qkv   skinny        row_rms, G.skinny(SK_STORE, cus), rope_kv
        skinny_fp8    row_rms, G.skinny_fp8(SK_STORE, cus), rope_kv
        tile_fp8      row_rms, G.gemm_fp8(split_cus), rope_kv
        tile_rows     ops.qkv_rope_rows(row scale, split_full)            takes the down GEMM's scales
        tile_normed   G.qkv_rope(rmsnorm(res))
        library       rmsnorm, F.linear or the split_qkv pair, rope_kv
  o /   skinny        G.skinny(SK_RESID, cus)
  down  tile          G.gemm_residual(split_cus)
        tile_rms      G.gemm_residual_rms                                 makes the next norm's scales
        library       res.addmm_
        skinny_fp8    G.skinny_fp8(SK_RESID, cus)
        tile_fp8      G.gemm_residual_fp8(split_cus)
  gate/ skinny        row_rms, G.skinny(SK_SWIGLU, cus)
  up    tile_split    G.gemm_swiglu(row scale, split_cus)                 takes the o GEMM's scales
        rows          ops.swiglu_rows(row scale)                          takes the o GEMM's scales
        tile_normed   G.gemm_swiglu(rmsnorm(res))
        mlp_up        ops.mlp_up(rmsnorm(res))
        skinny_fp8    row_rms, G.skinny_fp8(SK_SWIGLU, cus)
        tile_fp8      row_rms, G.gemm_swiglu_fp8(split_cus)
"""
from __future__ import annotations

from typing import NamedTuple, Optional

from ..ops import gemm as G

QKV_KINDS = ("skinny", "skinny_fp8", "tile_fp8", "tile_rows", "tile_normed", "library")
RESID_KINDS = ("skinny", "tile", "tile_rms", "library", "skinny_fp8", "tile_fp8")
GU_KINDS = ("skinny", "tile_split", "rows", "tile_normed", "mlp_up", "skinny_fp8", "tile_fp8")


class RouteFlags(NamedTuple):
    """What routing reads from a model, fixed when it is built."""
    hip: bool                    # impl == "hip"
    residual_in_gemm: bool
    split_qkv: bool
    fused_mlp: bool
    fused_qkv: bool
    row_scale_norm: bool
    fused_rms: bool
    prune_last: bool
    library_gemm: bool           # the effective one: also set without the HIP ops or fused_resid
    min_fused_tokens: int
    min_fused_qkv_tokens: int
    cus: int                     # CUs the serving stream may use; 0: no hand-written o / down (fused_resid off, no GPU)
    dim: int
    n_qkv: int                   # rows of wqkv


class Gemm(NamedTuple):
    """One GEMM's kernel and what its call is handed."""
    kind: str
    cus: int = 0                 # a skinny kind: the CUs its launch is sized for
    split_cus: int = 0           # a tile kind: split-K planned for that many CUs, 0: whole tiles
    split_full: Optional[int] = None   # qkv tile_rows: the ``split_all`` plan, None: the kernel's own split_plan
    makes_scale: bool = False    # returns the RMSNorm row scales of the rows it updated
    takes_scale: bool = False    # reads its row scales from the GEMM before it where that one made them


class Block(NamedTuple):
    """A layer's o projection and MLP at one row count."""
    o: Gemm
    gu: Gemm
    down: Gemm


class Step(NamedTuple):
    """What a step decides whatever its row count."""
    residual_norm: bool          # the residual_in_gemm=False body (``_hidden_residual_norm``)
    prune: bool                  # the last layer's o + MLP on the sampled rows only, else select after the trunk
    head_min_rows: int           # the heads' hand-written GEMM from this many sampled rows


def plan_step(f: RouteFlags, small_cus: int) -> Step:
    # a micro-forward, or a model without the library: the argmax / sampling epilogue at any row count
    hand = small_cus or not f.library_gemm
    return Step(not f.residual_in_gemm, f.prune_last and f.residual_in_gemm, 1 if hand else 256)


def _hand(f: RouteFlags, small: bool) -> bool:
    """The hand-written kernels at every row count, split-K where whole tiles
    leave CUs idle: on a micro-forward's CU partition (no library kernel,
    none of whose persistent / stream-K grids assume the whole chip) and on a
    library-free model."""
    return small or (not f.library_gemm and f.cus > 0)


def _qkv_on_tiles(f: RouteFlags, T: int, hand: bool) -> bool:
    return f.fused_qkv and (T >= f.min_fused_qkv_tokens or hand)


def _fp8(gemm: str, M: int, small: bool, cus: int) -> Gemm:
    """A quant forward's GEMM: never a bf16 kernel (a request sees one model
    in all its forwards).  The tile kernel's split-K plan is sized as the
    bf16 one; the skinny launch for 32 CUs where the model knows of none."""
    if G.fp8_plan(M, gemm, small) == "tile":
        return Gemm("tile_fp8", split_cus=cus)
    return Gemm("skinny_fp8", cus=cus or 32)


def plan_qkv(f: RouteFlags, T: int, small_cus: int, quant: bool) -> Gemm:
    """The qkv projection of a step of ``T`` rows.  A quant step of more
    rows than the fp8 kernels take has no plan: ValueError, before the step
    has run anything."""
    if quant and T > G.SKINNY_CHUNKED_MAX_M:
        raise ValueError(f"quant forward of {T} rows: the fp8 kernel takes at most {G.SKINNY_CHUNKED_MAX_M}")
    small = small_cus > 0 and f.hip
    hand = _hand(f, small)
    cus = small_cus if small else f.cus
    if quant:
        return _fp8("qkv", T, small, cus)
    # the skinny kernel up to SKINNY_PROJ_MAX_M rows, the split-K tiles above
    # (profiles/r6_skinny_chunked.jsonl); on a micro-forward's CU partition
    # only up to SKINNY_MAX_M: there the split-K tiles were faster for larger
    # steps.  Only with the norm weight folded into wqkv (fused_qkv): the
    # kernel applies the row scale alone.
    if hand and T <= (G.SKINNY_MAX_M if small else G.SKINNY_PROJ_MAX_M) \
            and f.row_scale_norm and f.fused_mlp and f.fused_qkv:
        return Gemm("skinny", cus=cus)
    if not _qkv_on_tiles(f, T, hand):
        return Gemm("library")
    if not f.row_scale_norm:
        return Gemm("tile_normed")
    # every tile split when twice the tiles fit one wave (split_all); else
    # the kernel's default half-empty-last-wave plan
    return Gemm("tile_rows", split_full=G.split_all(T, f.n_qkv, f.dim, cus) if hand else None, takes_scale=True)


def plan_block(f: RouteFlags, M: int, small_cus: int, quant: bool, last: bool = False) -> Block:
    """The o projection and the MLP of a layer over ``M`` rows.  ``last``:
    the last layer's, whose down GEMM feeds no qkv; any other block has the
    step's row count, and its down GEMM makes the next layer's row scales
    where that layer's qkv reads them."""
    small = small_cus > 0 and f.hip
    if quant:
        cus = small_cus or f.cus
        return Block(_fp8("o", M, small, cus), _fp8("gu", M, small, cus), _fp8("down", M, small, cus))
    hand = _hand(f, small)
    cus = small_cus if small else (f.cus if hand else 0)
    rows_mlp = f.fused_mlp and (M >= f.min_fused_tokens or hand)
    # o / down on whole tiles only where they fill whole waves of the chip
    tiles_ok = f.cus > 0 and G.residual_tiles_ok(M, f.dim, f.cus)
    # row scales out of the residual GEMM's epilogue: whole tiles of the LDS epilogue only
    rms = tiles_ok and f.fused_rms and G.RESID_EPI == G.EPI_RESID_LDS and not small
    # skinny: o / down up to SKINNY_RESID_MAX_M rows (past 256 its 128-row
    # chunks still beat 256x256 tiles whose 32-64 tiles leave most CUs
    # idle: profiles/r6_skinny_mid_m.jsonl), gate/up (N = 28,672: enough
    # tiles to fill the chip) only up to SKINNY_MAX_M
    skinny = hand and M <= (G.SKINNY_MAX_M if small else G.SKINNY_RESID_MAX_M) and f.row_scale_norm and f.fused_mlp

    def into_res(scale_wanted: bool) -> Gemm:
        if rms and scale_wanted:
            return Gemm("tile_rms", makes_scale=True)
        if skinny:
            return Gemm("skinny", cus=cus)
        if hand or tiles_ok:
            return Gemm("tile", split_cus=cus if (small or not tiles_ok) else 0)
        return Gemm("library")

    if skinny and M <= G.SKINNY_MAX_M:
        gu = Gemm("skinny", cus=cus)
    elif rows_mlp and f.row_scale_norm:
        gu = Gemm("tile_split", split_cus=cus, takes_scale=True) if hand else Gemm("rows", takes_scale=True)
    else:
        gu = Gemm("tile_normed" if rows_mlp else "mlp_up")
    return Block(into_res(rows_mlp and f.row_scale_norm), gu,
                 into_res(not last and f.row_scale_norm and _qkv_on_tiles(f, M, hand)))
