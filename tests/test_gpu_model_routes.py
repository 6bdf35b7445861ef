"""Route-by-route float64 tests of the Llama trunk's kernel wiring
(``LlamaStub.hidden`` / ``_mlp_block`` / ``forward``) at ``LlamaConfig.tiny()``
dims, with the cases, the float64 twin and the measure of
``tests/model_cases.py``.

For every route: the HIP model and a ``RefOps`` model (``impl="ref"`` on the
same device, its own caches) get the case's weights (non-unit norm weights,
q rows scaled up so that positions, RoPE and the caches matter); both and
the twin run the case's two steps; **B** is the largest per-row error of the
``RefOps`` model against the twin, and every row of every step of the HIP
model must be within ``2 B`` of the twin.  The HIP routes round to bf16 where
``RefOps`` does or at fewer places (the fused epilogues) and fp32 summation
order is far below one bf16 rounding, so their error is B up to the spread
between rows (1.1-1.4x between median and maximum); every single wiring
mutation of ``tests/test_model_cases_cpu.py`` is at least 4 B.  The bound is
never taken from the HIP output.

Every test also proves which kernels ran: the entry points are wrapped with
call-recording pass-throughs, and the exact sequence of calls of the second
step, with their row counts, is asserted.  The thresholds come from the
``ops.gemm`` constants and functions, so a threshold change moves the cases
with it, and a route that stops existing fails its witness.

The reference model of a route rounds where the route rounds: with the
row-scale (folded norm) paths at every row count for the library-free
routes, with the model's own ``min_fused_*`` thresholds for the
``library_gemm`` routes, and with materialised RMSNorm rows for the routes
that materialise them (``row_scale_norm=False``, ``residual_in_gemm=False``).
A quant route's reference is a bf16 model over the decoded codes.
"""
import dataclasses

import pytest
import torch

import model_cases as MC
from llm_message_queue_amd.models.llama_stub import LlamaConfig, LlamaStub
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops.llama_ops import HipOps

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = LlamaConfig.tiny()
NQKV = (CFG.heads + 2 * CFG.kv_heads) * CFG.head_dim
Q_GAIN = 2.0
BOUND = 2.0
NEVER = 1 << 30
EPI = {G.SK_STORE: "store", G.SK_RESID: "resid", G.SK_SWIGLU: "swiglu"}


def _cus() -> int:
    return G._cu_count(torch.device(DEV))


# ------------------------------------------------------------------------------------------ the witness
class Witness:
    """Call-recording pass-throughs around the trunk's entry points."""

    def __init__(self, monkeypatch):
        self.calls, self.on = [], False

        def wrap(owner, name, describe, method=False):
            orig = getattr(owner, name)

            def through(*a, **k):
                if self.on:
                    self.calls.append(name + "[" + describe(a[1:] if method else a, k) + "]")
                return orig(*a, **k)
            monkeypatch.setattr(owner, name, through)

        def rows(a, k):
            return str(a[0].shape[0])

        def skinny(epi_at):
            return lambda a, k: f"{EPI[a[epi_at]]},{a[0].shape[0]},cus={k.get('cus')}"

        def split(a, k):
            return f"{a[0].shape[0]},split={int(bool(k.get('split_cus', 0)))}"

        wrap(G, "skinny", skinny(3))
        wrap(G, "skinny_fp8", skinny(4))
        wrap(G, "gemm_residual", split)
        wrap(G, "gemm_residual_fp8", split)
        for name in ("gemm_residual_rms", "gemm_swiglu", "gemm_fp8", "gemm_swiglu_fp8"):
            wrap(G, name, rows)
        wrap(G, "qkv_rope", lambda a, k: f"{a[0].shape[0]},full={k.get('split_full')}")
        for name in ("qkv_rope_rows", "swiglu_rows", "rope_kv", "mlp_up", "row_rms", "rmsnorm"):
            wrap(HipOps, name, rows, method=True)
        # the library's share of a route: o / down by addmm_, the split qkv pair by torch.mm
        wrap(torch.Tensor, "addmm_", lambda a, k: str(a[0].shape[0]), method=True)
        wrap(torch, "mm", rows)

    def record(self, fn):
        self.calls, self.on = [], True
        try:
            out = fn()
        finally:
            self.on = False
        return out, self.calls


# per-layer call sequences; {T}: the step's rows, {M}: the rows of this layer's o + MLP block,
# {C}: the CUs the launch is sized for, {F}: the split_all plan handed to the tile qkv
QKV_SK = ["row_rms[{T}]", "skinny[store,{T},cus={C}]", "rope_kv[{T}]"]
QKV_TILE = ["row_rms[{T}]", "qkv_rope_rows[{T}]", "qkv_rope[{T},full={F}]"]
QKV_TILE_CARRIED = QKV_TILE[1:]
QKV_LIB = ["rmsnorm[{T}]", "rope_kv[{T}]"]
O_SK = ["skinny[resid,{M},cus={C}]"]
O_SPLIT = ["gemm_residual[{M},split=1]"]
O_WHOLE = ["gemm_residual[{M},split=0]"]
O_RMS = ["gemm_residual_rms[{M}]"]
O_LIB = ["addmm_[{M}]"]
GU_SK = ["row_rms[{M}]", "skinny[swiglu,{M},cus={C}]"]
GU_TILE = ["row_rms[{M}]", "gemm_swiglu[{M}]"]
GU_TILE_CARRIED = ["gemm_swiglu[{M}]"]
GU_ROWS = ["row_rms[{M}]", "swiglu_rows[{M}]", "gemm_swiglu[{M}]"]
GU_LIB = ["rmsnorm[{M}]", "mlp_up[{M}]"]
FINAL = ["rmsnorm[{M}]"]

ALL_SKINNY = QKV_SK + O_SK + GU_SK + O_SK
GU_ON_TILES = QKV_SK + O_SK + GU_TILE + O_SK
QKV_ON_TILES = QKV_TILE + O_SK + GU_TILE + O_SK
ALL_TILES = QKV_TILE + O_SPLIT + GU_TILE + O_SPLIT


def _expected(layers, T, M, C, F):
    out = []
    for i, seq in enumerate(layers):
        m = M if i == len(layers) - 1 else T
        out += [s.format(T=T, M=m, C=C, F=F) for s in seq]
    return out + [s.format(M=M) for s in FINAL]


# ------------------------------------------------------------------------------------------ models and references
def _hip(case, **kw):
    return MC.install(LlamaStub(dataclasses.replace(CFG, layers=case.layers), slots=case.slots,
                                max_ctx=case.max_ctx, device=DEV, impl="hip", **kw), case)


def _ref_kwargs(hip: LlamaStub) -> dict:
    kw = dict(fused_mlp=hip.fused_mlp, fused_qkv=hip.fused_qkv, residual_in_gemm=hip.residual_in_gemm)
    if not hip.row_scale_norm or not hip.residual_in_gemm:
        kw.update(min_fused_tokens=NEVER, min_fused_qkv_tokens=NEVER)        # materialised RMSNorm rows
    elif hip.library_gemm:
        kw.update(min_fused_tokens=hip.min_fused_tokens, min_fused_qkv_tokens=hip.min_fused_qkv_tokens)
    else:
        kw.update(min_fused_tokens=1, min_fused_qkv_tokens=1)                # the row-scale paths at any row count
    return kw


_CASES, _REFS = {}, {}


def _case(T, layers=2):
    key = (T, layers)
    if key not in _CASES:
        _CASES[key] = MC.make_case(CFG, T, layers=layers, seed=T % 97, q_gain=Q_GAIN)
    return _CASES[key]


def _reference(case, hip: LlamaStub, quant: bool):
    """(twin hidden per step, B) for the case and the HIP model's kind,
    computed once: the twin reads the HIP model's stored weights, the
    ``RefOps`` model gets the same tensors (the decoded codes for quant)."""
    kw = _ref_kwargs(hip)
    key = (id(case), quant, tuple(sorted(kw.items())))
    if key not in _REFS:
        ref = LlamaStub(hip.cfg, slots=case.slots, max_ctx=case.max_ctx, device=DEV, impl="ref", **kw)
        MC.install(ref, case, decoded_from=hip if quant else None)
        for a, b in zip(ref.layers, hip.layers):                             # identical tensors
            for k in ("attn_norm", "mlp_norm") + (() if quant else MC.QUANT_NAMES):
                assert torch.equal(a[k], b[k]), k
        outs = []
        for st in case.steps:                                                # pos / slot on the host: RefOps
            outs.append(ref.hidden(st.tokens.to(DEV), st.pos, st.slot,       # indexes its caches token by token
                                   tiles=st.tiles, n_dec=st.n_dec))
        h64 = MC.twin(hip, case, quant=quant)
        B = max(float(MC.row_errors(a, b).max()) for a, b in zip(outs, h64))
        _REFS[key] = (h64, B)
    return _REFS[key]


def _check_route(monkeypatch, name, case, hip, layers, run=None, rows=None, attention="tiles", bound=BOUND,
                 split_cus=None):
    """Run the case on ``hip`` (step 1 plain, step 2 recorded), compare every
    row of both steps with the twin and the call sequence of step 2 with
    ``layers``.  Returns the HIP model's outputs."""
    run = dict(run or {})
    quant = bool(run.get("quant"))
    h64, B = _reference(case, hip, quant)
    w = Witness(monkeypatch)
    s1, s2 = (s.to(DEV) for s in case.steps)

    def step(st, **kw):
        if attention == "tokens":
            return hip.hidden(*st.args, **run, **kw)
        n_dec = 0 if attention == "segments" else st.n_dec
        return hip.hidden(*st.args, tiles=st.tiles, n_dec=n_dec, **run, **kw)

    out1 = step(s1)
    out2, calls = w.record(lambda: step(s2, **({} if rows is None else {"rows": rows.to(DEV)})))
    T = s2.tokens.numel()
    M = T if rows is None else rows.numel()
    want2 = h64[1] if rows is None else h64[1].index_select(0, rows.to(DEV))
    assert out1.shape == h64[0].shape and out2.shape == want2.shape
    worst = max(float(MC.row_errors(out1, h64[0]).max()), float(MC.row_errors(out2, want2).max()) if M else 0.0)
    C = run.get("small_cus") or hip._cus
    F = G.split_all(T, NQKV, CFG.dim, split_cus if split_cus is not None else C)
    print(f"ROUTE {name} T={T} M_last={M} B={B:.3e} ratio={worst / B:.2f} witness={' '.join(calls)}")
    assert calls == _expected(layers, T, M, C, F)
    assert worst <= bound * B, (worst / B, B)
    return out1, out2


# ------------------------------------------------------------------------------------------ the default model
DEFAULT = [
    ("gu-skinny", G.SKINNY_MAX_M, ALL_SKINNY),
    ("gu-tiles", G.SKINNY_MAX_M + 1, GU_ON_TILES),
    ("qkv-skinny", G.SKINNY_PROJ_MAX_M, GU_ON_TILES),
    ("qkv-tiles", G.SKINNY_PROJ_MAX_M + 1, QKV_ON_TILES),
    ("resid-skinny", G.SKINNY_RESID_MAX_M, QKV_ON_TILES),
    ("resid-tiles", G.SKINNY_RESID_MAX_M + 1, ALL_TILES),
]
T_ABOVE = max(G.SKINNY_MAX_M, G.SKINNY_PROJ_MAX_M, G.SKINNY_RESID_MAX_M) + 1


@pytest.mark.parametrize("name,T,seq", DEFAULT, ids=[f"{n}-{t}" for n, t, _ in DEFAULT])
def test_default_model_thresholds(monkeypatch, name, T, seq):
    """The library-free model at each threshold and one row above it.  At
    these dims every tile qkv up to 2,560 rows has a ``split_all`` plan (0);
    the plan being None is witnessed by ``test_fused_rms_chain``."""
    case = _case(T)
    hip = _hip(case)
    assert not hip.library_gemm and hip._cus > 0
    if T > G.SKINNY_PROJ_MAX_M:
        assert G.split_all(T, NQKV, CFG.dim, hip._cus) == 0
    _check_route(monkeypatch, f"default/{name}", case, hip, [seq, seq])


@pytest.mark.parametrize("m_rows", [5, "all"])
def test_last_layer_pruned_to_the_sampled_rows(monkeypatch, m_rows):
    """``rows=``: the last layer's o + MLP on the sampled rows only -- 5 rows
    on the skinny kernels under a tile first layer; every row sampled is the
    full run."""
    case = _case(T_ABOVE)
    hip = _hip(case)
    if m_rows == "all":
        rows, last = torch.arange(T_ABOVE), ALL_TILES
    else:
        rows, last = torch.tensor(MC.spread_rows(T_ABOVE, m_rows)), QKV_TILE + O_SK + GU_SK + O_SK
        assert rows.numel() == 5 and set(rows.tolist()) - {int(t[0] + t[1] - 1) for t in case.steps[1].tiles}
    _check_route(monkeypatch, f"default/rows-{m_rows}", case, hip, [ALL_TILES, last], rows=rows)


def test_no_sampled_row_still_writes_the_caches(monkeypatch):
    """``rows`` empty returns [0, d] after the last layer's qkv: the caches
    hold what a full run writes, bit for bit."""
    case = _case(T_ABOVE)
    full = _hip(case)
    MC.run_steps(full, case)
    hip = _hip(case)
    w = Witness(monkeypatch)
    s1, s2 = (s.to(DEV) for s in case.steps)
    hip.hidden(*s1.args, tiles=s1.tiles, n_dec=s1.n_dec)
    out, calls = w.record(lambda: hip.hidden(*s2.args, tiles=s2.tiles, n_dec=s2.n_dec,
                                             rows=torch.empty(0, dtype=torch.int64, device=DEV)))
    assert tuple(out.shape) == (0, CFG.dim)
    F = G.split_all(T_ABOVE, NQKV, CFG.dim, hip._cus)
    want = _expected([ALL_TILES, QKV_TILE], T_ABOVE, T_ABOVE, hip._cus, F)[:-1]
    print(f"ROUTE default/rows-none T={T_ABOVE} M_last=0 witness={' '.join(calls)}")
    assert calls == want
    for a, b in zip(hip.kcache + hip.vcache, full.kcache + full.vcache):
        assert bool(a.any()) and torch.equal(a, b)


@pytest.mark.parametrize("attention", ["tokens", "segments", "tiles"])
def test_attention_forms(monkeypatch, attention):
    """Per-token attention (``tiles=None``), the tiles with ``n_dec`` = 0
    (the decode rows as 1-token segments) and with ``n_dec`` > 0."""
    T = G.SKINNY_MAX_M + 1
    case = _case(T)
    assert case.steps[1].n_dec > 0
    _check_route(monkeypatch, f"attention/{attention}", case, _hip(case), [GU_ON_TILES] * 2, attention=attention)


# ------------------------------------------------------------------------------------------ micro-forwards
@pytest.mark.parametrize("T", [G.SKINNY_MAX_M, G.SKINNY_MAX_M + 1])
@pytest.mark.parametrize("small_cus", [32, 64])
def test_small_cus(monkeypatch, small_cus, T):
    """A micro-forward on its CU partition: skinny up to ``SKINNY_MAX_M``
    rows, every GEMM on split-K tiles above."""
    case = _case(T)
    seq = ALL_SKINNY if T <= G.SKINNY_MAX_M else ALL_TILES
    if T > G.SKINNY_MAX_M:
        assert G.split_all(T, NQKV, CFG.dim, small_cus) == 0
    _check_route(monkeypatch, f"small_cus={small_cus}", case, _hip(case), [seq, seq], run={"small_cus": small_cus})


# ------------------------------------------------------------------------------------------ FP8 weights
def _quant_routes():
    out = []
    for place, table, run in (("small", G.FP8_TILE_MIN_M_SMALL, {"quant": True, "small_cus": 64}),
                              ("chip", G.FP8_TILE_MIN_M_CHIP, {"quant": True})):
        for v in sorted(set(table.values())):
            if v <= G.SKINNY_CHUNKED_MAX_M:
                out += [(place, v - 1, run), (place, v, run)]
    return out


QUANT = _quant_routes()


def _quant_layer(table, T):
    tile = {g for g in G.FP8_GEMMS if table[g] <= T}

    def pick(g, tiled, skinny):
        return [tiled if g in tile else skinny]

    return (["row_rms[{T}]"] + pick("qkv", "gemm_fp8[{T}]", "skinny_fp8[store,{T},cus={C}]") + ["rope_kv[{T}]"]
            + pick("o", "gemm_residual_fp8[{M},split=1]", "skinny_fp8[resid,{M},cus={C}]") + ["row_rms[{M}]"]
            + pick("gu", "gemm_swiglu_fp8[{M}]", "skinny_fp8[swiglu,{M},cus={C}]")
            + pick("down", "gemm_residual_fp8[{M},split=1]", "skinny_fp8[resid,{M},cus={C}]"))


@pytest.mark.parametrize("place,T,run", QUANT, ids=[f"{p}-{t}" for p, t, _ in QUANT])
def test_quant_routes(monkeypatch, place, T, run):
    """``quant=True`` just below and at every row count of the ``fp8_plan``
    tables: each GEMM of the layer on ``skinny_fp8`` or the FP8-weight tile
    kernel as its table says; the twin and the reference model compute with
    the decoded codes."""
    case = _case(T)
    hip = _hip(case, small_weights="fp8")
    table = G.FP8_TILE_MIN_M_SMALL if place == "small" else G.FP8_TILE_MIN_M_CHIP
    seq = _quant_layer(table, T)
    _check_route(monkeypatch, f"quant/{place}", case, hip, [seq, seq], run=run)


def test_quant_refuses_more_rows_than_the_fp8_kernel_takes():
    case = _case(G.SKINNY_MAX_M)
    hip = _hip(case, small_weights="fp8")
    T = G.SKINNY_CHUNKED_MAX_M + 1
    z = torch.zeros(T, dtype=torch.int32, device=DEV)
    before = [c.clone() for c in hip.kcache]
    with pytest.raises(ValueError, match="at most"):
        hip.hidden(z.long(), z, z, quant=True)
    assert all(torch.equal(a, b) for a, b in zip(before, hip.kcache))


# ------------------------------------------------------------------------------------------ the library routing
MIN_MLP, MIN_QKV = 48, 80       # min_fused_tokens / min_fused_qkv_tokens of the library models below
LIB_BELOW = QKV_LIB + O_LIB + GU_LIB + O_LIB
LIB_MLP = QKV_LIB + O_LIB + GU_ROWS + O_LIB
LIB_BOTH = QKV_TILE + O_LIB + GU_ROWS + O_LIB
LIBRARY = [(MIN_MLP - 1, LIB_BELOW), (MIN_MLP, LIB_MLP), (MIN_QKV - 1, LIB_MLP), (MIN_QKV, LIB_BOTH)]


@pytest.mark.parametrize("T,seq", LIBRARY, ids=[str(t) for t, _ in LIBRARY])
def test_library_routing(monkeypatch, T, seq):
    """``library_gemm=True`` around ``min_fused_tokens`` and
    ``min_fused_qkv_tokens``: the library's o / down (``addmm_``), ``mlp_up``,
    ``swiglu_rows`` and ``qkv_rope_rows``, every row scale from ``row_rms``
    (nothing carried: ``fused_rms`` is off) and no split plan handed down."""
    case = _case(T)
    hip = _hip(case, library_gemm=True, min_fused_tokens=MIN_MLP, min_fused_qkv_tokens=MIN_QKV)
    assert hip.library_gemm and (hip.min_fused_tokens, hip.min_fused_qkv_tokens) == (MIN_MLP, MIN_QKV)
    _check_route(monkeypatch, "library", case, hip, [seq, seq], split_cus=0)


# ------------------------------------------------------------------------------------------ fused_rms
def _first_full_wave(cus: int) -> int:
    T = 1
    while not G.residual_tiles_ok(T, CFG.dim, cus):
        T += 1
        assert T < 1 << 16
    return T


@pytest.mark.parametrize("fused_rms", [True, False])
def test_fused_rms_chain(monkeypatch, fused_rms):
    """Three layers at the smallest step whose residual tiles fill the chip.
    ``fused_rms``: the o GEMM's row scales feed gate/up, the down GEMM's feed
    the next layer's qkv (one ``row_rms`` in the whole step), and the last
    layer's down projection produces none.  Without it every scale comes
    from ``row_rms``.  At this row count the tile qkv has no ``split_all``
    plan (None)."""
    cus = _cus()
    T = _first_full_wave(cus)
    assert T > 1 and not G.residual_tiles_ok(T - 1, CFG.dim, cus)
    assert G.split_all(T, NQKV, CFG.dim, cus) is None
    case = _case(T, layers=3)
    hip = _hip(case, fused_rms=fused_rms)
    if fused_rms:
        layers = [QKV_TILE + O_RMS + GU_TILE_CARRIED + O_RMS,
                  QKV_TILE_CARRIED + O_RMS + GU_TILE_CARRIED + O_RMS,
                  QKV_TILE_CARRIED + O_RMS + GU_TILE_CARRIED + O_WHOLE]
    else:
        layers = [QKV_TILE + O_WHOLE + GU_TILE + O_WHOLE] * 3
    _check_route(monkeypatch, f"fused_rms={fused_rms}", case, hip, layers)


# ------------------------------------------------------------------------------------------ A/B flags still in the tree
T_FLAG = 72
UNSCALED = ["rmsnorm[{T}]", "qkv_rope[{T},full=None]"] + O_SPLIT + ["rmsnorm[{M}]", "gemm_swiglu[{M}]"] + O_SPLIT
SPLIT_QKV = ["rmsnorm[{T}]", "mm[{T}]", "mm[{T}]", "rope_kv[{T}]"] + O_SK + GU_TILE + O_SK
NORM_KERNELS = ["rmsnorm[{T}]", "rope_kv[{T}]", "rmsnorm[{T}]", "mlp_up[{T}]"]


def test_flag_row_scale_norm_off(monkeypatch):
    """``row_scale_norm=False``: the fused GEMMs over materialised RMSNorm
    rows (unit norm weights: folded)."""
    case = _case(T_FLAG)
    hip = _hip(case, row_scale_norm=False)
    assert bool((hip.layers[0]["attn_norm"] == 1).all())
    _check_route(monkeypatch, "flag/row_scale_norm=False", case, hip, [UNSCALED] * 2)


def test_flag_split_qkv(monkeypatch):
    """``split_qkv=True``: q and kv as two library GEMMs over rows normalised
    with the layer's own, unfolded, norm weight."""
    case = _case(T_FLAG)
    hip = _hip(case, split_qkv=True)
    assert not hip.fused_qkv and not bool((hip.layers[0]["attn_norm"] == 1).all())
    _check_route(monkeypatch, "flag/split_qkv", case, hip, [SPLIT_QKV] * 2)


def test_flag_residual_in_gemm_off(monkeypatch):
    """``residual_in_gemm=False``: library projections and the residual-add
    RMSNorm kernels (the first layer's norm has no residual to add: the
    second layer's first rmsnorm is the previous layer's closing one)."""
    case = _case(T_FLAG)
    hip = _hip(case, residual_in_gemm=False)
    _check_route(monkeypatch, "flag/residual_in_gemm=False", case, hip, [NORM_KERNELS] * 2)


# ------------------------------------------------------------------------------------------ forward against hidden
HEAD_MARGIN = 1e-3               # the argmax head's fp32-accumulation margin (tests/test_gpu_sampling.py)
# the library head under 256 rows takes the argmax of logits rounded to bf16: two logits may each move
# by half a bf16 ulp, at most 2^-8 of their size, before they are compared
LIBRARY_HEAD_MARGIN = HEAD_MARGIN + 2.0 ** -7
FORWARD = [
    ("skinny", G.SKINNY_MAX_M, {}, {}, HEAD_MARGIN),
    ("tiles", T_ABOVE, {}, {}, HEAD_MARGIN),
    ("tiles-unpruned", T_ABOVE, {"prune_last": False}, {}, HEAD_MARGIN),
    ("library", MIN_QKV, {"library_gemm": True, "min_fused_tokens": MIN_MLP, "min_fused_qkv_tokens": MIN_QKV}, {},
     LIBRARY_HEAD_MARGIN),
    ("quant", max(G.FP8_TILE_MIN_M_CHIP["gu"], G.SKINNY_MAX_M + 1), {"small_weights": "fp8"}, {"quant": True},
     HEAD_MARGIN),
]


@pytest.mark.parametrize("name,T,build,run,margin", FORWARD, ids=[f[0] for f in FORWARD])
def test_forward_is_the_argmax_of_its_hidden_rows(name, T, build, run, margin):
    """``forward`` returns the argmax of the float64 logits of the model's
    own ``hidden`` rows (pruned to the sampled rows where ``forward``
    prunes, selected from every row where it does not), wherever the top-2
    gap exceeds the head's margin times ``max|logit|`` of the row: the
    ``prune_last`` / ``index_select`` split and the head's ``min_rows``
    choice (the argmax epilogue at any row count without the library, the
    library's bf16 logits under 256 rows with it)."""
    case = _case(T)
    hip = _hip(case, **build)
    s1, s2 = (s.to(DEV) for s in case.steps)
    clear = 0
    for st in (s1, s2):
        kw = dict(tiles=st.tiles, n_dec=st.n_dec, **run)
        assert 0 < st.rows.numel() < st.tokens.numel()
        ids = hip.forward(*st.args, st.rows, **kw)
        if hip.prune_last:
            h = hip.hidden(*st.args, rows=st.rows, **kw)
        else:
            h = hip.hidden(*st.args, **kw).index_select(0, st.rows)
        logits = h.double() @ hip.lm_head.double().t()
        top = torch.topk(logits, 2, dim=-1)
        ok = (top.values[:, 0] - top.values[:, 1]) > margin * logits.abs().max(dim=-1).values
        clear += int(ok.sum())
        assert ids.dtype == torch.int32 and ids.shape == (st.rows.numel(),)
        assert torch.equal(ids.long()[ok], top.indices[:, 0][ok])
    assert clear >= (s1.rows.numel() + s2.rows.numel()) // 2
