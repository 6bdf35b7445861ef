"""The kernel calls of ``LlamaStub.hidden`` / ``forward``, route by route,
against a recorded run -- on the CPU, with every entry point faked.

``tests/test_gpu_model_routes.py`` proves on the GPU that each route computes
the right numbers and witnesses its call sequence at the thresholds of the
chip it runs on.  This file pins the routing itself, everywhere: a grid over
the row count, the CU count, ``small_cus``, ``quant``, ``rows=`` and the
routing flags, each run's exact sequence of calls compared with
``tests/golden/trunk_routes.json``.

The model is built on the CPU with the reference ops at dims the kernels'
shape checks accept (dim 512, 4 query heads, 1 kv head: qkv is 768 wide and
K = 512 splits), then told it is the HIP model by assignment (``impl``,
``_cus``, ``library_gemm``).  Every entry point the GPU witness wraps -- the
``ops.gemm`` GEMMs, the ops' norm / rope / attention / row-GEMM methods,
``Tensor.addmm_``, ``torch.mm`` -- and ``F.linear`` and ``greedy_head`` is
replaced by a fake that records its name, its row count and the arguments a
route decides (epilogue, ``cus=``, ``split=``, ``full=``, whether a row scale
or a residual was passed, the head's ``min_rows``) and returns an
uninitialised tensor of the right shape.  No arithmetic runs, so nothing
here depends on values.

The file uses only what a restructuring of the routing leaves alone: the
constructor, ``hidden`` / ``forward``, the attributes above, the entry
points' names and signatures, and that the trunk iterates ``model.layers``
once per layer (a marker there cuts a run's calls into layers).  So it
passes unchanged before and after one, and the fixture is what the tree
before it records:

    python tests/test_trunk_routes_golden.py --write

Row counts are stored as ``T`` (the step's rows) or ``M`` (the sampled rows)
and each distinct per-layer sequence once, so the fixture stays small.

Where the tree has the pure plan (``models.routes``) the same grid also
proves that its declared kinds are exactly the reachable ones.
"""
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from llm_message_queue_amd.models import llama_stub as LS
from llm_message_queue_amd.models.llama_stub import LlamaConfig, LlamaStub
from llm_message_queue_amd.ops import gemm as G

try:
    from llm_message_queue_amd.models import routes as R
except ImportError:          # a tree whose trunk routes inline: it records the fixture, it has no kinds to compare
    R = None

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunk_routes.json")
CFG = LlamaConfig(vocab=256, dim=512, layers=3, heads=4, kv_heads=1, ffn=512)
NQ = CFG.heads * CFG.head_dim
EPI = {G.SK_STORE: "store", G.SK_RESID: "resid", G.SK_SWIGLU: "swiglu"}
CUS = (8, 64)
SMALL_CUS = (0, 8, 32)
MIN_MLP, MIN_QKV = 48, 80


def _first_full_wave(cus: int) -> int:
    T = 1
    while not G.residual_tiles_ok(T, CFG.dim, cus):
        T += 1
    return T


def _around(*vs):
    return [v + d for v in vs for d in (-1, 0, 1)]


THRESHOLDS = sorted({1, *_around(G.SKINNY_MAX_M, G.SKINNY_PROJ_MAX_M, G.SKINNY_RESID_MAX_M, G.SKINNY_CHUNKED_MAX_M),
                     *(_first_full_wave(c) for c in CUS)})
FP8_ROWS = sorted({v + d for t in (G.FP8_TILE_MIN_M_SMALL, G.FP8_TILE_MIN_M_CHIP) for v in t.values()
                   for d in (-1, 0)})
ALL_T = sorted({*THRESHOLDS, *FP8_ROWS})
LIBRARY_T = sorted({MIN_MLP - 1, MIN_MLP, MIN_QKV - 1, MIN_QKV, *THRESHOLDS})
ROWS_T = (G.SKINNY_MAX_M + 1, G.SKINNY_RESID_MAX_M + 1, _first_full_wave(CUS[0]))

# name -> (constructor arguments, library_gemm asked for, module globals to set)
SETTINGS = {
    "default": ({}, False, {}),
    "library": (dict(min_fused_tokens=MIN_MLP, min_fused_qkv_tokens=MIN_QKV), True, {}),
    "fused_rms": (dict(fused_rms=True), False, {}),
    "row_scale_norm=0": (dict(row_scale_norm=False), False, {}),
    "split_qkv": (dict(split_qkv=True), False, {}),
    "residual_in_gemm=0": (dict(residual_in_gemm=False), False, {}),
    "fused_mlp=0": (dict(fused_mlp=False), False, {}),
    "fused_qkv=0": (dict(fused_qkv=False), False, {}),
    "fused_resid=0": (dict(fused_resid=False), False, {}),
    "prune_last=0": (dict(prune_last=False), False, {}),
    "resid_epi=regs,fused_rms": (dict(fused_rms=True), False, {"RESID_EPI": G.EPI_RESID}),
}


def _model(cus: int, quant: bool, ctor: dict, library: bool) -> LlamaStub:
    """The HIP model's flags on a CPU model: built on the reference ops with
    the defaults ``impl="hip"`` would give, then ``impl`` and what the
    constructor derives from it and from the device assigned."""
    kw = dict(fused_mlp=True, fused_head=True, fused_resid=True)
    kw.update(ctor)
    kw.setdefault("fused_qkv", not kw.get("split_qkv", False))
    m = LlamaStub(CFG, slots=1, max_ctx=8, device="cpu", impl="ref", small_weights="fp8" if quant else "bf16", **kw)
    m.impl = "hip"
    m.library_gemm = library or not m.fused_resid
    m._cus = cus if m.fused_resid else 0
    snapshot = getattr(m, "_route_flags", None)     # a tree that reads its flags once, at construction
    if snapshot is not None:
        m.route_flags = snapshot()
    return m


class Recorder:
    """Recording fakes in place of every entry point of the trunk."""

    def __init__(self, mp, ops_cls):
        self.calls, self.kinds = [], {"qkv": set(), "resid": set(), "gu": set()}

        def rec(name, x, args="{n}"):                    # ``{n}``: where the row count of ``x`` goes
            self.calls.append((name, x.shape[0], args))

        def rs(row_scale):
            return ",rs" if row_scale is not None else ""

        def sk(name, at):
            def fake(*a, **k):
                rec(name, a[0], f"{EPI[a[at]]},{{n}},cus={k.get('cus')}{rs(k.get('row_scale'))}")
                return a[at - 1]
            mp.setattr(G, name, fake)

        sk("skinny", 3)
        sk("skinny_fp8", 4)

        def gemm_residual(x, w, res, split_cus=0):
            rec("gemm_residual", x, f"{{n}},split={split_cus}")
            return res

        def gemm_residual_fp8(x, codes, scale, res, split_cus=0):
            rec("gemm_residual_fp8", x, f"{{n}},split={split_cus}")
            return res

        def gemm_residual_rms(x, w, res, eps):
            rec("gemm_residual_rms", x, f"{{n}}")
            return torch.empty(G.row_scale_len(x.shape[0]), dtype=torch.float32)

        def gemm_swiglu(x, w, out=None, row_scale=None, split_cus=0):
            rec("gemm_swiglu", x, f"{{n}},split={split_cus}{rs(row_scale)}")
            return torch.empty((x.shape[0], w.shape[0] // 2), dtype=x.dtype)

        def gemm_fp8(x, codes, scale, out=None, row_scale=None, split_cus=0):
            rec("gemm_fp8", x, f"{{n}},split={split_cus}{rs(row_scale)}")
            return out

        def gemm_swiglu_fp8(x, codes, scale, out=None, row_scale=None, split_cus=0):
            rec("gemm_swiglu_fp8", x, f"{{n}},split={split_cus}{rs(row_scale)}")
            return out

        def qkv_rope(x, wqkv, *a, **k):
            rec("qkv_rope", x, f"{{n}},full={k.get('split_full')}{rs(k.get('row_scale'))}")
            return torch.empty((x.shape[0], NQ), dtype=x.dtype)

        for f in (gemm_residual, gemm_residual_fp8, gemm_residual_rms, gemm_swiglu, gemm_fp8, gemm_swiglu_fp8,
                  qkv_rope):
            mp.setattr(G, f.__name__, f)

        def rmsnorm(self, x, w, eps, residual=None, out=None):
            rec("rmsnorm", x, f"{{n}}{',residual' if residual is not None else ''}")
            return torch.empty_like(x)

        def row_rms(self, x, eps):
            rec("row_rms", x, f"{{n}}")
            return torch.empty(G.row_scale_len(x.shape[0]), dtype=torch.float32)

        def rope_kv(self, qkv, *a, **k):
            rec("rope_kv", qkv, f"{{n}}")
            return torch.empty((qkv.shape[0], NQ), dtype=qkv.dtype)

        def qkv_rope_rows(self, x, wqkv, r, *a, **k):
            rec("qkv_rope_rows", x, f"{{n}},full={k.get('split_full')}")
            return torch.empty((x.shape[0], NQ), dtype=x.dtype)

        def swiglu_rows(self, x, w_perm, r):
            rec("swiglu_rows", x, f"{{n}}")
            return torch.empty((x.shape[0], w_perm.shape[0] // 2), dtype=x.dtype)

        def mlp_up(self, x, w_gu, fused, min_fused_tokens):
            rec("mlp_up", x, f"{{n}},fused={int(fused)},min={min_fused_tokens}")
            return torch.empty((x.shape[0], w_gu.shape[0] // 2), dtype=x.dtype)

        def attention(self, q, *a, **k):
            rec("attention", q, f"{{n}}")
            return torch.empty_like(q)

        def attention_tiles(self, q, *a, **k):
            rec("attention_tiles", q, f"{{n}}")
            return torch.empty_like(q)

        def greedy_head(self, x, w, fused=True, min_rows=256):
            rec("greedy_head", x, f"{{n}},fused={int(fused)},min_rows={min_rows}")
            return torch.empty(x.shape[0], dtype=torch.int32)

        for f in (rmsnorm, row_rms, rope_kv, qkv_rope_rows, swiglu_rows, mlp_up, attention, attention_tiles,
                  greedy_head):
            mp.setattr(ops_cls, f.__name__, f)

        def addmm_(self, x, wt):
            rec("addmm_", self, f"{{n}}")
            return self

        def mm(x, w, out=None):
            rec("mm", x, f"{{n}}")
            return out

        def linear(x, w):
            rec("linear", x, f"{{n}}")
            return torch.empty((x.shape[0], w.shape[0]), dtype=x.dtype)

        mp.setattr(torch.Tensor, "addmm_", addmm_)
        mp.setattr(torch, "mm", mm)
        mp.setattr(LS.F, "linear", linear)

        if R is not None:
            plan_qkv, plan_block = R.plan_qkv, R.plan_block

            def seen_qkv(*a, **k):
                p = plan_qkv(*a, **k)
                self.kinds["qkv"].add(p.kind)
                return p

            def seen_block(*a, **k):
                p = plan_block(*a, **k)
                self.kinds["resid"] |= {p.o.kind, p.down.kind}
                self.kinds["gu"].add(p.gu.kind)
                return p

            mp.setattr(R, "plan_qkv", seen_qkv)
            mp.setattr(R, "plan_block", seen_block)


class _Marked(list):
    """``model.layers`` that notes every layer the trunk starts."""

    def __init__(self, layers, rec):
        super().__init__(layers)
        self._rec = rec

    def __iter__(self):
        for L in list.__iter__(self):
            self._rec("|")
            yield L


def _run(model, rec, T, rows, small_cus, quant):
    """One step's calls, by layer (the last with the final norm and the head
    behind it), row counts named: ``rows`` "-" is ``hidden`` without
    ``rows=``, else ``forward`` sampling 5 rows, every row or none."""
    tokens = torch.zeros(T, dtype=torch.int64)
    pos = slot = torch.zeros(T, dtype=torch.int32)
    del rec.calls[:]
    run = dict(small_cus=small_cus, quant=quant)
    if rows == "-":
        M = T
        model.hidden(tokens, pos, slot, **run)
    else:
        idx = {"5": torch.arange(0, T, max(1, T // 5))[:5], "all": torch.arange(T),
               "none": torch.empty(0, dtype=torch.int64)}[rows]
        M = idx.numel()
        model.forward(tokens, pos, slot, idx, **run)

    def rows_name(n):
        return "T" if n == T else "M" if n == M else str(n)

    layers, first = [[]], True                          # calls ahead of the first layer count with it
    for c in rec.calls:
        if c == "|":
            if not first:
                layers.append([])
            first = False
        else:
            name, n, args = c
            layers[-1].append(f"{name}[{args.format(n=rows_name(n))}]")
    return [" ".join(seq) for seq in layers]


def _grid():
    """(key, setting, cus, small_cus, quant, T, rows) of every run."""
    out = []
    for name in SETTINGS:
        for cus in CUS:
            if name == "default":
                runs = [(T, "-", s, q) for T in ALL_T for s in SMALL_CUS for q in (False, True)
                        if not q or T <= G.SKINNY_CHUNKED_MAX_M]
                runs += [(T, r, s, q) for T in ROWS_T for r in ("5", "all", "none") for s in SMALL_CUS
                         for q in (False, True)]
            elif name == "prune_last=0":
                runs = [(T, "5", s, False) for T in ROWS_T for s in (0, 32)]
            else:
                runs = [(T, "-", s, False) for T in (LIBRARY_T if name == "library" else THRESHOLDS)
                        for s in (0, 32)]
                runs += [(T, "5", 0, False) for T in ROWS_T]
            for T, rows, s, q in runs:
                out.append((f"{name}|cus={cus}|small_cus={s}|quant={int(q)}|T={T}|rows={rows}",
                            name, cus, s, q, T, rows))
    return out


def _record():
    """Run the grid: ({key: [per-layer sequences]}, kinds seen by GEMM)."""
    grid = _grid()
    models = {}
    for _, name, cus, _, q, _, _ in grid:                # built before the fakes go in
        if (name, cus, q) not in models:
            models[name, cus, q] = _model(cus, q, *SETTINGS[name][:2])
    runs = {}
    with pytest.MonkeyPatch.context() as mp:
        rec = Recorder(mp, type(models["default", CUS[0], False].ops))
        for m in models.values():
            m.layers = _Marked(m.layers, rec.calls.append)
        for key, name, cus, s, q, T, rows in grid:
            with pytest.MonkeyPatch.context() as mp_run:
                for g, v in SETTINGS[name][2].items():
                    mp_run.setattr(G, g, v)
                runs[key] = _run(models[name, cus, q], rec, T, rows, s, q)
    return runs, rec.kinds


def _packed(runs: dict) -> dict:
    seqs = sorted({s for layers in runs.values() for s in layers})
    at = {s: i for i, s in enumerate(seqs)}
    return {"layers": seqs, "runs": {k: [at[s] for s in v] for k, v in runs.items()}}


@pytest.fixture(scope="module")
def recorded():
    return _record()


def test_call_sequences_match_the_recorded_ones(recorded):
    runs, _ = recorded
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(runs) == sorted(gold["runs"])
    for key, layers in runs.items():
        assert layers == [gold["layers"][i] for i in gold["runs"][key]], key


def test_the_grid_reaches_every_route():
    """The fixture itself: every entry point the fakes replace is called in
    some run, with and without a split plan, a carried scale and a residual."""
    with open(GOLDEN) as f:
        layers = json.load(f)["layers"]
    text = " ".join(layers)
    for call in ("skinny[store", "skinny[resid", "skinny[swiglu", "skinny_fp8[store", "skinny_fp8[resid",
                 "skinny_fp8[swiglu", "gemm_fp8[", "gemm_swiglu_fp8[", "gemm_residual_fp8[",
                 "gemm_residual[T,split=0]", "gemm_residual[T,split=8]", "gemm_residual_rms[", "addmm_[",
                 "gemm_swiglu[T,split=0]", "gemm_swiglu[T,split=8,rs]", "swiglu_rows[", "mlp_up[T,fused=1",
                 "mlp_up[T,fused=0", "qkv_rope_rows[T,full=0]", "qkv_rope_rows[T,full=None]", "qkv_rope[T,full=None]",
                 "mm[", "linear[", "rmsnorm[T,residual]", "min_rows=1]", "min_rows=256]"):
        assert call in text, call
    # carried row scales: a middle layer whose tile qkv and gate/up have no row_rms before them,
    # and a last layer whose down projection makes none
    assert "qkv_rope_rows[T,full=None] attention[T] gemm_residual_rms[T] gemm_swiglu[T,split=8,rs] " \
           "gemm_residual_rms[T]" in layers
    assert "qkv_rope_rows[T,full=None] attention[T] gemm_residual_rms[T] gemm_swiglu[T,split=8,rs] " \
           "gemm_residual[T,split=0] rmsnorm[T]" in layers


def test_every_declared_kind_is_reached_and_no_other(recorded):
    """The kinds the plan returned over the grid are the plan module's
    declared kinds, GEMM by GEMM: a kind that can no longer be reached has to
    leave the declaration."""
    if R is None:
        return
    _, kinds = recorded
    assert kinds["qkv"] == set(R.QKV_KINDS)
    assert kinds["resid"] == set(R.RESID_KINDS)
    assert kinds["gu"] == set(R.GU_KINDS)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_trunk_routes_golden.py --write")
    packed = _packed(_record()[0])
    with open(GOLDEN, "w") as f:
        json.dump(packed, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(packed['runs'])} runs, {len(packed['layers'])} distinct layer sequences -> {GOLDEN}")
