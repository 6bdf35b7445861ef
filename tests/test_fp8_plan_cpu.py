"""The FP8 kernel choice of a quant forward (``ops.gemm.fp8_plan``), the
argument checks of the FP8-weight tile wrappers that need no device, and the
reference path's independence of the plan -- all on the CPU."""
import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import quant as Q


@pytest.mark.parametrize("small", [True, False])
@pytest.mark.parametrize("gemm", ["qkv", "o", "gu", "down"])
def test_plan_is_monotone_bounded_and_follows_the_constants(gemm, small):
    table = G.FP8_TILE_MIN_M_SMALL if small else G.FP8_TILE_MIN_M_CHIP
    assert set(table) == set(G.FP8_GEMMS) == {"qkv", "o", "gu", "down"}
    thr = table[gemm]
    assert isinstance(thr, int) and thr >= 65                 # the graph buckets stop at 64 rows
    plans = [G.fp8_plan(M, gemm, small) for M in range(1, G.SKINNY_CHUNKED_MAX_M + 200)]
    assert set(plans) <= {"skinny", "tile"}
    assert all(p == "skinny" for p in plans[:64])
    assert all(p == "skinny" for p in plans[G.SKINNY_CHUNKED_MAX_M:])          # never a tile past 1,024 rows
    inside = plans[:G.SKINNY_CHUNKED_MAX_M]
    first = inside.index("tile") if "tile" in inside else len(inside)
    assert all(p == "tile" for p in inside[first:])           # monotone in M up to the limit
    assert first + 1 == min(thr, G.SKINNY_CHUNKED_MAX_M + 1)


def test_plan_never_leaves_the_skinny_kernel_at_graph_sizes(monkeypatch):
    """Whatever the constants say, M <= 64 stays on the skinny kernel."""
    monkeypatch.setattr(G, "FP8_TILE_MIN_M_SMALL", {g: 1 for g in G.FP8_GEMMS})
    monkeypatch.setattr(G, "FP8_TILE_MIN_M_CHIP", {g: 80 for g in G.FP8_GEMMS})
    assert [G.fp8_plan(M, "qkv", True) for M in (1, 64, 65, 1024, 1025)] == \
        ["skinny", "skinny", "tile", "tile", "skinny"]
    assert [G.fp8_plan(M, "down", False) for M in (64, 79, 80, 1024, 1025)] == \
        ["skinny", "skinny", "tile", "tile", "skinny"]
    with pytest.raises(ValueError):
        G.fp8_plan(100, "lm_head", True)


def test_limits_the_plan_rests_on():
    assert G.SKINNY_MAX_M == 64 and G.SKINNY_CHUNKED_MAX_M == 1024


def test_wrappers_refuse_bad_operands_without_a_device():
    """Every check that comes before the native module is asked for."""
    x = torch.zeros(4, 512, dtype=torch.bfloat16)
    codes = torch.zeros(256, 512, dtype=torch.uint8)
    cs = torch.ones(256)
    out = torch.zeros(4, 256, dtype=torch.bfloat16)
    bad = (ValueError, TypeError)
    for fn in (G.gemm_fp8, G.gemm_swiglu_fp8):
        with pytest.raises(bad):
            fn(x.float(), codes, cs)
        with pytest.raises(bad):
            fn(x, codes.view(torch.int8), cs)
        with pytest.raises(bad):
            fn(x, codes.t().contiguous().t(), cs)
        with pytest.raises(bad):
            fn(x, codes, cs[:128])
        with pytest.raises(bad):
            fn(x, codes, cs.double())
        with pytest.raises(bad):
            fn(x, codes[:, :384].contiguous(), cs)            # inner dimensions differ
        with pytest.raises(bad):
            fn(x[:, :192].contiguous(), codes[:, :192].contiguous(), cs)       # K % 128
        with pytest.raises(bad):
            fn(x, codes[:128].contiguous(), cs[:128].contiguous())             # N % 256
        with pytest.raises(bad):
            fn(x, codes, cs, out=torch.zeros(4, 384, dtype=torch.bfloat16))
        with pytest.raises(bad):
            fn(x, codes, cs, row_scale=torch.ones(4))         # not whole 256-row tiles
    with pytest.raises(bad):
        G.gemm_residual_fp8(x, codes, cs, out[:, :128])
    with pytest.raises(bad):
        G.gemm_residual_fp8(x, codes, cs, out, row_scale=torch.ones(256))


# ---------------------------------------------------------------------- engine (reference ops)
def _engine(mode, **kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=8, max_ctx=64, token_budget=32, device="cpu", impl="ref", seed=3,
                         realtime_mode=mode, micro_slots=4, **kw)


def _requests(n=8, seed=0, gen=3):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(seed)
    return [Request(req_id=i, prompt=rng.integers(0, 1000, size=24 + i % 5).astype(np.int32), gen_tokens=gen,
                    tier=i % 2) for i in range(n)]


def _serve(eng, reqs):
    got = {}
    pend = list(reqs)
    for _ in range(200):
        if not pend and not eng.active and not eng.queued_steps():
            break
        adm = eng.admit(pend)
        ids = {id(r) for r in adm}
        pend = [r for r in pend if id(r) not in ids]
        eng.launch()
        eng.pump_micro()
        for r in eng.finish(block=True).completed:
            got[r.req_id] = (r.out_tokens.tolist(), r.micro)
    return got


def test_reference_path_ignores_the_plan(monkeypatch):
    """``impl="ref"`` with ``micro_weights="fp8"`` computes on the decoded
    weights whatever ``fp8_plan`` says: with every threshold at 65 (the
    micro-forwards here carry ~100 prefill rows) the tokens are those of the
    default constants, and the micro pool's are those of a model holding the
    requantised weights."""
    from llm_message_queue_amd.models.llama_stub import QUANT_NAMES
    base = _serve(_engine("micro", micro_weights="fp8"), _requests())
    monkeypatch.setattr(G, "FP8_TILE_MIN_M_SMALL", {g: 65 for g in G.FP8_GEMMS})
    monkeypatch.setattr(G, "FP8_TILE_MIN_M_CHIP", {g: 65 for g in G.FP8_GEMMS})
    low = _serve(_engine("micro", micro_weights="fp8"), _requests())
    assert sorted(base) == list(range(8)) and low == base
    assert all(len(ids) == 3 for ids, _ in base.values())
    deq = _engine("off")
    for L in deq.model.layers:
        for k in QUANT_NAMES:
            L[k] = Q.requantized(L[k])
    want = _serve(deq, _requests())
    micro = [k for k, v in base.items() if v[1]]
    assert len(micro) >= 4
    for k in micro:
        assert base[k][0] == want[k][0], k
