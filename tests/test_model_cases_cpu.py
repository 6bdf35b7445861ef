"""The trunk cases of ``tests/model_cases.py`` on the CPU: the float64 twin
against the ``RefOps`` trunk, and that every wiring mutation of the twin is
visible in the measure ``tests/test_gpu_model_routes.py`` uses.

**B** is the largest per-row relative rms error of the ``RefOps`` trunk
against the twin, ``rms(h_ref - h_64) / rms(h_64)``, over every row of every
step: the reference path's own rounding error (bf16 at every place the HIP
routes round too).
"""
import pytest
import torch

import model_cases as MC
from llm_message_queue_amd.models.llama_stub import LlamaConfig, LlamaStub

CFG = LlamaConfig(vocab=512, dim=512, layers=2, heads=4, kv_heads=2, ffn=512)
T = 61
Q_GAIN = 8.0
# Every mutation must move a row by at least this many B.  A condition on
# the inputs: a case that misses it is changed, never the factor.
MIN_MUTATION = 4.0
# An upper limit for B itself from the number formats: a row passes about
# eight bf16 roundings a layer (qkv, q/k after RoPE, the attention output,
# the residual twice, the activation, the final norm), each a relative rms
# error of about 2^-9 / sqrt(3) = 1.1e-3 against values of the row's own
# size; sixteen of them add to about 4.5e-3 and the residual's cancellation
# can double that.  A cache mix-up in the twin is 80 B and more.
B_MAX = 2e-2


def _model(**kw):
    return LlamaStub(CFG, slots=MC.SLOTS, max_ctx=_case().max_ctx, device="cpu", impl="ref", fused_mlp=True,
                     fused_qkv=True, min_fused_tokens=1, min_fused_qkv_tokens=1, **kw)


_CACHE = {}


def _case():
    if "case" not in _CACHE:
        _CACHE["case"] = MC.make_case(CFG, T, layers=2, seed=3, q_gain=Q_GAIN)
    return _CACHE["case"]


def _base():
    """(model, RefOps hidden per step, twin hidden per step, per-row errors, B, score std), computed once."""
    if "base" not in _CACHE:
        case = _case()
        m = MC.install(_model(), case)
        ref = MC.run_steps(m, case)
        stats = {}
        h64 = MC.twin(m, case, stats=stats)
        errs = [MC.row_errors(a, b) for a, b in zip(ref, h64)]
        _CACHE["base"] = (m, ref, h64, errs, max(float(e.max()) for e in errs), MC.score_std(stats))
    return _CACHE["base"]


def test_case_layout():
    case = _case()
    s1, s2 = case.steps
    assert s2.tokens.numel() == T and s2.n_dec == 2
    slots1, slots2 = s1.slot.tolist(), s2.slot.tolist()
    order = list(dict.fromkeys(slots1 + slots2))
    assert order != sorted(order) and sorted(order) != list(range(len(order)))     # not in row order, not contiguous
    assert set(slots1) - set(slots2)                                               # a slot step 2 leaves alone
    assert (s2.tiles[:s2.n_dec, 1] == 1).all() and (s2.tiles[:s2.n_dec, 3] > 0).all()
    cont = [(sl, p) for sl, p in zip(slots2, s2.pos.tolist()) if sl == 6]
    assert cont[0][1] == 5 and cont[-1][1] >= 32                                  # continues step 1, crosses 32 keys
    big = MC.make_case(CFG, 130)
    assert max(p for sl, p in zip(big.steps[1].slot.tolist(), big.steps[1].pos.tolist()) if sl == 6) >= 64
    # the sampled rows are not only the chunks' last rows
    ends = {int(t[0] + t[1] - 1) for t in s2.tiles}
    assert set(s2.rows.tolist()) - ends
    assert int(s2.slot[case.mut_row]) == 6 and int(s2.pos[case.mut_row]) > 0
    assert MC.spread_rows(10, 10) == list(range(10)) and MC.spread_rows(10, 0) == []
    assert MC.spread_rows(513, 5) == [0, 128, 256, 384, 512]


def test_install_gives_the_model_its_own_layout():
    case = _case()
    m = MC.install(_model(), case)
    raw = MC._raw_weights(case, m.device)
    for L, R in zip(m.layers, raw["layers"]):
        assert not bool((R["attn_norm"] == 1).all()) and bool((L["attn_norm"] == 1).all())
        assert bool((L["mlp_norm"] == 1).all())
        assert torch.equal(L["wqkv"], (R["wqkv"].float() * R["attn_norm"].float()[None]).to(torch.bfloat16))
        assert torch.equal(MC.G.swiglu_unpermute(L["w_gu"]),
                           (R["w_gu"].float() * R["mlp_norm"].float()[None]).to(torch.bfloat16))
    assert not bool((m.final_norm == 1).all())
    plain = MC.install(LlamaStub(CFG, slots=MC.SLOTS, max_ctx=case.max_ctx, device="cpu", impl="ref"), case)
    for L, R in zip(plain.layers, raw["layers"]):                                   # unfused: nothing folded
        assert torch.equal(L["attn_norm"], R["attn_norm"]) and torch.equal(L["wqkv"], R["wqkv"])
        assert torch.equal(L["mlp_norm"], R["mlp_norm"]) and torch.equal(L["w_gu"], R["w_gu"])
    q = MC.install(_model(small_weights="fp8"), case)
    for L in q.layers:
        for k in MC.QUANT_NAMES:
            codes, scale = q._quantize(L[k])
            assert torch.equal(L["fp8"][k][0], codes) and torch.equal(L["fp8"][k][1], scale)
    # the folded and the unfolded model are the same function: their twins agree to the fold's bf16 rounding
    a, b = MC.twin(m, case)[1], MC.twin(plain, case)[1]
    assert float(MC.row_errors(a, b).max()) < _base()[4]


def test_attention_scores_are_spread():
    std = _base()[5]
    print(f"attention score std {std:.3f}")
    assert 1.0 <= std <= 4.0


def test_twin_agrees_with_refops_over_two_steps():
    """Step 2 reads the K/V step 1 wrote (two decode rows and a continued
    chunk): the ``RefOps`` trunk stays within the rounding limit ``B_MAX`` of
    the twin on both steps, and the rows that read the carried cache are no
    worse than twice the rows of step 1, which read none."""
    _, _, _, errs, B, _ = _base()
    print(f"B = {B:.3e}; step 1 max {float(errs[0].max()):.3e}, step 2 max {float(errs[1].max()):.3e}")
    assert B <= B_MAX
    assert float(errs[1].max()) <= 2 * float(errs[0].max())


@pytest.mark.parametrize("mutation", MC.MUTATIONS)
def test_every_mutation_moves_a_row(mutation):
    m, _, h64, _, B, _ = _base()
    got = MC.twin(m, _case(), mutate=mutation)
    moved = max(float(MC.row_errors(a, b).max()) for a, b in zip(got, h64))
    print(f"{mutation}: {moved / B:.1f} B")
    assert moved >= MIN_MUTATION * B


def test_refops_trunk_tiles_and_rows():
    """The ``RefOps`` trunk with the case's ``tiles`` / ``n_dec`` equals
    per-token attention bit for bit (the same operations in the same order).
    ``rows=`` pruning against ``index_select`` of the full result is the same
    arithmetic, but the last layer's three fp32 GEMMs then run over 8 rows
    instead of 61, and a CPU BLAS does not promise one summation order for
    both: an fp32 sum that moves by its last bits (K * 2^-24 of its size,
    about 3e-5 at K = 512) turns one bf16 rounding in about a hundred (a
    bf16 step is 2^-8).  So: no element apart by more than two bf16 steps of
    its size, at most one element in twenty apart at all."""
    m, ref, _, _, _, _ = _base()
    case = _case()
    MC.install(m, case)
    tokens = MC.run_steps(m, case, attention="tokens")
    for a, b in zip(ref, tokens):
        assert torch.equal(a, b)
    MC.install(m, case)
    s1, s2 = case.steps
    m.hidden(*s1.args, tiles=s1.tiles, n_dec=s1.n_dec)
    assert 0 < s2.rows.numel() < T
    pruned = m.hidden(*s2.args, tiles=s2.tiles, n_dec=s2.n_dec, rows=s2.rows).float()
    want = ref[1].index_select(0, s2.rows).float()
    apart = (pruned - want).abs()
    print(f"rows=: {int((apart != 0).sum())} of {apart.numel()} elements apart, max {float(apart.max()):.3e}")
    assert bool((apart <= 2 * 2.0 ** -7 * torch.maximum(pruned.abs(), want.abs())).all())
    assert int((apart != 0).sum()) <= apart.numel() // 20
    every = m.hidden(*s2.args, tiles=s2.tiles, n_dec=s2.n_dec, rows=torch.arange(T))
    assert torch.equal(every, ref[1])                                            # every row sampled: the full run
