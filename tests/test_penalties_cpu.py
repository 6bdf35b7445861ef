"""Presence / frequency / repetition penalties without a GPU: the numpy twin
of ``csrc/kernels/penalty_kernels.h`` on hand-made rows, the parser, the
dispatch descriptor, the HTTP route and the router's lenient path, and the CPU
reference engine's device-side history window."""
import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import sampling as S

V = 16


def _row(vals):
    return S.bf16_bits(np.asarray(vals, dtype=np.float32))


def _edit(vals, h, n_p, pp, fp, rp, vocab=V):
    return S.bf16_values(S.penalise_reference(_row(vals), vocab, h, n_p, pp, fp, rp))


def _f32(x):
    return np.float32(x)


# --------------------------------------------------------------------------- the twin
def test_prompt_only_generated_only_and_both():
    base = np.full(V, 4.0, dtype=np.float32)
    # id 1: prompt only; id 2: generated only; id 3: both; id 4: generated three times
    h, n_p = [1, 3, 2, 3, 4, 4, 4], 2
    pp, fp, rp = 0.5, 0.25, 2.0
    out = _edit(base, h, n_p, pp, fp, rp)
    assert out[1] == 2.0                                              # rp alone
    assert out[2] == 4.0 / 2 - 0.25 * 1 - 0.5                         # all three
    assert out[3] == 4.0 / 2 - 0.25 * 1 - 0.5                         # the prompt occurrence counts for rp only
    assert out[4] == 4.0 / 2 - 0.25 * 3 - 0.5                         # counts above 1; presence once
    untouched = np.setdiff1d(np.arange(V), [1, 2, 3, 4])
    assert (out[untouched] == 4.0).all()
    # without rp a prompt-only token keeps its bits
    out = _edit(base, h, n_p, pp, fp, 1.0)
    assert out[1] == 4.0 and out[3] == 4.0 - 0.25 - 0.5


def test_repetition_on_positive_zero_and_negative_logits():
    vals = np.zeros(V, dtype=np.float32)
    vals[[1, 2, 3]] = [3.0, 0.0, -3.0]
    out = _edit(vals, [1, 2, 3], 3, 0.0, 0.0, 1.5)
    assert out.tolist()[1:4] == [2.0, 0.0, -4.5]                      # a positive logit divided, the rest multiplied
    out = _edit(vals, [1, 2, 3], 3, 0.0, 0.0, 0.5)                    # below 1: a reward
    assert out.tolist()[1:4] == [6.0, 0.0, -1.5]
    out = _edit(vals, [1, 2, 3], 0, -1.0, 0.0, 1.0)                   # a negative presence penalty raises
    assert out.tolist()[1:4] == [4.0, 1.0, -2.0]


def test_ids_outside_the_vocabulary_are_ignored():
    ld = 24
    rng = np.random.default_rng(0)
    bits = _row(rng.standard_normal(ld))
    out = S.penalise_reference(bits, V, [-1, V, V + 3, 2 ** 31 - 1], 1, 1.0, 1.0, 1.5)
    assert np.array_equal(out, bits)
    out = S.penalise_reference(bits, V, [-1, 5, V, V + 3, 5], 0, 1.0, 1.0, 1.5)
    assert np.array_equal(np.flatnonzero(out != bits), [5])           # padding and every other column keep their bits


def test_non_finite_logits_at_history_columns():
    vals = np.ones(V, dtype=np.float32)
    vals[[1, 2, 3]] = [np.inf, -np.inf, np.nan]
    out = _edit(vals, [1, 2, 3, 1], 0, 1.0, 0.5, 1.3)
    assert out[1] == np.inf and out[2] == -np.inf and np.isnan(out[3])
    bits = S.penalise_reference(_row(vals), V, [3], 0, 1.0, 0.5, 1.3)
    assert bits[3] == 0x7FC0
    big = np.full(V, -3.3e38, dtype=np.float32)                       # an overflow becomes an infinity
    assert _edit(big, [4], 0, 0.0, 0.0, 2.0)[4] == -np.inf


def test_round_to_nearest_even_in_both_directions():
    one = np.ones(V, dtype=np.float32)
    fp = 2.0 ** -9
    assert 1.0 - fp == 0.998046875 and 1.0 - 3 * fp == 0.994140625
    assert _edit(one, [7], 0, 0.0, fp, 1.0)[7] == 1.0                 # a tie: to the even mantissa, up
    assert _edit(one, [7, 7, 7], 0, 0.0, fp, 1.0)[7] == 0.9921875     # a tie: to the even mantissa, down
    # torch's bf16 rounding agrees
    t = torch.tensor([0.998046875, 0.994140625]).to(torch.bfloat16).float().tolist()
    assert t == [1.0, 0.9921875]
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32) * 100
    assert np.array_equal(S.bf16_bits(x), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_each_step_rounds_once_in_float32():
    # the quotient is the correctly rounded float32 one, the fma has one rounding
    x, rp, fp, pp = _f32(7.0), _f32(1.3), _f32(0.31), _f32(0.75)
    q = _f32(x / rp)
    f = _f32(np.float64(q) - np.float64(fp) * 2)                      # (exact in float64 here, then rounded once)
    want = S.bf16_values(S.bf16_bits(np.array([_f32(f - pp)])))[0]
    vals = np.full(V, 7.0, dtype=np.float32)
    assert _edit(vals, [0, 9, 9], 1, pp, fp, rp)[9] == want
    assert S._fma_f32(_f32(-2.0 ** -30), 1, _f32(1.0)) == _f32(1.0)
    assert S._fma_f32(_f32(-1.0), 3, _f32(3.0)) == 0.0 and not np.signbit(S._fma_f32(_f32(-1.0), 3, _f32(3.0)))
    assert np.signbit(S._fma_f32(_f32(-0.5), 0, _f32(-0.0)))          # -0 + -0


def test_greedy_pick_over_finite_columns():
    bits = np.stack([_row([1, 5, 5, 2] + [9] * 4), _row([np.nan, np.inf, -np.inf, np.nan] + [9] * 4),
                     _row([np.inf, -7, np.nan, -8] + [9] * 4)])
    assert S.penalised_pick_reference(bits, 4).tolist() == [1, 0, 1]  # ties to the lower column; none: token 0


def test_rows_reference_reads_its_window_only():
    hist = np.array([[1, 2, 3, 4, 5, 6], [7, 7, 7, 7, 7, 7]], dtype=np.int32)
    bits = np.stack([_row(np.full(V, 2.0))] * 3)
    out = S.bf16_values(S.penalise_rows_reference(bits, V, hist, [[0, 1, 3, 5], [1, 0, 0, 6], [2, 0, 0, 6]],
                                                  [[1.0, 0.0, 2.0]] * 3))
    assert np.flatnonzero(out[0] != 2.0).tolist() == [2, 3, 4, 5]
    assert out[0, [2, 3]].tolist() == [1.0, 1.0] and out[0, [4, 5]].tolist() == [0.0, 0.0]
    assert np.flatnonzero(out[1] != 2.0).tolist() == [7] and (out[2] == 2.0).all()      # (no such slot: untouched)


# --------------------------------------------------------------------------- parser
def test_penalty_parser_ranges_and_rounding():
    from llm_message_queue_amd.models.message import SamplingParseError, penalties_from_metadata as p
    assert p(None) == (0.0, 0.0, 1.0) and p({}) == (0.0, 0.0, 1.0) and p({"sampling": {}}) == (0.0, 0.0, 1.0)
    assert p({"sampling": {"temperature": 0.7}}) == (0.0, 0.0, 1.0)   # an absent key is off
    assert p({"sampling": {"presence_penalty": 2, "frequency_penalty": -2.0, "repetition_penalty": 0.5}}) \
        == (2.0, -2.0, 0.5)
    assert p({"sampling": {"presence_penalty": 0.126, "frequency_penalty": -0.004, "repetition_penalty": 1.234}}) \
        == (0.13, 0.0, 1.23)
    assert p({"sampling": {"repetition_penalty": 2}}) == (0.0, 0.0, 2.0)
    for bad in ({"presence_penalty": 2.01}, {"presence_penalty": -2.5}, {"frequency_penalty": 3},
                {"frequency_penalty": "0.5"}, {"frequency_penalty": True}, {"repetition_penalty": 0.49},
                {"repetition_penalty": 2.1}, {"repetition_penalty": 0}, {"repetition_penalty": False},
                {"presence_penalty": None}, {"presence_penalty": float("nan")}, {"repetition_penalty": [1.0]}):
        with pytest.raises(SamplingParseError):
            p({"sampling": bad})
    with pytest.raises(SamplingParseError):
        p({"sampling": "x"})


# --------------------------------------------------------------------------- descriptor, write-back, route
def _msgs():
    from llm_message_queue_amd.models.message import Message
    sp = [{"presence_penalty": 2.0, "frequency_penalty": -2.0, "repetition_penalty": 0.5},
          {"presence_penalty": -2.0, "frequency_penalty": 2.0, "repetition_penalty": 2.0},
          {"temperature": 0.8, "seed": 7, "top_k": 5, "frequency_penalty": 0.31},
          {"presence_penalty": 0, "frequency_penalty": 0.0, "repetition_penalty": 1.0},      # named, all off
          {"temperature": 0.8, "seed": 7},
          None,
          {"presence_penalty": 9, "repetition_penalty": 1.2},                                 # one bad value
          {"repetition_penalty": 1.004, "logprobs": 2}]                                       # rounds to off
    msgs = [Message(id=f"p{i}", content="x", metadata={"sampling": s} if s is not None else {})
            for i, s in enumerate(sp)]
    for i, m in enumerate(msgs):
        m.tier = i % 4
        m.prompt_ids = np.arange(4, dtype=np.uint32) + i
    return msgs


def test_descriptor_round_trip_of_the_penalties():
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, pack_penalties, unpack_penalties
    from tests.test_tier_caps import _gateway
    assert DESC_HDR == 20
    assert pack_penalties(0.0, 0.0, 1.0) == 0
    for tier in (0, 1, 3, 4):
        for v in ((2.0, -2.0, 0.5), (-2.0, 2.0, 2.0), (0.01, -0.01, 0.99), (0.0, 0.0, 1.0), (1.37, 0.0, 1.01)):
            col = tier | pack_penalties(*v)
            assert 0 <= col < 1 << 30 and unpack_penalties(col) == (tier,) + v
    assert unpack_penalties(-1) == (-1, 0.0, 0.0, 1.0)
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _msgs()
    buf = np.zeros((len(msgs), DESC_HDR + 8), dtype=np.int32)
    gw._fill_descs(buf, msgs, 1, 8, {})
    reqs = gw._foreign_requests(buf, 8)
    got = [(r.presence_penalty, r.frequency_penalty, r.repetition_penalty) for r in reqs]
    assert got == [(2.0, -2.0, 0.5), (-2.0, 2.0, 2.0), (0.0, 0.31, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0),
                   (0.0, 0.0, 1.0), (0.0, 0.0, 1.2), (0.0, 0.0, 1.0)]
    assert [r.tier for r in reqs] == [0, 1, 2, 3, 0, 1, 2, 3]         # the tier is intact after masking
    assert (reqs[2].top_k, reqs[7].logprobs >= 0) == (5, True)
    # a row without penalties is what it is without the feature: the bare tier, nothing above bit 3
    assert buf[[3, 4, 5, 7], 4].tolist() == [3, 0, 1, 3]
    stripped = _msgs()
    for m, o in zip(stripped, msgs):
        m.handle, m.arrival_ns, m.enqueued_at = o.handle, o.arrival_ns, o.enqueued_at
        sp = m.metadata.get("sampling")
        for k in ("presence_penalty", "frequency_penalty", "repetition_penalty"):
            if sp:
                sp.pop(k, None)
    ref = np.zeros_like(buf)
    gw._fill_descs(ref, stripped, 1, 8, {})
    assert (ref[:, 4] == np.arange(8) % 4).all()
    keep = [3, 4, 5, 7]
    assert np.array_equal(buf[keep], ref[keep])
    others = np.delete(np.arange(buf.shape[1]), 4)
    assert np.array_equal(buf[:, others], ref[:, others])             # the penalties touch the tier column only
    # the local path gives the engine the same numbers as the remote one
    for m, r in zip(_msgs(), reqs):
        loc = gw._make_request(m, 2)
        assert (loc.presence_penalty, loc.frequency_penalty, loc.repetition_penalty) \
            == (r.presence_penalty, r.frequency_penalty, r.repetition_penalty), m.id


def test_effective_penalties_are_written_back_only_when_in_effect():
    from llm_message_queue_amd.models.message import default_seed
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _msgs()
    for m in msgs:
        gw._make_request(m, 2)
    md = [m.metadata for m in msgs]
    assert md[0]["sampling"] == {"temperature": 0.0, "seed": default_seed("p0"), "presence_penalty": 2.0,
                                 "frequency_penalty": -2.0, "repetition_penalty": 0.5}      # greedy: in effect too
    assert md[2]["sampling"] == {"temperature": 0.8, "seed": 7, "top_k": 5, "frequency_penalty": 0.31}
    assert set(md[3]["sampling"]) == {"temperature", "seed"}          # named but off: not written
    assert md[4]["sampling"] == {"temperature": 0.8, "seed": 7}       # named none: exactly as before
    assert "sampling" not in md[5] and "sampling_error" not in md[5]
    # the lenient path: the bad penalty is off and reported, the good one stays
    assert "presence_penalty" in md[6]["sampling_error"] and "repetition" not in md[6]["sampling_error"]
    assert set(md[6]["sampling"]) == {"temperature", "seed", "repetition_penalty"}
    assert md[6]["sampling"]["repetition_penalty"] == 1.2
    assert set(md[7]["sampling"]) == {"temperature", "seed", "logprobs"}
    assert all("sampling_error" not in md[i] for i in (0, 1, 2, 3, 4, 7))
    # a replay of the written-back values parses to the same
    r = gw._make_request(msgs[0], 2)
    assert (r.presence_penalty, r.frequency_penalty, r.repetition_penalty) == (2.0, -2.0, 0.5)


def test_post_message_rejects_a_bad_penalty():
    from fastapi.testclient import TestClient
    from llm_message_queue_amd.api.server import create_app
    from llm_message_queue_amd.gateway.app import GatewayApp
    from llm_message_queue_amd.utils.config import default_config
    cfg = default_config()
    cfg.preprocessor.batch_window_us = 200
    app = GatewayApp(cfg, use_gpu=False, simulate_ms=(1, 1, 1, 1))
    try:
        with TestClient(create_app(app)) as c:
            def post(sp):
                return c.post("/api/v1/messages", json={"content": "hi", "metadata": {"sampling": sp}})
            for key, bad in (("presence_penalty", 2.5), ("frequency_penalty", "1"), ("repetition_penalty", 0.1),
                             ("repetition_penalty", True)):
                r = post({key: bad})
                assert r.status_code == 400 and key in r.text, (key, bad)
            assert post({"presence_penalty": 1.0, "frequency_penalty": 0.5, "repetition_penalty": 1.2}).status_code == 202
            assert post({"temperature": 0.9, "seed": 11, "top_k": 40, "repetition_penalty": 1.1}).status_code == 202
    finally:
        app.stop()


# --------------------------------------------------------------------------- engine on the CPU
PEN = dict(presence_penalty=1.2, frequency_penalty=0.6, repetition_penalty=1.5)


def _engine(slots=32, **kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=slots, max_ctx=64, token_budget=256, device="cpu", impl="ref", **kw)


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=5, **kw)


def _spy(eng, seen):
    """Record, per penalised row of every ``penalised_head`` call, the slot
    and the history handed over with its prompt / generated split."""
    inner = eng.model.ops.penalised_head

    def penalised_head(x, w, inv_temp, keys, top_k, top_p, hist, spans, params, n_greedy=0):
        assert hist.dtype == torch.int32 and tuple(hist.shape) == (eng.n_all, eng.max_ctx)
        for (s, a, m, b), pv in zip(spans.tolist(), params.tolist()):
            seen.append((s, hist[s, a:b].tolist(), m - a, tuple(np.float32(pv).tolist())))
        return inner(x, w, inv_temp, keys, top_k, top_p, hist, spans, params, n_greedy=n_greedy)

    eng.model.ops.penalised_head = penalised_head


def _run(reqs, slots=32, eng=None):
    eng = eng or _engine(slots)
    seen = []
    _spy(eng, seen)
    assert len(eng.admit(reqs)) == len(reqs)
    done = eng.drain()
    assert len(done) == len(reqs)
    return {r.req_id: r for r in done}, eng, seen


@pytest.fixture(scope="module")
def engine_runs():
    def others():
        return [_req(i) for i in range(12)] + [_req(12 + i, temperature=0.9, seed=i) for i in range(4)]
    alone, e_alone, seen = _run([_req(100, **PEN)])
    crowd, e_crowd, seen_crowd = _run(others() + [_req(100, **PEN)])
    moved, _, _ = _run([_req(i) for i in range(3)] + [_req(100, **PEN)])
    plain, e_plain, seen_plain = _run(others())
    return dict(alone=alone, crowd=crowd, moved=moved, plain=plain, seen=seen, seen_crowd=seen_crowd,
                seen_plain=seen_plain, engines=dict(alone=e_alone, crowd=e_crowd, plain=e_plain))


def test_engine_hands_over_the_own_prompt_and_the_tokens_generated_so_far(engine_runs):
    r = engine_runs["alone"][100]
    seen = engine_runs["seen"]
    assert len(seen) == 5 and len(r.out_tokens) == 5
    want_params = tuple(np.array([1.2, 0.6, 1.5], dtype=np.float32).tolist())
    for g, (slot, h, n_p, pv) in enumerate(seen):
        assert slot == r.slot and pv == want_params
        assert h == r.prompt.tolist() + r.out_tokens[:g].tolist(), g
        assert n_p == len(r.prompt)
    # in a crowd the same windows, whatever slot
    mine = [s for s in engine_runs["seen_crowd"] if s[0] == engine_runs["crowd"][100].slot]
    assert [s[1:] for s in mine] == [s[1:] for s in seen]
    assert len(mine) == len(engine_runs["seen_crowd"])                # (nobody else is penalised)


def test_engine_penalised_request_is_reproducible_across_batches_and_slots(engine_runs):
    a, b, c = engine_runs["alone"][100], engine_runs["crowd"][100], engine_runs["moved"][100]
    assert len({a.slot, b.slot, c.slot}) == 3
    assert np.array_equal(a.out_tokens, b.out_tokens) and np.array_equal(a.out_tokens, c.out_tokens)


def test_engine_neighbours_are_untouched_and_nothing_runs_when_nobody_asks(engine_runs):
    for i in range(16):
        assert np.array_equal(engine_runs["crowd"][i].out_tokens, engine_runs["plain"][i].out_tokens), i
    e = engine_runs["engines"]
    assert e["plain"].penalised_steps == 0 and e["plain"].d_hist is None and engine_runs["seen_plain"] == []
    assert e["alone"].penalised_steps == 5 and 0 < e["crowd"].penalised_steps <= 5 + 1


def test_engine_a_row_with_top_k_and_a_penalty_is_drawn_again_once(engine_runs):
    hot = dict(PEN, temperature=0.8, seed=7, top_k=3)
    got, eng, seen = _run([_req(100, **hot), _req(101, temperature=0.8, seed=7, top_k=3), _req(1)])
    assert eng.penalised_steps == 5 and len(seen) == 5
    calls = []
    inner = eng.model.ops.truncated_head
    eng.model.ops.truncated_head = lambda *a: calls.append(a[0].shape[0]) or inner(*a)
    again = _run([_req(100, **hot), _req(101, temperature=0.8, seed=7, top_k=3), _req(1)], eng=eng)[0]
    assert calls and set(calls) == {1}                                # only request 101 is in the truncated set
    assert np.array_equal(again[100].out_tokens, got[100].out_tokens)
    alone = _run([_req(100, **hot)])[0][100]
    assert np.array_equal(alone.out_tokens, got[100].out_tokens)
    # its unpenalised neighbour with the same seed and top_k draws what it draws alone
    ref = _run([_req(101, temperature=0.8, seed=7, top_k=3)])[0][101]
    assert np.array_equal(ref.out_tokens, got[101].out_tokens)


def test_engine_window_of_a_dialog_turn_is_the_same_resident_and_replayed():
    from llm_message_queue_amd.backend.engine import Request
    prompts = [np.arange(3, 14, dtype=np.int32), np.arange(40, 47, dtype=np.int32)]
    ck = 4242

    def serve(eng, r):
        assert eng.admit([r]) == [r]
        done = eng.drain()
        assert done == [r]
        return r

    res, seen_res = _engine(8), []
    _spy(res, seen_res)
    serve(res, Request(1, prompts[0].copy(), 3, conv=ck))
    a = serve(res, Request(2, prompts[1].copy(), 4, conv=ck, **PEN))
    assert a.reused > 0
    rep, seen_rep = _engine(8), []
    _spy(rep, seen_rep)
    r1 = serve(rep, Request(1, prompts[0].copy(), 3, conv=ck))
    hist = np.concatenate([prompts[0], r1.out_tokens[:-1]])
    rep.drop_parked(ck)                                               # evicted: the next turn must replay
    b = serve(rep, Request(2, prompts[1].copy(), 4, conv=ck, history=hist, **PEN))
    assert b.reused == 0 and len(b.prompt) == len(hist) + len(prompts[1])
    assert a.out_tokens.tolist() == b.out_tokens.tolist()
    assert len(seen_res) == len(seen_rep) == 4
    for g, (x, y) in enumerate(zip(seen_res, seen_rep)):
        assert x[1] == y[1] == prompts[1].tolist() + a.out_tokens[:g].tolist()      # earlier turns do not count
        assert x[2] == y[2] == len(prompts[1])


def test_micro_pool_serves_a_penalised_request_with_the_same_tokens():
    from tests.test_realtime_micro import _engine as micro_engine, _serve
    from llm_message_queue_amd.backend.engine import Request

    def reqs():
        rng = np.random.default_rng(9)
        return [Request(req_id=i, prompt=rng.integers(0, 1000, size=5 + i).astype(np.int32), gen_tokens=4, tier=i % 3,
                        **(PEN if i in (0, 1) else {})) for i in range(6)]
    a = _serve(micro_engine("off"), reqs())
    eng = micro_engine("micro")
    seen = []
    _spy(eng, seen)
    b = _serve(eng, reqs())
    assert b[0][1] and not b[1][1]                                    # request 0 (tier 0) ran on the micro pool
    assert {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}
    assert eng.penalised_steps > 0 and eng.micro_steps > 0
    assert any(s[0] >= eng.slots for s in seen) and any(s[0] < eng.slots for s in seen)


def test_engine_refuses_a_context_above_the_history_cap():
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    with pytest.raises(ValueError):
        BackendEngine(LlamaConfig.tiny(), slots=2, max_ctx=S.PEN_HIST_MAX + 1, token_budget=8, device="cpu", impl="ref")


def test_sim_engine_forward_ignores_pen():
    from llm_message_queue_amd.backend.sim_engine import SimEngine
    out = SimEngine._forward(None, None, None, torch.zeros(3), pen=(None,) * 8)
    assert out.shape == (3,)
