"""Top-k / top-p sampling, the parts that need no GPU: the numpy twin of the
selection contract (``csrc/kernels/sample_truncate_kernels.h``), the parser,
the descriptor bits, the gateway's write-back rule, the REST route and a
truncating request through the CPU reference engine."""
import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import sampling as S


def _bf16(a) -> np.ndarray:
    return torch.tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


# --------------------------------------------------------------------------- twin semantics
def test_top_k_keeps_the_whole_group_tied_at_the_kth_value():
    lg = np.array([1.0, 3.0, 2.0, 2.0, 0.5, 2.0, -1.0])
    assert S.truncation_keep(lg, 1.0, 2, 1.0).tolist() == [False, True, True, True, False, True, False]
    assert S.truncation_keep(lg, 1.0, 4, 1.0).tolist() == [False, True, True, True, False, True, False]
    assert S.truncation_keep(lg, 1.0, 5, 1.0).tolist() == [True, True, True, True, False, True, False]
    assert S.truncation_keep(lg, 1.0, 0, 1.0).all() and S.truncation_keep(lg, 1.0, 100, 1.0).all()


def test_top_k_1_is_the_argmax_group():
    lg = np.array([0.0, 5.0, 5.0, 4.0])
    assert S.truncation_keep(lg, 0.5, 1, 1.0).tolist() == [False, True, True, False]


def test_top_p_keeps_the_shortest_prefix_and_always_the_first_group():
    # masses at T = 1: 1, e^-1, e^-2, e^-3 -> shares 0.6439, 0.2369, 0.0871, 0.0321
    lg = np.array([-3.0, 0.0, -1.0, -2.0])
    assert S.truncation_keep(lg, 1.0, 0, 0.5).tolist() == [False, True, False, False]
    assert S.truncation_keep(lg, 1.0, 0, 0.65).tolist() == [False, True, True, False]
    assert S.truncation_keep(lg, 1.0, 0, 0.88).tolist() == [False, True, True, False]
    assert S.truncation_keep(lg, 1.0, 0, 0.89).tolist() == [False, True, True, True]
    assert S.truncation_keep(lg, 1.0, 0, 0.999).all() and S.truncation_keep(lg, 1.0, 0, 1.0).all()
    assert S.truncation_keep(lg, 1.0, 0, 1e-6).tolist() == [False, True, False, False]       # the first group stays
    # the temperature comes first: at T = 0.25 the maximum alone holds 98 %
    assert S.truncation_keep(lg, 4.0, 0, 0.9).tolist() == [False, True, False, False]
    # a group's mass is count * exp(...): two columns at -1 weigh 2 e^-1
    lg2 = np.array([0.0, -1.0, -1.0, -5.0])
    assert S.truncation_keep(lg2, 1.0, 0, 0.99).tolist() == [True, True, True, False]


def test_the_order_is_top_k_then_top_p():
    # top_k = 2 keeps {0, -1}: shares 0.731, 0.269 of THEIR total; over the full row the first would hold 0.64
    lg = np.array([0.0, -1.0, -2.0, -3.0])
    assert S.truncation_keep(lg, 1.0, 2, 0.7).tolist() == [True, False, False, False]
    assert S.truncation_keep(lg, 1.0, 0, 0.7).tolist() == [True, True, False, False]
    assert S.truncation_keep(lg, 1.0, 2, 0.74).tolist() == [True, True, False, False]


def test_an_all_equal_row_keeps_everything():
    lg = np.full(37, -2.5)
    for k, p in ((1, 1.0), (0, 0.001), (5, 0.3)):
        assert S.truncation_keep(lg, 1.0, k, p).all()
    z = np.array([0.0, -0.0, 0.0])                                    # +0 and -0 are one value
    assert S.truncation_keep(z, 1.0, 1, 0.1).all()


def test_nan_and_infinite_logits_are_never_kept():
    lg = np.array([np.nan, 1.0, np.nan, 0.5, np.inf, -np.inf])
    assert S.truncation_keep(lg, 1.0, 0, 1.0).tolist() == [False, True, False, True, False, False]
    assert S.truncation_keep(lg, 1.0, 1, 1.0).tolist() == [False, True, False, False, False, False]
    assert not S.truncation_keep(np.array([np.nan, np.nan]), 1.0, 3, 0.5).any()
    keys = S.row_keys(3, [0, 1])
    picks = S.sample_truncated_reference(np.array([[np.nan, np.nan, np.nan], [np.nan, -4.0, np.nan]]), 1.0, keys,
                                         0, 1.0)
    assert picks.tolist() == [0, 1]                                   # (no finite logit: token 0)


def test_reference_without_truncation_equals_the_plain_reference_sampler():
    rng = np.random.default_rng(5)
    lg = _bf16(3 * rng.standard_normal((16, 700)))
    keys = S.row_keys(11, np.arange(16))
    it = np.full(16, 1 / 0.7, dtype=np.float32)
    plain = S.sample_reference(lg, it, keys)
    assert np.array_equal(S.sample_truncated_reference(lg, it, keys, 0, 1.0), plain)
    cut = S.sample_truncated_reference(lg, it, keys, 3, 1.0)
    assert (cut != plain).any()
    for r in range(16):
        assert S.truncation_keep(lg[r], it[r], 3, 1.0)[cut[r]]
    # per-row parameters
    tk = np.array([0, 1] * 8)
    mixed = S.sample_truncated_reference(lg, it, keys, tk, np.ones(16, dtype=np.float32))
    assert np.array_equal(mixed[::2], plain[::2]) and np.array_equal(mixed[1::2], lg.argmax(axis=1)[1::2])


# --------------------------------------------------------------------------- parser
def test_truncation_parser_ranges_and_rounding():
    from llm_message_queue_amd.models.message import (SamplingParseError, default_seed, sampling_from_metadata,
                                                      truncation_from_metadata as p)
    assert p(None) == (0, 1.0) and p({}) == (0, 1.0) and p({"sampling": {"temperature": 0.8}}) == (0, 1.0)
    assert p({"sampling": {"top_k": 40, "top_p": 0.9}}) == (40, 0.9)
    assert p({"sampling": {"top_k": 0, "top_p": 1}}) == (0, 1.0)
    assert p({"sampling": {"top_k": 1023}}) == (1023, 1.0)
    assert p({"sampling": {"top_p": 0.12345}}) == (0, 0.123)
    assert p({"sampling": {"top_p": 0.9996}}) == (0, 1.0)            # rounds to off
    assert p({"sampling": {"top_p": 0.001}}) == (0, 0.001) and p({"sampling": {"top_p": 0.0006}}) == (0, 0.001)
    for bad in ({"top_k": 0.5}, {"top_k": -1}, {"top_k": 1024}, {"top_k": True}, {"top_k": "3"}, {"top_k": 3.0},
                {"top_p": 0}, {"top_p": 0.0004}, {"top_p": -0.1}, {"top_p": 1.001}, {"top_p": "0.5"},
                {"top_p": True}, {"top_p": float("nan")}, "hot", [1]):
        with pytest.raises(SamplingParseError):
            p({"sampling": bad})
    # the (temperature, seed) parser keeps its 2-tuple and ignores the new keys
    md = {"sampling": {"temperature": 0.8, "seed": 7, "top_k": 3, "top_p": 0.5}}
    assert sampling_from_metadata(md, "a") == (0.8, 7)
    assert sampling_from_metadata({"sampling": {"top_k": 3}}, "a") == (0.0, default_seed("a"))


# --------------------------------------------------------------------------- descriptor, write-back, route
def _msgs():
    from llm_message_queue_amd.models.message import Message
    msgs = [Message(id="t0", content="x", metadata={"sampling": {"temperature": 0.7, "seed": 5, "top_k": 40,
                                                                 "top_p": 0.9}}),
            Message(id="t1", content="x", metadata={"sampling": {"temperature": 1.0, "top_k": 1023}}),
            Message(id="t2", content="x", metadata={"sampling": {"temperature": 1.0, "seed": 1, "top_p": 0.0014}}),
            Message(id="t3", content="x", metadata={"sampling": {"temperature": 0.8, "seed": 7}}),
            Message(id="t4", content="x"),
            Message(id="t5", content="x", metadata={"sampling": {"temperature": 0, "top_k": 5, "top_p": 0.5}}),
            Message(id="t6", content="x", metadata={"sampling": {"temperature": 0.8, "seed": 2, "top_k": 0.5}}),
            Message(id="t7", content="x", conversation_id="c7",
                    metadata={"sampling": {"temperature": 0.8, "seed": 3, "top_k": 0, "top_p": 1.0}})]
    for i, m in enumerate(msgs):
        m.tier = 2
        m.prompt_ids = np.arange(4, dtype=np.uint32) + i
    return msgs


def test_descriptor_round_trip_of_top_k_and_top_p():
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, DIALOG_TURN
    from llm_message_queue_amd.models.message import default_seed
    from tests.test_tier_caps import _gateway
    assert DESC_HDR == 20
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _msgs()
    buf = np.zeros((len(msgs), DESC_HDR + 8), dtype=np.int32)
    gw._fill_descs(buf, msgs, 1, 8, {})
    reqs = gw._foreign_requests(buf, 8)
    assert [r.top_k for r in reqs] == [40, 1023, 0, 0, 0, 0, 0, 0]
    assert [r.top_p for r in reqs] == [0.9, 1.0, 0.001, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert [r.temperature for r in reqs][:4] == [float(np.float32(0.7)), 1.0, 1.0, float(np.float32(0.8))]
    assert reqs[1].seed == default_seed("t1") and reqs[0].seed == 5
    # flags of messages without (active) truncation are what they were: nothing above bit 9
    assert buf[3:, 11].tolist() == [0, 0, 0, 0, DIALOG_TURN]
    assert buf[0, 11] == (40 << 10) | (900 << 20) and buf[1, 11] == 1023 << 10 and buf[2, 11] == 1 << 20
    # the local path gives the engine the same numbers as the remote one
    for m, r in zip(_msgs(), reqs):
        loc = gw._make_request(m, 2)
        assert (loc.top_k, loc.top_p) == (r.top_k, r.top_p), m.id
        assert np.float32(loc.temperature) == np.float32(r.temperature)


def test_effective_values_are_written_back_only_when_active():
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _msgs()
    for m in msgs:
        gw._make_request(m, 2)
    md = [m.metadata for m in msgs]
    assert md[0]["sampling"] == {"temperature": 0.7, "seed": 5, "top_k": 40, "top_p": 0.9}
    assert set(md[1]["sampling"]) == {"temperature", "seed", "top_k"} and md[1]["sampling"]["top_k"] == 1023
    assert md[2]["sampling"] == {"temperature": 1.0, "seed": 1, "top_p": 0.001}
    assert md[3]["sampling"] == {"temperature": 0.8, "seed": 7}                   # named neither: exactly as before
    assert "sampling" not in md[4] and "sampling_error" not in md[4]
    assert set(md[5]["sampling"]) == {"temperature", "seed"} and "sampling_error" not in md[5]   # greedy: no effect
    assert md[6]["sampling"] == {"temperature": 0.8, "seed": 2} and "top_k" in md[6]["sampling_error"]
    assert md[7]["sampling"] == {"temperature": 0.8, "seed": 3}
    # a bad truncation value keeps the temperature; a replay of the written-back values parses to the same
    r = gw._make_request(msgs[6], 2)
    assert (r.temperature, r.seed, r.top_k, r.top_p) == (0.8, 2, 0, 1.0)
    r = gw._make_request(msgs[0], 2)
    assert (r.temperature, r.seed, r.top_k, r.top_p) == (0.7, 5, 40, 0.9)


def test_post_message_rejects_a_bad_top_k_or_top_p():
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
            r = post({"temperature": 0.8, "top_k": 0.5})
            assert r.status_code == 400 and "top_k" in r.text
            r = post({"temperature": 0.8, "top_p": 0})
            assert r.status_code == 400 and "top_p" in r.text
            assert post({"temperature": 0.9, "seed": 11, "top_k": 40, "top_p": 0.95}).status_code == 202
            assert post({"top_k": 5, "top_p": 0.5}).status_code == 202          # greedy: accepted, no effect
    finally:
        app.stop()


# --------------------------------------------------------------------------- engine on the CPU
def _engine(slots=32):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=slots, max_ctx=64, token_budget=256, device="cpu", impl="ref")


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=5, **kw)


def _run(reqs, slots=32, spy=False):
    eng = _engine(slots)
    seen = []
    if spy:
        inner = eng.model.ops.truncated_head

        def truncated_head(x, w, inv_temp, keys, top_k, top_p):
            out = inner(x, w, inv_temp, keys, top_k, top_p)
            lg = (x.float() @ w.float().t()).to(torch.bfloat16).float().numpy()
            for r in range(x.shape[0]):
                keep = S.truncation_keep(lg[r], float(inv_temp[r]), int(top_k[r]), float(top_p[r]))
                seen.append((int(out[r]), keep, int(top_k[r]), float(top_p[r])))
            return out

        eng.model.ops.truncated_head = truncated_head
    assert len(eng.admit(reqs)) == len(reqs)
    done = eng.drain()
    assert len(done) == len(reqs)
    return {r.req_id: r for r in done}, eng, seen


@pytest.fixture(scope="module")
def engine_runs():
    def others():
        return [_req(i) for i in range(12)] + [_req(12 + i, temperature=0.9, seed=i) for i in range(4)]
    trunc = dict(temperature=0.8, seed=7, top_k=3)
    alone, e_alone, seen = _run([_req(100, **trunc)], spy=True)
    crowd, e_crowd, _ = _run(others() + [_req(100, **trunc)])
    moved, _, _ = _run([_req(i) for i in range(3)] + [_req(100, **trunc)])
    plain, e_plain, _ = _run(others() + [_req(100, temperature=0.8, seed=7)])
    greedy_k, e_greedy, _ = _run([_req(100, top_k=3, top_p=0.5), _req(101)])
    return dict(alone=alone, crowd=crowd, moved=moved, plain=plain, greedy_k=greedy_k, seen=seen,
                steps=dict(alone=(e_alone.sampled_steps, e_alone.truncated_steps),
                           crowd=(e_crowd.sampled_steps, e_crowd.truncated_steps),
                           plain=(e_plain.sampled_steps, e_plain.truncated_steps),
                           greedy=(e_greedy.sampled_steps, e_greedy.truncated_steps)))


def test_engine_truncating_request_is_reproducible_across_batches_and_slots(engine_runs):
    a, b, c = engine_runs["alone"][100], engine_runs["crowd"][100], engine_runs["moved"][100]
    assert a.out_tokens is not None and len(a.out_tokens) == 5
    assert len({a.slot, b.slot, c.slot}) == 3
    assert np.array_equal(a.out_tokens, b.out_tokens) and np.array_equal(a.out_tokens, c.out_tokens)


def test_engine_neighbours_are_untouched_by_a_truncating_request(engine_runs):
    for i in range(16):
        assert np.array_equal(engine_runs["crowd"][i].out_tokens, engine_runs["plain"][i].out_tokens), i


def test_engine_counts_truncated_steps_only_where_a_row_truncates(engine_runs):
    st = engine_runs["steps"]
    assert st["alone"][0] > 0 and st["alone"][1] == st["alone"][0]
    assert 0 < st["crowd"][1] <= st["crowd"][0]
    assert st["plain"][0] > 0 and st["plain"][1] == 0
    assert st["greedy"] == (0, 0)                                     # top_k / top_p without a temperature: no effect
    g = engine_runs["greedy_k"]
    ref, _, _ = _run([_req(100), _req(101)])
    assert np.array_equal(g[100].out_tokens, ref[100].out_tokens)


def test_engine_every_token_of_a_truncating_request_lies_in_its_kept_set(engine_runs):
    seen = engine_runs["seen"]
    toks = engine_runs["alone"][100].out_tokens.tolist()
    assert len(seen) == 5 and [s[0] for s in seen] == toks
    for tok, keep, k, p in seen:
        assert (k, p) == (3, 1.0) and keep[tok] and 3 <= keep.sum() < 1024
    # top_k = 3 of 1,024 columns is a real restriction: the same request without it draws other tokens
    assert engine_runs["plain"][100].out_tokens.tolist() != toks


def test_micro_pool_passes_the_truncation_through():
    """A realtime request served by the micro-forwards (``realtime_mode =
    "micro"``) draws the tokens it draws on the serving pool."""
    from tests.test_realtime_micro import _engine as micro_engine, _serve
    from llm_message_queue_amd.backend.engine import Request

    def reqs():
        rng = np.random.default_rng(9)
        return [Request(req_id=i, prompt=rng.integers(0, 1000, size=5 + i).astype(np.int32), gen_tokens=4, tier=i % 3,
                        **(dict(temperature=0.8, seed=7, top_k=3, top_p=0.9) if i in (0, 1) else {}))
                for i in range(6)]
    a = _serve(micro_engine("off"), reqs())
    eng = micro_engine("micro")
    b = _serve(eng, reqs())
    assert b[0][1] and not b[1][1]                                     # request 0 (tier 0) ran on the micro pool
    assert {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}
    assert eng.truncated_steps > 0 and eng.micro_steps > 0


def test_sim_engine_forward_ignores_trunc():
    from llm_message_queue_amd.backend.sim_engine import SimEngine
    out = SimEngine._forward(None, None, None, torch.zeros(3), inv_temp=torch.ones(256), keys=torch.zeros(256, 2),
                             trunc=(torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32),
                                    torch.ones(1)))
    assert out.shape == (3,)
