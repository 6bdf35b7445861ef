"""Generated tokens and their log-probabilities, the parts that need no GPU:
the parser and the REST route, the gateway's write-back rule, the numpy twin of
``csrc/kernels/logprob_kernels.h``, a request that asks for them through the
CPU reference engine, and the descriptor flag and K_LOGP rows between ranks."""
import os
import threading

import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import sampling as S


# --------------------------------------------------------------------------- parser, route, write-back
def test_logprobs_parser_accepts_0_to_5_and_rejects_the_rest():
    from llm_message_queue_amd.models.message import SamplingParseError, logprobs_from_metadata as p
    assert p(None) == -1 and p({}) == -1 and p({"sampling": {"temperature": 0.8}}) == -1
    for n in range(6):
        assert p({"sampling": {"logprobs": n}}) == n
    assert p({"sampling": {"temperature": 0.8, "top_k": 3, "logprobs": 2}}) == 2
    for bad in ({"logprobs": True}, {"logprobs": False}, {"logprobs": 1.0}, {"logprobs": 0.5}, {"logprobs": "3"},
                {"logprobs": -1}, {"logprobs": 6}, {"logprobs": None}, {"logprobs": [1]}, "hot", [1]):
        with pytest.raises(SamplingParseError):
            p({"sampling": bad})


def test_post_message_rejects_a_bad_logprobs_value():
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
            for bad in (6, -1, True, 1.5, "2"):
                r = post({"logprobs": bad})
                assert r.status_code == 400 and "logprobs" in r.text, bad
            assert post({"logprobs": 0}).status_code == 202
            assert post({"temperature": 0.9, "seed": 11, "top_k": 40, "logprobs": 5}).status_code == 202
    finally:
        app.stop()


def _msgs():
    from llm_message_queue_amd.models.message import Message
    msgs = [Message(id="l0", content="x", metadata={"sampling": {"temperature": 0.7, "seed": 5, "top_k": 40,
                                                                 "logprobs": 3}}),
            Message(id="l1", content="x", metadata={"sampling": {"logprobs": 0}}),
            Message(id="l2", content="x", metadata={"sampling": {"temperature": 0.8, "seed": 7}}),
            Message(id="l3", content="x"),
            Message(id="l4", content="x", metadata={"sampling": {"temperature": 0.8, "seed": 2, "logprobs": 9}}),
            Message(id="l5", content="x", metadata={"sampling": {"temperature": 0, "logprobs": 5}})]
    for i, m in enumerate(msgs):
        m.tier = 2
        m.prompt_ids = np.arange(4, dtype=np.uint32) + i
    return msgs


def test_effective_logprobs_is_written_back_only_when_named():
    from llm_message_queue_amd.models.message import default_seed
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _msgs()
    reqs = [gw._make_request(m, 2) for m in msgs]
    md = [m.metadata for m in msgs]
    assert [r.logprobs for r in reqs] == [3, 0, -1, -1, -1, 5]
    assert md[0]["sampling"] == {"temperature": 0.7, "seed": 5, "top_k": 40, "logprobs": 3}
    assert md[1]["sampling"] == {"temperature": 0.0, "seed": default_seed("l1"), "logprobs": 0}     # greedy
    assert reqs[1].temperature == 0.0
    assert md[2]["sampling"] == {"temperature": 0.8, "seed": 7}                   # did not name it: exactly as before
    assert "sampling" not in md[3] and "sampling_error" not in md[3]
    assert md[4]["sampling"] == {"temperature": 0.8, "seed": 2} and "logprobs" in md[4]["sampling_error"]
    assert reqs[4].temperature == 0.8                                             # a bad value keeps the rest
    assert md[5]["sampling"] == {"temperature": 0.0, "seed": default_seed("l5"), "logprobs": 5}
    # a replay of the written-back values parses to the same
    again = [gw._make_request(m, 2) for m in msgs]
    assert [r.logprobs for r in again] == [3, 0, -1, -1, -1, 5]


# --------------------------------------------------------------------------- twin, exact cases
def test_twin_one_finite_column_has_log_probability_zero():
    lp, ids = S.logprob_reference(np.array([[np.nan, -np.inf, -7.5, np.inf, np.nan]]), [2])
    assert lp[0].tolist() == [0.0, 0.0, -np.inf, -np.inf, -np.inf, -np.inf]
    assert ids[0].tolist() == [2, -1, -1, -1, -1]


@pytest.mark.parametrize("k", [1, 2, 5, 7, 1000])
def test_twin_k_equal_columns_have_minus_log_k(k):
    lp, ids = S.logprob_reference(np.full((1, k), 1.25), [k - 1])
    want = -np.log(k)
    n = min(k, 5)
    assert np.allclose(lp[0, :1 + n], want, rtol=0, atol=1e-15)
    assert ids[0, :n].tolist() == list(range(n)) and (ids[0, n:] == -1).all() and (lp[0, 1 + n:] == -np.inf).all()


def test_twin_a_tie_at_the_fifth_place_goes_to_the_lower_column():
    row = np.array([0.0, 9.0, 3.0, 8.0, 3.0, 7.0, 6.0, 3.0, -0.0, 0.0])
    lp, ids = S.logprob_reference(row[None], [4])
    assert ids[0].tolist() == [1, 3, 5, 6, 2]
    assert lp[0, 0] == lp[0, 5]                                        # the tied token has the value, not the place
    z = np.array([[-0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0]])            # +0 and -0 are one value
    lp, ids = S.logprob_reference(z, [5])
    assert ids[0].tolist() == [0, 1, 2, 3, 4] and np.allclose(lp[0], -np.log(7), atol=1e-15)


def test_twin_non_finite_columns_and_tokens():
    row = np.array([np.nan, 2.0, np.inf, 1.0, -np.inf, np.nan, 0.5])
    lg = np.stack([row, row, row, row, np.full(7, np.nan)])
    lp, ids = S.logprob_reference(lg, [0, 2, -1, 7, 1])
    assert (lp[:, 0] == -np.inf).all()                                 # on a NaN, on an inf, out of range twice, no candidate
    for r in range(4):
        assert ids[r].tolist() == [1, 3, 6, -1, -1] and (lp[r, 4:] == -np.inf).all()
        assert np.isfinite(lp[r, 1:4]).all() and abs(np.exp(lp[r, 1:4]).sum() - 1) < 1e-12
    assert (ids[4] == -1).all() and (lp[4] == -np.inf).all()
    lp, _ = S.logprob_reference(lg[:1], [3])
    assert lp[0, 0] == lp[0, 2]


def test_twin_rows_are_normalised():
    rng = np.random.default_rng(4)
    lg = torch.tensor(3 * rng.standard_normal((6, 700)), dtype=torch.float32).to(torch.bfloat16).double().numpy()
    lg[1, ::7] = np.nan
    lg[2, 5] = -np.inf
    for r in range(6):
        cand = np.flatnonzero(np.isfinite(lg[r]))
        lp, _ = S.logprob_reference(np.repeat(lg[r:r + 1], len(cand), axis=0), cand)
        assert abs(np.exp(lp[:, 0]).sum() - 1.0) < 1e-12, r
        want = torch.log_softmax(torch.tensor(lg[r][cand]), dim=0).numpy()
        assert np.allclose(lp[:, 0], want, rtol=0, atol=1e-12)


def test_bound_meets_the_condition_at_the_serving_vocabulary():
    assert 0 < S.logprob_bound(1) < S.logprob_bound(2048) < S.logprob_bound(128256) <= 1e-4
    assert S.logprob_bound(128256, 256.0) > S.logprob_bound(128256)


# --------------------------------------------------------------------------- engine on the CPU
def _engine(slots=32):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=slots, max_ctx=64, token_budget=256, device="cpu", impl="ref")


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=5, **kw)


def _run(reqs, spy=False):
    eng = _engine()
    seen = []
    if spy:
        inner = eng.model.ops.logprob_head

        def logprob_head(x, w, tok):
            lp, ids = inner(x, w, tok)
            lg = (x.float() @ w.float().t()).to(torch.bfloat16).float().numpy()
            want_lp, want_ids = S.logprob_reference(lg, tok.numpy())
            for r in range(x.shape[0]):
                seen.append((int(tok[r]), lp[r].numpy().copy(), ids[r].numpy().copy(), want_lp[r], want_ids[r]))
            return lp, ids

        eng.model.ops.logprob_head = logprob_head
    assert len(eng.admit(reqs)) == len(reqs)
    done = eng.drain()
    assert len(done) == len(reqs)
    return {r.req_id: r for r in done}, eng, seen


def _others():
    return [_req(i) for i in range(9)] + [_req(9 + i, temperature=0.9, seed=i) for i in range(4)] \
        + [_req(13 + i, temperature=0.9, seed=i, top_k=4) for i in range(3)]


MINE = dict(temperature=0.8, seed=7)


@pytest.fixture(scope="module")
def engine_runs():
    alone, e_alone, seen = _run([_req(100, logprobs=3, **MINE)], spy=True)
    crowd, e_crowd, _ = _run(_others() + [_req(100, logprobs=3, **MINE)])
    moved, _, _ = _run([_req(i) for i in range(3)] + [_req(100, logprobs=3, **MINE)])
    plain, e_plain, _ = _run(_others() + [_req(100, **MINE)])
    greedy, _, _ = _run([_req(100, logprobs=1), _req(101)])
    wide, _, seen_wide = _run([_req(100, logprobs=5, temperature=2.0, seed=3, top_k=200)], spy=True)
    return dict(alone=alone, crowd=crowd, moved=moved, plain=plain, greedy=greedy, wide=wide, seen=seen,
                seen_wide=seen_wide, steps=dict(alone=e_alone.logprob_steps, crowd=e_crowd.logprob_steps,
                                                plain=e_plain.logprob_steps))


def _bits(r):
    return (r.out_tokens.tolist(), r.out_logprobs.view(np.uint32).tolist(), r.out_top_ids.tolist(),
            r.out_top_logprobs.view(np.uint32).tolist())


def test_engine_logprobs_are_the_same_alone_in_a_crowd_and_in_another_slot(engine_runs):
    a, b, c = engine_runs["alone"][100], engine_runs["crowd"][100], engine_runs["moved"][100]
    assert len(a.out_tokens) == 5 and a.out_logprobs.shape == (5,) and a.out_top_ids.shape == (5, 5)
    assert a.out_top_logprobs.shape == (5, 5) and a.out_logprobs.dtype == np.float32
    assert len({a.slot, b.slot, c.slot}) == 3
    assert _bits(a) == _bits(b) == _bits(c)


def test_engine_asking_for_logprobs_changes_no_token(engine_runs):
    crowd, plain = engine_runs["crowd"], engine_runs["plain"]
    assert np.array_equal(crowd[100].out_tokens, plain[100].out_tokens)
    assert plain[100].out_logprobs is None and plain[100].out_top_ids is None
    for i in range(16):
        assert np.array_equal(crowd[i].out_tokens, plain[i].out_tokens), i
        assert crowd[i].out_logprobs is None


def test_engine_counts_logprob_steps_only_where_a_row_asks(engine_runs):
    st = engine_runs["steps"]
    assert st["plain"] == 0 and st["alone"] > 0 and st["crowd"] > 0


def test_engine_every_reported_value_equals_the_twin_on_recomputed_logits(engine_runs):
    seen, r = engine_runs["seen"], engine_runs["alone"][100]
    assert len(seen) == 5 and [s[0] for s in seen] == r.out_tokens.tolist()
    for g, (tok, lp, ids, want_lp, want_ids) in enumerate(seen):
        assert np.array_equal(ids, want_ids) and np.array_equal(lp, want_lp.astype(np.float32))
        assert r.out_logprobs[g] == lp[0] and np.array_equal(r.out_top_logprobs[g], lp[1:])
        assert np.array_equal(r.out_top_ids[g], ids)


def test_engine_a_greedy_token_is_the_first_alternative(engine_runs):
    g = engine_runs["greedy"]
    ref, eng, _ = _run([_req(100), _req(101)])
    assert eng.logprob_steps == 0 and np.array_equal(g[100].out_tokens, ref[100].out_tokens)
    assert np.array_equal(g[100].out_top_ids[:, 0], g[100].out_tokens)
    assert np.array_equal(g[100].out_top_logprobs[:, 0], g[100].out_logprobs)
    assert g[101].out_logprobs is None


def test_engine_a_truncating_token_outside_the_alternatives_still_has_its_value(engine_runs):
    r, seen = engine_runs["wide"][100], engine_runs["seen_wide"]
    outside = [g for g in range(5) if r.out_tokens[g] not in r.out_top_ids[g]]
    assert outside, "top_k = 200 at T = 2 should draw beyond the five most likely at least once in five tokens"
    for g in outside:
        assert np.isfinite(r.out_logprobs[g]) and r.out_logprobs[g] < r.out_top_logprobs[g, 4]
        assert r.out_logprobs[g] == np.float32(seen[g][3][0])


def test_micro_pool_scores_the_requests_that_ask():
    """A realtime request served by the micro-forwards reports what it reports
    on the serving pool."""
    from tests.test_realtime_micro import _engine as micro_engine
    from llm_message_queue_amd.backend.engine import Request

    def serve(eng):
        rng = np.random.default_rng(9)
        pend = [Request(req_id=i, prompt=rng.integers(0, 1000, size=5 + i).astype(np.int32), gen_tokens=4, tier=i % 3,
                        **(dict(logprobs=2) if i in (0, 1) else {})) for i in range(6)]
        got = {}
        for _ in range(200):
            if not pend and not eng.active and not eng.queued_steps():
                break
            adm = {id(r) for r in eng.admit(pend)}
            pend = [r for r in pend if id(r) not in adm]
            eng.launch()
            eng.pump_micro()
            for r in eng.finish(block=True).completed:
                got[r.req_id] = r
        return got
    a = serve(micro_engine("off"))
    eng = micro_engine("micro")
    b = serve(eng)
    assert b[0].micro and not b[1].micro and eng.micro_steps > 0 and eng.logprob_steps > 0
    for i in range(6):
        assert np.array_equal(a[i].out_tokens, b[i].out_tokens)
    for i in (0, 1):
        assert _bits(a[i]) == _bits(b[i]) and a[i].out_logprobs.shape == (4,)
    assert all(b[i].out_logprobs is None for i in range(2, 6))


def test_sim_engine_reports_no_logprobs():
    from llm_message_queue_amd.backend.engine import Request
    from llm_message_queue_amd.backend.sim_engine import SimEngine
    eng = SimEngine(slots=8, max_ctx=32, token_budget=64)
    eng.admit([Request(req_id=1, prompt=np.arange(3, dtype=np.int32), gen_tokens=2, logprobs=2)])
    done = eng.drain()
    assert len(done) == 1 and done[0].out_logprobs is None and eng.logprob_steps == 0


# --------------------------------------------------------------------------- wire
def test_descriptor_carries_the_logprobs_flag_beside_top_k_and_top_p():
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, K_LOGP, LOGPROBS
    from tests.test_tier_caps import _gateway
    assert DESC_HDR == 20 and LOGPROBS == 1 << 30 and K_LOGP == 9
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _msgs()
    buf = np.zeros((len(msgs), DESC_HDR + 8), dtype=np.int32)
    gw._fill_descs(buf, msgs, 1, 8, {})
    assert buf[:, 11].tolist() == [(40 << 10) | LOGPROBS, LOGPROBS, 0, 0, 0, LOGPROBS]
    reqs = gw._foreign_requests(buf, 8)
    assert [r.logprobs >= 0 for r in reqs] == [True, True, False, False, False, True]
    assert [r.top_k for r in reqs] == [40, 0, 0, 0, 0, 0] and [r.top_p for r in reqs] == [1.0] * 6


@pytest.mark.parametrize("cap", [1, 7, 32])
def test_logprob_stream_is_cut_into_rows_and_reassembled_exactly(cap):
    from llm_message_queue_amd.gateway import descriptors as D
    rng = np.random.default_rng(cap)
    n = 5
    tokens = rng.integers(0, 128256, n).astype(np.int32)
    lp = rng.standard_normal(n).astype(np.float32)
    lp[2] = -np.inf
    ids = rng.integers(-1, 128256, (n, 5)).astype(np.int32)
    top = rng.standard_normal((n, 5)).astype(np.float32)
    top[1, 3] = np.nan
    stream = D.pack_logprob_stream(tokens, lp, ids, top)
    assert stream.dtype == np.int32 and len(stream) == n * D.LP_WORDS
    chunks = D.logprob_chunks(len(stream), cap)
    assert len(chunks) == -(-len(stream) // cap) > 1 and sum(c for _o, c in chunks) == len(stream)
    rows = np.zeros((len(chunks), D.DESC_HDR + cap), dtype=np.int32)
    rows[:, 0] = D.K_LOGP
    D._put64(rows, 1, [(1 << 40) + 5] * len(chunks))
    rows[:, 3] = 1
    for row, (off, c) in zip(rows, chunks):
        row[4] = off
        row[7] = len(stream)
        D.fill_logprob_row(row, stream, off, c)
    assert rows[:, 10].max() <= cap
    parts = {}
    half = len(rows) // 2
    D.take_logprob_rows(parts, 1, rows[:half])                         # (the rows may arrive in two exchanges)
    D.take_logprob_rows(parts, 1, rows[half:])
    assert list(parts) == [(1, (1 << 40) + 5)]
    back = D.unpack_logprob_stream(parts[(1, (1 << 40) + 5)])
    for got, want in zip(back, (tokens, lp, ids, top)):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got.view(np.int32), want.view(np.int32))


def _gen_msgs(n, flagged=True):
    """Messages with content-derived prompts; every third asks for nothing."""
    from llm_message_queue_amd.gateway.workload import Workload
    msgs = Workload(seed=11).make(n)
    for i, m in enumerate(msgs):
        m.id = f"g{i}"
        m.priority = 3
        if i % 3 != 2:
            sp = {"logprobs": i % 6} if flagged else {}                # (unflagged: the same draw, nothing asked)
            if i % 2:
                sp.update(temperature=0.9, seed=i)
            m.metadata = {"sampling": sp}
    return msgs


def _wire_cfg():
    from llm_message_queue_amd.utils.config import default_config
    c = default_config()
    c.queue.enable_metrics = False
    return c


def _wire_engine():
    from tests.test_gateway_distributed import engine
    return engine(slots=4, seed=0)                                     # (the same model on every rank)


def _serve_local(n, flagged=True):
    from llm_message_queue_amd.gateway.router import Gateway
    from tests.test_gateway_distributed import run_until_done
    gw = Gateway(_wire_cfg(), engine=_wire_engine(), use_gpu_preprocess=False, prompt_cap=8, gen_tokens=3)
    msgs = _gen_msgs(n, flagged)
    gw.submit(msgs)
    assert run_until_done([gw], n)
    return {m.id: m.metadata.get("generation") for m in msgs}


def _check_generation(gen, i):
    n = i % 6
    assert len(gen["tokens"]) == 3 and len(gen["token_logprobs"]) == 3
    assert all(lp is not None and lp <= 0 for lp in gen["token_logprobs"])
    if n == 0:
        assert "top_logprobs" not in gen
    else:
        assert len(gen["top_logprobs"]) == 3 and all(len(t) == n for t in gen["top_logprobs"])
        for t in gen["top_logprobs"]:
            assert all(set(e) == {"token", "logprob"} for e in t)
            assert [e["logprob"] for e in t] == sorted((e["logprob"] for e in t), reverse=True)


def _two_ranks(flagged, dialog=False, n=12):
    """``n`` messages submitted on rank 0 of two ranks in threads; returns the
    messages, the gateways and every row rank 1 sent to rank 0."""
    from llm_message_queue_amd.gateway.router import Gateway
    from llm_message_queue_amd.parallel.comm import FakeComm
    from tests.test_gateway_distributed import run_until_done
    comms = FakeComm.make(2)
    gws = [Gateway(_wire_cfg(), engine=_wire_engine(), comm=comms[r], use_gpu_preprocess=False, prompt_cap=8,
                   gen_tokens=3) for r in range(2)]
    rows = []
    inner = comms[1].all_to_all_rows_async

    def spy(send, recv_counts, width):
        rows.extend(np.array(r) for r in send[0])
        return inner(send, recv_counts, width)

    comms[1].all_to_all_rows_async = spy
    msgs = _gen_msgs(n, flagged)
    if dialog:
        for i, m in enumerate(msgs):
            m.conversation_id = f"c{i}"
    gws[0].submit(msgs)
    assert run_until_done(gws, n)
    assert gws[0].counters["remote_sent"] > 0 and not gws[0]._lp_parts and not gws[1]._done_lp[0]
    return msgs, gws, rows


def _done_rows_by_message(msgs, rows):
    """Message id -> its K_DONE row with the handle and the two times zeroed
    (they differ from run to run); every other column is compared."""
    from llm_message_queue_amd.gateway.descriptors import K_DONE, _get64
    by_handle = {m.handle: m.id for m in msgs}
    out = {}
    for r in rows:
        if r[0] == K_DONE:
            mid = by_handle[int(_get64(r.reshape(1, -1), 1)[0])]
            assert mid not in out
            r = r.copy()
            r[1:3] = 0
            r[5:9] = 0
            out[mid] = r
    return out


def test_generation_of_a_request_served_on_another_rank_equals_the_local_one():
    """Two ranks in threads: K_LOGP rows (36 words a request, 8 a row) ride
    ahead of the K_DONE, whose rows stay what they are without the flag."""
    import json
    from llm_message_queue_amd.gateway.descriptors import K_DONE, K_LOGP, _get64
    local = _serve_local(12)
    msgs, _gws, sent = _two_ranks(True)
    remote = [m for m in msgs if m.endpoint_id == "gpu1"]
    assert any("generation" in m.metadata for m in remote)
    for i, m in enumerate(msgs):
        if i % 3 == 2:
            assert "generation" not in m.metadata
            continue
        _check_generation(m.metadata["generation"], i)
        assert m.metadata["generation"] == local[m.id], (m.id, m.endpoint_id)
        json.dumps(m.metadata, allow_nan=False)
    plain_msgs, _gws, plain_sent = _two_ranks(False)
    assert all("generation" not in m.metadata for m in plain_msgs)
    # the K_DONE rows: column by column what they are without the flag (but for handle and times),
    # header only (no dialog turn here: nothing from col 9 on)
    done, plain_done = _done_rows_by_message(msgs, sent), _done_rows_by_message(plain_msgs, plain_sent)
    assert sorted(done) == sorted(plain_done) and len(done) > 0
    assert any(i % 3 != 2 for i in (int(mid[1:]) for mid in done))       # (flagged requests among them)
    for mid, r in done.items():
        assert np.array_equal(r, plain_done[mid]), mid
        assert r[3] == 1 and not r[9:].any()
    # K_LOGP rows only in the flagged run, each ahead of its K_DONE
    assert not [r for r in plain_sent if r[0] == K_LOGP]
    seen_done = set()
    lrows = 0
    for r in sent:
        h = int(_get64(r.reshape(1, -1), 1)[0])
        if r[0] == K_DONE:
            seen_done.add(h)
        elif r[0] == K_LOGP:
            lrows += 1
            assert h not in seen_done and 0 < r[10] <= 8 and r[7] == 36 and r[4] % 8 == 0
    assert lrows >= 5                                                  # (36 words, 8 a row: 5 rows a request)


def test_a_dialog_turn_that_asks_for_logprobs_keeps_its_history():
    """A conversation turn served on another rank carries its generated ids
    home in the K_DONE row's payload; the K_LOGP rows queued ahead of it
    under the same handle must not take them."""
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR
    msgs, gws, sent = _two_ranks(True, dialog=True)
    plain_msgs, plain_gws, plain_sent = _two_ranks(False, dialog=True)
    done, plain_done = _done_rows_by_message(msgs, sent), _done_rows_by_message(plain_msgs, plain_sent)
    assert sorted(done) == sorted(plain_done) and any(int(mid[1:]) % 3 != 2 for mid in done)
    for mid, r in done.items():
        assert r[10] == 3 and r[DESC_HDR:DESC_HDR + 3].any(), mid     # the turn's three generated ids
        assert np.array_equal(r, plain_done[mid]), mid
    for gw in (gws[0], plain_gws[0]):
        assert gw.counters["dialog_ids_real"] == 12 and gw.counters["dialog_ids_placeholder"] == 0
    hist, plain_hist = gws[0].conv_hist, plain_gws[0].conv_hist
    assert sorted(hist) == sorted(plain_hist) == sorted(f"c{i}" for i in range(12))
    for cid in hist:
        assert np.array_equal(hist[cid], plain_hist[cid]), cid
    for i, m in enumerate(msgs):                                       # ... and the log-probabilities arrive as well
        assert ("generation" in m.metadata) == (i % 3 != 2)
        if i % 3 != 2:
            _check_generation(m.metadata["generation"], i)


def _spawn_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from llm_message_queue_amd.gateway.router import Gateway
    from llm_message_queue_amd.parallel.comm import TorchComm
    comm = TorchComm()
    gw = Gateway(_wire_cfg(), engine=_wire_engine(), comm=comm, use_gpu_preprocess=False, prompt_cap=8, gen_tokens=3)
    msgs = _gen_msgs(12) if rank == 0 else []
    if msgs:
        gw.submit(msgs)
    done = False
    for _ in range(300):
        gw.tick()
        tot = comm.all_gather_i64(np.array([gw.counters["completed"]]))
        if tot.sum() >= 12:
            done = True
            break
    if rank == 0:
        out.put((done, {m.id: (m.endpoint_id, m.metadata.get("generation")) for m in msgs}))
    dist.destroy_process_group()


def test_generation_across_two_processes_equals_the_local_one():
    import queue as _q
    import torch.multiprocessing as mp
    from tests.test_gateway_distributed import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_spawn_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    local = _serve_local(12)                                           # (while the two ranks run)
    res = None
    for _ in range(240):
        try:
            res = q.get(timeout=1)
            break
        except _q.Empty:
            if any(p.exitcode not in (None, 0) for p in ps):
                break
    for p in ps:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert res is not None, [p.exitcode for p in ps]
    done, got = res
    assert done and any(ep == "gpu1" and gen is not None for ep, gen in got.values())
    for mid, (ep, gen) in got.items():
        assert gen == local[mid], (mid, ep)
    assert sum(gen is not None for _ep, gen in got.values()) == 8
