"""Stop tokens, stop sequences, ``max_tokens`` and ``min_tokens`` without a
GPU: the numpy twin of ``csrc/kernels/stop_kernels.h`` against a tail
comparison written here, the parser, the descriptors, the engine on the
reference ops (reap-time completion at several run-ahead depths), the gateway
on one rank and on two.  Everything is integer: every comparison is exact."""
import json
import os
import threading

import numpy as np
import pytest

from llm_message_queue_amd.ops.sampling import (STOP_ENT_WORDS, STOP_ENTRIES, STOP_LEN, STOP_ROW_WORDS, stop_match_reference,
                                                stop_table)


# --------------------------------------------------------------------------- the twin
def naive_stop(tok, hist, rows, ent):
    """The contract read literally: build the window as a list, compare
    tails entry by entry."""
    out = []
    for r, t0 in enumerate(tok):
        slot, a, b, mn, off, cnt = (int(x) for x in rows[r])
        w = []
        if hist is not None and 0 <= slot < hist.shape[0]:
            a = min(max(a, 0), hist.shape[1])
            b = min(max(b, a), hist.shape[1])
            w = list(hist[slot, a:b])
        w = [int(x) for x in w] + [int(t0)]
        hit = -1
        off = min(max(off, 0), len(ent))
        cnt = min(max(cnt, 0), STOP_ENTRIES, len(ent) - off)
        for k in range(cnt):
            ln = int(ent[off + k][0])
            if not 1 <= ln <= STOP_LEN or ln > len(w) or len(w) < mn:
                continue
            if all(int(ent[off + k][1 + i]) == w[len(w) - ln + i] for i in range(ln)):
                hit = k
                break
        out.append(hit)
    return np.asarray(out, dtype=np.int32)


def random_stop_case(rng, R, n_slots=5, stride=37, vocab=6):
    """Rows over a small vocabulary (so tails match often), with slots
    outside the table, spans that need clamping, lengths 0 and 9, entry
    ranges that leave the table."""
    hist = rng.integers(0, vocab, (n_slots, stride)).astype(np.int32)
    N = int(rng.integers(1, 4 * R + 2))
    ent = np.zeros((N, STOP_ENT_WORDS), dtype=np.int32)
    ent[:, 0] = rng.choice([0, 1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 9], N)
    ent[:, 1:] = rng.integers(0, vocab, (N, STOP_LEN))
    rows = np.zeros((R, STOP_ROW_WORDS), dtype=np.int32)
    rows[:, 0] = rng.integers(-1, n_slots + 1, R)
    rows[:, 1] = rng.integers(-3, stride + 3, R)
    rows[:, 2] = rows[:, 1] + rng.integers(-2, 12, R)
    rows[:, 3] = rng.integers(0, 6, R)
    rows[:, 4] = rng.integers(-1, N + 2, R)
    rows[:, 5] = rng.integers(-1, STOP_ENTRIES + 3, R)
    tok = rng.integers(0, vocab, R).astype(np.int32)
    # plant matches: copy a row's true tail into one of its entries
    for r in range(0, R, 3):
        s, a, b = int(rows[r, 0]), int(rows[r, 1]), int(rows[r, 2])
        off, cnt = int(rows[r, 4]), int(rows[r, 5])
        if 0 <= s < n_slots and 0 <= a <= b <= stride and 0 <= off and cnt > 0 and off + cnt <= N:
            w = list(hist[s, a:b]) + [int(tok[r])]
            ln = min(len(w), int(rng.integers(1, STOP_LEN + 1)))
            k = off + int(rng.integers(0, min(cnt, STOP_ENTRIES)))
            ent[k, 0] = ln
            ent[k, 1:1 + ln] = w[len(w) - ln:]
    return tok, hist, rows, ent


def test_twin_agrees_with_a_naive_tail_comparison_on_random_cases():
    rng = np.random.default_rng(5)
    hits = 0
    for _ in range(60):
        tok, hist, rows, ent = random_stop_case(rng, int(rng.integers(1, 40)))
        got = stop_match_reference(tok, hist, rows, ent)
        assert got.dtype == np.int32 and np.array_equal(got, naive_stop(tok, hist, rows, ent))
        hits += int((got >= 0).sum())
    assert hits > 100                                                   # (the cases do match)


def test_twin_on_constructed_cases():
    hist = np.full((3, 20), -7, dtype=np.int32)
    hist[1, 4:9] = [10, 11, 12, 13, 14]                                # generated so far, gen_from = 4
    hist[1, 0:4] = [12, 13, 14, 15]                                    # before the window
    ent = stop_table([[15], [14, 15], [10, 11, 12, 13, 14, 15], [12, 13, 14, 15], [9, 10, 11, 12, 13, 14, 15], [99]])
    T = np.array([15], dtype=np.int32)

    def one(row, tok=T):
        return int(stop_match_reference(tok, hist, np.array([row], dtype=np.int32), ent)[0])

    assert one([1, 4, 9, 0, 0, 6]) == 0                                # the lowest matching entry wins
    assert one([1, 4, 9, 0, 1, 5]) == 0 and one([1, 4, 9, 0, 2, 4]) == 0   # (offsets: [14 15] / the whole window)
    assert one([1, 4, 9, 0, 4, 2]) == -1                               # one longer than the window: no match
    assert one([1, 7, 9, 0, 3, 1]) == -1                               # [12 13 14 15] needs what lies before gen_from = 7
    assert one([1, 6, 9, 0, 3, 1]) == 0
    assert one([1, 0, 4, 0, 3, 1], np.array([16], dtype=np.int32)) == -1
    assert one([1, 4, 9, 6, 0, 6]) == 0 and one([1, 4, 9, 7, 0, 6]) == -1   # min_tokens at g + 1 and above
    assert one([-1, 4, 9, 0, 0, 6]) == 0 and one([3, 4, 9, 0, 1, 5]) == -1  # a slot outside: only t0 is compared
    assert one([1, 4, 9, 0, 5, 1]) == -1 and one([1, 4, 9, 0, 5, 1], np.array([99], dtype=np.int32)) == 0
    assert one([1, 4, 9, 0, 0, 0]) == -1 and one([1, 4, 9, 0, 6, 3]) == -1  # no entries; a range past the table
    assert one([1, -5, 99, 0, 0, 1]) == 0                              # a span clamped to the table
    bad = ent.copy()
    bad[0, 0], bad[1, 0] = 0, 9                                        # lengths 0 and 9 are ignored
    assert int(stop_match_reference(T, hist, np.array([[1, 4, 9, 0, 0, 6]], dtype=np.int32), bad)[0]) == 2
    assert int(stop_match_reference(T, None, np.array([[1, 4, 9, 0, 0, 6]], dtype=np.int32), ent)[0]) == 0
    with pytest.raises(ValueError):
        stop_table([[]])
    with pytest.raises(ValueError):
        stop_table([list(range(9))])
    assert stop_table([[1 << 31, -1, 5]]).tolist() == [[3, -1, -1, 5, 0, 0, 0, 0, 0]]


# --------------------------------------------------------------------------- the parser
def test_parser_ranges_and_defaults():
    from llm_message_queue_amd.models.message import SamplingParseError, stop_from_metadata as p
    assert p(None, 6) == p({}, 6) == p({"sampling": {"temperature": 0.5}}, 6) == (0, 0, [], 0)
    assert p({"sampling": {"max_tokens": 1}}, 6)[0] == 1 and p({"sampling": {"max_tokens": 6}}, 6)[0] == 6
    assert p({"sampling": {"max_tokens": 4, "min_tokens": 4}}, 6)[:2] == (4, 4)
    assert p({"sampling": {"min_tokens": 6}}, 6)[1] == 6 and p({"sampling": {"min_tokens": 0}}, 6)[1] == 0
    top = (1 << 31) - 1
    assert p({"sampling": {"stop_token_ids": [0, top]}}, 6) == (0, 0, [[0], [top]], 2)
    mx, mn, ent, n_tok = p({"sampling": {"stop_sequences": [[5, 5], list(range(8))], "stop_token_ids": [9, 3]}}, 6)
    assert ent == [[9], [3], [5, 5], list(range(8))] and n_tok == 2    # the stop tokens in the order given, then sequences
    assert len(p({"sampling": {"stop_token_ids": list(range(8))}}, 6)[2]) == 8
    assert len(p({"sampling": {"stop_token_ids": [1, 2, 3], "stop_sequences": [[4]] * 5}}, 6)[2]) == 8
    for bad in ({"max_tokens": 0}, {"max_tokens": 7}, {"max_tokens": 2.0}, {"max_tokens": True}, {"max_tokens": "3"},
                {"min_tokens": -1}, {"min_tokens": 7}, {"min_tokens": 1.5}, {"max_tokens": 3, "min_tokens": 4},
                {"stop_token_ids": []}, {"stop_token_ids": list(range(9))}, {"stop_token_ids": [1, 1]},
                {"stop_token_ids": [-1]}, {"stop_token_ids": [1 << 31]}, {"stop_token_ids": [1.0]},
                {"stop_token_ids": 5}, {"stop_token_ids": [True]},
                {"stop_sequences": []}, {"stop_sequences": [[]]}, {"stop_sequences": [list(range(9))]},
                {"stop_sequences": [5]}, {"stop_sequences": [[1, -2]]}, {"stop_sequences": [[1 << 31]]},
                {"stop_sequences": [[1]] * 9}, {"stop_token_ids": [1, 2, 3, 4], "stop_sequences": [[4]] * 5}):
        with pytest.raises(SamplingParseError):
            p({"sampling": bad}, 6)
    with pytest.raises(SamplingParseError):
        p({"sampling": 3}, 6)
    assert p({"sampling": {"max_tokens": 4096}}, 0)[0] == 4096          # (no configured count known: no cap)


def _stop_msgs():
    from llm_message_queue_amd.models.message import Message
    sp = [{"max_tokens": 1},
          {"stop_token_ids": [7, 3], "stop_sequences": [[1, 2, 3]], "min_tokens": 2},
          {"min_tokens": 0},
          {"temperature": 0.8, "seed": 7},
          None,
          {"max_tokens": 2, "stop_token_ids": [5, 5], "min_tokens": 1},                    # one bad key
          {"max_tokens": 9, "min_tokens": 2, "stop_sequences": [[4, 4]]},                  # above the configured 2
          {"stop_token_ids": [1, 2, 3, 4], "stop_sequences": [[4]] * 5, "logprobs": 1},    # 9 entries together
          {"min_tokens": 2, "max_tokens": 1},
          {"stop_token_ids": [9, 9], "stop_sequences": [[1, 2]]},                          # a bad list, a good one
          {"stop_token_ids": [9, 8], "stop_sequences": [[1, 2], []]}]
    msgs = [Message(id=f"s{i}", content="x", metadata={"sampling": s} if s is not None else {}) for i, s in enumerate(sp)]
    for i, m in enumerate(msgs):
        m.tier = i % 4
        m.prompt_ids = np.arange(4, dtype=np.uint32) + i
    return msgs


def test_lenient_path_and_write_back_only_where_in_effect():
    from llm_message_queue_amd.models.message import default_seed
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])                                   # (gen_tokens = 2)
    msgs = _stop_msgs()
    reqs = [gw._make_request(m, 2) for m in msgs]
    md = [m.metadata for m in msgs]
    assert md[0]["sampling"] == {"temperature": 0.0, "seed": default_seed("s0"), "max_tokens": 1}
    assert reqs[0].gen_tokens == 1 and reqs[0].finish and reqs[0].stop is None
    assert md[1]["sampling"] == {"temperature": 0.0, "seed": default_seed("s1"), "min_tokens": 2,
                                 "stop_token_ids": [7, 3], "stop_sequences": [[1, 2, 3]]}
    assert reqs[1].gen_tokens == 2 and reqs[1].min_tokens == 2 and reqs[1].stop == [[7], [3], [1, 2, 3]] and reqs[1].finish
    assert set(md[2]["sampling"]) == {"temperature", "seed"} and not reqs[2].finish        # the default, named
    assert md[3]["sampling"] == {"temperature": 0.8, "seed": 7} and not reqs[3].finish and reqs[3].gen_tokens == 2
    assert "sampling" not in md[4] and not reqs[4].finish and reqs[4].stop is None
    assert all("sampling_error" not in md[i] for i in range(5))
    # a bad key is off and reported, the others stay in effect
    assert "stop_token_ids" in md[5]["sampling_error"] and "max_tokens" not in md[5]["sampling_error"]
    assert set(md[5]["sampling"]) == {"temperature", "seed", "max_tokens", "min_tokens"}
    assert reqs[5].stop is None and reqs[5].min_tokens == 1 and reqs[5].gen_tokens == 2
    assert "max_tokens" in md[6]["sampling_error"] and "stop_sequences" not in md[6]["sampling_error"]
    assert reqs[6].gen_tokens == 2 and reqs[6].min_tokens == 2 and reqs[6].stop == [[4, 4]]
    assert "max_tokens" not in md[6]["sampling"] and md[6]["sampling"]["stop_sequences"] == [[4, 4]]
    assert "entries" in md[7]["sampling_error"] and reqs[7].stop is None and not reqs[7].finish
    assert set(md[7]["sampling"]) == {"temperature", "seed", "logprobs"}
    assert "min_tokens" in md[8]["sampling_error"] and reqs[8].gen_tokens == 1 and reqs[8].min_tokens == 0
    # a bad list turns itself off and leaves the other list in effect
    assert "stop_token_ids" in md[9]["sampling_error"] and "stop_sequences" not in md[9]["sampling_error"]
    assert reqs[9].stop == [[1, 2]] and md[9]["sampling"]["stop_sequences"] == [[1, 2]]
    assert "stop_token_ids" not in md[9]["sampling"] and reqs[9].finish
    assert "stop_sequences" in md[10]["sampling_error"] and "stop_token_ids" not in md[10]["sampling_error"]
    assert reqs[10].stop == [[9], [8]] and md[10]["sampling"]["stop_token_ids"] == [9, 8]
    assert "stop_sequences" not in md[10]["sampling"]
    # a replay of the written-back values parses to the same
    again = gw._make_request(msgs[1], 2)
    assert again.stop == reqs[1].stop and again.min_tokens == 2 and "sampling_error" not in md[1]


def test_rest_answers_400_on_a_bad_stop_key():
    from starlette.testclient import TestClient
    from llm_message_queue_amd.api.server import create_app
    from llm_message_queue_amd.gateway.app import GatewayApp
    from llm_message_queue_amd.utils.config import default_config
    cfg = default_config()
    cfg.preprocessor.batch_window_us = 200
    n = cfg.backend.gen_tokens
    app = GatewayApp(cfg, use_gpu=False, simulate_ms=(1, 1, 1, 1))
    try:
        with TestClient(create_app(app)) as c:
            def post(sp):
                return c.post("/api/v1/messages", content=json.dumps({"content": "hi", "metadata": {"sampling": sp}}),
                              headers={"content-type": "application/json"})
            for bad in ({"max_tokens": n + 1}, {"max_tokens": 0}, {"min_tokens": n + 1}, {"stop_token_ids": []},
                        {"stop_token_ids": [3, 3]}, {"stop_sequences": [[]]}, {"stop_sequences": [list(range(9))]},
                        {"stop_token_ids": [1, 2, 3, 4, 5], "stop_sequences": [[1], [2], [3], [4]]},
                        {"max_tokens": 1, "min_tokens": 2}):
                r = post(bad)
                assert r.status_code == 400 and any(k in r.text for k in bad), bad
            assert post({"max_tokens": n, "min_tokens": 1, "stop_token_ids": [5], "stop_sequences": [[1, 2]]}).status_code == 202
            assert post({"max_tokens": 1, "temperature": 0.9, "seed": 3, "top_k": 5}).status_code == 202
    finally:
        app.stop()


# --------------------------------------------------------------------------- descriptors
def test_stop_section_rides_behind_the_first_two_sections_which_do_not_change():
    from llm_message_queue_amd.gateway.descriptors import (pack_extension, pack_stop_section, unpack_extension,
                                                            unpack_stop_section)
    old = pack_extension([5, 6], [1, 2, 3], [0.5, -1.0, 100.0])
    none = np.zeros(0, dtype=np.int32)
    assert unpack_stop_section(old) == (0, []) and unpack_stop_section(none) == (0, [])
    assert pack_stop_section(old, 3, []) is not None and pack_stop_section(old, 3, []).tolist() == old.tolist()
    assert len(pack_stop_section(none, 3, None)) == 0                   # min_tokens alone: nothing travels
    ents = [[7], [(1 << 31) - 1], [1, 2, 3], list(range(8))]
    for ext in (old, none, pack_extension([9], None, None)):
        w = pack_stop_section(ext, 2, ents)
        assert w.dtype == np.int32
        a, bi, bv = unpack_extension(w)
        a0, bi0, bv0 = unpack_extension(ext)
        assert a.tolist() == a0.tolist() and bi.tolist() == bi0.tolist() and bv.tolist() == bv0.tolist()
        mn, got = unpack_stop_section(w)
        assert mn == 2 and [e.tolist() for e in got] == ents
        if len(ext):
            assert w[:len(ext)].tolist() == ext.tolist()                # old streams keep their words
    # a stream cut short ends the list where it leaves the stream
    w = pack_stop_section(none, 0, [[1, 2], [3, 4, 5]])
    assert [e.tolist() for e in unpack_stop_section(w[:-1])[1]] == [[1, 2]]
    assert unpack_stop_section(w[:3]) == (0, [])


def test_finish_column_and_flag_round_trip():
    from llm_message_queue_amd.gateway.descriptors import (DESC_HDR, FINISH, GEN_MASK, pack_finish, pack_gen, unpack_finish,
                                                            unpack_gen)
    assert DESC_HDR == 20 and FINISH & GEN_MASK == 0
    for gen in (1, 4, 4096):
        for pm in (0, 1, 1000):
            assert unpack_gen(pack_gen(gen, pm / 1000.0) | FINISH) == (gen, pm / 1000.0)
            assert not pack_gen(gen, pm / 1000.0) & FINISH
    assert unpack_finish(0) == ("", -1) and unpack_finish(pack_finish("length")) == ("length", -1)
    for k in range(STOP_ENTRIES):
        assert unpack_finish(pack_finish("stop", k)) == ("stop", k)
    assert unpack_finish(pack_finish("", 3)) == ("", -1) and unpack_finish(99) == ("", -1)


def test_dispatch_row_carries_the_own_count_and_the_flag_and_nothing_else_changes():
    from llm_message_queue_amd.backend.engine import Request
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, EXTENSION, FINISH, unpack_stop_section
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    gw._hist_wait, gw._await_hist, gw._hist_len = {}, {}, {}
    msgs = _stop_msgs()
    buf = np.zeros((len(msgs), DESC_HDR + 8), dtype=np.int32)
    ctx = gw._fill_descs(buf, msgs, 1, 8, {})
    reqs = gw._foreign_requests(buf, 8)
    assert [r.gen_tokens for r in reqs] == [1, 2, 2, 2, 2, 2, 2, 2, 1, 2, 2]
    assert [r.finish for r in reqs] == [True, True, False, False, False, True, True, False, True, True, True]
    assert [bool(c & FINISH) for c in buf[:, 9].tolist()] == [r.finish for r in reqs]
    # only a request with stop entries waits for an extension; max_tokens / min_tokens alone do not
    waits = [False, True, False, False, False, False, True, False, False, True, True]
    assert [bool(c & EXTENSION) for c in buf[:, 4].tolist()] == waits
    assert [len(c[2]) > 0 for c in ctx] == waits
    mn, ent = unpack_stop_section(ctx[1][2])
    assert mn == 2 and [e.tolist() for e in ent] == [[7], [3], [1, 2, 3]]
    # ... and arrives with the K_HIST stream
    block_pub = {1: [(m.handle, c[1], c[0], c[2]) for m, c in zip(msgs, ctx) if len(c[2])]}
    gw._hist_pub = block_pub
    block = gw._hist_block(1, 0, 8, DESC_HDR + 8)
    for r in (reqs[1], reqs[6]):
        gw._hist_wait[(1, r.meta[1])] = r
        gw._await_hist[(1, r.meta[1])] = r
    block[:, 3] = 1
    ready = gw._take_histories(1, block)
    assert len(ready) == 2 and [e.tolist() for e in reqs[1].stop] == [[7], [3], [1, 2, 3]] and reqs[1].min_tokens == 2
    assert [e.tolist() for e in reqs[6].stop] == [[4, 4]] and reqs[6].allowed is None and reqs[6].logit_bias is None
    assert isinstance(reqs[1], Request)
    # rows that name no stop key in effect are what they are without the feature
    stripped = _stop_msgs()
    for m, o in zip(stripped, msgs):
        m.handle, m.arrival_ns, m.enqueued_at = o.handle, o.arrival_ns, o.enqueued_at
        sp = m.metadata.get("sampling")
        for k in ("max_tokens", "min_tokens", "stop_token_ids", "stop_sequences"):
            if sp:
                sp.pop(k, None)
    ref = np.zeros_like(buf)
    gw._fill_descs(ref, stripped, 1, 8, {})
    assert np.array_equal(buf[[2, 3, 4, 7]], ref[[2, 3, 4, 7]])
    others = np.delete(np.arange(buf.shape[1]), [4, 9])
    assert np.array_equal(buf[:, others], ref[:, others])


# --------------------------------------------------------------------------- the engine on the reference ops
GEN = 6


def _engine(inflight=1, slots=8, **kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=slots, max_ctx=64, token_budget=256, device="cpu", impl="ref",
                         max_inflight=inflight, **kw)


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=GEN, **kw)


def drive(eng, reqs=()):
    """Launch until nothing is active, never reaping by hand: a step is
    reaped when ``max_inflight`` newer ones are queued, so a stop becomes
    known that many launches late, as on a GPU."""
    if reqs:
        assert len(eng.admit(list(reqs))) == len(reqs)
    for _ in range(200):
        if not eng.active:
            break
        eng.launch()
    return {r.req_id: r for r in eng.finish(block=True).completed}


_BASE = {}


def baseline():
    """Greedy tokens of requests 0..3 with no stop key, computed once."""
    if not _BASE:
        done = drive(_engine(), [_req(i) for i in range(4)])
        _BASE.update({i: done[i].out_tokens.copy() for i in range(4)})
        assert all(len(t) == GEN for t in _BASE.values())
    return _BASE


def expected_cut(tokens, entries, min_tokens=0):
    """The baseline cut after the first match, by the twin: (tokens, entry)."""
    ent = stop_table(entries)
    hist = np.asarray(tokens, dtype=np.int32)[None, :]
    for g in range(len(tokens)):
        k = int(stop_match_reference(hist[0, g:g + 1], hist, [[0, 0, g, min_tokens, 0, len(ent)]], ent)[0])
        if k >= 0:
            return list(tokens[:g + 1]), k
    return list(tokens), -1


def first_index(tokens, want):
    """The first index i >= want whose token does not occur before it.  A
    greedy baseline of the random-weight model has one; an output that repeats
    itself from ``want`` on is a broken engine, and fails here."""
    for i in range(want, len(tokens)):
        if int(tokens[i]) not in [int(t) for t in tokens[:i]]:
            return i
    raise AssertionError(f"the baseline repeats every token from index {want} on: {list(tokens)}")


def fresh_at(base, i):
    """The lowest request id of the baseline whose token ``i`` does not occur
    before it in its own output (there has to be one, as above)."""
    for j in sorted(base):
        if int(base[j][i]) not in [int(t) for t in base[j][:i]]:
            return j
    raise AssertionError(f"every baseline request repeats an earlier token at index {i}: "
                         f"{ {j: list(t) for j, t in base.items()} }")


@pytest.mark.parametrize("inflight", [1, 2, 3])
@pytest.mark.parametrize("kind", ["token", "sequence"])
def test_engine_stops_request_1_on_its_own_baseline_token(inflight, kind):
    base = baseline()
    b1 = base[1]
    i = first_index(b1, 2)
    entries = [[int(b1[i])]] if kind == "token" else [[int(b1[i - 1]), int(b1[i])]]
    want, k = expected_cut(b1, [[1 << 20]] + entries)
    assert k == 1 and 2 <= len(want) < GEN
    eng = _engine(inflight)
    got = drive(eng, [_req(j, stop=([[1 << 20]] + entries) if j == 1 else None, finish=j == 1) for j in range(4)])
    r = got[1]
    assert r.out_tokens.tolist() == want and r.generated == len(want)
    assert r.finish_reason == "stop" and r.stop_entry == 1
    for j in (0, 2, 3):
        assert got[j].out_tokens.tolist() == base[j].tolist() and got[j].finish_reason == "length"
    assert eng.stopped_total == 1 and eng.completed_total == 4 and eng.stop_steps >= len(want)
    # rows computed after the stop: the run-ahead, as far as the request still had tokens to go
    assert eng.stop_dropped_rows == min(inflight - 1, GEN - len(want))
    assert eng.completed_tokens == sum(len(got[j].prompt) + got[j].generated - 1 for j in range(4))
    assert sorted(eng.free) == list(range(8)) and not eng.active
    assert (eng.d_hist is not None) == (kind == "sequence")            # stop tokens alone read no history


def test_engine_inflight_depths_agree():
    base = baseline()
    b2 = base[2]
    entries = [[int(b2[1]), int(b2[2])], [int(b2[0])]]
    outs = []
    for inflight in (1, 2):
        got = drive(_engine(inflight), [_req(j, stop=entries if j == 2 else None) for j in range(4)])
        outs.append({j: (got[j].out_tokens.tolist(), got[j].finish_reason, got[j].stop_entry, got[j].generated)
                     for j in range(4)})
    assert outs[0] == outs[1] and outs[0][2] == ([int(b2[0])], "stop", 1, 1)


def test_min_tokens_filters_the_stop_decision():
    base = baseline()
    b1 = base[1]
    entries = [[int(b1[0])]]
    for inflight in (1, 2):
        r = drive(_engine(inflight), [_req(1, stop=entries)])[1]
        assert r.out_tokens.tolist() == [int(b1[0])] and r.finish_reason == "stop"
        r = drive(_engine(inflight), [_req(1, stop=entries, min_tokens=2)])[1]
        want, k = expected_cut(b1, entries, min_tokens=2)
        assert len(want) >= 2 and r.out_tokens.tolist() == want        # not at index 0; the tokens are unchanged
        assert r.finish_reason == ("stop" if k >= 0 else "length")


def test_max_tokens_gives_length_and_needs_no_kernel():
    base = baseline()
    for inflight in (1, 2):
        eng = _engine(inflight)
        got = drive(eng, [_req(j, max_tokens=2 if j == 1 else 0) for j in range(4)])
        assert got[1].out_tokens.tolist() == base[1][:2].tolist() and got[1].finish_reason == "length"
        assert got[1].gen_tokens == 2 and got[1].generated == 2 and got[1].stop_entry == -1
        assert all(got[j].out_tokens.tolist() == base[j].tolist() for j in (0, 2, 3))
        assert eng.stop_steps == 0 and eng.h_stop is None and eng.stopped_total == 0
        assert eng.completed_tokens == sum(len(got[j].prompt) + got[j].generated - 1 for j in range(4))
    r = drive(_engine(), [_req(1, max_tokens=99)])[1]                   # the configured count stays the cap
    assert r.generated == GEN


def test_a_request_completed_at_launch_before_its_stop_was_reaped_is_cut():
    """Run-ahead 3 and a stop at the last-but-one token: the launch of the
    last token completes the request, and parks its dialog, before the reap
    sees the match.  The request is the first of the baseline whose
    last-but-one token is new in its output, so the match is there and nowhere
    earlier."""
    from llm_message_queue_amd.backend.engine import LP_TOP
    base = baseline()
    i = GEN - 2
    who = fresh_at(base, i)
    b = base[who]
    eng = _engine(3)
    plain = drive(_engine(3), [_req(j, logprobs=2 if j == who else -1) for j in range(4)])[who]
    got = drive(eng, [_req(j, stop=[[int(b[i])]] if j == who else None, logprobs=2 if j == who else -1,
                           conv=55 if j == who else -1) for j in range(4)])
    r = got[who]
    assert r.out_tokens.tolist() == b[:i + 1].tolist() and r.finish_reason == "stop" and r.generated == i + 1
    assert r.out_logprobs.shape == (i + 1,) and r.out_top_ids.shape == (i + 1, LP_TOP) \
        and r.out_top_logprobs.shape == (i + 1, LP_TOP)
    assert np.array_equal(r.out_logprobs, plain.out_logprobs[:i + 1])       # cut, not recomputed
    assert np.array_equal(r.out_top_ids, plain.out_top_ids[:i + 1])
    assert np.array_equal(r.out_top_logprobs, plain.out_top_logprobs[:i + 1])
    assert eng.stop_dropped_rows == 1 and eng.stopped_total == 1
    assert eng.completed_tokens == sum(len(got[j].prompt) + got[j].generated - 1 for j in range(4))
    # the context parked at the launch of the last token is corrected to what the cut turn holds
    assert eng.resident_context(55) == len(r.prompt) + r.generated - 1
    for j in range(4):
        if j != who:
            assert got[j].out_tokens.tolist() == base[j].tolist() and got[j].finish_reason == "length"
    # a match on the very last token is a stop too, and cuts nothing
    last = fresh_at(base, GEN - 1)
    r = drive(_engine(2), [_req(last, stop=[[int(base[last][GEN - 1])]])])[last]
    assert r.out_tokens.tolist() == base[last].tolist() and r.finish_reason == "stop" and r.generated == GEN


def test_a_request_admitted_into_the_freed_slot_gets_its_solo_tokens():
    base = baseline()
    b1 = base[1]
    i = first_index(b1, 1)
    for inflight in (1, 2, 3):
        eng = _engine(inflight, slots=1)
        assert len(eng.admit([_req(1, stop=[[int(b1[i - 1]), int(b1[i])]])])) == 1
        late = _req(2)
        done, admitted_at = {}, -1
        for step in range(60):
            if admitted_at < 0 and eng.free:
                assert len(eng.admit([late])) == 1                      # the moment the reap freed the slot
                admitted_at = step
            if not eng.active:
                break
            eng.launch()
            done.update({r.req_id: r for r in eng.finish(block=False).completed} if inflight == 1 else {})
        done.update({r.req_id: r for r in eng.finish(block=True).completed})
        assert done[1].out_tokens.tolist() == b1[:i + 1].tolist() and done[1].slot == done[2].slot == 0
        assert done[2].out_tokens.tolist() == base[2].tolist()          # rows queued for request 1 did not reach it
        # admitted as soon as the stop was reaped, not after the configured count
        assert admitted_at <= 1 + i + inflight


def test_a_dialog_turn_that_stops_early_parks_what_it_generated():
    base = baseline()
    b1 = base[1]
    i = first_index(b1, 1)
    for inflight in (1, 2, 3):
        eng = _engine(inflight)
        turn = _req(1, stop=[[int(b1[i])]], conv=77)
        r = drive(eng, [turn])[1]
        plen = len(r.prompt)
        assert r.generated == i + 1 and eng.resident_context(77) == plen + r.generated - 1
        nxt = _req(2, conv=77)
        r2 = drive(eng, [nxt])[2]
        assert r2.reused == plen + i and r2.slot == r.slot
        # ... and the next turn computes what it computes over a dialog prefilled in one piece
        solo = _engine()
        full = _req(2)
        full.prompt = np.concatenate([r.prompt, r.out_tokens[:-1], full.prompt]).astype(np.int32)
        assert drive(solo, [full])[2].out_tokens.tolist() == r2.out_tokens.tolist()


def test_an_aborted_attempt_is_not_stopped_by_its_old_steps():
    base = baseline()
    b1 = base[1]
    i = first_index(b1, 1)
    eng = _engine(3)
    r = _req(1, stop=[[int(b1[i])]])
    eng.admit([r])
    for _ in range(i + 1):
        eng.launch()                                                    # the matching token is launched, not reaped
    assert eng.cancel([1]) == [r] and r.aborted
    assert eng.finish(block=True).completed == [] and r.finish_reason == "" and eng.stopped_total == 0
    again = drive(eng, [r])[1]                                          # the retry is a new attempt
    assert again.out_tokens.tolist() == b1[:i + 1].tolist() and eng.stopped_total == 1


def test_without_the_keys_the_staging_buffer_and_the_launches_are_what_they_were():
    """An engine that has served a stop request stages, for requests that name
    no key, byte for byte what a fresh engine of this tree stages, and passes
    ``forward`` no ``stop``: no state of a stop request leaks into later
    steps.  It does not compare with the bytes of the tree before the
    feature; that the default buffer is unchanged follows from the code (the
    stop block is appended behind every earlier block and has zero length
    when no sampled row has an entry)."""
    base = baseline()
    plain = lambda: [_req(j) for j in (0, 2, 3)]                        # noqa: E731
    used = _engine()
    drive(used, [_req(1, stop=[[int(base[1][0]), 5], [int(base[1][1])]])])
    assert used.h_stop is not None and used.d_hist is not None
    fresh = _engine()
    seen = []
    for eng in (used, fresh):
        fwd = eng.model.forward

        def spy(*a, _f=fwd, **kw):
            seen.append(sorted(kw))
            return _f(*a, **kw)
        eng.model.forward = spy
        eng.admit(plain())
    for _ in range(GEN):                                                # the prompts' step, then GEN - 1 decode steps
        for eng in (used, fresh):
            for p in eng._pins:
                p.zero_()
        n0 = len(seen)
        used.launch()
        fresh.launch()
        assert seen[n0] == seen[n0 + 1] == ["n_dec", "tiles"]
        k = (used.step_id - 1) % len(used._pins), (fresh.step_id - 1) % len(fresh._pins)
        assert used._pins[k[0]].numpy().tobytes() == fresh._pins[k[1]].numpy().tobytes()
        used.finish(block=True)
        fresh.finish(block=True)
    assert not used.active and not fresh.active
    assert used.stop_steps == 2 and fresh.stop_steps == 0


def test_forward_with_stop_returns_the_flags_beside_the_tokens():
    import torch
    from llm_message_queue_amd.models.llama_stub import HeadOut, LlamaConfig, LlamaStub, Stops
    m = LlamaStub(LlamaConfig.tiny(), 4, 32, device=torch.device("cpu"), impl="ref", seed=0)
    tok = torch.tensor([5, 6, 7, 8, 9], dtype=torch.long)
    pos = torch.tensor([0, 1, 2, 0, 1], dtype=torch.int32)
    slot = torch.tensor([0, 0, 0, 2, 2], dtype=torch.int32)
    samp = torch.tensor([2, 4], dtype=torch.long)
    plain = m.forward(tok, pos, slot, samp)
    assert torch.is_tensor(plain)
    t0 = [int(x) for x in plain]
    hist = torch.full((4, 32), -1, dtype=torch.int32)
    ent = torch.from_numpy(stop_table([[7, t0[0]], [t0[1]], [8, 9, t0[1]]]))
    rows = torch.tensor([[0, 2, 3, 0, 0, 1], [2, 0, 2, 0, 1, 2]], dtype=torch.int32)
    rec = torch.tensor([2, 3, 4], dtype=torch.int32)
    res = m.forward(tok, pos, slot, samp, stop=Stops(hist, rec, torch.tensor([0, 1]), rows, ent))
    assert isinstance(res, HeadOut) and res.lp is None and res.ids is None
    out, flags = res.tokens, res.stop_flags
    assert out.tolist() == t0 and flags.dtype == torch.int32 and flags.tolist() == [0, 0]
    assert hist[0, 2] == 7 and hist[2, 0] == 8 and hist[2, 1] == 9 and hist[0, 0] == -1
    rows[1, 4], rows[1, 5] = 2, 1                                       # only the three-token entry
    res = m.forward(tok, pos, slot, samp, logp=torch.tensor([1]),
                    stop=Stops(hist, rec, torch.tensor([1]), rows[1:].contiguous(), ent))
    assert res.tokens.tolist() == t0 and res.stop_flags.tolist() == [0] and res.lp.shape == (1, 6)
    assert res.ids.shape == (1, 5)
    res = m.forward(tok, pos, slot, samp, logp=torch.tensor([1]))
    assert res.tokens.tolist() == t0 and res.lp.shape == (1, 6) and res.stop_flags is None


# --------------------------------------------------------------------------- the gateway, one rank and two
def _cfg():
    from llm_message_queue_amd.utils.config import default_config
    c = default_config()
    c.queue.enable_metrics = False
    return c


def _gw_engine(slots):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    micro = LlamaConfig(vocab=512, dim=2048, layers=1, heads=16, kv_heads=4, ffn=256)
    return BackendEngine(micro, slots=slots, max_ctx=64, token_budget=64, device="cpu", impl="ref", seed=0)


def _gw_msgs(sps, conv=""):
    from llm_message_queue_amd.models.message import Message
    return [Message(id=f"m{i}", content=f"hello number {i} how are you today", priority=3, user_id="u",
                    conversation_id=conv, metadata={"sampling": dict(sp)} if sp is not None else {})
            for i, sp in enumerate(sps)]


def _gateway(engine, comm=None):
    from llm_message_queue_amd.gateway.router import Gateway
    kw = {"comm": comm} if comm is not None else {}
    return Gateway(_cfg(), engine=engine, use_gpu_preprocess=False, prompt_cap=8, gen_tokens=GEN, **kw)


def _tick_until(gws, n, max_ticks=400):
    for _ in range(max_ticks):
        if len(gws) == 1:
            gws[0].tick()
        else:
            ths = [threading.Thread(target=g.tick) for g in gws]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
        if sum(g.counters["completed"] for g in gws) >= n:
            return True
    return False


N_GW = 12
_GW_BASE = []


def gateway_baseline():
    """``generation.tokens`` of the N_GW messages at the configured count."""
    if not _GW_BASE:
        gw = _gateway(_gw_engine(16))
        msgs = _gw_msgs([{"max_tokens": GEN}] * N_GW)
        gw.submit(msgs)
        assert _tick_until([gw], N_GW)
        for m in msgs:
            g = m.metadata["generation"]
            assert g["finish_reason"] == "length" and len(g["tokens"]) == GEN and set(g) == {"tokens", "finish_reason"}
            _GW_BASE.append(g["tokens"])
    return _GW_BASE


def _stop_sps(bt):
    kinds = (lambda t: {"stop_token_ids": [t[2]]},
             lambda t: {"stop_sequences": [[t[1], t[2]]], "logprobs": 2},
             lambda t: {"max_tokens": 3},
             lambda t: {"stop_token_ids": [t[0]], "min_tokens": 2, "stop_sequences": [[t[3], t[4]]]})
    return [kinds[i % 4](t) for i, t in enumerate(bt)]


def _check_generation(m, sp, t):
    g = m.metadata["generation"]
    st = [[x] for x in sp.get("stop_token_ids", [])] + sp.get("stop_sequences", [])
    want, k = expected_cut(t[:sp.get("max_tokens", GEN)], st, sp.get("min_tokens", 0)) if st \
        else (t[:sp.get("max_tokens", GEN)], -1)
    assert g["tokens"] == want, (sp, g, t)
    assert g["finish_reason"] == ("stop" if k >= 0 else "length")
    if k >= 0:
        assert g["stop_reason"] == (st[k][0] if k < len(sp.get("stop_token_ids", [])) else st[k])
    else:
        assert "stop_reason" not in g
    if "logprobs" in sp:
        assert len(g["token_logprobs"]) == len(g["top_logprobs"]) == len(want)
        assert all(len(a) == sp["logprobs"] for a in g["top_logprobs"])
    else:
        assert set(g) <= {"tokens", "finish_reason", "stop_reason"}


def test_gateway_writes_finish_reason_and_leaves_other_messages_alone():
    bt = gateway_baseline()
    sps = _stop_sps(bt)
    sps[5], sps[6] = {"logprobs": 1}, None                              # no stop key: today's records
    gw = _gateway(_gw_engine(16))
    msgs = _gw_msgs(sps)
    gw.submit(msgs)
    assert _tick_until([gw], N_GW)
    for i, (m, sp, t) in enumerate(zip(msgs, sps, bt)):
        if i == 5:
            g = m.metadata["generation"]
            assert set(g) == {"tokens", "token_logprobs", "top_logprobs"} and g["tokens"] == t
        elif i == 6:
            assert "generation" not in m.metadata and "sampling" not in m.metadata
        else:
            _check_generation(m, sp, t)
    assert gw.engine.stopped_total >= 6


def gw_conv_key(cid):
    from llm_message_queue_amd.gateway.descriptors import conv_key
    return conv_key(cid)


def test_gateway_dialog_history_keeps_the_matched_tokens():
    bt = gateway_baseline()
    gw = _gateway(_gw_engine(16))
    m = _gw_msgs([{"stop_token_ids": [bt[0][2]]}], conv="c1")[0]
    gw.submit([m])
    assert _tick_until([gw], 1)
    want, _k = expected_cut(bt[0], [[bt[0][2]]])
    assert m.metadata["generation"]["tokens"] == want
    nxt = _gw_msgs([None], conv="c1")[0]
    nxt.id = "m-next"
    hist, _pre = gw._dialog_context(nxt)
    # what the parked KV holds: the prompt and every generated id but the last, which was never fed back
    assert [int(t) for t in hist[-(len(want) - 1):]] == want[:-1] and len(want) == 3
    assert len(hist) == gw.engine.resident_context(gw_conv_key("c1")) == len(m.prompt_ids[:8]) + len(want) - 1


def test_null_engine_writes_no_generation():
    from llm_message_queue_amd.backend.null_engine import NullEngine
    import inspect
    kw = {"slots": 8} if "slots" in inspect.signature(NullEngine.__init__).parameters else {}
    gw = _gateway(NullEngine(**kw))
    msgs = _gw_msgs([{"max_tokens": 2, "stop_token_ids": [1]}])
    gw.submit(msgs)
    assert _tick_until([gw], 1)
    assert "generation" not in msgs[0].metadata and msgs[0].metadata["sampling"]["max_tokens"] == 2


def _gloo_stop_worker(rank, world, port, sps, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from llm_message_queue_amd.parallel.comm import TorchComm
    comm = TorchComm()
    gw = _gateway(_gw_engine(4), comm)
    msgs = _gw_msgs(sps) if rank == 0 else []
    if rank == 0:
        gw.submit(msgs)
    for _ in range(400):
        gw.tick()
        if comm.all_gather_i64(np.array([gw.counters["completed"]])).sum() >= len(sps):
            break
    g = comm.all_gather_i64(np.array([gw.counters["remote_sent"], gw.engine.stopped_total]))
    if rank == 0:
        out.put(([m.metadata.get("generation") for m in msgs], [m.metadata.get("sampling") for m in msgs],
                 [m.endpoint_id for m in msgs], g.tolist()))
    dist.destroy_process_group()


def test_two_ranks_on_gloo_return_the_generation_a_local_run_returns():
    import queue as _q
    import torch.multiprocessing as mp
    from tests.test_gateway_distributed import _free_port
    bt = gateway_baseline()
    sps = _stop_sps(bt)
    local = _gw_msgs(sps)
    gw = _gateway(_gw_engine(16))
    gw.submit(local)
    assert _tick_until([gw], N_GW)
    for m, sp, t in zip(local, sps, bt):
        _check_generation(m, sp, t)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_gloo_stop_worker, args=(r, 2, port, sps, q)) for r in range(2)]
    for p in ps:
        p.start()
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
    gens, samplings, where, g = res
    assert g[0][0] > 0 and g[1][1] > 0 and "gpu1" in where              # the other rank served and stopped some
    assert {where[i] for i in range(N_GW) if i % 4 != 2} >= {"gpu0", "gpu1"}
    for m, gen, sp in zip(local, gens, samplings):
        assert gen == m.metadata["generation"] and sp == m.metadata["sampling"]
