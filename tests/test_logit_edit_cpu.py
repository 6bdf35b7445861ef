"""``logit_bias``, ``allowed_token_ids`` and ``min_p`` without a GPU: the numpy
twin of ``csrc/kernels/logit_edit_kernels.h`` on hand-built rows, the ``min_p``
rule of the truncation twin, the parser, the HTTP route and the router's
lenient path, the dispatch descriptor and the K_HIST extension stream, the CPU
reference engine, and two ranks in threads."""
import threading

import numpy as np
import pytest

from llm_message_queue_amd.models.message import MessageStatus
from llm_message_queue_amd.ops import sampling as S

V = 16
NEG_INF = 0xFF80


def _row(vals):
    return S.bf16_bits(np.asarray(vals, dtype=np.float32))


def _edit(bits, vocab, allow=(), bias=(), vals=()):
    """One row under an allow list and bias entries (the lists laid out allow first)."""
    ids = list(allow) + list(bias)
    v = [0.0] * len(allow) + list(vals)
    return S.logit_edit_reference(np.asarray(bits).reshape(1, -1), vocab, np.asarray(ids, dtype=np.int32),
                                  np.asarray(v, dtype=np.float32), [[0, len(allow), len(allow), len(bias)]])[0]


# --------------------------------------------------------------------------- the edit's twin
def test_allow_list_masks_everything_else_and_leaves_allowed_bits_and_padding_alone():
    ld = 24
    bits = _row(np.random.default_rng(0).standard_normal(ld))
    out = _edit(bits, V, allow=[3, 9, 9, 0])
    assert np.array_equal(out[[0, 3, 9]], bits[[0, 3, 9]])
    others = np.setdiff1d(np.arange(V), [0, 3, 9])
    assert (out[others] == NEG_INF).all()
    assert np.array_equal(out[V:], bits[V:])                          # the padding keeps its bits
    assert (S.bf16_values(out[others]) == -np.inf).all()


def test_bias_is_rounded_once_to_fp32_then_to_bf16_by_nearest_even():
    # 1 + 2^-8 is the midpoint of the bf16 neighbours 1 and 1 + 2^-7; 2^-30 more lies above it.  The
    # float32 sum drops the 2^-30 and the tie goes to the even mantissa, 1; one rounding of the exact
    # sum would give 1 + 2^-7
    x = np.float32(1.0 + 2.0 ** -8)
    assert S.bf16_values(_row([x]))[0] != x                           # (not itself a bf16: start from 1 and add)
    b = np.float32(2.0 ** -8 + 2.0 ** -30)
    assert np.float64(1.0) + np.float64(b) > 1.0 + 2.0 ** -8          # the exact sum is above the midpoint
    bits = _row(np.ones(V))
    out = S.bf16_values(_edit(bits, V, bias=[5], vals=[b]))
    assert out[5] == 1.0 and (np.delete(out, 5) == 1.0).all()
    # ties in both directions
    assert S.bf16_values(_edit(bits, V, bias=[5], vals=[2.0 ** -8]))[5] == 1.0
    assert S.bf16_values(_edit(bits, V, bias=[5], vals=[3 * 2.0 ** -8]))[5] == 1.0 + 2.0 ** -6
    assert S.bf16_values(_edit(bits, V, bias=[5], vals=[100.0]))[5] == 101.0
    assert S.bf16_values(_edit(bits, V, bias=[5], vals=[-100.0]))[5] == -99.0


def test_duplicate_bias_id_uses_the_first_entry():
    out = S.bf16_values(_edit(_row(np.zeros(V)), V, bias=[4, 7, 4, 4], vals=[1.0, 2.0, 8.0, 16.0]))
    assert out[4] == 1.0 and out[7] == 2.0 and np.count_nonzero(out) == 2


def test_ids_outside_the_vocabulary_are_ignored():
    ld = 24
    bits = _row(np.arange(ld))
    assert np.array_equal(_edit(bits, V, bias=[-1, V, V + 3, 2 ** 31 - 1], vals=[1, 1, 1, 1]), bits)
    out = _edit(bits, V, allow=[-1, V, 2, ld - 1])
    assert out[2] == bits[2] and (np.delete(out[:V], 2) == NEG_INF).all() and np.array_equal(out[V:], bits[V:])
    # an allow list with no id inside the vocabulary leaves no candidate: token 0 downstream
    out = _edit(bits, V, allow=[V, -5])
    assert (out[:V] == NEG_INF).all() and np.array_equal(out[V:], bits[V:])
    assert S.penalised_pick_reference(out.reshape(1, -1), V).tolist() == [0]


def test_a_biased_column_that_is_not_allowed_stays_minus_infinity():
    out = _edit(_row(np.ones(V)), V, allow=[1, 2], bias=[2, 3], vals=[4.0, 100.0])
    assert S.bf16_values(out)[[1, 2]].tolist() == [1.0, 5.0]
    assert out[3] == NEG_INF and (out[[0] + list(range(3, V))] == NEG_INF).all()


def test_nan_and_infinities():
    vals = np.ones(V, dtype=np.float32)
    vals[[1, 2, 3]] = [np.nan, np.inf, -np.inf]
    bits = _row(vals)
    bits[1] = 0xFFC1                                                  # (a NaN with a payload and a sign)
    out = _edit(bits, V, bias=[1, 2, 3, 4], vals=[1.0, -5.0, 5.0, 3.0e38])
    assert out[1] == 0x7FC0 and out[2] == 0x7F80 and out[3] == NEG_INF
    big = _edit(_row(np.full(V, 3.0e38)), V, bias=[4], vals=[3.0e38])
    assert big[4] == 0x7F80                                           # an overflow becomes an infinity
    assert _edit(_row(vals), V, bias=[2], vals=[-np.inf])[2] == 0x7FC0    # inf - inf


def test_an_empty_row_is_a_no_op_and_spans_are_clamped():
    bits = np.stack([_row(np.arange(V) + r) for r in range(5)])
    ids = np.array([1, 2, 3, 4], dtype=np.int32)
    vals = np.array([0, 0, 8, 8], dtype=np.float32)
    spans = [[0, 0, 0, 0],            # empty
             [2, 99, 0, 0],           # the allow count is cut at the end of the lists: ids 3, 4
             [-7, 1, 4, 5],           # a negative offset is 0; a bias span at the end is empty
             [0, -3, 3, 70],          # a negative count is 0; bias (4, 8.0)
             [99, 5, 99, 5]]          # both offsets past the end
    out = S.logit_edit_reference(bits, V, ids, vals, spans)
    assert np.array_equal(out[0], bits[0]) and np.array_equal(out[4], bits[4])
    assert np.flatnonzero(out[1] != NEG_INF).tolist() == [3, 4]
    assert np.flatnonzero(out[2] != NEG_INF).tolist() == [1]
    assert np.flatnonzero(out[3] != bits[3]).tolist() == [4] and S.bf16_values(out[3])[4] == 4 + 3 + 8
    many = np.arange(100, dtype=np.int32) % V
    out = S.logit_edit_reference(bits[:1], V, np.arange(100, dtype=np.int32), np.zeros(100, dtype=np.float32),
                                 [[0, 100, 0, 0]])
    assert S.LE_MAX == 64 and (out[0] != NEG_INF).sum() == V and many.max() == V - 1   # (ids 0..63 cover the row)
    out = S.logit_edit_reference(bits[:1], V, np.arange(100, dtype=np.int32)[::-1].copy(),
                                 np.zeros(100, dtype=np.float32), [[0, 100, 0, 0]])
    assert (out[0] == NEG_INF).all()                                  # (ids 99..36: the cap keeps 0..15 out)


# --------------------------------------------------------------------------- min_p in the truncation twin
def _lg(vals):
    return S.bf16_values(_row(vals)).astype(np.float64)


def test_min_p_one_keeps_exactly_the_group_of_the_maximum():
    row = _lg([1.0, 3.5, -2.0, 3.5, np.nan, 3.484375, np.inf, 3.5])
    keep = S.truncation_keep(row, 0.7, 0, 1.0, min_p=1.0)
    assert np.flatnonzero(keep).tolist() == [1, 3, 7]
    assert S.min_p_log(1.0) == 0.0 and S.min_p_log(0.0) == -np.inf and S.min_p_log(0.0004) == -np.inf
    assert S.min_p_log(0.001) == np.float32(np.log(0.001))


def test_min_p_off_reproduces_the_kept_sets_of_today():
    rng = np.random.default_rng(3)
    for i in range(40):
        row = _lg(rng.standard_normal(300) * 3)
        it, tk, tp = np.float32(rng.uniform(0.5, 2)), int(rng.integers(0, 50)) * (i % 2), (0.9 if i % 3 else 1.0)
        base = S.truncation_keep(row, it, tk, tp)
        assert np.array_equal(base, S.truncation_keep(row, it, tk, tp, min_p=None))
        assert np.array_equal(base, S.truncation_keep(row, it, tk, tp, min_p=0.0))
        assert np.array_equal(base, S.truncation_keep(row, it, tk, tp, log_min_p=np.float32(-np.inf)))
    keys = S.row_keys(5, np.arange(6))
    lg = _lg(rng.standard_normal((6, 300)) * 3)
    assert np.array_equal(S.sample_truncated_reference(lg, 1.0, keys, 7, 0.8),
                          S.sample_truncated_reference(lg, 1.0, keys, 7, 0.8, log_min_p=-np.inf))


def test_min_p_threshold_exactly_on_a_value_keeps_it():
    # (v - max) * inv_temp for v = 2, max = 4, inv_temp = 0.5 is exactly -1
    row = _lg([4.0, 2.0, 1.9921875, 2.0, 0.0])
    keep = S.truncation_keep(row, 0.5, 0, 1.0, log_min_p=np.float32(-1.0))
    assert np.flatnonzero(keep).tolist() == [0, 1, 3]
    below = np.nextafter(np.float32(-1.0), np.float32(0.0))           # the next threshold up excludes it
    assert np.flatnonzero(S.truncation_keep(row, 0.5, 0, 1.0, log_min_p=below)).tolist() == [0]
    # the rule is evaluated in float32, each operation rounded once
    it = np.float32(1.0 / 0.7)
    d = np.float32(np.float32(-3.0) * it)
    row = _lg([5.0, 2.0, 1.0])
    assert np.flatnonzero(S.truncation_keep(row, it, 0, 1.0, log_min_p=d)).tolist() == [0, 1]
    assert np.flatnonzero(S.truncation_keep(row, it, 0, 1.0, log_min_p=np.nextafter(d, np.float32(0)))).tolist() == [0]


def test_min_p_intersects_with_top_k_and_top_p():
    row = _lg([0.0, -1.0, -2.0, -3.0, -4.0, -5.0])
    lm = np.float32(-3.5)                                             # min_p keeps 0 .. -3
    assert np.flatnonzero(S.truncation_keep(row, 1.0, 0, 1.0, log_min_p=lm)).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(S.truncation_keep(row, 1.0, 2, 1.0, log_min_p=lm)).tolist() == [0, 1]
    assert np.flatnonzero(S.truncation_keep(row, 1.0, 5, 1.0, log_min_p=lm)).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(S.truncation_keep(row, 1.0, 0, 0.7, log_min_p=lm)).tolist() == [0, 1]
    assert np.flatnonzero(S.truncation_keep(row, 1.0, 0, 0.7, log_min_p=np.float32(-0.5))).tolist() == [0]
    # the draw stays among the kept columns
    keys = S.row_keys(11, np.arange(50))
    picks = S.sample_truncated_reference(np.tile(row, (50, 1)), 1.0, keys, 0, 1.0, log_min_p=np.float32(-1.5))
    assert set(picks.tolist()) == {0, 1}


# --------------------------------------------------------------------------- parser
def test_parser_accepted_forms():
    from llm_message_queue_amd.models.message import (allowed_from_metadata as al, eligibility_from_metadata,
                                                      logit_bias_from_metadata as lb, min_p_from_metadata as mp)
    for md in (None, {}, {"sampling": {}}, {"sampling": {"temperature": 0.7}}):
        assert mp(md) == 0.0 and len(al(md)) == 0 and len(lb(md)[0]) == 0 and len(lb(md)[1]) == 0
    assert [mp({"sampling": {"min_p": v}}) for v in (0, 0.0, 1, 1.0, 0.05, 0.0504, 0.0004, 0.0005001)] \
        == [0.0, 0.0, 1.0, 1.0, 0.05, 0.05, 0.0, 0.001]
    ids, vals = lb({"sampling": {"logit_bias": {"17": 5, "0": -100, "2147483647": 100.0, "3": 0, "9": 0.25}}})
    assert ids.dtype == np.int32 and vals.dtype == np.float32
    assert ids.tolist() == [17, 0, 2147483647, 9] and vals.tolist() == [5.0, -100.0, 100.0, 0.25]   # the 0 is dropped
    assert lb({"sampling": {"logit_bias": {}}})[0].tolist() == []
    assert lb({"sampling": {"logit_bias": {"5": 0.1}}})[1][0] == np.float32(0.1)
    a = al({"sampling": {"allowed_token_ids": [5, 0, 2147483647]}})
    assert a.dtype == np.int32 and a.tolist() == [5, 0, 2147483647]
    full = {str(i): 1 for i in range(64)}
    assert len(lb({"sampling": {"logit_bias": full}})[0]) == 64
    assert len(al({"sampling": {"allowed_token_ids": list(range(64))}})) == 64
    mpv, (bi, bv), aa = eligibility_from_metadata({"sampling": {"min_p": 0.1, "logit_bias": {"1": 2},
                                                                "allowed_token_ids": [1]}})
    assert (mpv, bi.tolist(), bv.tolist(), aa.tolist()) == (0.1, [1], [2.0], [1])


BAD = [{"min_p": -0.01}, {"min_p": 1.001}, {"min_p": "0.5"}, {"min_p": True}, {"min_p": None}, {"min_p": float("nan")},
       {"logit_bias": {"018": 1}}, {"logit_bias": {"+7": 1}}, {"logit_bias": {"-1": 1}}, {"logit_bias": {"1.5": 1}},
       {"logit_bias": {"": 1}}, {"logit_bias": {" 7": 1}}, {"logit_bias": {"x": 1}}, {"logit_bias": {"2147483648": 1}},
       {"logit_bias": {"00": 1}}, {"logit_bias": {"1" * 5000: 1}}, {"logit_bias": {"12345678901": 1}}, {"logit_bias": {"7": 100.5}}, {"logit_bias": {"7": -101}}, {"logit_bias": {"7": "1"}},
       {"logit_bias": {"7": True}}, {"logit_bias": {"7": None}}, {"logit_bias": {"7": float("inf")}},
       {"logit_bias": [[7, 1]]}, {"logit_bias": 3}, {"logit_bias": {str(i): 1 for i in range(65)}},
       {"allowed_token_ids": []}, {"allowed_token_ids": list(range(65))}, {"allowed_token_ids": [1, 1]},
       {"allowed_token_ids": [-1]}, {"allowed_token_ids": [2147483648]}, {"allowed_token_ids": [1.0]},
       {"allowed_token_ids": ["1"]}, {"allowed_token_ids": [True]}, {"allowed_token_ids": 5},
       {"allowed_token_ids": {"1": 1}}]


def test_parser_rejections():
    from llm_message_queue_amd.models.message import SamplingParseError, eligibility_from_metadata
    for bad in BAD:
        with pytest.raises(SamplingParseError):
            eligibility_from_metadata({"sampling": bad})
    with pytest.raises(SamplingParseError):
        eligibility_from_metadata({"sampling": "x"})


def test_post_message_rejects_every_bad_value_with_a_400():
    import json
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
                body = json.dumps({"content": "hi", "metadata": {"sampling": sp}})       # (NaN / Infinity as Python writes them)
                return c.post("/api/v1/messages", content=body, headers={"content-type": "application/json"})
            for bad in BAD:
                r = post(bad)
                assert r.status_code == 400 and next(iter(bad)) in r.text, bad
            assert post({"logit_bias": {"17": 5}}).status_code == 202
            assert post({"allowed_token_ids": [1, 2, 3], "logit_bias": {"2": -3.5}}).status_code == 202
            assert post({"temperature": 0.9, "seed": 11, "min_p": 0.05, "top_k": 40}).status_code == 202
            assert post({"min_p": 0.5}).status_code == 202                               # greedy: accepted, no effect
    finally:
        app.stop()


def _sp_msgs():
    from llm_message_queue_amd.models.message import Message
    sp = [{"logit_bias": {"17": 5, "3": 0}},                                              # greedy, one entry in effect
          {"allowed_token_ids": [4, 2], "temperature": 0.8, "seed": 7, "min_p": 0.0504},
          {"min_p": 0.5},                                                                 # greedy: min_p has no effect
          {"temperature": 0.8, "seed": 7, "min_p": 0.0004, "logit_bias": {"3": 0}},       # both round to off
          {"temperature": 0.8, "seed": 7},
          None,
          {"logit_bias": {"018": 1}, "allowed_token_ids": [9], "repetition_penalty": 1.2},     # one bad key
          {"allowed_token_ids": [], "min_p": 7, "logit_bias": {"5": -2.5}, "temperature": 0.8, "seed": 1},
          {"logit_bias": {"1" * 5000: 1}, "allowed_token_ids": [9]}]      # a key longer than int() converts
    msgs = [Message(id=f"e{i}", content="x", metadata={"sampling": s} if s is not None else {})
            for i, s in enumerate(sp)]
    for i, m in enumerate(msgs):
        m.tier = i % 4
        m.prompt_ids = np.arange(4, dtype=np.uint32) + i
    return msgs


def test_lenient_path_and_write_back_only_where_in_effect():
    from llm_message_queue_amd.models.message import default_seed
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = _sp_msgs()
    reqs = [gw._make_request(m, 2) for m in msgs]
    md = [m.metadata for m in msgs]
    assert md[0]["sampling"] == {"temperature": 0.0, "seed": default_seed("e0"), "logit_bias": {"17": 5.0}}
    assert md[1]["sampling"] == {"temperature": 0.8, "seed": 7, "min_p": 0.05, "allowed_token_ids": [4, 2]}
    assert set(md[2]["sampling"]) == {"temperature", "seed"} and reqs[2].min_p == 0.0
    assert md[3]["sampling"] == {"temperature": 0.8, "seed": 7}
    assert md[4]["sampling"] == {"temperature": 0.8, "seed": 7}
    assert "sampling" not in md[5] and "sampling_error" not in md[5]
    assert all("sampling_error" not in md[i] for i in range(6))
    # a bad key is off and reported, the other keys stay in effect
    assert "logit_bias" in md[6]["sampling_error"] and "allowed" not in md[6]["sampling_error"]
    assert set(md[6]["sampling"]) == {"temperature", "seed", "allowed_token_ids", "repetition_penalty"}
    assert reqs[6].logit_bias is None and reqs[6].allowed.tolist() == [9] and reqs[6].repetition_penalty == 1.2
    assert "allowed_token_ids" in md[7]["sampling_error"] and "min_p" in md[7]["sampling_error"]
    assert md[7]["sampling"] == {"temperature": 0.8, "seed": 1, "logit_bias": {"5": -2.5}}
    assert reqs[7].allowed is None and reqs[7].min_p == 0.0 and reqs[7].logit_bias[1].tolist() == [-2.5]
    # a key too long for int(): a parse error like any other, through the local and the remote path
    assert "logit_bias" in md[8]["sampling_error"] and reqs[8].logit_bias is None and reqs[8].allowed.tolist() == [9]
    assert set(md[8]["sampling"]) == {"temperature", "seed", "allowed_token_ids"}
    # the request carries what the metadata says
    assert reqs[0].logit_bias[0].tolist() == [17] and reqs[0].allowed is None and reqs[0].min_p == 0.0
    assert reqs[1].allowed.tolist() == [4, 2] and reqs[1].min_p == 0.05 and reqs[1].logit_bias is None
    assert reqs[4].allowed is None and reqs[4].logit_bias is None and reqs[4].min_p == 0.0
    # a replay of the written-back values parses to the same
    again = gw._make_request(msgs[0], 2)
    assert again.logit_bias[0].tolist() == [17] and again.logit_bias[1].tolist() == [5.0]
    assert "sampling_error" not in md[0]


# --------------------------------------------------------------------------- descriptors
def test_min_p_rides_in_the_gen_column_with_gen_intact():
    from llm_message_queue_amd.gateway.descriptors import pack_gen, unpack_gen
    for gen in (1, 4, 4096):
        assert pack_gen(gen) == gen and unpack_gen(gen) == (gen, 0.0)
        for pm in (1, 50, 500, 1000):
            col = pack_gen(gen, pm / 1000.0)
            assert 0 < col < 1 << 31 and unpack_gen(col) == (gen, pm / 1000.0)
        for off in (0.0, 0.0004, -1.0, 1.5, float("nan")):
            assert pack_gen(gen, off) == gen


def test_gateway_refuses_a_gen_tokens_the_dispatch_row_cannot_carry():
    from llm_message_queue_amd.gateway.descriptors import GEN_MASK
    from llm_message_queue_amd.gateway.router import Gateway
    from llm_message_queue_amd.utils.config import default_config
    cfg = default_config()
    cfg.queue.enable_metrics = False
    assert GEN_MASK == 0xFFFF
    with pytest.raises(ValueError):
        Gateway(cfg, engine=None, use_gpu_preprocess=False, prompt_cap=8, gen_tokens=GEN_MASK + 1)


def test_tier_bit_30_leaves_unpack_penalties_unchanged():
    from llm_message_queue_amd.gateway.descriptors import EXTENSION, pack_penalties, unpack_penalties
    assert EXTENSION == 1 << 30
    for tier in (0, 1, 3, 4):
        for v in ((2.0, -2.0, 0.5), (-2.0, 2.0, 2.0), (0.0, 0.0, 1.0), (1.37, -0.01, 1.01)):
            col = tier | pack_penalties(*v)
            assert not col & EXTENSION
            assert unpack_penalties(col | EXTENSION) == unpack_penalties(col) == (tier,) + v


def test_extension_stream_packs_and_unpacks():
    from llm_message_queue_amd.gateway.descriptors import pack_extension, unpack_extension
    assert len(pack_extension(None, None, None)) == 0 and len(pack_extension([], [], [])) == 0
    a, bi, bv = unpack_extension(np.zeros(0, dtype=np.int32))
    assert len(a) == len(bi) == len(bv) == 0
    for allow, ids, vals in (([5, 6], [1, 2, 3], [0.5, -1.0, 100.0]), ([], [7], [1.5]), ([2147483647, 0], [], []),
                             (list(range(64)), list(range(64, 128)), list(np.linspace(-100, 100, 64)))):
        w = pack_extension(allow, ids, vals)
        assert w.dtype == np.int32 and len(w) == 2 + len(allow) + 2 * len(ids)
        a, bi, bv = unpack_extension(w)
        assert a.tolist() == allow and bi.tolist() == ids
        assert np.array_equal(bv, np.asarray(vals, dtype=np.float32)) and bv.dtype == np.float32
    # counts that leave the stream are clamped to it
    a, bi, bv = unpack_extension(np.array([9, 1, 2], dtype=np.int32))
    assert a.tolist() == [1, 2] and len(bi) == 0
    a, bi, bv = unpack_extension(np.array([1, 5, 40, 3, 4], dtype=np.int32))
    assert a.tolist() == [5] and bi.tolist() == [3] and bv.view(np.int32).tolist() == [4]


def _hist_gateway():
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    gw._hist_wait, gw._await_hist, gw._hist_len = {}, {}, {}
    return gw


def test_hist_block_with_prefix_history_and_extension_reassembles_over_several_rows():
    from llm_message_queue_amd.backend.engine import Request
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, K_HIST, pack_extension
    gw = _hist_gateway()
    cap, width = 8, DESC_HDR + 8
    pre, hist = np.arange(100, 103, dtype=np.int32), np.arange(200, 211, dtype=np.int32)
    ext = pack_extension([5, 6, 7], [1, 2], [0.5, -3.0])
    only = pack_extension([9], None, None)
    gw._hist_pub = {1: [(77, pre, hist, ext), (78, None, None, only), (79, None, hist, np.zeros(0, np.int32))]}
    assert gw._hist_rows(1) == 3 + 1 + 2                               # 3 + 11 + 9 = 23 words; 3; 11
    block = gw._hist_block(1, 0, cap, width)
    assert block.shape == (6, width) and (block[:, 0] == K_HIST).all()
    assert block[:, 16].tolist() == [9, 9, 9, 3, 0, 0] and block[:, 10].tolist() == [8, 8, 7, 3, 8, 3]
    held = {h: Request(req_id=h, prompt=np.zeros(1, np.int32), gen_tokens=1, meta=(0, h, 2, 0, 0, 0))
            for h in (77, 78, 79)}
    for h, r in held.items():
        gw._hist_wait[(0, h)] = r
        gw._await_hist[(0, h)] = r
    ready = gw._take_histories(0, block[::-1])                         # (row order does not matter)
    assert sorted(r.req_id for r in ready) == [77, 78, 79] and not gw._hist_wait and not gw._await_hist
    r = held[77]
    assert r.prefix.tolist() == pre.tolist() and r.history.tolist() == hist.tolist()
    assert r.allowed.tolist() == [5, 6, 7] and r.logit_bias[0].tolist() == [1, 2]
    assert r.logit_bias[1].tolist() == [0.5, -3.0]
    r = held[78]
    assert r.prefix is None and r.history is None and r.allowed.tolist() == [9] and r.logit_bias is None
    r = held[79]
    assert r.history.tolist() == hist.tolist() and r.allowed is None and r.logit_bias is None


def test_hist_block_without_an_extension_is_what_it_was():
    """Rebuilt by hand from the layout the rows had before the extension
    existed: kind, handle, origin, offset, count, history and prefix lengths,
    the tokens, zero everywhere else."""
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, K_HIST, _put64
    gw = _hist_gateway()
    cap, width = 8, DESC_HDR + 8
    pre, hist = np.arange(100, 103, dtype=np.int32), np.arange(200, 211, dtype=np.int32)
    none = np.zeros(0, dtype=np.int32)
    gw._hist_pub = {1: [(77, pre, hist, none), (79, None, hist, none)]}
    block = gw._hist_block(1, 3, cap, width)
    want = np.zeros((4, width), dtype=np.int32)
    k = 0
    for h, p, hh in ((77, pre, hist), (79, none, hist)):
        allt = np.concatenate([p, hh])
        for off in range(0, len(allt), cap):
            n = min(cap, len(allt) - off)
            want[k, 0], want[k, 3], want[k, 4], want[k, 10], want[k, 14], want[k, 15] = K_HIST, 3, off, n, len(hh), len(p)
            want[k, DESC_HDR:DESC_HDR + n] = allt[off:off + n]
            _put64(want[k:k + 1], 1, [h])
            k += 1
    assert block.tobytes() == want.tobytes()


def test_dispatch_row_carries_min_p_and_the_extension_flag_and_nothing_else_changes():
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR, EXTENSION, unpack_extension
    gw = _hist_gateway()
    msgs = _sp_msgs()
    buf = np.zeros((len(msgs), DESC_HDR + 8), dtype=np.int32)
    ctx = gw._fill_descs(buf, msgs, 1, 8, {})
    reqs = gw._foreign_requests(buf, 8)
    assert [r.gen_tokens for r in reqs] == [2] * 9                     # gen is intact
    assert [r.min_p for r in reqs] == [0.0, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert [bool(c & EXTENSION) for c in buf[:, 4].tolist()] \
        == [True, True, False, False, False, False, True, True, True]
    assert [r.tier for r in reqs] == [0, 1, 2, 3, 0, 1, 2, 3, 0] and reqs[6].repetition_penalty == 1.2
    assert "logit_bias" in msgs[8].metadata["sampling_error"] and unpack_extension(ctx[8][2])[0].tolist() == [9]
    assert all(r.allowed is None and r.logit_bias is None for r in reqs)    # the lists follow one tick later
    exts = [unpack_extension(e) for _h, _p, e in ctx]
    assert exts[0][1].tolist() == [17] and exts[0][2].tolist() == [5.0] and exts[1][0].tolist() == [4, 2]
    assert exts[6][0].tolist() == [9] and exts[7][1].tolist() == [5] and all(len(ctx[i][2]) == 0 for i in (2, 3, 4, 5))
    # rows that name none of the three keys in effect are what they are without the feature
    stripped = _sp_msgs()
    for m, o in zip(stripped, msgs):
        m.handle, m.arrival_ns, m.enqueued_at = o.handle, o.arrival_ns, o.enqueued_at
        sp = m.metadata.get("sampling")
        for k in ("min_p", "logit_bias", "allowed_token_ids"):
            if sp:
                sp.pop(k, None)
    ref = np.zeros_like(buf)
    gw._fill_descs(ref, stripped, 1, 8, {})
    assert np.array_equal(buf[[2, 3, 4, 5]], ref[[2, 3, 4, 5]])
    others = np.delete(np.arange(buf.shape[1]), [4, 9])
    assert np.array_equal(buf[:, others], ref[:, others])


# --------------------------------------------------------------------------- engine on the CPU
def _engine(slots=32, **kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=slots, max_ctx=64, token_budget=256, device="cpu", impl="ref", **kw)


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=5, **kw)


def _run(reqs, slots=32, eng=None):
    eng = eng or _engine(slots)
    assert len(eng.admit(reqs)) == len(reqs)
    done = eng.drain()
    assert len(done) == len(reqs)
    return {r.req_id: r for r in done}, eng


ALLOW = np.array([900, 7, 313, 5000, 64], dtype=np.int32)              # (5000 is outside the vocabulary of 1,024)
I32, F32 = (lambda v: np.asarray(v, dtype=np.int32)), (lambda v: np.asarray(v, dtype=np.float32))


def _others():
    return [_req(i) for i in range(12)] + [_req(12 + i, temperature=0.9, seed=i, top_k=(5 if i % 2 else 0))
                                           for i in range(4)]


def _edited():
    return [_req(100, allowed=ALLOW.copy()),
            _req(101, allowed=ALLOW.copy(), temperature=0.9, seed=3),
            _req(102, logit_bias=(I32([17, 5000]), F32([100.0, 100.0]))),
            _req(103, logit_bias=(I32([17, 40]), F32([2.5, -1.0])), temperature=0.9, seed=4, top_k=8, min_p=0.05,
                 logprobs=3),
            _req(104, temperature=0.9, seed=5, min_p=0.3),
            _req(105, allowed=ALLOW.copy(), logit_bias=(I32([7, 8]), F32([3.0, 100.0])), presence_penalty=1.0,
                 repetition_penalty=1.3, temperature=1.1, seed=6, min_p=0.01)]


@pytest.fixture(scope="module")
def engine_runs():
    plain, e_plain = _run(_others())
    alone = {}
    for r in _edited():
        alone.update(_run([r])[0])
    crowd, e_crowd = _run(_others() + _edited())
    moved, _ = _run([_req(i) for i in range(3)] + _edited()[::-1])
    return dict(plain=plain, alone=alone, crowd=crowd, moved=moved, e_plain=e_plain, e_crowd=e_crowd)


def test_engine_allow_list_bounds_every_generated_token(engine_runs):
    inside = set(ALLOW[ALLOW < 1024].tolist())
    for rid in (100, 101, 105):
        for run in ("alone", "crowd", "moved"):
            toks = engine_runs[run][rid].out_tokens
            assert len(toks) == 5 and set(toks.tolist()) <= inside, (rid, run, toks)
    assert 8 not in engine_runs["alone"][105].out_tokens              # a +100 bias on a token that is not allowed


def test_engine_a_plus_100_bias_forces_its_token_when_greedy(engine_runs):
    assert engine_runs["alone"][102].out_tokens.tolist() == [17] * 5


def test_engine_a_minus_100_bias_on_the_greedy_token_changes_the_pick():
    base = _run([_req(7)])[0][7].out_tokens
    got = _run([_req(7, logit_bias=(I32([base[0]]), F32([-100.0])))])[0][7].out_tokens
    assert got[0] != base[0] and base[0] not in got.tolist()


def test_engine_tokens_do_not_depend_on_batch_or_slot(engine_runs):
    for rid in range(100, 106):
        a, b, c = (engine_runs[k][rid] for k in ("alone", "crowd", "moved"))
        assert len({a.slot, b.slot, c.slot}) >= 2
        assert np.array_equal(a.out_tokens, b.out_tokens) and np.array_equal(a.out_tokens, c.out_tokens), rid
    for i in range(16):                                               # the neighbours draw what they draw without them
        assert np.array_equal(engine_runs["crowd"][i].out_tokens, engine_runs["plain"][i].out_tokens), i


def test_engine_min_p_alone_takes_the_truncated_path_and_changes_the_draw_only_by_the_rule(engine_runs):
    eng = _engine()
    calls = []
    inner = eng.model.ops.truncated_head

    def spy(*a, **kw):
        calls.append((a[0].shape[0], None if kw.get("log_min_p") is None else kw["log_min_p"].tolist()))
        return inner(*a, **kw)
    eng.model.ops.truncated_head = spy
    got = _run([_req(104, temperature=0.9, seed=5, min_p=0.3), _req(1)], eng=eng)[0][104]
    assert np.array_equal(got.out_tokens, engine_runs["alone"][104].out_tokens)
    assert len(calls) == 5 and all(c == (1, [float(np.float32(np.log(0.3)))]) for c in calls)
    assert eng.truncated_steps == 5 and eng.edited_steps == 0 and eng.penalised_steps == 0
    # min_p = 1.0 keeps the maximum only: the greedy tokens
    greedy = _run([_req(104)])[0][104].out_tokens
    one = _run([_req(104, temperature=0.9, seed=5, min_p=1.0)])[0][104].out_tokens
    assert np.array_equal(one, greedy)
    # a greedy request ignores it
    eng = _engine()
    assert np.array_equal(_run([_req(104, min_p=0.3)], eng=eng)[0][104].out_tokens, greedy)
    assert eng.truncated_steps == 0 and eng.sampled_steps == 0


def test_engine_a_step_without_such_a_request_stages_the_same_bytes_and_launches_nothing_new(engine_runs):
    e = engine_runs["e_plain"]
    assert e.edited_steps == 0 and e.penalised_steps == 0 and e.h_eids is None and e.d_hist is None
    assert engine_runs["e_crowd"].edited_steps > 0
    # the staged bytes: an engine that has served an edited request stages, for plain traffic, what a fresh one does
    def staged(eng):
        seen = []
        inner = eng.model.forward

        def fwd(tok, pos, slot, samp, **kw):
            seen.append((tok.numel() + pos.numel() + slot.numel() + samp.numel(), sorted(kw)))
            return inner(tok, pos, slot, samp, **kw)
        eng.model.forward = fwd
        got = _run(_others(), eng=eng)[0]
        return seen, got, eng._pins[0].numpy().copy()
    fresh = staged(_engine())
    used_eng = _engine()
    _run(_edited(), eng=used_eng)
    steps = used_eng.edited_steps
    used = staged(used_eng)
    assert fresh[0] == used[0] and used_eng.edited_steps == steps
    assert all("pen" not in kw for _n, kw in used[0])
    for i in range(16):
        assert np.array_equal(fresh[1][i].out_tokens, used[1][i].out_tokens)


def test_engine_logprobs_are_unchanged_by_a_bias(engine_runs):
    # the same tokens forced with and without the bias: an allow-list of one token, then a +100 bias on top
    a = _run([_req(9, allowed=I32([17]), logprobs=5)])[0][9]
    b = _run([_req(9, allowed=I32([17]), logit_bias=(I32([17, 40]), F32([100.0, -100.0])), logprobs=5)])[0][9]
    assert a.out_tokens.tolist() == b.out_tokens.tolist() == [17] * 5
    assert np.array_equal(a.out_logprobs, b.out_logprobs) and np.array_equal(a.out_top_ids, b.out_top_ids)
    assert np.array_equal(a.out_top_logprobs, b.out_top_logprobs)
    assert (a.out_logprobs < 0).all()                                 # the model's own distribution, not the masked one
    r = engine_runs["alone"][103]
    assert r.out_logprobs is not None and len(r.out_logprobs) == 5


def test_engine_an_edited_row_without_a_penalty_reads_no_history():
    eng = _engine()
    seen = []
    inner = eng.model.ops.penalised_head

    def spy(x, w, it, kk, tk, tp, hist, spans, params, **kw):
        seen.append((hist, spans[:, 0].tolist(), kw["edit"][2].tolist()))
        return inner(x, w, it, kk, tk, tp, hist, spans, params, **kw)
    eng.model.ops.penalised_head = spy
    _run([_req(100, allowed=ALLOW.copy()), _req(1)], eng=eng)
    assert len(seen) == 5 and all(h is None and s == [-1] and e == [[0, 5, 5, 0]] for h, s, e in seen)
    assert eng.d_hist is None
    # next to a penalised request: a history exists, the edited row still names no slot of it
    seen.clear()
    got = _run([_req(100, allowed=ALLOW.copy()), _req(2, repetition_penalty=1.5)], eng=eng)[0]
    assert eng.d_hist is not None and all(sorted(s)[0] == -1 and len(s) == 2 for _h, s, _e in seen)
    assert np.array_equal(got[100].out_tokens, _run([_req(100, allowed=ALLOW.copy())])[0][100].out_tokens)


def test_micro_pool_serves_an_edited_request_with_the_same_tokens():
    from tests.test_realtime_micro import _engine as micro_engine, _serve
    from llm_message_queue_amd.backend.engine import Request

    def reqs():
        rng = np.random.default_rng(9)
        kw = {0: dict(allowed=I32([5, 6, 7])), 1: dict(logit_bias=(I32([3]), F32([100.0])))}
        return [Request(req_id=i, prompt=rng.integers(0, 1000, size=5 + i).astype(np.int32), gen_tokens=4, tier=i % 3,
                        **kw.get(i, {})) for i in range(6)]
    a = _serve(micro_engine("off"), reqs())
    eng = micro_engine("micro")
    b = _serve(eng, reqs())
    assert b[0][1] and not b[1][1]                                    # request 0 (tier 0) ran on the micro pool
    assert {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}
    assert set(a[0][0]) <= {5, 6, 7} and list(a[1][0]) == [3] * 4
    assert eng.edited_steps > 0 and eng.micro_steps > 0


def test_sim_and_null_engines_accept_and_ignore_the_new_fields():
    import torch
    from llm_message_queue_amd.backend.sim_engine import SimEngine
    out = SimEngine._forward(None, None, None, torch.zeros(3), pen=(None,) * 10, trunc=(None,) * 4)
    assert out.shape == (3,)
    eng = SimEngine(slots=4, max_ctx=32, token_budget=64)
    r = _req(1, allowed=I32([1]), logit_bias=(I32([2]), F32([1.0])), min_p=0.5, temperature=0.9)
    assert eng.admit([r]) == [r] and not eng.s_edit.any() and eng.h_eids is None
    from llm_message_queue_amd.backend.engine import Request
    import dataclasses
    names = {f.name for f in dataclasses.fields(Request)}
    assert {"min_p", "logit_bias", "allowed"} <= names


# --------------------------------------------------------------------------- two ranks in threads
def _wire_cfg():
    from llm_message_queue_amd.utils.config import default_config
    c = default_config()
    c.queue.enable_metrics = False
    return c


def _wire_engine(slots=4):
    from tests.test_gateway_distributed import engine
    return engine(slots=slots, seed=0)                                 # (the same model on every rank)


def _wire_msgs(n):
    """Content-derived prompts; two in three carry a list, a bias or a min_p,
    and all of them ask for their tokens back (``logprobs`` 0)."""
    from llm_message_queue_amd.gateway.workload import Workload
    msgs = Workload(seed=11).make(n)
    kinds = [{"allowed_token_ids": [5, 77, 300, 9999]},
             {"logit_bias": {"41": 100}},
             {},
             {"allowed_token_ids": [8, 9, 10, 11], "logit_bias": {"9": 1.5, "200": 100}, "temperature": 0.9, "seed": 3,
              "min_p": 0.02},
             {"temperature": 0.9, "seed": 4, "min_p": 0.25},
             {"temperature": 0.9, "seed": 5}]
    for i, m in enumerate(msgs):
        m.id = f"w{i}"
        m.priority = 3
        m.metadata = {"sampling": dict(kinds[i % 6], logprobs=0)}
    return msgs


def _tick_all(gws):
    errs = []

    def run(g):
        try:
            g.tick()
        except BaseException as e:                                    # noqa: BLE001 -- re-raised on the test thread
            errs.append(e)
    ths = [threading.Thread(target=run, args=(g,)) for g in gws]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errs:
        raise errs[0]


def _two_ranks(slots=4):
    from llm_message_queue_amd.gateway.router import Gateway
    from llm_message_queue_amd.parallel.comm import FakeComm
    comms = FakeComm.make(2, timeout_s=20)
    return [Gateway(_wire_cfg(), engine=_wire_engine(slots), comm=comms[r], use_gpu_preprocess=False, prompt_cap=8,
                    gen_tokens=3) for r in range(2)]


def test_the_same_message_generates_the_same_tokens_locally_and_on_the_foreign_rank():
    from llm_message_queue_amd.gateway.router import Gateway
    from tests.test_gateway_distributed import run_until_done
    n = 12
    gw = Gateway(_wire_cfg(), engine=_wire_engine(), use_gpu_preprocess=False, prompt_cap=8, gen_tokens=3)
    local = _wire_msgs(n)
    gw.submit(local)
    assert run_until_done([gw], n)
    want = {m.id: m.metadata["generation"]["tokens"] for m in local}
    assert set(want["w0"]) <= {5, 77, 300} and want["w1"] == [41, 41, 41] and set(want["w3"]) <= {8, 9, 10, 11}
    gws = _two_ranks()
    msgs = _wire_msgs(n)
    gws[0].submit(msgs)
    assert run_until_done(gws, n)
    remote = [m for m in msgs if m.endpoint_id == "gpu1"]
    assert {int(m.id[1:]) % 6 for m in remote} >= {0, 1, 3}, [m.id for m in remote]   # edited requests went abroad
    for m in msgs:
        assert m.metadata["generation"]["tokens"] == want[m.id], (m.id, m.endpoint_id)
    assert gws[1].engine.edited_steps > 0
    for g in gws:
        assert not g._hist_wait and not g._await_hist and not g._hist_out


def test_a_foreign_request_with_an_extension_is_admitted_exactly_one_tick_after_its_dispatch_row():
    from llm_message_queue_amd.gateway.descriptors import EXTENSION, K_DISPATCH, K_HIST, _get64, pack_extension
    gws = _two_ranks()
    tick = [0]
    seen_disp, seen_hist, adm = {}, {}, {}
    inner = gws[0].comm.all_to_all_rows_async

    def spy(send, recv_counts, width):
        for r in send[1]:
            h = int(_get64(np.asarray(r).reshape(1, -1), 1)[0])
            if r[0] == K_DISPATCH:
                seen_disp[h] = (tick[0], bool(r[4] & EXTENSION))
            elif r[0] == K_HIST:
                seen_hist[h] = (tick[0], int(r[16]), int(r[14]), int(r[15]))
        return inner(send, recv_counts, width)
    gws[0].comm.all_to_all_rows_async = spy
    inner_admit = gws[1].engine.admit

    def admit(reqs):
        got = inner_admit(reqs)
        for r in got:
            adm[r.meta[1]] = (tick[0], r)                              # (rank 1 serves foreign requests only)
        return got
    gws[1].engine.admit = admit
    msgs = _wire_msgs(12)
    gws[0].submit(msgs)
    for _ in range(100):
        tick[0] += 1
        _tick_all(gws)
        if all(m.status == MessageStatus.COMPLETED for m in msgs):
            break
    assert all(m.status == MessageStatus.COMPLETED and not m.conversation_id for m in msgs)
    flagged = [h for h, (_t, fl) in seen_disp.items() if fl]
    plain = [h for h, (_t, fl) in seen_disp.items() if not fl]
    assert flagged and plain and sorted(seen_hist) == sorted(flagged)
    by_handle = {m.handle: m for m in msgs}
    for h in flagged:
        t_disp = seen_disp[h][0]
        r = adm[h][1]
        al = r.allowed if r.allowed is not None else ()
        bias = r.logit_bias if r.logit_bias is not None else ((), ())
        assert seen_hist[h] == (t_disp + 1, len(pack_extension(al, *bias)), 0, 0)    # no dialog: the extension alone
        assert adm[h][0] == t_disp + 1, by_handle[h].id                # exactly one tick later
        sp = by_handle[h].metadata["sampling"]
        assert list(al) == [int(t) for t in sp.get("allowed_token_ids", [])]
        assert {str(int(t)): float(v) for t, v in zip(*bias)} == sp.get("logit_bias", {})
    for h in plain:                                                    # a request with only min_p does not wait
        assert adm[h][0] == seen_disp[h][0], by_handle[h].id
    assert any(by_handle[h].metadata["sampling"].get("min_p") for h in plain)
    for g in gws:
        assert not g._hist_wait and not g._await_hist


def _hold_one_waiting():
    """Two ranks, rank 0's messages submitted; stops at the tick in which
    rank 1 has the dispatch row of a request with an extension but not yet
    its lists.  Returns the gateways, that message and the others."""
    gws = _two_ranks()
    msgs = _wire_msgs(12)
    gws[0].submit(msgs)
    for _ in range(60):
        _tick_all(gws)
        if gws[1]._await_hist:
            break
    else:
        raise AssertionError("no request ever waited on rank 1")
    (_o, h), r = next(iter(gws[1]._await_hist.items()))
    m = next(x for x in msgs if x.handle == h)
    assert m.endpoint_id == "gpu1" and not m.conversation_id and r.conv < 0 and (0, h) in gws[1]._hist_wait
    return gws, m, [x for x in msgs if x is not m]


def _settle(gws, msgs, ticks=200):
    for _ in range(ticks):
        _tick_all(gws)
        if all(x.status in (MessageStatus.COMPLETED, MessageStatus.CANCELLED, MessageStatus.FAILED) for x in msgs) \
                and all(g.engine.inflight() == 0 for g in gws):
            break


def _assert_nothing_left(gws):
    for g in gws:
        assert not g._hist_wait and not g._await_hist and not g.foreign and not g.remote_out and not g.local
        assert int(g.inflight_by_tier.sum()) == 0 and g.engine.inflight() == 0 and g.pending() == 0


def test_a_cancel_while_it_waits_leaves_nothing_behind():
    gws, m, others = _hold_one_waiting()
    f = gws[0].request_cancel(m)
    _settle(gws, others + [m])
    assert f.result(timeout=2) == "forwarded"
    assert m.status == MessageStatus.CANCELLED and all(x.status == MessageStatus.COMPLETED for x in others)
    assert gws[1].engine.cancelled_total == 0                          # (it never reached the engine)
    _assert_nothing_left(gws)


def test_a_failure_while_it_waits_hands_the_request_back():
    gws, m, others = _hold_one_waiting()
    gws[1].set_healthy(False, "test")                                  # evacuates what rank 1 holds
    assert not gws[1]._hist_wait and not gws[1]._await_hist
    _settle(gws, others + [m])
    # handed back untouched and served by the healthy rank, its lists in effect
    assert all(x.status == MessageStatus.COMPLETED for x in others + [m])
    assert m.endpoint_id == "gpu0" and m.retry_count == 0, (m.endpoint_id, m.retry_count)
    toks = m.metadata["generation"]["tokens"]
    sp = m.metadata["sampling"]
    if "allowed_token_ids" in sp:
        assert set(toks) <= set(sp["allowed_token_ids"])
    _assert_nothing_left(gws)
