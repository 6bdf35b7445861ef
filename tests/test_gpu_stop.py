"""Stop tokens and stop sequences on the GPU: ``stop_match_kernel`` against
its numpy twin (exact: everything is integer), ``HipOps.stop_match`` against
``RefOps``, ``LlamaStub.forward(stop=...)`` on the tiny model, and stop
requests end to end through the HIP engine, on the serving pool (run-ahead 2:
the stop is acted on when the step is reaped) and on the micro pool."""
import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S
from tests.test_stop_cpu import GEN, drive, expected_cut, first_index, naive_stop, random_stop_case

DEV = "cuda:0"
N_SLOTS, STRIDE = 5, 37                               # (a stride that is no multiple of 64)
TOP = (1 << 31) - 1


def _launch(tok, hist, rows, ent):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)   # noqa: E731
    out = G.stop_match(d(tok), None if hist is None else d(hist), d(rows), d(ent))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def built_cases():
    """Hand-built rows; returns (tok, hist, rows, ent, want) with ``want``
    the result each row was built to give."""
    rng = np.random.default_rng(11)
    hist = rng.integers(100, 200, (N_SLOTS, STRIDE)).astype(np.int32)
    hist[3, 20] = -1                                                   # ids that are no token at all
    hist[3, 21] = TOP
    tok, rows, ent, want = [], [], [], []

    def add(t0, slot, a, b, mn, entries, res):
        tok.append(t0)
        rows.append([slot, a, b, mn, len(ent), len(entries)])
        for e in entries:
            ent.append([len(e) if not isinstance(e, tuple) else e[0]] + list(e if not isinstance(e, tuple) else e[1])
                       + [0] * (S.STOP_LEN - len(e if not isinstance(e, tuple) else e[1])))
        want.append(res)

    for g in range(10):                                                # generated before this step: 0..9
        a = 12
        b = a + g
        t0 = 300 + g
        w = hist[1, :b].tolist() + [t0]                               # (with what lies before gen_from)
        for ln in range(1, S.STOP_LEN + 1):
            tail = w[len(w) - ln:]
            # one longer than, equal to and shorter than the window; where it is longer, the positions before
            # gen_from would complete the match, so a read outside the window shows
            add(t0, 1, a, b, 0, [tail], 0 if ln <= g + 1 else -1)
            if ln <= g + 1:
                miss_old, miss_new = list(tail), list(tail)
                miss_old[0] += 1
                miss_new[-1] += 1
                add(t0, 1, a, b, 0, [miss_old], -1)                    # a near miss at the oldest position
                add(t0, 1, a, b, 0, [miss_new], -1)                    # ... and at the newest
                add(t0, 1, a, b, 0, [miss_old, miss_new, tail, [t0]], 2)
        # min_tokens at g (below g + 1: passes), g + 1 and g + 2
        add(t0, 1, a, b, g, [[t0]], 0)
        add(t0, 1, a, b, g + 1, [[t0]], 0)
        add(t0, 1, a, b, g + 2, [[t0]], -1)
    w = hist[2, 5:9].tolist() + [77]
    eight = [[1], [2], [3], [4], [5], [6], [7], w[-3:]]
    add(77, 2, 5, 9, 0, [w[-2:]] + eight[1:], 0)                       # entries 0 and 7 at once: the lowest wins
    add(77, 2, 5, 9, 0, eight, 7)                                      # only entry 7
    add(77, 2, 5, 9, 0, [(0, [77]), (9, w[-1:] * 8), [77]], 2)         # lengths 0 and 9 are ignored
    add(77, -1, 5, 9, 0, [w[-2:], [77]], 1)                            # slot -1: only t0 is compared
    add(77, N_SLOTS, 5, 9, 0, [w[-2:], [77]], 1)                       # slot n_slots likewise
    add(77, N_SLOTS + 1000, 0, STRIDE, 0, [w[-2:]], -1)
    w = hist[4, :].tolist() + [78]
    add(78, 4, -9, STRIDE + 50, 0, [w[-8:]], 0)                        # a span clamped to the table on both sides
    add(78, 4, STRIDE + 5, STRIDE + 9, 0, [w[-2:]], -1)                # clamped to nothing: g = 0
    add(78, 4, STRIDE + 5, STRIDE + 9, 0, [[78]], 0)
    add(78, 4, 9, 3, 0, [[hist[4, 8], 78]], -1)                        # end before from: g = 0
    add(TOP, 3, 19, 22, 0, [[-1, TOP, TOP]], 0)                        # ids -1 and 2^31 - 1
    add(-1, 3, 19, 21, 0, [[int(hist[3, 19]), -1, -1]], 0)
    add(TOP, 3, 19, 22, 0, [[-1, TOP, TOP - 1], [TOP - 1]], -1)
    return (np.asarray(tok, dtype=np.int32), hist, np.asarray(rows, dtype=np.int32), np.asarray(ent, dtype=np.int32),
            np.asarray(want, dtype=np.int32))


def test_built_cases_are_what_they_were_built_to_be():
    tok, hist, rows, ent, want = built_cases()
    assert np.array_equal(S.stop_match_reference(tok, hist, rows, ent), want)
    assert np.array_equal(naive_stop(tok, hist, rows, ent), want)
    assert (want >= 0).sum() > 80 and (want < 0).sum() > 80 and {0, 2, 7} <= set(want.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 7, 4 * 1024 + 3])                    # (4,099: above the block cap, no multiple of 4)
def test_stop_match_kernel_equals_the_twin(R):
    from llm_message_queue_amd import _native
    h = _native.require_hipops()
    assert (h.STOP_ENTRIES, h.STOP_LEN, h.STOP_ROW_WORDS, h.STOP_ENT_WORDS) \
        == (S.STOP_ENTRIES, S.STOP_LEN, S.STOP_ROW_WORDS, S.STOP_ENT_WORDS)
    assert R <= 7 or R > 4 * h.STOP_MAX_BLOCKS
    tok, hist, rows, ent, want = built_cases()
    if R <= len(tok):
        for lo in range(0, len(tok) - R + 1, max(1, R)):               # every built row, R at a time
            sl = slice(lo, lo + R)
            assert np.array_equal(_launch(tok[sl], hist, rows[sl], ent), want[sl]), lo
    else:
        rng = np.random.default_rng(R)
        rt, rh, rr, re = random_stop_case(rng, R - len(tok), n_slots=N_SLOTS, stride=STRIDE)
        rr[:, 4] += len(ent)                                           # (the random rows' entries behind the built ones)
        tok, rows, ent = np.concatenate([tok, rt]), np.concatenate([rows, rr]), np.concatenate([ent, re])
        hist = np.concatenate([hist, rh])                              # slots 5.. hold the random table
        rows[len(want):, 0] = np.where(rows[len(want):, 0] >= 0, rows[len(want):, 0] + N_SLOTS, -1)
        twin = S.stop_match_reference(tok, hist, rows, ent)
        assert np.array_equal(twin[:len(want)], want) and (twin[len(want):] >= 0).sum() > 200
        got = _launch(tok, hist, rows, ent)
        assert got.dtype == np.int32 and np.array_equal(got, twin)


@pytest.mark.gpu
def test_stop_match_without_a_table_and_its_argument_checks():
    tok, hist, rows, ent, want = built_cases()
    one = np.flatnonzero(np.asarray([all(ent[o:o + c, 0] == 1) and c > 0 for o, c in rows[:, 4:6].tolist()]))
    assert len(one) > 20
    r1 = rows[one].copy()
    r1[:, 0] = -1                                                      # entries of one token: no history is read
    got = _launch(tok[one], None, r1, ent)
    assert np.array_equal(got, S.stop_match_reference(tok[one], None, r1, ent)) and (got >= 0).sum() > 10
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)   # noqa: E731
    with pytest.raises(ValueError):
        G.stop_match(d(tok), d(hist), d(rows[:3]), d(ent))             # fewer records than rows
    with pytest.raises(ValueError):
        G.stop_match(d(tok).long(), d(hist), d(rows), d(ent))
    with pytest.raises(ValueError):
        G.stop_match(d(tok), d(hist), d(rows)[:, :5].contiguous(), d(ent))
    with pytest.raises(ValueError):
        G.stop_match(d(tok), d(hist).cpu(), d(rows), d(ent))
    from llm_message_queue_amd import _native
    h = _native.require_hipops()
    t, r, e, o = d(tok), d(rows), d(ent), torch.empty(len(tok), dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for bad in ((0, len(tok), 0, 0, 0, r.data_ptr(), e.data_ptr(), len(ent), o.data_ptr(), st),          # null tok
                (t.data_ptr(), len(tok), 0, 3, 7, r.data_ptr(), e.data_ptr(), len(ent), o.data_ptr(), st),   # no table, a shape
                (t.data_ptr(), len(tok), t.data_ptr(), 0, 7, r.data_ptr(), e.data_ptr(), len(ent), o.data_ptr(), st),
                (t.data_ptr(), -1, 0, 0, 0, r.data_ptr(), e.data_ptr(), len(ent), o.data_ptr(), st),
                (t.data_ptr(), len(tok), 0, 0, 0, r.data_ptr() + 2, e.data_ptr(), len(ent), o.data_ptr(), st),
                (t.data_ptr(), len(tok), 0, 0, 0, r.data_ptr(), 0, len(ent), o.data_ptr(), st)):
        with pytest.raises(ValueError):
            h.stop_match(*bad)


@pytest.mark.gpu
def test_hip_ops_stop_match_equals_ref_ops():
    from llm_message_queue_amd.ops.llama_ops import HipOps, RefOps
    tok, hist, rows, ent, want = built_cases()
    t = lambda a: torch.from_numpy(a)                                  # noqa: E731
    ref = RefOps().stop_match(t(tok), t(hist), t(rows), t(ent))
    got = HipOps().stop_match(t(tok).to(DEV), t(hist).to(DEV), t(rows).to(DEV), t(ent).to(DEV))
    assert got.dtype == ref.dtype == torch.int32 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref.numpy()) and np.array_equal(ref.numpy(), want)


@pytest.mark.gpu
def test_forward_with_stop_on_the_tiny_model():
    """The returned flags are the twin's over the returned tokens and the
    history the forward recorded; the tokens are what they are without
    ``stop``."""
    from llm_message_queue_amd.models.llama_stub import LlamaConfig, LlamaStub, Stops
    m = LlamaStub(LlamaConfig.tiny(), 4, 32, device=torch.device(DEV), impl="hip", seed=0)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)     # noqa: E731
    tok = torch.tensor([5, 6, 7, 8, 9], dtype=torch.long, device=DEV)
    pos, slot = i32([0, 1, 2, 0, 1]), i32([0, 0, 0, 2, 2])
    samp = torch.tensor([2, 4], dtype=torch.long, device=DEV)
    t0 = m.forward(tok, pos, slot, samp)
    assert torch.is_tensor(t0)
    a0 = [int(x) for x in t0.cpu()]
    pos1, slot1 = i32([3, 2]), i32([0, 2])
    s1 = torch.tensor([0, 1], dtype=torch.long, device=DEV)
    a1 = [int(x) for x in m.forward(t0.long(), pos1, slot1, s1).cpu()]
    # slot 0: prompt 3 tokens, slot 2: prompt 2; entries over the tokens just learnt
    ent = torch.from_numpy(S.stop_table([[a0[0]], [a0[0], a1[0]], [1 << 20], [9, a0[1], a1[1]], [a0[1], a1[1]]])).to(DEV)
    hist = torch.full((4, 32), -5, dtype=torch.int32, device=DEV)
    rows0 = i32([[0, 3, 3, 0, 0, 2], [2, 2, 2, 0, 2, 3]])
    res = m.forward(tok, pos, slot, samp, stop=Stops(hist, i32([0, 1, 2, 3, 4]), s1, rows0, ent))
    torch.cuda.synchronize()
    assert res.lp is None and res.ids is None
    out, flags = res.tokens, res.stop_flags
    assert out.cpu().tolist() == a0 and flags.dtype == torch.int32
    want0 = S.stop_match_reference(out.cpu().numpy(), hist.cpu().numpy(), rows0.cpu().numpy(), ent.cpu().numpy())
    assert flags.cpu().tolist() == want0.tolist() == [0, -1]
    assert hist[0, :3].cpu().tolist() == [5, 6, 7] and hist[2, :2].cpu().tolist() == [8, 9] and int(hist[0, 3]) == -5
    rows1 = i32([[0, 3, 4, 0, 1, 1], [2, 2, 3, 0, 2, 3]])
    res = m.forward(out.long(), pos1, slot1, s1, logp=torch.tensor([1], device=DEV),
                    stop=Stops(hist, i32([0, 1]), s1, rows1, ent))
    torch.cuda.synchronize()
    out, lp, ids, flags = res.tokens, res.lp, res.ids, res.stop_flags
    assert out.cpu().tolist() == a1 and lp.shape == (1, 6) and ids.shape == (1, 5)
    assert int(hist[0, 3]) == a0[0] and int(hist[2, 2]) == a0[1]       # the decode rows' tokens, recorded before the head
    want1 = S.stop_match_reference(out.cpu().numpy(), hist.cpu().numpy(), rows1.cpu().numpy(), ent.cpu().numpy())
    # slot 2: [9 t0 t1] reaches before gen_from = 2 and must not match; [t0 t1] does
    assert flags.cpu().tolist() == want1.tolist() == [0, 2]


# --------------------------------------------------------------------------- the HIP engine
def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=GEN, **kw)


def _hip_engine(**kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=8, max_ctx=64, token_budget=64, device=DEV, impl="hip", **kw)


@pytest.mark.gpu
def test_stop_requests_through_the_hip_engine():
    """Six requests, at most 6 * 7 = 42 tokens a step, so every step runs the
    same kernels with and without the stop and tokens compare exactly."""
    eng = _hip_engine()
    assert eng.max_inflight == 2
    base = {k: r.out_tokens.copy() for k, r in drive(eng, [_req(i) for i in range(6)]).items()}
    assert eng.stop_steps == 0 and eng.h_stop is None and all(len(t) == GEN for t in base.values())
    b1 = base[1]
    i = first_index(b1, 2)
    runs = (("token", [[1 << 20], [int(b1[i])]]), ("sequence", [[1 << 20], [int(b1[i - 1]), int(b1[i])]]))
    stopped = 0
    for kind, entries in runs:
        want, k = expected_cut(b1, entries)
        assert k == 1 and len(want) == i + 1 < GEN
        dropped = eng.stop_dropped_rows
        got = drive(eng, [_req(j, stop=entries if j == 1 else None, finish=j == 1) for j in range(6)])
        r = got[1]
        print(kind, r.out_tokens.tolist(), want, eng.stop_steps, eng.stop_dropped_rows)
        assert r.out_tokens.tolist() == want and r.finish_reason == "stop" and r.stop_entry == 1
        for j in (0, 2, 3, 4, 5):
            assert got[j].out_tokens.tolist() == base[j].tolist() and got[j].finish_reason == "length", (kind, j)
        stopped += 1
        assert eng.stopped_total == stopped and eng.stop_dropped_rows - dropped == min(1, GEN - len(want))
        assert sorted(eng.free) == list(range(8)) and not eng.active
    assert (eng.d_hist is not None) and eng.stop_steps >= 2 * (i + 1)
    # min_tokens, max_tokens, and a request admitted into the freed slot
    r = drive(eng, [_req(1, stop=[[int(b1[0])]], min_tokens=2, max_tokens=4)])[1]
    want, k = expected_cut(b1[:4], [[int(b1[0])]], min_tokens=2)
    assert r.out_tokens.tolist() == want and len(want) >= 2 and r.finish_reason == ("stop" if k >= 0 else "length")
    one = _hip_engine()
    solo2 = drive(one, [_req(2)])[2].out_tokens.tolist()
    assert len(one.admit([_req(1, stop=[[int(b1[i])]])])) == 1
    done, late = {}, None
    for _ in range(40):
        if late is None and len(one.free) == 8:                        # the reap freed the slot request 1 held:
            late = _req(2)                                             # the next admission takes it (reused first)
            assert len(one.admit([late])) == 1
        if not one.active:
            break
        one.launch()
    done = {r.req_id: r for r in one.finish(block=True).completed}
    assert done[1].out_tokens.tolist() == b1[:i + 1].tolist() and done[2].slot == done[1].slot
    assert done[2].out_tokens.tolist() == solo2
    eng.close()
    one.close()


@pytest.mark.gpu
def test_stop_request_on_the_micro_pool_goes_eager_and_others_replay_a_graph():
    from tests.test_realtime_micro import _serve
    base = _hip_engine()
    b7 = drive(base, [_req(7, tier=0)])[7].out_tokens
    base.close()
    i = first_index(b7, 2)
    eng = _hip_engine(realtime_mode="micro", micro_slots=4)
    eng.warm_shapes([1, 8, 64])
    assert eng._mg
    plain = _serve(eng, [_req(7, tier=0)])
    assert plain[7] == (b7.tolist(), True) and eng.micro_graph_steps > 0 and eng.stop_steps == 0
    g = eng.micro_graph_steps
    got = _serve(eng, [_req(7, tier=0, stop=[[int(b7[i - 1]), int(b7[i])]]), _req(1, tier=2)])
    assert got[7] == (b7[:i + 1].tolist(), True) and not got[1][1]
    assert eng.micro_graph_steps == g and eng.stop_steps == i + 1 and eng.stopped_total == 1   # eager, every step
    again = _serve(eng, [_req(7, tier=0, max_tokens=3)])
    assert again[7] == (b7[:3].tolist(), True) and eng.micro_graph_steps > g and eng.stop_steps == i + 1
    assert len(eng.free_micro) == 4
    eng.close()
