"""Presence / frequency / repetition penalties on the GPU: ``penalise_kernel``
against the numpy twin bit for bit over whole tensors (padding included),
``penalised_argmax_kernel`` and ``history_record_kernel`` against theirs,
``HipOps.penalised_head`` over exact logits, and a penalised request end to
end through the HIP engine, on the serving pool and on the micro pool."""
import numpy as np
import pytest
import torch

import gemm_cases as GC
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S

DEV = "cuda:0"
STRIDE = 600
LENGTHS = (0, 1, 255, 256, 257, 513, 19, 40)         # across the block size (256) and its multiple
# (presence, frequency, repetition): each alone, repetition below 1, a negative presence, all three, all off
MIXES = ((1.25, 0.0, 1.0), (0.0, 0.5, 1.0), (0.0, 0.0, 1.7), (0.0, 0.0, 0.55), (-1.5, 0.0, 1.0), (0.75, 0.31, 1.3),
         (-2.0, -2.0, 2.0), (0.0, 0.0, 1.0))


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _case(V, R, seed, lengths=LENGTHS):
    """Logits [R][ld] (ld = V rounded up to 256, padding random too), a
    history table whose every entry is a valid id (so a read outside a row's
    window would show), per-row windows with heavy duplication, ids outside
    [0, V) -- among them ids in [V, ld) -- and non-finite logits on history
    columns."""
    rng = np.random.default_rng(seed)
    ld = (V + 255) // 256 * 256
    lg = torch.from_numpy((3.0 * rng.standard_normal((R, ld))).astype(np.float32)).to(torch.bfloat16)
    hist = rng.integers(0, V, (R + 3, STRIDE)).astype(np.int32)
    spans = np.zeros((R, 4), dtype=np.int32)
    params = np.zeros((R, 3), dtype=np.float32)
    outside = [-1, V, V + 3, 2 ** 31 - 1, -2 ** 31] + ([ld - 1, V + (ld - V) // 2] if ld > V else [])
    for r in range(R):
        n = lengths[r % len(lengths)]
        a = r % 5
        slot = (r * 7 + 1) % (R + 3)
        w = hist[slot, a:a + n]
        if r % 3 == 0 and n:                                          # heavy duplication: 7 ids
            w[:] = rng.choice(rng.integers(0, V, 7), n)
        if r % 2 == 0 and n > 4:                                      # ids the kernel must ignore
            w[rng.permutation(n)[:min(n // 4, len(outside))]] = outside[:min(n // 4, len(outside))]
        spans[r] = (slot, a, a + (n * (r % 4)) // 3 if r % 4 else a, a + n)
        spans[r, 2] = min(spans[r, 2], a + n)
        params[r] = MIXES[(r // 2) % len(MIXES)]
    lgv = lg.view(torch.int16).numpy().view(np.uint16)
    for r in range(0, R, 3):                                          # non-finite logits on history columns
        s, a, _m, b = spans[r]
        ok = [int(t) for t in hist[s, a:b] if 0 <= t < V][:3]
        for t, v in zip(ok, (0x7F80, 0xFF80, 0x7FC1)):                # inf, -inf, a NaN
            lgv[r, t] = v
    return lg, hist, spans, params, ld


@pytest.mark.gpu
@pytest.mark.parametrize("V,R", [(1000, 5), (4099, 40), (128256, 8), (1000, 1030)])
def test_penalise_equals_the_twin_bit_for_bit(V, R):
    from llm_message_queue_amd import _native
    assert 1030 > _native.require_hipops().PEN_MAX_BLOCKS            # (R = 1030 runs the grid-stride loop)
    assert _native.require_hipops().PEN_HIST_MAX == S.PEN_HIST_MAX   # (the package's copy of the header's constant)
    lg, hist, spans, params, ld = _case(V, R, seed=V + R, lengths=LENGTHS if R < 1000 else (19, 3, 40, 0, 257))
    before = _bits(lg).copy()
    want = S.penalise_rows_reference(before, V, hist, spans, params)
    d = lg.to(DEV)
    out = G.penalise(d, torch.from_numpy(hist).to(DEV), torch.from_numpy(spans).to(DEV),
                     torch.from_numpy(params).to(DEV), vocab=V)
    assert out.data_ptr() == d.data_ptr()
    got = _bits(d)
    changed = (want != before)
    print(f"V={V} ld={ld} R={R}: the twin edits {int(changed.sum())} columns, {int(changed.any(axis=1).sum())} rows")
    assert changed.sum() > R                                          # (the case does exercise the edit)
    assert not changed[:, V:].any()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(r), int(c), hex(before[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]


@pytest.mark.gpu
def test_penalise_refuses_a_history_above_its_cap_and_ignores_a_bad_slot():
    V = 1000
    lg, hist, spans, params, _ = _case(V, 5, seed=3)
    d = lg.to(DEV)
    big = torch.zeros((2, S.PEN_HIST_MAX + 1), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        G.penalise(d, big, torch.from_numpy(spans).to(DEV), torch.from_numpy(params).to(DEV), vocab=V)
    spans = spans.copy()
    spans[1, 0], spans[3, 0] = -1, len(hist)                          # rows without a slot: untouched
    spans[2, 1:] = (-5, 2, STRIDE + 50)                               # a span past the table: clamped to it
    want = S.penalise_rows_reference(_bits(lg), V, hist, spans, params)
    G.penalise(d, torch.from_numpy(hist).to(DEV), torch.from_numpy(spans).to(DEV), torch.from_numpy(params).to(DEV),
               vocab=V)
    got = _bits(d)
    assert np.array_equal(got, want)
    assert np.array_equal(got[1], _bits(lg)[1]) and np.array_equal(got[3], _bits(lg)[3])


@pytest.mark.gpu
def test_penalised_argmax_equals_the_twin():
    V, ld, R = 4099, 4352, 40
    rng = np.random.default_rng(5)
    lg = torch.from_numpy((3.0 * rng.standard_normal((R, ld))).astype(np.float32)).to(torch.bfloat16)
    lg[:, V:] = 3.0e38                                                # padding is never picked
    lg[0, :V] = -1.0
    lg[0, [77, 3000, 4098]] = 5.0                                     # a tie for the maximum: the lower column
    lg[1, :V] = float("nan")                                          # no finite column: token 0
    lg[2, :V] = float("inf")
    lg[3, :V] = float("-inf")
    lg[3, 4098] = -3.0e38                                             # the only candidate, in the last column
    lg[4, 9] = float("inf")                                           # an infinity is no candidate
    lg[5, :V] = -2.0
    lg[5, 1234] = 4.0                                                 # the maximum is a history column: displaced
    lg[5, 4000] = 3.5
    hist = np.full((1, 8), 1234, dtype=np.int32)
    spans = np.tile(np.array([[-1, 0, 0, 0]], dtype=np.int32), (R, 1))
    spans[5] = (0, 0, 2, 8)
    params = np.tile(np.array([[1.0, 0.25, 1.0]], dtype=np.float32), (R, 1))
    d = lg.to(DEV)
    G.penalise(d, torch.from_numpy(hist).to(DEV), torch.from_numpy(spans).to(DEV), torch.from_numpy(params).to(DEV),
               vocab=V)
    bits = _bits(d)
    assert np.array_equal(bits, S.penalise_rows_reference(_bits(lg), V, hist, spans, params))
    want = S.penalised_pick_reference(bits, V)
    assert want[0] == 77 and want[1] == 0 and want[2] == 0 and want[3] == 4098 and want[5] == 4000
    got = G.penalised_argmax(d, vocab=V).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero(got != want)
    # with inv_temp only the greedy rows are written
    it = torch.zeros(R, dtype=torch.float32, device=DEV)
    it[::2] = 0.8
    out = torch.full((R,), -9, dtype=torch.int32, device=DEV)
    got2 = G.penalised_argmax(d, vocab=V, inv_temp=it, out=out).cpu().numpy()
    assert (got2[::2] == -9).all() and np.array_equal(got2[1::2], want[1::2])
    # above the launcher's block cap
    many = d[:8].repeat(140, 1).contiguous()
    assert np.array_equal(G.penalised_argmax(many, vocab=V).cpu().numpy(), np.tile(want[:8], 140))


@pytest.mark.gpu
def test_history_record_scatters_the_listed_rows_only():
    rng = np.random.default_rng(9)
    slots, stride, T = 10, 64, 300
    cells = rng.permutation(slots * stride)[:T]                       # distinct (slot, pos) pairs
    slot, pos = (cells // stride).astype(np.int32), (cells % stride).astype(np.int32)
    tok = rng.integers(0, 128256, T).astype(np.int64)
    rows = np.flatnonzero((slot % 3 == 1) | (np.arange(T) % 11 == 0)).astype(np.int32)
    hist0 = rng.integers(-9, 0, (slots, stride)).astype(np.int32)
    want = hist0.copy()
    want[slot[rows], pos[rows]] = tok[rows]
    rows_d = np.concatenate([rows, np.array([-1, T, T + 7], dtype=np.int32)])   # out of range: nothing written
    slot_d, pos_d = slot.copy(), pos.copy()
    free = np.setdiff1d(np.arange(T), rows)
    slot_d[free[:3]] = (-1, slots, 3)
    pos_d[free[:3]] = (0, 0, stride)                                  # (unlisted anyway)
    h = torch.from_numpy(hist0).to(DEV)
    G.history_record(h, torch.from_numpy(tok).to(DEV), torch.from_numpy(pos_d).to(DEV),
                     torch.from_numpy(slot_d).to(DEV), torch.from_numpy(rows_d).to(DEV))
    got = h.cpu().numpy()
    assert (want != hist0).sum() == len(rows)
    assert np.array_equal(got, want)
    # a listed row with a slot or a position outside the table writes nothing
    bad = np.array([0, 1, 2], dtype=np.int32)
    G.history_record(h, torch.from_numpy(tok[:3]).to(DEV), torch.tensor([0, stride, -1], dtype=torch.int32, device=DEV),
                     torch.tensor([slots, 0, 0], dtype=torch.int32, device=DEV), torch.from_numpy(bad).to(DEV))
    assert np.array_equal(h.cpu().numpy(), want)


@pytest.mark.gpu
def test_penalised_head_over_exact_logits_equals_the_reference():
    """x and w over {-1, 0, 1}: the logits are integers, exact in fp32 and in
    bf16, so the store-epilogue GEMM's tensor is the reference's, the edit is
    the twin's bit for bit and the picks must agree row for row, greedy and
    sampling rows mixed; a row with every penalty off equals
    ``truncated_head``."""
    from llm_message_queue_amd.ops.llama_ops import HipOps, RefOps
    from tests.test_gpu_truncated_sampling import _params
    M, N, K = 37, 1024, 256
    c = GC.int_case(M, N, K, 11)
    rng = np.random.default_rng(4)
    keys = S.row_keys(np.arange(M, dtype=np.uint64) + np.uint64(31), np.arange(M) % 5)
    it, tk, tp = _params(M)
    it[np.arange(M) % 3 == 0] = 0.0                                   # greedy rows among the sampling ones
    hist = rng.integers(0, N, (M + 2, 64)).astype(np.int32)
    hist[:, ::4] = hist[:, 1::4]                                      # repeats
    spans = np.stack([(np.arange(M) * 5 + 1) % (M + 2), np.arange(M) % 7, np.arange(M) % 7 + np.arange(M) % 11,
                      np.arange(M) % 7 + 11 + np.arange(M) % 40], axis=1).astype(np.int32)
    params = np.array([MIXES[r % len(MIXES)] for r in range(M)], dtype=np.float32)
    off = (params == np.array([0, 0, 1], dtype=np.float32)).all(axis=1)
    assert off.sum() >= 3 and (off & (it > 0)).sum() >= 2 and (off & (it == 0)).sum() >= 1
    x, w = c.x.to(DEV), c.w.to(DEV)
    kd = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32))
    rowwise = [torch.from_numpy(it), kd, torch.from_numpy(tk), torch.from_numpy(tp)]
    tail = [torch.from_numpy(spans), torch.from_numpy(params)]
    hd = torch.from_numpy(hist)
    got = HipOps().penalised_head(x, w, *[a.to(DEV) for a in rowwise], hd.to(DEV),
                                  *[a.to(DEV) for a in tail]).cpu().numpy()
    want = RefOps().penalised_head(c.x, c.w, *rowwise, hd, *tail).numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    # the reference's logits are the exact integers
    assert np.array_equal((c.x.float() @ c.w.float().t()).numpy(), c.ref.numpy())
    plain = S.sample_truncated_reference(c.ref.numpy(), np.where(it > 0, it, 1.0), keys, tk, tp)
    assert (want[it > 0] != plain[it > 0]).any()                      # (the penalties are not a no-op here)
    hot = off & (it > 0)
    trunc = HipOps().truncated_head(x[torch.from_numpy(hot)], w, torch.from_numpy(it[hot]).to(DEV),
                                    kd[torch.from_numpy(hot)].to(DEV),
                                    torch.from_numpy(tk[hot]).to(DEV), torch.from_numpy(tp[hot]).to(DEV)).cpu().numpy()
    assert np.array_equal(got[hot], trunc)
    cold = off & (it == 0)
    assert np.array_equal(got[cold], S.penalised_pick_reference(S.bf16_bits(c.ref.numpy()[cold]), N))
    # greedy rows first and the hint: the same picks
    order = np.argsort(it > 0, kind="stable")
    g = int((it == 0).sum())
    o = torch.from_numpy(order)
    again = HipOps().penalised_head(x[o.to(DEV)], w, *[a[o].to(DEV) for a in rowwise], hd.to(DEV),
                                    *[a[o].to(DEV) for a in tail], n_greedy=g).cpu().numpy()
    assert np.array_equal(again, want[order])


# --------------------------------------------------------------------------- tiny model end to end
PEN = dict(presence_penalty=1.2, frequency_penalty=0.6, repetition_penalty=1.5)


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(2000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 6).astype(np.int32), gen_tokens=6, **kw)


def _drain(eng, reqs):
    assert len(eng.admit(reqs)) == len(reqs)
    done = {r.req_id: r for r in eng.drain()}
    assert len(done) == len(reqs)
    return done


class _Spy:
    """Wraps ``ops.gemm.penalise``: per call the logits before and after, and
    the twin applied to the captured input."""

    def __init__(self, monkeypatch):
        self.calls = 0
        self.inner = G.penalise
        monkeypatch.setattr(G, "penalise", self)

    def __call__(self, logits, hist, spans, params, vocab=None):
        R, V = logits.shape[0], int(vocab)
        before = _bits(logits).copy()
        out = self.inner(logits, hist, spans, params, vocab=vocab)
        torch.cuda.synchronize()
        after = _bits(logits)
        h, sp, pa = hist.cpu().numpy(), spans[:R].cpu().numpy(), params[:R].cpu().numpy()
        assert np.array_equal(after, S.penalise_rows_reference(before, V, h, sp, pa))
        for r in range(R):
            s, a, m, b = sp[r]
            assert 0 <= a <= m <= b <= h.shape[1] and b > a
            cols = np.unique(h[s, a:b])
            cols = cols[(cols >= 0) & (cols < V)]
            diff = np.flatnonzero(after[r] != before[r])
            assert np.isin(diff, cols).all(), (r, diff, cols)         # nowhere but at history columns
            v = S.bf16_values(before[r, cols])
            moved = np.isfinite(v) & (v != 0)                         # (rp scales a zero to itself)
            assert np.isin(cols[moved], diff).all(), (r, cols[moved], diff)
        self.calls += 1
        return out


@pytest.mark.gpu
def test_penalised_request_through_the_hip_engine(monkeypatch):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=64, max_ctx=64, token_budget=512, device=DEV, impl="hip")
    spy = _Spy(monkeypatch)

    def crowd():
        return [_req(i) for i in range(30)] + [_req(30 + i, temperature=0.9, seed=i) for i in range(10)]
    without = _drain(eng, crowd())
    assert eng.penalised_steps == 0 and eng.d_hist is None and spy.calls == 0   # (nobody asked: nothing new)
    alone = _drain(eng, [_req(100, **PEN)])[100]
    n = eng.penalised_steps
    assert n == 6 and spy.calls == 6
    again = _drain(eng, crowd())
    assert eng.penalised_steps == n
    among = _drain(eng, crowd() + [_req(100, **PEN)])
    assert eng.penalised_steps == n + 6
    hot = dict(PEN, temperature=0.8, seed=7, top_k=5)
    hot_alone = _drain(eng, [_req(101, **hot)])[101]
    t = eng.truncated_steps
    hot_among = _drain(eng, crowd() + [_req(101, **hot), _req(100, **PEN)])
    assert eng.truncated_steps == t                                   # (a penalised row is drawn again once)
    torch.cuda.synchronize()
    print("greedy", alone.out_tokens.tolist(), "sampling", hot_alone.out_tokens.tolist(),
          "unpenalised", _drain(eng, [_req(100)])[100].out_tokens.tolist())
    assert len(alone.out_tokens) == 6 and np.array_equal(alone.out_tokens, among[100].out_tokens)
    assert np.array_equal(alone.out_tokens, hot_among[100].out_tokens)
    assert np.array_equal(hot_alone.out_tokens, hot_among[101].out_tokens)
    for i in range(40):
        assert np.array_equal(among[i].out_tokens, without[i].out_tokens), i
        assert np.array_equal(again[i].out_tokens, without[i].out_tokens), i
        assert np.array_equal(hot_among[i].out_tokens, without[i].out_tokens), i
    eng.close()


@pytest.mark.gpu
def test_penalised_request_on_the_micro_pool(monkeypatch):
    """A realtime request with a penalty on the micro pool: eager decode
    steps (the captured graphs hold no such path), the same tokens as on the
    serving pool."""
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    from tests.test_realtime_micro import _serve
    kw = dict(slots=64, max_ctx=64, token_budget=512, device=DEV, impl="hip")
    base = BackendEngine(LlamaConfig.tiny(), **kw)
    want = _drain(base, [_req(100, tier=0, **PEN)])[100].out_tokens
    base.close()
    eng = BackendEngine(LlamaConfig.tiny(), realtime_mode="micro", micro_slots=4, **kw)
    eng.warm_shapes([1, 8, 64])
    assert eng._mg
    spy = _Spy(monkeypatch)
    plain = _serve(eng, [_req(7, tier=0)])
    assert plain[7][1] and eng.micro_graph_steps > 0 and eng.penalised_steps == 0
    g = eng.micro_graph_steps
    got = _serve(eng, [_req(100, tier=0, **PEN), _req(1, tier=2), _req(2, tier=1)])
    assert got[100][1] and not got[1][1]
    assert eng.micro_graph_steps == g and eng.penalised_steps == 6 and spy.calls == 6
    assert got[100][0] == want.tolist()
    eng.close()
