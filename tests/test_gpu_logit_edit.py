"""``logit_bias``, ``allowed_token_ids`` and ``min_p`` on the GPU:
``logit_edit_kernel`` against the numpy twin bit for bit over whole tensors
(padding included), ``sample_truncated_kernel`` with ``log_min_p`` against its
twin, ``HipOps.penalised_head`` / ``truncated_head`` over exact logits against
the reference ops, and edited requests end to end through the HIP engine."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as GC
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S

DEV = "cuda:0"
NEG_INF = 0xFF80
SENTINEL = 0x7B5A                                    # a finite bf16 pattern for the padding (about 1.1e36)
NOISE = 1e-3                                         # the noise-arithmetic bound of test_gpu_sampling.py
SIZES = (0, 1, 64)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _from_bits(b: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).view(torch.bfloat16)


def _lists(rng, V, n, kind):
    """``n`` ids: the edges 0, V - 1 and the ignored V, -1 first, then random
    ids with repeats (``kind`` 0), or distinct ids (``kind`` 1)."""
    edge = [0, V - 1, V, -1, V + 5, 2 ** 31 - 1, -2 ** 31]
    if n == 1:
        return np.array([edge[kind % 2]], dtype=np.int32)
    if kind == 0:
        body = rng.integers(0, V, max(n - len(edge), 0) // 2 + 1)
        ids = np.concatenate([edge, body, body])[:n]                  # every body id twice
    else:
        ids = np.concatenate([edge, rng.permutation(V)[:max(n - len(edge), 0)]])[:n]
    out = np.resize(ids, n).astype(np.int64)
    return rng.permutation(out).astype(np.int32)


def _edit_case(V, ld, R, seed):
    """Logits [R][ld] with the padding set to a sentinel, and per row an allow
    list and a bias list of every pair of sizes in {0, 1, 64}; lists share
    ids (a column both allowed and biased), hold repeats and ids outside
    [0, V); some rows are all NaN, +inf or -inf."""
    rng = np.random.default_rng(seed)
    lg = _bits(torch.from_numpy((3.0 * rng.standard_normal((R, ld))).astype(np.float32)).to(torch.bfloat16)).copy()
    lg[:, V:] = SENTINEL
    ids, vals, spans = [np.array([7, 7, 7], dtype=np.int32)], [np.zeros(3, dtype=np.float32)], []    # (an unused head)
    off = 3
    for r in range(R):
        na, nb = SIZES[r % 3], SIZES[(r // 3) % 3]
        al = _lists(rng, V, na, r % 2) if na else np.zeros(0, dtype=np.int32)
        bi = _lists(rng, V, nb, (r + 1) % 2) if nb else np.zeros(0, dtype=np.int32)
        if na and nb:
            bi[:min(3, nb, na)] = al[:min(3, nb, na)]                 # ids both allowed and biased
        bv = rng.choice(np.array([100.0, -100.0, 0.5, -3.25, 2.0 ** -8, 1e-3, 17.3], dtype=np.float32), nb)
        ids += [al, bi]
        vals += [rng.standard_normal(na).astype(np.float32), bv]      # (values beside allow ids are never read)
        spans.append((off, na, off + na, nb))
        off += na + nb
        if r % 9 == 4:
            lg[r, :V] = (0x7FC1, 0x7F80, NEG_INF)[(r // 9) % 3]       # a row of NaN, +inf, -inf
    return lg, np.concatenate(ids), np.concatenate(vals), np.array(spans, dtype=np.int32)


def _run_edit(lg, ids, vals, spans, V):
    d = _from_bits(lg).to(DEV)
    out = G.logit_edit(d, torch.from_numpy(ids).to(DEV), torch.from_numpy(vals).to(DEV), torch.from_numpy(spans).to(DEV),
                       vocab=V)
    assert out.data_ptr() == d.data_ptr()
    return _bits(d)


def _assert_equal(got, want, before):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(r), int(c), hex(before[r, c]), hex(got[r, c]), hex(want[r, c])) for r, c in bad[:8]]


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld,R", [(1003, 1008, 3), (1003, 1008, 27), (8, 8, 2), (8, 8, 27), (128256, 128256, 2),
                                    (128256, 128256, 9), (4099, 4104, 18)])
def test_logit_edit_equals_the_twin_bit_for_bit(V, ld, R):
    from llm_message_queue_amd import _native
    assert _native.require_hipops().LE_MAX == S.LE_MAX == 64          # (the package's copy of the header's constant)
    lg, ids, vals, spans = _edit_case(V, ld, R, seed=V + R)
    want = S.logit_edit_reference(lg, V, ids, vals, spans)
    got = _run_edit(lg, ids, vals, spans, V)
    changed = want != lg
    print(f"V={V} ld={ld} R={R}: the twin edits {int(changed.sum())} columns in {int(changed.any(axis=1).sum())} rows")
    assert changed.any() and not changed[:, V:].any()
    assert (got[:, V:] == SENTINEL).all()                             # the partial last vector left the padding alone
    _assert_equal(got, want, lg)


@pytest.mark.gpu
def test_logit_edit_hand_built_rows():
    V, ld = 1003, 1008
    rng = np.random.default_rng(2)
    lg = _bits(torch.from_numpy(rng.standard_normal((8, ld)).astype(np.float32)).to(torch.bfloat16)).copy()
    lg[:, V:] = SENTINEL
    lg[5, :V] = 0x7FC1
    lg[6, :V] = 0x7F80
    lg[7, :V] = NEG_INF
    ids = np.array([0, V - 1, V, -1, 500, 500,            # 0..6: an allow list with the edges and a repeat
                    500, 0, 500, V - 1, V, -1,            # 6..12: biases; 500 twice (the first counts), the edges
                    1002, 1000, 1001], dtype=np.int32)    # 12..15
    vals = np.array([0, 0, 0, 0, 0, 0, 2.5, -100, 64, 100, 9, 9, 1, 1, 1], dtype=np.float32)
    spans = np.array([[0, 6, 6, 6],        # allow + bias, ids both allowed and biased
                      [0, 0, 0, 0],        # all zero: a no-op
                      [0, 0, 6, 6],        # bias only
                      [12, 3, 0, 0],       # allow only, in the last, partial vector
                      [2, 2, 10, 2],       # only ids outside the vocabulary: the row is masked, no bias lands
                      [0, 6, 6, 6], [0, 6, 6, 6], [0, 6, 6, 6]], dtype=np.int32)     # NaN, +inf, -inf rows
    want = S.logit_edit_reference(lg, V, ids, vals, spans)
    got = _run_edit(lg, ids, vals, spans, V)
    _assert_equal(got, want, lg)
    assert np.flatnonzero(got[0, :V] != NEG_INF).tolist() == [0, 500, V - 1]
    assert S.bf16_values(got[0, [500]])[0] == S.bf16_values(S.bf16_bits(S.bf16_values(lg[0, [500]]) + np.float32(2.5)))[0]
    assert np.array_equal(got[1], lg[1])
    assert np.flatnonzero(got[2] != lg[2]).tolist() == [0, 500, V - 1]
    assert np.flatnonzero(got[3, :V] != NEG_INF).tolist() == [1000, 1001, 1002]
    assert np.array_equal(got[3, [1000, 1001, 1002]], lg[3, [1000, 1001, 1002]])
    assert (got[4, :V] == NEG_INF).all()
    assert (got[5, [0, 500, V - 1]] == 0x7FC0).all() and got[6, 0] == 0x7F80 and (got[7, :V] == NEG_INF).all()
    assert (got[:, V:] == SENTINEL).all()
    # spans that leave the lists are clamped to them, a count is capped at LE_MAX
    wild = np.array([[-5, 3, 13, 99], [14, 99, -1, 0], [99, 9, 99, 9], [0, -4, 0, -4], [2 ** 31 - 1, 2 ** 31 - 1, 6, 4],
                     [0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.int32)
    want = S.logit_edit_reference(lg, V, ids, vals, wild)
    _assert_equal(_run_edit(lg, ids, vals, wild, V), want, lg)
    assert np.array_equal(want[2], lg[2]) and np.array_equal(want[3], lg[3])
    long_ids = (np.arange(100, dtype=np.int32) * 7) % V
    one = np.array([[0, 100, 0, 0]], dtype=np.int32)
    got = _run_edit(lg[:1], long_ids, np.zeros(100, dtype=np.float32), one, V)
    assert np.flatnonzero(got[0, :V] != NEG_INF).tolist() == sorted(long_ids[:64].tolist())
    # wrong arguments are refused
    d = _from_bits(lg).to(DEV)
    i, v, s = (torch.from_numpy(a).to(DEV) for a in (ids, vals, spans))
    for bad in ((d, i.long(), v, s), (d, i, v[:-1], s), (d, i, v, s[:, :3].contiguous()), (d, i, v, s[:4]),
                (d.float(), i, v, s), (d[:, 1:], i, v, s)):
        with pytest.raises(ValueError):
            G.logit_edit(*bad, vocab=V if bad[0].shape[1] >= V else None)
    with pytest.raises(ValueError):
        G.logit_edit(d, i, v, s, vocab=ld + 1)


@pytest.mark.gpu
def test_logit_edit_above_the_block_cap():
    from llm_message_queue_amd import _native
    cap = _native.require_hipops().LE_MAX_BLOCKS
    V, ld, R = 24, 24, cap + 7                                        # (the grid-stride loop: rows cap .. cap + 6)
    lg, ids, vals, spans = _edit_case(V, ld, R, seed=5)
    want = S.logit_edit_reference(lg, V, ids, vals, spans)
    assert (want[cap:] != lg[cap:]).any()
    _assert_equal(_run_edit(lg, ids, vals, spans, V), want, lg)


# --------------------------------------------------------------------------- min_p in the sampler
PERMILLE = (1, 50, 500, 1000)
MODES = {"alone": (0, 1.0), "top_k": (40, 1.0), "top_p": (0, 0.9)}


def _launch(lg: torch.Tensor, V, it, keys, tk, tp, lmp=None) -> np.ndarray:
    R = lg.shape[0]
    ld = (V + 7) // 8 * 8
    d = torch.full((R, ld), 3.0e38, dtype=torch.bfloat16, device=DEV)         # (the padding must never be picked)
    d[:, :V] = lg.to(DEV)
    got = G.sample_truncated(d, torch.from_numpy(it).to(DEV),
                             torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).to(DEV),
                             torch.from_numpy(tk).to(DEV), torch.from_numpy(tp).to(DEV), vocab=V,
                             log_min_p=None if lmp is None else torch.from_numpy(lmp).to(DEV))
    return got.cpu().numpy().astype(np.int64)


def _scores(row64, it, key):
    sc = row64 * float(it) + S.gumbel(key.reshape(1, 2), np.arange(len(row64), dtype=np.uint32))[0]
    return np.where(np.isfinite(row64), sc, -np.inf)


def _check_pick(r, got, row64, it, key, keep):
    """The pick is the twin's, or -- the device's scores being fp32 -- a kept
    column whose float64 score is within the noise bound of the twin's."""
    sc = np.where(keep, _scores(row64, it, key), -np.inf)
    want = int(sc.argmax())
    assert keep[got], (r, got, "is not kept")                         # the keep rule itself is exact
    if got != want:
        gap = sc[want] - sc[got]
        margin = NOISE + 2.0 ** -22 * np.abs(sc[np.isfinite(sc)]).max()
        print(f"  row {r}: got {got} twin {want} gap {gap:.3e} margin {margin:.3e}")
        assert 0 <= gap <= margin, (r, got, want, gap)
    return got == want


@functools.lru_cache(maxsize=None)
def _rows(V):
    rng = np.random.default_rng(V)
    lg = torch.from_numpy((3.0 * rng.standard_normal((4, V))).astype(np.float32)).to(torch.bfloat16)
    keys = S.row_keys(np.arange(4, dtype=np.uint64) + np.uint64(900), np.arange(4))
    it = (1.0 / np.array([0.25, 0.7, 1.0, 2.0])).astype(np.float32)
    return lg, keys, it


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("V", [1003, 128256])
def test_min_p_kernel_matches_the_twin(V, mode):
    lg, keys, it = _rows(V)
    k, p = MODES[mode]
    tk, tp = np.full(4, k, dtype=np.int32), np.full(4, p, dtype=np.float32)
    lmp = S.min_p_log(np.array(PERMILLE) / 1000.0)
    assert lmp.dtype == np.float32 and lmp[3] == 0.0
    got = _launch(lg, V, it, keys, tk, tp, lmp)
    rows64 = lg.double().numpy()
    equal = 0
    for r in range(4):
        keep = S.truncation_keep(rows64[r], it[r], tk[r], tp[r], log_min_p=lmp[r])
        base = S.truncation_keep(rows64[r], it[r], tk[r], tp[r])
        print(f"V={V} {mode} permille={PERMILLE[r]}: keeps {int(keep.sum())} of {int(base.sum())}")
        assert keep.sum() <= base.sum() and (r < 3 or keep.sum() == 1)
        if tp[r] < 1:
            # top_p's own threshold is a float sum on the device: accept the twin's set at top_p (1 -+ 1e-3) too
            sets = [S.truncation_keep(rows64[r], it[r], tk[r], np.float32(tp[r]) * np.float32(f), log_min_p=lmp[r])
                    for f in (1.0, 1.0 - 1e-3, 1.0 + 1e-3)]
            keep = next((s for s in sets if s[got[r]]), keep)
        equal += _check_pick(r, int(got[r]), rows64[r], it[r], keys[r], keep)
    assert equal >= 3
    # min_p does change what is kept at these shapes (not a no-op)
    assert any(S.truncation_keep(rows64[r], it[r], tk[r], tp[r], log_min_p=lmp[r]).sum()
               < S.truncation_keep(rows64[r], it[r], tk[r], tp[r]).sum() for r in range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1003, 128256])
def test_min_p_off_reproduces_the_kernel_without_the_argument(V):
    lg, keys, it = _rows(V)
    for k, p in MODES.values():
        tk, tp = np.full(4, k, dtype=np.int32), np.full(4, p, dtype=np.float32)
        base = _launch(lg, V, it, keys, tk, tp)
        off = _launch(lg, V, it, keys, tk, tp, np.full(4, -np.inf, dtype=np.float32))
        assert np.array_equal(base, off), (V, k, p)
        mixed = np.array([-np.inf, 0.0, -np.inf, 0.0], dtype=np.float32)     # per row: rows 0 and 2 off
        got = _launch(lg, V, it, keys, tk, tp, mixed)
        assert np.array_equal(got[[0, 2]], base[[0, 2]])
        assert np.array_equal(got[[1, 3]], lg.float().numpy()[[1, 3]].argmax(axis=1))   # min_p = 1: the maximum


@pytest.mark.gpu
@pytest.mark.parametrize("V", [1003, 128256])
def test_min_p_ties_at_the_maximum_and_a_threshold_exactly_on_a_value(V):
    """Rows whose kept set is known column by column.  The draw among the kept
    columns is decided by noise the host knows in float64, so the rows' keys
    are chosen, on the host, to make the twin's pick win by a clear margin
    (>= 0.05): then the device's pick must be exactly the twin's.  For every
    boundary there are also keys under which a column just below the
    threshold would win if it were kept, so the exclusion is tested too."""
    rng = np.random.default_rng(7)
    tie_cols = np.sort(rng.permutation(V)[:5])
    thr_cols = np.sort(rng.permutation(V)[:6])
    base = np.minimum(-6.0 - np.abs(rng.standard_normal(V)), -6.0).astype(np.float32)
    tie = base.copy()
    tie[tie_cols] = 3.5                                               # five columns share the maximum
    tie[(tie_cols[0] + 1) % V] = 3.484375                             # ... the next bf16 below it must go
    thr = base.copy()
    thr[thr_cols[0]] = 4.0
    thr[thr_cols[1:4]] = 2.0                                          # (2 - 4) * 0.5 = -1 exactly: kept at -1
    thr[thr_cols[4:]] = 1.9921875                                     # the next bf16 below: never kept
    below = np.nextafter(np.float32(-1.0), np.float32(0.0))
    # (row, inv_temp, log_min_p, the kept columns, the trap: the columns just below the threshold)
    cases = [(tie, np.float32(0.7), np.float32(0.0), set(tie_cols.tolist()), {int((tie_cols[0] + 1) % V)}),
             (thr, np.float32(0.5), np.float32(-1.0), set(thr_cols[:4].tolist()), set(thr_cols[4:].tolist())),
             (thr, np.float32(0.5), below, {int(thr_cols[0])}, set(thr_cols[1:4].tolist())),
             (thr, np.float32(0.5), np.float32(-1.5), set(thr_cols.tolist()), set())]
    rows, its, lmps, keys, wants = [], [], [], [], []
    trapped = 0
    for ci, (row, it, lm, kept, trap) in enumerate(cases):
        row64 = torch.from_numpy(row).to(torch.bfloat16).double().numpy()
        keep = S.truncation_keep(row64, it, 0, 1.0, log_min_p=lm)
        assert set(np.flatnonzero(keep).tolist()) == kept, ci
        wide = keep.copy()
        wide[sorted(trap)] = True
        found, traps = {}, {}
        for seed in range(2000):
            key = S.row_keys(np.uint64(seed + 10000 * ci), 0)[0]
            full = _scores(row64, it, key)
            sc = np.sort(np.where(keep, full, -np.inf))
            win = int(np.where(keep, full, -np.inf).argmax())
            clear = len(kept) == 1 or sc[-1] - sc[-2] >= 0.05
            # keys that make each kept column win clearly ...
            if clear and win not in found and len(found) < min(len(kept), 3):
                found[win] = key
            # ... and keys under which a trap column would win clearly if the kernel kept it: a kernel that
            # keeps the columns just below the threshold picks that column, not the twin's
            ws = np.sort(np.where(wide, full, -np.inf))
            wwin = int(np.where(wide, full, -np.inf).argmax())
            if trap and clear and wwin in trap and ws[-1] - ws[-2] >= 0.05 and wwin not in traps and len(traps) < 2:
                traps[wwin] = (key, win)
            if len(found) == min(len(kept), 3) and len(traps) == min(len(trap), 2):
                break
        assert len(found) == min(len(kept), 3) and len(traps) == min(len(trap), 2), (ci, found, traps)
        for win, key in found.items():
            rows.append(row), its.append(it), lmps.append(lm), keys.append(key), wants.append(win)
        for _col, (key, win) in traps.items():
            rows.append(row), its.append(it), lmps.append(lm), keys.append(key), wants.append(win)
            trapped += 1
    assert trapped >= 5
    lg = torch.from_numpy(np.stack(rows)).to(torch.bfloat16)
    R = len(rows)
    got = _launch(lg, V, np.array(its, dtype=np.float32), np.stack(keys), np.zeros(R, dtype=np.int32),
                  np.ones(R, dtype=np.float32), np.array(lmps, dtype=np.float32))
    assert got.tolist() == wants
    assert len(set(wants) & set(thr_cols[1:4].tolist())) >= 1         # a column exactly on the threshold was drawn


# --------------------------------------------------------------------------- the heads over exact logits
@pytest.mark.gpu
def test_heads_over_exact_logits_equal_the_reference_ops():
    """x and w over {-1, 0, 1}: the logits are integers, exact in fp32 and in
    bf16, so the store-epilogue GEMM's tensor is the reference's, both edits
    are the twins' bit for bit and the picks must agree row for row."""
    from llm_message_queue_amd.ops.llama_ops import HipOps, RefOps
    from tests.test_gpu_penalties import MIXES
    from tests.test_gpu_truncated_sampling import _params
    M, N, K = 37, 1024, 256
    c = GC.int_case(M, N, K, 11)
    rng = np.random.default_rng(4)
    keys = S.row_keys(np.arange(M, dtype=np.uint64) + np.uint64(31), np.arange(M) % 5)
    it, tk, tp = _params(M)
    it[np.arange(M) % 3 == 0] = 0.0                                   # greedy rows among the sampling ones
    lmp = S.min_p_log(np.array([0.0, 0.001, 0.05, 0.5, 1.0])[np.arange(M) % 5])
    hist = rng.integers(0, N, (M + 2, 64)).astype(np.int32)
    spans = np.stack([(np.arange(M) * 5 + 1) % (M + 2), np.arange(M) % 7, np.arange(M) % 7 + np.arange(M) % 11,
                      np.arange(M) % 7 + 11 + np.arange(M) % 40], axis=1).astype(np.int32)
    params = np.array([MIXES[r % len(MIXES)] for r in range(M)], dtype=np.float32)
    nopen = np.arange(M) % 4 == 1                                     # rows with an edit but no penalty ...
    spans[nopen, 0] = -1
    ids, vals, espans = [], [], []
    off = 0
    for r in range(M):
        na, nb = (0, 1, 5, 64)[r % 4], (3, 0, 64, 1)[(r // 2) % 4]
        if r < 4:
            na, nb = 3, 2                                             # (penalty + allow + bias + min_p together)
        al = rng.integers(0, N, na).astype(np.int32)
        bi = np.concatenate([al[:nb // 2], rng.integers(-2, N + 2, nb - min(nb // 2, na))]).astype(np.int32)[:nb]
        bv = rng.choice(np.array([100.0, -100.0, 2.5, -0.75, 6.0], dtype=np.float32), len(bi))
        ids += [al, bi]
        vals += [np.zeros(na, dtype=np.float32), bv]
        espans.append((off, na, off + na, len(bi)))
        off += na + len(bi)
    ids, vals, espans = np.concatenate(ids), np.concatenate(vals), np.array(espans, dtype=np.int32)
    assert ((~nopen) & (espans[:, 1] > 0) & (espans[:, 3] > 0) & (lmp > -np.inf) & (it > 0)).any()
    x, w = c.x.to(DEV), c.w.to(DEV)
    kd = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32))
    rowwise = [torch.from_numpy(it), kd, torch.from_numpy(tk), torch.from_numpy(tp)]
    tail = [torch.from_numpy(spans), torch.from_numpy(params)]
    hd = torch.from_numpy(hist)
    edit = tuple(torch.from_numpy(a) for a in (ids, vals, espans))
    lm = torch.from_numpy(lmp)

    def hip(h, ed=edit, m=lm, **kw):
        return HipOps().penalised_head(x, w, *[a.to(DEV) for a in rowwise], None if h is None else h.to(DEV),
                                       *[a.to(DEV) for a in tail], edit=None if ed is None else tuple(a.to(DEV) for a in ed),
                                       log_min_p=None if m is None else m.to(DEV), **kw).cpu().numpy()
    got = hip(hd)
    want = RefOps().penalised_head(c.x, c.w, *rowwise, hd, *tail, edit=edit, log_min_p=lm).numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    for r in np.flatnonzero(espans[:, 1] > 0):                        # an allow list bounds the row's pick
        a = ids[espans[r, 0]:espans[r, 0] + espans[r, 1]]
        assert got[r] in a.tolist(), r
    # the same call without the new inputs: what it was (the old signature still works), and the edit is no no-op
    old = HipOps().penalised_head(x, w, *[a.to(DEV) for a in rowwise], hd.to(DEV), *[a.to(DEV) for a in tail]).cpu().numpy()
    assert np.array_equal(old, RefOps().penalised_head(c.x, c.w, *rowwise, hd, *tail).numpy())
    assert (old != got).sum() > M // 2
    # a row with a bias but no penalty: the history it might have read holds garbage, and it does not matter
    garbage = torch.from_numpy(rng.integers(0, N, hist.shape).astype(np.int32))
    assert np.array_equal(hip(garbage)[nopen], got[nopen])
    sp2 = spans.copy()
    sp2[:, 0] = -1
    tail[0] = torch.from_numpy(sp2)
    none = hip(None)                                                  # no history at all: every penalty off
    assert np.array_equal(none, hip(garbage)) and np.array_equal(none[nopen], got[nopen])
    assert np.array_equal(none, RefOps().penalised_head(c.x, c.w, *rowwise, None, *tail, edit=edit, log_min_p=lm).numpy())
    # truncated_head with min_p
    hot = np.flatnonzero(it > 0)
    h = torch.from_numpy(hot)
    args = [torch.from_numpy(it[hot]), kd[h], torch.from_numpy(tk[hot]), torch.from_numpy(tp[hot])]
    tgot = HipOps().truncated_head(x[h.to(DEV)], w, *[a.to(DEV) for a in args], log_min_p=lm[h].to(DEV)).cpu().numpy()
    twant = RefOps().truncated_head(c.x[h], c.w, *args, log_min_p=lm[h]).numpy()
    assert np.array_equal(tgot, twant), np.flatnonzero(tgot != twant)
    plain = HipOps().truncated_head(x[h.to(DEV)], w, *[a.to(DEV) for a in args]).cpu().numpy()
    assert np.array_equal(plain, RefOps().truncated_head(c.x[h], c.w, *args).numpy())
    assert (plain != tgot).any()
    one = lmp[hot] == 0.0                                             # min_p = 1: the row's maximum
    assert one.any() and np.array_equal(tgot[one], c.ref.numpy()[hot][one].argmax(axis=1))


# --------------------------------------------------------------------------- tiny model end to end
ALLOW = np.array([900, 7, 313, 5000, 64], dtype=np.int32)            # (5000 is outside the vocabulary of 1,024)
I32, F32 = (lambda v: np.asarray(v, dtype=np.int32)), (lambda v: np.asarray(v, dtype=np.float32))


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
    """Wraps ``ops.gemm.logit_edit``, ``penalised_argmax`` and
    ``sample_truncated``: the edit's output is the twin's over its captured
    input, and every pick over edited logits is the twin's pick over them."""

    def __init__(self, monkeypatch):
        self.calls = self.picks = self.draws = 0
        self.edit, self.argmax, self.sample = G.logit_edit, G.penalised_argmax, G.sample_truncated
        self.edited = None
        monkeypatch.setattr(G, "logit_edit", self.logit_edit)
        monkeypatch.setattr(G, "penalised_argmax", self.penalised_argmax)
        monkeypatch.setattr(G, "sample_truncated", self.sample_truncated)

    def logit_edit(self, logits, ids, vals, spans, vocab=None):
        R = logits.shape[0]
        before = _bits(logits).copy()
        out = self.edit(logits, ids, vals, spans, vocab=vocab)
        torch.cuda.synchronize()
        after = _bits(logits)
        assert np.array_equal(after, S.logit_edit_reference(before, int(vocab), ids.cpu().numpy(), vals.cpu().numpy(),
                                                            spans[:R].cpu().numpy()))
        assert (after != before).any()
        self.edited = logits.data_ptr()
        self.calls += 1
        return out

    def penalised_argmax(self, logits, vocab=None, **kw):
        out = self.argmax(logits, vocab=vocab, **kw)
        assert np.array_equal(out.cpu().numpy(), S.penalised_pick_reference(_bits(logits), int(vocab)))
        self.picks += logits.shape[0]
        return out

    def sample_truncated(self, logits, inv_temp, keys, top_k, top_p, vocab=None, out=None, log_min_p=None):
        got = self.sample(logits, inv_temp, keys, top_k, top_p, vocab=vocab, out=out, log_min_p=log_min_p)
        R, V = logits.shape[0], int(vocab)
        rows = S.bf16_values(_bits(logits)[:, :V]).astype(np.float64)
        it, tk, tp = (a[:R].cpu().numpy() for a in (inv_temp, top_k, top_p))
        kk = keys[:R].cpu().contiguous().view(torch.int32).numpy().view(np.uint32)
        lm = None if log_min_p is None else log_min_p[:R].cpu().numpy()
        for r, g in enumerate(got.cpu().numpy().tolist()):
            keep = S.truncation_keep(rows[r], it[r], tk[r], tp[r], log_min_p=None if lm is None else lm[r])
            _check_pick(r, g, rows[r], it[r], kk[r], keep)
            self.draws += 1
        return got


def _edited():
    return [_req(100, allowed=ALLOW.copy()),
            _req(101, allowed=ALLOW.copy(), temperature=0.9, seed=3),
            _req(102, logit_bias=(I32([17, 5000]), F32([100.0, 100.0]))),
            _req(103, logit_bias=(I32([17, 40]), F32([2.5, -1.0])), temperature=0.9, seed=4, min_p=0.05),
            _req(104, temperature=0.9, seed=5, min_p=0.3),
            _req(105, allowed=ALLOW.copy(), logit_bias=(I32([7, 8]), F32([3.0, 100.0])), presence_penalty=1.0,
                 repetition_penalty=1.3, temperature=1.1, seed=6, min_p=0.01)]


@pytest.mark.gpu
def test_edited_requests_through_the_hip_engine(monkeypatch):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=64, max_ctx=64, token_budget=512, device=DEV, impl="hip")
    spy = _Spy(monkeypatch)

    def crowd():
        return [_req(i) for i in range(30)] + [_req(30 + i, temperature=0.9, seed=i) for i in range(10)]
    without = _drain(eng, crowd())
    assert eng.edited_steps == 0 and eng.penalised_steps == 0 and eng.h_eids is None and spy.calls == 0
    alone = {}
    for r in _edited():
        alone.update(_drain(eng, [r]))
    n = eng.edited_steps
    assert n == 6 * 5 and spy.calls == n and eng.d_hist is not None   # (request 104 has min_p only: no edit)
    again = _drain(eng, crowd())
    assert eng.edited_steps == n
    among = _drain(eng, crowd() + _edited())
    assert eng.edited_steps == n + 6
    torch.cuda.synchronize()
    inside = set(ALLOW[ALLOW < 1024].tolist())
    for rid in (100, 101, 105):
        assert set(alone[rid].out_tokens.tolist()) <= inside, (rid, alone[rid].out_tokens)
    assert alone[102].out_tokens.tolist() == [17] * 6                 # the +100 bias, greedy
    print({rid: alone[rid].out_tokens.tolist() for rid in sorted(alone)})
    for rid in range(100, 106):
        assert len(alone[rid].out_tokens) == 6 and np.array_equal(alone[rid].out_tokens, among[rid].out_tokens), rid
    for i in range(40):
        assert np.array_equal(among[i].out_tokens, without[i].out_tokens), i
        assert np.array_equal(again[i].out_tokens, without[i].out_tokens), i
    assert spy.picks > 0 and spy.draws > 0
    eng.close()
