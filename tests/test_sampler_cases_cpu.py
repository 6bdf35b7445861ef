"""Construction checks for sampler_cases.py: every case is what it claims on
the float64 twin, every witness key decides its draw clearly over the WHOLE
row, the two mutant kept sets (one group more, one group fewer) flip the pick
of every trap and edge witness -- so the GPU test would fail on a select that
is off by one group -- and the key helper agrees with a brute-force sort of
all 65,536 bf16 patterns.  No GPU."""
import numpy as np
import pytest

import sampler_cases as SC
from llm_message_queue_amd.ops import sampling as S

VOCABS = (1003, 16384, 18437)
V_SERVE = 128256


def _scores(c, key):
    sc = c.row64 * float(c.inv_temp) + S.gumbel(np.asarray(key).reshape(1, 2), np.arange(c.V, dtype=np.uint32))[0]
    return np.where(np.isfinite(c.row64), sc, -np.inf)


def _pick(sc, keep):
    """(the winner among ``keep``, its gap to the runner-up)."""
    m = np.where(keep, sc, -np.inf)
    win = int(m.argmax())
    rest = np.delete(m, win)
    return win, (np.inf if not np.isfinite(rest.max(initial=-np.inf)) else m[win] - rest.max())


# ----------------------------------------------------------------------------- the key helper
def test_key_helper_against_a_sort_of_every_bf16_pattern():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    val = SC.values64(bits)
    key = SC.st_key(bits)
    fin = np.isfinite(val)
    assert (key[~fin] == -1).all() and (key[fin] >= 0).all() and (~fin).sum() == 256
    order = np.argsort(val[fin], kind="stable")
    v, k = val[fin][order], key[fin][order]
    # order-preserving on finite values; equal values (+0, -0) share a key
    assert np.array_equal(np.diff(v) > 0, np.diff(k) > 0) and (np.diff(k) >= 0).all()
    assert (np.diff(v) == 0).sum() == 1 and key[0x0000] == key[0x8000] == SC.KEY_ZERO == 32768
    assert len(np.unique(k)) == 65536 - 256 - 1 and 0x7FFF not in k
    assert k.max() == key[SC.TOP_FINITE] == SC.KEY_TOP == 65407 and k.min() == key[SC.LOW_FINITE] == SC.KEY_BOTTOM == 128
    # key_bits inverts it (-0 comes back as +0)
    for kk in np.unique(k):
        assert int(SC.st_key(SC.key_bits(kk))) == kk
    assert SC.key_bits(SC.KEY_ZERO) == 0x0000


def test_worked_offsets_below_3_984375():
    m = SC.bits_of(3.984375)
    assert m == SC.M_BITS
    for value, off in ((2.0, 127), (1.9921875, 128), (-0.99609375, 32767), (-1.0, 32768), (3.0, 63)):
        assert SC.offset_of(m, SC.bits_of(value)) == off, value
        assert SC.bits_at(m, off) == SC.bits_of(value)
    assert 32767 // SC.ST_WIN == 0 and 32768 // SC.ST_WIN == 1 and 127 // SC.ST_CHUNK == 0 and 128 // SC.ST_CHUNK == 1


# ----------------------------------------------------------------------------- the cases
def _check_case(c):
    # the kept set: the planted groups down to the claimed one, stable under DELTA for a top-p case
    keep = S.truncation_keep(c.row64, c.inv_temp, c.top_k, c.top_p)
    assert np.array_equal(keep, c.keep)
    if c.top_p < 1:
        for f in (1.0 - SC.DELTA, 1.0 + SC.DELTA):
            assert np.array_equal(S.truncation_keep(c.row64, c.inv_temp, c.top_k, np.float32(c.top_p) * np.float32(f)), keep)
    key = SC.st_key(c.bits)
    assert key.max() == c.kmax
    if len(c.edge_cols):
        assert (c.kmax - key[c.edge_cols] == c.edge_off).all() and c.row64[keep].min() == c.row64[c.edge_cols[0]]
        assert keep[c.edge_cols].all()
    if len(c.trap_cols):
        assert (c.kmax - key[c.trap_cols] == c.trap_off).all() and not keep[c.trap_cols].any()
        # the trap is the next group: no candidate lies strictly between it and the lowest kept value
        between = np.isfinite(c.row64) & (c.row64 < c.row64[keep].min()) & (c.row64 > c.row64[c.trap_cols[0]])
        assert not between.any()
        assert np.array_equal(np.flatnonzero(c.more & ~keep), np.sort(c.trap_cols))
    assert (c.more | keep).sum() == c.more.sum() and (c.fewer & keep).sum() == c.fewer.sum()
    # every key decides its draw clearly over the whole row (the search looked at the live columns only)
    for k, want, kind, trap_win in zip(c.keys, c.wants, c.kinds, c.trap_wins):
        sc = _scores(c, k)
        win, gap = _pick(sc, keep)
        assert win == want and gap >= SC.CLEAR, (c.name, kind, win, want, gap)
        if kind == "edge":
            assert want in c.edge_cols
            if c.fewer.sum() < keep.sum():                            # (the first group cannot be dropped)
                assert _pick(sc, c.fewer)[0] != want
        elif kind == "trap":
            mwin, mgap = _pick(sc, c.more)
            assert mwin == trap_win and trap_win in c.trap_cols and mwin != want and mgap >= SC.CLEAR
        else:
            assert want not in c.edge_cols and keep[want]
    # no column outside the live ones can come within CLEAR of the maximum's score under any key
    dead = np.isfinite(c.row64)
    dead[c.live] = False
    if dead.any():
        assert (c.row64.max(initial=-np.inf, where=np.isfinite(c.row64)) - c.row64[dead].max()) * float(c.inv_temp) > SC.REACH


def _check_claims(cs):
    by = {c.name: c for c in cs}
    for cls, e, t in SC.CUTS:
        for mode in ("top_k", "top_p"):
            c = by.get(f"{cls}/{mode}")
            if c is None:
                continue
            assert (c.edge_off, c.trap_off) == (e, t)
            assert (c.top_k > 0) == (mode == "top_k") and (c.top_p < 1) == (mode == "top_p")
    if "chunk_127/top_k" in by:
        assert by["chunk_127/top_k"].edge_off % 128 == 127 and by["chunk_128/top_p"].edge_off % 128 == 0
        assert by["mid_chunk_511/top_k"].edge_off // 128 == 3 and by["mid_chunk_512/top_k"].edge_off // 128 == 4
        assert by["wave_8191/top_k"].edge_off // 128 == 63 and by["wave_8191/top_k"].trap_off // 128 == 64
        # ties: the count before the boundary group against top_k
        t = by["tie/before=k-1"]
        before = int((t.row64 > t.row64[t.edge_cols[0]]).sum())
        assert before == t.top_k - 1 == 4 and len(t.edge_cols) == 3
        t = by["tie/straddle"]
        assert before < t.top_k < before + len(t.edge_cols)
        t = by["tie/before=k"]
        assert int((t.row64 > t.row64[t.trap_cols[0]]).sum()) == t.top_k
        t = by["tie/k=1"]
        assert t.top_k == 1 and len(t.edge_cols) == 3 and t.keep.sum() == 3
        # the window loop
        c = by["all_kept/nan_inf"]
        fin = np.isfinite(c.row64)
        assert c.top_k > fin.sum() and np.array_equal(c.keep, fin) and c.edge_window == 1
        assert np.isnan(c.row64).any() and np.isposinf(c.row64).any() and np.isneginf(c.row64).any()
        for n in ("negative/top_k", "negative/top_p", "negative/both"):
            assert by[n].kmax < SC.ST_WIN and by[n].row64[np.isfinite(by[n].row64)].max() < 0
        assert by["negative/both"].top_k > 0 and by["negative/both"].top_p < 1
        c = by["top_p/second_window"]
        assert c.top_k == 0 and c.edge_window == 1 and c.trap_window == 1
        c = by["top_k_second/top_p_second"]
        assert c.edge_window == 1 and S.truncation_keep(c.row64, c.inv_temp, c.top_k, 1.0).sum() > c.keep.sum()
        c = by["top_p_near_1"]
        assert c.top_p < 1 and np.array_equal(S.truncation_keep(c.row64, c.inv_temp, c.top_k, 1.0), c.keep)
        assert by["top_p_tiny"].keep.sum() == 1
        assert by["extreme/top_k"].kmax == SC.KEY_TOP and by["extreme/top_k"].top_k == 2 ** 31 - 1
        fin_keys = SC.st_key(by["extreme/top_k"].bits)
        assert fin_keys[fin_keys >= 0].min() == SC.KEY_BOTTOM and by["extreme/top_k"].keep.all()
        c = by["inv_temp_20"]
        assert c.inv_temp == 20 and np.float32(np.exp(np.float32((-2.0 - 4.0) * 20.0))) == 0 and abs(c.top_p - 0.999) < 1e-6
        with np.errstate(under="ignore"):
            lost = np.exp(((c.row64[np.isfinite(c.row64)] - 4.0) * 20.0).astype(np.float32)) == 0
        assert lost.sum() >= c.V - 8                                  # the lower groups' fp32 masses are 0
    c = by.get("top_k_second/top_p_first")
    if c is not None:
        # top-k's own cut lies in the second window, top-p's back in the first
        kk = S.truncation_keep(c.row64, c.inv_temp, c.top_k, 1.0)
        assert (c.kmax - SC.st_key(c.bits)[kk]).max() >= SC.ST_WIN and c.edge_window == 0 and c.trap_window == 0
    for n in ("zero/boundary/top_k", "zero/boundary/top_p", "zero/trap/top_k", "zero/trap/top_p"):
        c = by.get(n)
        if c is None:
            continue
        zeros = c.trap_cols if "trap" in n else c.edge_cols
        assert set(c.bits[zeros].tolist()) == {SC.ZERO_POS, SC.ZERO_NEG}       # the group mixes +0 and -0
        assert (c.bits == SC.SUB_POS).sum() == 2 and (c.bits == SC.SUB_NEG).sum() == 2
        kind = "trap" if "trap" in n else "edge"
        cols = [tw if kind == "trap" else w for w, tw, k in zip(c.wants, c.trap_wins, c.kinds) if k == kind]
        assert set(c.bits[cols].tolist()) == {SC.ZERO_POS, SC.ZERO_NEG}        # ... and both signs are witnessed
    for n in ("subnormal_max/top_k", "subnormal_max/top_p"):
        c = by.get(n)
        if c is not None:
            assert 0 < c.row64[np.isfinite(c.row64)].max() < 2.0 ** -126 and c.kmax == 0x8002


@pytest.mark.parametrize("V", VOCABS)
def test_cases_are_what_they_claim(V):
    cs = SC.cases(V)
    assert len(cs) >= 40
    for c in cs:
        _check_case(c)
    _check_claims(cs)
    bits, it, keys, tk, tp, wants, tags = SC.witness_rows(cs)
    SC.check_coverage(tags, V)
    assert S.sample_truncated_reference(SC.values64(bits), it, keys, tk, tp).tolist() == wants
    print(f"V={V}: {len(cs)} cases, {len(wants)} rows, at most {max(c.seeds_used for c in cs)} seeds a case, "
          f"search {SC.SEARCH_SECONDS[0]:.2f} s so far")
    for cls, (e, t, p) in sorted(SC.tally(tags).items()):
        print(f"  {cls}: {e} edge, {t} trap, {p} plain")


def test_serving_vocabulary_cases_are_what_they_claim():
    cs = SC.cases(V_SERVE, SC.SERVING_CLASSES)
    assert {c.cls for c in cs} == set(SC.SERVING_CLASSES)
    for c in cs:
        _check_case(c)
    _check_claims(cs)
    bits, it, keys, tk, tp, wants, tags = SC.witness_rows(cs)
    SC.check_coverage(tags, V_SERVE, SC.SERVING_CLASSES)
    assert S.sample_truncated_reference(SC.values64(bits), it, keys, tk, tp).tolist() == wants


def test_cases_do_not_depend_on_the_vocabulary():
    """The planted groups, parameters and claimed offsets are the same at every V."""
    a, b = SC.cases(VOCABS[0]), SC.cases(VOCABS[2])
    for x, y in zip(a, b):
        assert (x.name, x.top_k if x.cls != "all_kept" else 0, x.edge_off, x.trap_off, x.group_values) == \
               (y.name, y.top_k if y.cls != "all_kept" else 0, y.edge_off, y.trap_off, y.group_values)
