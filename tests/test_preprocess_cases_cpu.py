"""The constructions of preprocess_cases.py do what they claim, and every
comparison the GPU tests use rejects single injected faults.  CPU only."""
import numpy as np
import pytest

import preprocess_cases as PC

f32 = np.float32


# ----------------------------------------------------------------------------- GELU
def test_gelu_is_relu_on_the_exact_cases_pre_activations():
    """fp32 tanh-GELU == max(z, 0) bit for bit at z = 0 and every integer
    |z| >= 6 (so at every multiple of 8), also with the exponential 1 % off."""
    z = np.concatenate([[0.0], np.arange(6, 4000), -np.arange(6, 4000), [262144.0, -262144.0, 2.0 ** 23]]).astype(f32)
    for rel in (0.0, 0.01, -0.01):
        g = PC.gelu_f32(z, exp_rel=rel)
        assert np.array_equal(g, np.maximum(z, f32(0))), rel
    assert not np.array_equal(PC.gelu_f32(f32([3.0])), f32([3.0]))


def test_gelu_fp32_emulation_stays_inside_its_share_of_the_bound():
    z = np.random.default_rng(0).uniform(-7, 7, 100_000).astype(f32)
    err = np.abs(PC.gelu_f32(z).astype(np.float64) - PC.gelu64(z))
    assert (err <= PC.GELU_F32_ULP24 * np.abs(z.astype(np.float64)) * PC.U).all()
    # the slope bound used for the general case
    x = np.linspace(-8, 8, 200_001)
    slope = np.abs(np.diff(PC.gelu64(x)) / np.diff(x)).max()
    assert 1.12 < slope <= PC.GELU_LIPSCHITZ


def test_gelu_probe_construction_and_check():
    c = PC.gelu_probe_case()
    z = c.z.astype(np.float64)
    assert c.z.shape == (63, 256) and np.isfinite(c.z).all()
    assert ((np.abs(z) <= 12.1).sum() > 4000) and (np.abs(z) > 1e29).any() and (z > 0).any() and (z < 0).any()
    assert np.isnan(c.E[0].float().numpy()).all() and ((c.hashes[:, 0] & (c.V - 1)) != 0).all()
    assert ((c.E[1:].float().numpy() != 0).sum(1) <= 1).all()         # (e = 0 once: z = b1 alone)
    good = PC.gelu_f32(c.z)
    ok, worst = PC.gelu_check(good, c.z)
    assert ok and worst <= PC.GELU_F32_ULP24
    # an exponential with the allowed error passes, the issue's fault does not
    assert PC.gelu_check(PC.gelu_f32(c.z, exp_rel=PC.EXPF_ULP24 * PC.U), c.z)[0]
    bad = (good.astype(np.float64) + 1e-5 * np.abs(z)).astype(f32)
    assert not PC.gelu_check(bad, c.z)[0]
    nan = good.copy()
    nan[5, 5] = np.nan
    assert not PC.gelu_check(nan, c.z)[0]
    assert PC.expf_ulp24_needed(good, c.z) <= 0.0 < PC.expf_ulp24_needed(PC.gelu_f32(c.z, exp_rel=4 * PC.U), c.z)


# ----------------------------------------------------------------------------- embed_pool
def _parts(ntok):
    """Tile parts per message."""
    off = np.concatenate([[0], np.cumsum(ntok)])
    return [0 if n == 0 else (off[m + 1] - 1) // PC.TM - off[m] // PC.TM + 1 for m, n in enumerate(ntok)]


def test_token_patterns_reach_every_layout():
    P = {n: PC.token_pattern(n, 160) for n in ("inside", "edge63", "straddle", "parts66", "parts128", "parts150",
                                               "tail1", "tail63", "zeros_edges", "zeros_run")}
    off = {n: np.concatenate([[0], np.cumsum(p)]) for n, p in P.items()}
    assert max(_parts(P["inside"])) == 1
    assert off["edge63"][2] == 64 and off["edge63"][3] == 128                 # ends on row 63 / starts on row 64
    assert 2 in _parts(P["straddle"]) and 2 in _parts(P["edge63"])
    for name, n, parts in (("parts66", 66, 3), ("parts128", 128, 3), ("parts150", 150, 4)):
        assert off[name][1] == 63 and P[name][1] == n and _parts(P[name])[1] == parts
    assert P["parts150"].sum() % 64 == 1 and P["tail1"].sum() % 64 == 1 and P["tail63"].sum() % 64 == 63
    z = P["zeros_edges"]
    assert z[0] == 0 and z[-1] == 0
    zr = P["zeros_run"]
    assert (zr[1:71] == 0).all() and off["zeros_run"][72] > 64 > off["zeros_run"][71]   # > 64 messages in tile 0
    ones = PC.one_token_counts()
    assert len(ones) == 5000 and 64 ** 2 < len(ones) and (ones[100:230] == 0).all() and ones[-1] == 0 and ones[0] == 0
    assert sorted({c[1] for c in PC.EMBED_CASES}) == [64, 1024] and sorted({c[2] for c in PC.EMBED_CASES}) == [256, 512, 1024]
    assert sorted({c[3] for c in PC.EMBED_CASES}) == [64, 160]
    assert {1, 3, 255, 256, 257, 513} <= {PC.embed_case(*c).B for c in PC.EMBED_CASES if c[0].startswith("rand")}


@pytest.mark.parametrize("name,V,H,L", [c for c in PC.EMBED_CASES if c[0] in ("straddle", "parts66", "parts150", "zeros_run")])
def test_embed_exact_case_construction(name, V, H, L):
    c = PC.embed_case(name, V, H, L)
    used = np.concatenate([c.hashes[m, :n] for m, n in enumerate(c.ntok)]) & (V - 1)
    assert (used != 0).all() and (used != c.poison).all() and (used >= V // 2).any()
    past = np.concatenate([c.hashes[m, n:] for m, n in enumerate(c.ntok)]) & (V - 1)
    assert (past == c.poison).all()
    assert np.isnan(c.E64[0]).all() and (c.E64[c.poison] == 1024).all()
    assert set(np.unique(c.E64[1:c.poison])) <= {-8.0, 0.0, 8.0} and set(np.unique(c.W64)) == {-1.0, 0.0, 1.0}
    assert (c.b64 % 8 == 0).all() and (c.b64 != 0).any()
    ref = PC.embed_exact_ref(c)                           # asserts multiples of 8 and exact sums itself
    assert PC.embed_exact_check(ref.main, ref) == 0
    assert (ref.main[c.ntok == 0] == 0).all() and (ref.main[c.ntok > 0] != 0).any(1).all()
    for m, alts in ref.alts.items():
        assert _parts(c.ntok)[m] >= 3 and c.ntok[m] & (c.ntok[m] - 1)
        for a in alts:                                    # every order of the parts is accepted, nothing else
            got = ref.main.copy()
            got[m] = a
            assert PC.embed_exact_check(got, ref) == 0
        got = ref.main.copy()
        got[m] = np.nextafter(alts.max(0), f32(np.inf))
        assert PC.embed_exact_check(got, ref) > 0
    if name in ("parts66", "parts150"):
        assert ref.alts
    one_ulp = ref.main.copy()
    m = int(np.flatnonzero(c.ntok > 0)[0])
    j = int(np.flatnonzero(one_ulp[m])[0])
    one_ulp[m, j] = np.nextafter(one_ulp[m, j], f32(np.inf))
    assert PC.embed_exact_check(one_ulp, ref) == 1


EMBED_FAULTS = ("boundary_row", "tile_rows_mean", "drop_part", "store_second", "swap_w1t_cols", "drop_k_chunk",
                "no_bias", "half_mask", "token_off_by_one")


@pytest.mark.parametrize("fault", EMBED_FAULTS)
def test_embed_exact_check_rejects(fault):
    c = PC.embed_case("straddle", 64, 1024, 64)
    ref = PC.embed_exact_ref(c)
    bad = PC.embed_exact_ref(c, fault)
    assert PC.embed_exact_check(bad.main, ref) > 0, fault


@pytest.fixture(scope="module")
def general_case():
    import torch
    g = torch.Generator().manual_seed(1234)
    V, H = 4096, 256
    E = (torch.randn(V, PC.D, generator=g) * 0.5).to(torch.bfloat16)
    W = (torch.randn(H, PC.D, generator=g) / PC.D ** 0.5).to(torch.bfloat16)
    b = (torch.randn(H, generator=g) * 0.02).float()
    c = PC.with_weights(PC.embed_random_case("straddle", 64, vocab=V, hidden=H), E, W, b)
    return c, PC.embed_general_ref(c)


def test_embed_general_bound_is_tight_and_holds_for_fp32(general_case):
    c, (ref, bound) = general_case
    assert np.isfinite(bound).all() and (bound[c.ntok > 0] > 0).all() and (bound[c.ntok == 0] == 0).all()
    assert bound.max() < 5e-4                             # the old tolerance was 2e-2
    # a plain fp32 evaluation of the same operation stays inside it
    own, X, W, b = PC._embed_rows(c)
    hid = PC.gelu_f32((X.astype(f32) @ W.T.astype(f32) + b.astype(f32)))
    got = np.zeros((c.B, c.H), dtype=f32)
    np.add.at(got, own, hid)
    got = got * (f32(1) / np.maximum(c.ntok, 1).astype(f32))[:, None]
    ok, worst = PC.embed_general_check(got, ref, bound)
    assert ok and worst < 1.0


# (the faults of the tiling -- a part dropped, stored, averaged over its rows -- are shown on the exact case)
@pytest.mark.parametrize("fault", [f for f in EMBED_FAULTS if f not in ("drop_part", "store_second", "tile_rows_mean")])
def test_embed_general_check_rejects(general_case, fault):
    c, (ref, bound) = general_case
    bad, _ = PC.embed_general_ref(c, fault)
    assert not PC.embed_general_check(bad.astype(f32), ref, bound)[0]


# ----------------------------------------------------------------------------- classify_head
@pytest.mark.parametrize("B", PC.HEAD_B)
def test_head_exact_case_plants_ties(B):
    c = PC.head_case(B, 256)
    logits, pred = PC.head_exact_ref(c)
    assert np.array_equal(logits.astype(np.float64), np.round(logits)) and PC.head_check(logits, pred, (logits, pred))
    assert c.planted[0] == PC.HEAD_PLANTS[0] and pred[0] == 1
    if B >= 5:
        want = {0: 1, 1: 1, 2: 2, 3: 3, 4: 1}
        for row, p in want.items():
            assert pred[row] == p and pred[B - 1 - row] == p if B >= 10 else pred[row] == p
        assert logits[3, 4:].max() > logits[3, :4].max()
    assert set(np.unique(c.W2)) <= set(range(-3, 4)) and (c.b2 != 0).any()


@pytest.mark.parametrize("fault", ["swap_w2_cols", "tie_high", "shift_in_wave"])
@pytest.mark.parametrize("B", [5, 1027])
def test_head_check_rejects(fault, B):
    c = PC.head_case(B, 1024)
    ref = PC.head_exact_ref(c)
    bad = PC.head_exact_ref(c, fault)
    assert not PC.head_check(bad[0], bad[1], ref), fault
    if fault == "tie_high":                               # the logits are right: only pred shows it
        assert PC.same_bits(bad[0], ref[0]) and all(bad[1][r] != ref[1][r] for r, t in c.planted.items() if t[3] >= max(t[:3]))


@pytest.mark.parametrize("B,H", [(1041, 1024), (1024, 256)])
def test_head_general_case_leaves_under_one_percent_undecided(B, H):
    c = PC.head_general_case(B, H)
    assert (~c.decided).mean() < 0.01
    assert c.bound.max() < 1e-3 and (c.bound > 0).all()
    got = (c.x @ c.W2 + c.b2).astype(f32)                 # an fp32 product stays inside the bound
    assert (np.abs(got.astype(np.float64) - c.ref) <= c.bound).all()
    assert np.array_equal((1 + np.argmax(got[:, :4], axis=1))[c.decided], c.pred[c.decided])


# ----------------------------------------------------------------------------- scan_rows
@pytest.mark.parametrize("B", PC.SCAN_B)
def test_scan_counts(B):
    n = PC.scan_counts(B)
    assert len(n) == B and (B < 3 or ((n == 0).any() and n.max() == 1 << 29))


# ----------------------------------------------------------------------------- summarise_project
@pytest.mark.parametrize("C", PC.SUMMARISE_C)
def test_summarise_exact_case_construction(C):
    c = PC.summarise_case(C, 0.75)
    assert c.rows.shape == (c.M, PC.SM_H) and np.array_equal(c.rows, np.round(c.rows))
    if C >= 15:
        assert {1, 2, 16, 17, 40, 0} <= set(c.counts.tolist()) and 0 < c.first.sum() < C
    if C > 32:
        assert (c.counts[16:32] == 0).all() and c.counts[:16].any() and c.counts[32:].any()
    ref, bound = PC.summarise_ref(c)
    assert (bound == 0).all() and np.array_equal(ref, np.round(ref * 4) / 4) and np.abs(ref).max() < 2 ** 20
    # the fp32 mean the kernel forms rounds to the same bf16 vector
    for i in range(C):
        lo, hi = c.seg[i], c.seg[i + 1]
        if hi > lo:
            s = c.rows[lo:hi].sum(0, dtype=f32) * (f32(1) / f32(hi - lo))
            assert np.array_equal(PC.bf16(s).float().numpy(), c.rows[lo:hi].astype(np.float64).mean(0).astype(f32))
    assert PC.summarise_check(ref.astype(f32), ref, bound, True)[0]


SUMMARISE_FAULTS = ("swap_rows", "drop_k_quarter", "swap_alpha", "ignore_first", "empty_mean_stale")


@pytest.mark.parametrize("fault", SUMMARISE_FAULTS)
def test_summarise_checks_reject(fault):
    c = PC.summarise_case(17, 0.75)
    ref, bound = PC.summarise_ref(c)
    bad, _ = PC.summarise_ref(c, fault)
    assert not PC.summarise_check(bad.astype(f32), ref, bound, True)[0], fault
    r = PC.summarise_random_case(17, 0.6)
    ref, bound = PC.summarise_ref(r)
    bad, _ = PC.summarise_ref(r, fault)
    assert not PC.summarise_check(bad.astype(f32), ref, bound, False)[0], fault


def test_summarise_general_bound_is_tight_and_holds_for_fp32():
    r = PC.summarise_random_case(33, 0.6)
    ref, bound = PC.summarise_ref(r)
    assert 0 < bound[r.counts > 0].max() < 3e-3           # the old tolerance was 3e-2
    a = f32(0.6)
    got = np.zeros((r.C, PC.SM_DS), dtype=f32)
    for i in range(r.C):
        lo, hi = r.seg[i], r.seg[i + 1]
        mean = r.rows[lo:hi].sum(0, dtype=f32) * (f32(1) / f32(hi - lo)) if hi > lo else np.zeros(PC.SM_H, dtype=f32)
        proj = PC.bf16(mean).float().numpy() @ r.Pt.float().numpy().T
        got[i] = proj if r.first[i] else a * r.state[i] + (f32(1) - a) * proj
    ok, worst = PC.summarise_check(got, ref, bound, False)
    assert ok, worst


# ----------------------------------------------------------------------------- salient_topk
def test_salient_cases_reach_every_path():
    c = PC.salient_case("paths")
    n = np.diff(c.seg)
    assert list(n[:4]) == [300, 256, 0, 257] and all((c.ntok[c.seg[i]:c.seg[i + 1]] == 0).any() for i in (0, 1, 3))
    toks = np.concatenate([c.hashes[m, :k] for m, k in enumerate(c.ntok)])
    assert (toks == 0).any() and (toks == 1).any() and (toks == 3).any()
    oh, oc, ov = PC.salient_ref(c.hashes, c.ntok, c.seg, c.stop, c.K)
    assert not ov.any() and (oh != 0).all(1)[[0, 1, 3]].all() and not (oh == 3).any() and (oc[2] == 0).all()
    assert list(oh[4][:2]) == [1, 7] and list(oc[4]) == [3, 1, 0, 0, 0]          # 0, 1, 0 fold into three of 1
    s16 = PC.salient_case("paths_stride16")
    assert s16.stride == 16 and s16.tab.shape[1] == 16 and np.array_equal(s16.ntok, c.ntok) and (s16.tab[:, 0] == -99).all()
    k64 = PC.salient_case("paths_k64")
    oc64 = PC.salient_ref(k64.hashes, k64.ntok, k64.seg, k64.stop, 64)[1]
    assert (oc64[0] > 0).sum() == 37 and (oc64[0][37:] == 0).all()
    assert PC.salient_case("paths_k1").K == 1
    assert len(PC.salient_case("stop128").stop) == PC.SAL_MAX_STOP and len(PC.salient_case("stop129").stop) == 129
    for name, flag in (("distinct2048", 0), ("distinct2049", 1)):
        d = PC.salient_case(name)
        t = np.concatenate([d.hashes[m, :k] for m, k in enumerate(d.ntok[:d.seg[1]])])
        assert len(set(t.tolist()) - {3, 4}) == int(name[8:])
        rh, rc, rv = PC.salient_ref(d.hashes, d.ntok, d.seg, d.stop, d.K)
        assert list(rv) == [flag, 0] and (flag or list(rc[0]) == [3, 3, 3, 2, 2])
    p = PC.salient_case("probe_chain")
    keys = PC.colliding_keys(2040, 40)
    assert all((k * PC.SAL_MULT) % 2 ** 32 % PC.SAL_TABLE == 2040 for k in keys) and 2040 + 40 > PC.SAL_TABLE


@pytest.mark.parametrize("fault,case", [("tie_by_hash", "paths"), ("count_stop", "paths_k64"), ("segment_off_by_one", "paths"),
                                        ("no_fold", "paths"), ("count_stop", "stop129"), ("tie_by_hash", "probe_chain")])
def test_salient_check_rejects(fault, case):
    c = PC.salient_case(case)
    ref = PC.salient_ref(c.hashes, c.ntok, c.seg, c.stop, c.K)
    assert PC.salient_check(ref, ref)
    assert not PC.salient_check(PC.salient_ref(c.hashes, c.ntok, c.seg, c.stop, c.K, fault), ref), fault
    flag = (ref[0], ref[1], 1 - ref[2])
    assert not PC.salient_check(flag, ref)
