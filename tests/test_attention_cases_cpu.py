"""Construction checks of the attention probes (tests/attention_cases.py):
the fp64 reference really is what each probe claims, the inputs are exact in
bf16, and a correct segment kernel (emulated) stays inside the derived bound
on the very inputs the GPU test uses."""
import math

import numpy as np
import pytest
import torch

import attention_cases as AC


def _covered(case):
    return case.edge.covered.nonzero().flatten().tolist()


def _roundtrips(t):
    return torch.equal(t.float().to(torch.bfloat16).float(), t.float())


def test_edge_set_shape():
    e = AC.edge_set()
    t = e.tiles
    assert e.n_dec == len(AC.DEC_CTX) and (t[:e.n_dec, 1] == 1).all()
    assert sorted((t[:e.n_dec, 3] + 1).tolist()) == sorted(AC.DEC_CTX)
    got = {(int(p0), int(n)) for _, n, _, p0 in t[e.n_dec:]}
    assert set(AC.PREFILL) <= got and {(40, 16), (56, 16), (72, 1)} <= got      # the long segment, cut
    assert (t[:, 1] >= 1).all() and (t[:, 1] <= 16).all() and (t[:, 3] + t[:, 1]).max() == AC.MAX_CTX
    assert (~e.covered).sum() >= 3 and not e.covered[0] and not e.covered[-1]
    assert int(e.covered.sum()) == int(t[:, 1].sum())
    # adjacent tiles come from different slots; rows are neither in tile nor in slot order
    assert (t[1:, 2] != t[:-1, 2]).sum() >= len(t) - 4 and len(set(t[:, 2].tolist())) == AC.N_SLOTS
    assert (np.diff(t[:, 0]) < 0).any()
    s = e.slot[e.covered]
    assert (s[1:] < s[:-1]).any()
    sub = AC.edge_set(129)
    assert (sub.tiles[:, 3] + sub.tiles[:, 1]).max() == 129 and sub.n_dec == 13


def test_value_code_separates_keys():
    v = AC.v_code(AC.N_SLOTS, 2)
    assert _roundtrips(v) and v.float().abs().min() >= 1 and v.float().abs().max() <= 31
    for s, g in ((0, 0), (3, 1)):
        x = v[s, g].to(torch.int16)
        same = (x[:, None, :] == x[None, :, :]).sum(-1)
        same.fill_diagonal_(0)
        assert int(same.max()) <= 16, int(same.max())      # any two keys differ in >= 112 of 128 dims


@pytest.mark.parametrize("Hkv,group", [(2, 4), (1, 4), (8, 4), (1, 1), (3, 2)])
def test_needle_reference_is_the_target_row(Hkv, group):
    c = AC.needle(Hkv, group)
    ref, A, W = c.ref()
    assert _roundtrips(c.q) and _roundtrips(c.kc)
    G = group
    for t in _covered(c):
        p, s = int(c.edge.pos[t]), int(c.edge.slot[t])
        for h in range(c.Hq):
            k = int(c.target[t, h])
            assert 0 <= k <= p
            assert W[t, h, k] >= 1 - 2.0 ** -20, (t, h, k, float(W[t, h, k]))
            assert torch.equal(ref[t, h].float().to(torch.bfloat16), c.vc[s, h // G, k]), (t, h, k)
        if p >= 3:
            for g in range(Hkv):
                assert len(set(c.target[t, g * G:(g + 1) * G].tolist())) == G, (t, g)


def test_needle_targets_cover_edges_per_kernel():
    c = AC.needle()
    e = c.edge
    for rows in (e.dec_row, e.covered & ~e.dec_row):
        tg = c.target[rows]
        seen = set(tg.flatten().tolist())
        assert {0, *AC.EDGE_KEYS} <= seen, sorted({0, *AC.EDGE_KEYS} - seen)
        diag = (tg == e.pos[rows][:, None]).any(dim=1)
        assert diag.sum() >= rows.sum() // 2
    # every visible edge key is a target of its row unless the row has more candidates than heads
    for t in _covered(c):
        p = int(e.pos[t])
        want = {0, p, *[k for k in AC.EDGE_KEYS if k <= p]}
        if len(want) <= c.Hq:
            assert want <= set(c.target[t].tolist()), t


def test_needle_sweep_addresses_every_key():
    c = AC.needle(sweep=True)
    e = c.edge
    for rows in (e.dec_row, e.covered & ~e.dec_row):
        assert set(c.target[rows].flatten().tolist()) == set(range(128))
    assert (c.target[e.covered] <= e.pos[e.covered][:, None]).all()
    ref, A, W = c.ref()
    for t in _covered(c):
        for h in range(c.Hq):
            k = int(c.target[t, h])
            assert W[t, h, k] >= 1 - 2.0 ** -20
            assert torch.equal(ref[t, h].float().to(torch.bfloat16), c.vc[1, h // 4, k])


@pytest.mark.parametrize("a", [8, 2])
def test_ladder_steps_and_mass(a):
    c = AC.ladder(a)
    assert _roundtrips(c.q) and _roundtrips(c.kc) and _roundtrips(c.vc)
    step = 32 * a * AC.SCALE
    assert abs(step - {8: 22.627, 2: 5.657}[a]) < 1e-3
    # the score is step * position, for every key of the cache
    sc = (c.q[1, :AC.HD].double() @ c.kc[0, 0].double().t()) * AC.SCALE
    assert torch.allclose(sc, step * torch.arange(AC.MAX_CTX, dtype=torch.float64), rtol=1e-12, atol=0)
    assert float((c.q[1, :AC.HD].float() @ c.kc[0, 0].float().t()).max()) < 2 ** 24      # exact in fp32
    ref, A, W = c.ref()
    r = math.exp(-step)
    for t in _covered(c):
        p, s = int(c.edge.pos[t]), int(c.edge.slot[t])
        for h in (0, c.Hq - 1):
            if a == 8:
                assert 1 - W[t, h, p] <= 1.5e-10
                assert torch.equal(ref[t, h].float().to(torch.bfloat16), c.vc[s, h // 4, p])
            else:
                assert abs(float(W[t, h, p]) - (1 - r) / (1 - r ** (p + 1))) < 1e-12
                if p >= 1:
                    assert abs(float(W[t, h, p - 1] / W[t, h, p]) - r) < 1e-12
            assert W[t, h, p + 1:].sum() == 0


def test_twins_share_the_mass_equally():
    c = AC.twins()
    assert _roundtrips(c.q)
    ref, A, W = c.ref()
    crossing = set()
    for t in _covered(c):
        p, s = int(c.edge.pos[t]), int(c.edge.slot[t])
        for h in range(c.Hq):
            k1, k2 = int(c.target[t, h]), int(c.target2[t, h])
            assert 0 <= k1 <= p and 0 <= k2 <= p
            if k1 == k2:
                assert W[t, h, k1] >= 1 - 2.0 ** -20
                continue
            assert abs(float(W[t, h, k1] - W[t, h, k2])) <= 1e-14, (t, h)
            # the twins score 4 (128 + c) / sqrt(128), any other key 4 N(0, 256) / sqrt(128):
            # sd 5.7 nats against 45 +- 4, so the rest of the row holds well under 2^-10
            assert W[t, h, k1] + W[t, h, k2] >= 1 - 2.0 ** -10, (t, h, float(W[t, h, k1]))
            mid = (c.vc[s, h // 4, k1].double() + c.vc[s, h // 4, k2].double()) / 2
            assert (ref[t, h] - mid).abs().max() <= 31 * 2.0 ** -9
            crossing.add((k1, k2))
    assert set(AC.TWIN_PAIRS) <= crossing


@pytest.mark.parametrize("sigma", [0.5, 2, 4])
@pytest.mark.parametrize("Hkv", [2])
def test_segment_emulation_stays_inside_the_bound(sigma, Hkv):
    """P rounded to bf16, exact row sum, output rounded to bf16 -- on the
    exact probe-4 inputs of the GPU test -- is inside the segment bound: a
    correct kernel can meet it."""
    c = AC.spread(sigma, Hkv)
    e = c.edge
    ref, A, W = c.ref()
    emu = AC.emulate_segment(c.q, c.kc, c.vc, e.pos, e.slot, c.Hq, c.Hkv, c.scale)
    m = e.covered
    ratio = ((emu - ref).abs()[m] / A[m]).max().item()
    print(f"segment emulation sigma={sigma}: max err/A = {ratio / 2 ** -7:.3f} * 2^-7")
    assert ((emu - ref).abs()[m] <= AC.seg_bound(ref, A)[m]).all(), ratio
    # the spread really differs between the regimes: the heaviest key of a 320-key row
    big = W[(e.pos == AC.MAX_CTX - 1)].max(dim=-1).values.mean().item()
    assert big < 0.02 if sigma == 0.5 else big > 0.1, big


def test_reference_matches_refops_on_tiles():
    """The fp64 reference and RefOps.attention_tiles expand tiles alike."""
    from llm_message_queue_amd.ops.llama_ops import RefOps
    c = AC.spread(2)
    e = c.edge
    ref, A, W = c.ref()
    o = RefOps().attention_tiles(c.q, c.kc, c.vc, torch.from_numpy(e.tiles), c.Hq, c.Hkv, c.scale)
    o = o.double().view(e.T, c.Hq, AC.HD)
    m = e.covered
    assert ((o - ref).abs()[m] <= AC.U * ref.abs()[m] + 2.0 ** -11 * A[m]).all()
    assert torch.allclose(W[m].sum(-1), torch.ones((), dtype=torch.float64), atol=1e-12)
    assert (A >= ref.abs() - 1e-12).all()
