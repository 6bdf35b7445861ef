"""Per-request temperature sampling on the GPU: the device noise generator
against the numpy twin, ``lm_head_sample`` (GM_EPI_SAMPLE) against the
float64 reference sampler, greedy rows against ``lm_head_argmax``, the
distribution of the device's draws, and a sampled request end to end through
the HIP engine."""
import functools
import math

import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S
from tests.test_sampling_cpu import CHI2_8, DIST_V, dist_chi2, dist_keys, dist_logits

DEV = "cuda:0"


def _keys_t(keys: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).to(DEV)


@pytest.mark.gpu
def test_sample_bits_equal_the_numpy_twin():
    keys = S.row_keys(np.array([0, 1, 7, 7, 99, 2 ** 40, 2 ** 63 - 1, 12345], dtype=np.uint64),
                      np.array([0, 0, 0, 1, 500, 3, 63, 9]))
    n0 = 128256 - 4096 + 3                                          # (an odd first column, up to the vocabulary's end)
    got = G.sample_bits(_keys_t(keys), n0, 4096).cpu().numpy().view(np.uint32)
    want = S.noise_bits(keys, np.arange(n0, n0 + 4096, dtype=np.uint32))
    assert got.shape == (8, 4096) and np.array_equal(got, want)


@functools.lru_cache(maxsize=None)
def _case(M, V, K):
    """Inputs and the float64 reference of one shape, computed once: bf16
    x / w, fp32 logits (as float64, on the host), the twin's noise."""
    g = torch.Generator(device=DEV).manual_seed(M + V + K)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g, device=DEV) * (0.02 * math.sqrt(4096 / K))).to(torch.bfloat16)
    lg = (x.float() @ w.float().t()).cpu().numpy().astype(np.float64)
    keys = S.row_keys(np.arange(M, dtype=np.uint64) + np.uint64(1000), np.arange(M) % 7)
    noise = np.concatenate([S.gumbel(keys[i:i + 64], np.arange(V, dtype=np.uint32)) for i in range(0, M, 64)])
    lg.setflags(write=False)
    noise.setflags(write=False)
    return x, w, lg, keys, noise


SHAPES = [(300, 1024, 256), (300, 17920, 512), (520, 4096, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1.0, 0.7, 0.25])
@pytest.mark.parametrize("M,V,K", SHAPES)
def test_lm_head_sample_matches_the_reference_sampler(M, V, K, T):
    """A pick may differ from the float64 reference only where the
    reference's score gap is within the fp32-accumulation margin of the
    greedy head's test (1e-3 * max|logit| of the row, here scaled by 1 / T)
    plus twice the noise arithmetic bound (2 x ~2.4e-4 -> 1e-3), and in at
    most max(2, M // 50) rows."""
    x, w, lg, keys, noise = _case(M, V, K)
    it = np.full(M, np.float32(1.0 / T), dtype=np.float32)
    got = G.lm_head_sample(x, w, torch.from_numpy(it).to(DEV), _keys_t(keys)).cpu().numpy().astype(np.int64)
    sc = lg * it.astype(np.float64)[:, None] + noise
    exp = sc.argmax(axis=1)
    assert (exp != lg.argmax(axis=1)).mean() > 0.2                   # (the noise decides: this is not the greedy head)
    bad = np.flatnonzero(got != exp)
    print(f"M={M} V={V} K={K} T={T}: {len(bad)} rows differ from the reference")
    assert ((got >= 0) & (got < V)).all()
    for i in bad.tolist():
        gap = sc[i, exp[i]] - sc[i, got[i]]
        margin = 1e-3 * np.abs(lg[i]).max() / T + 1e-3
        print(f"  row {i}: gap {gap:.3e} margin {margin:.3e}")
        assert 0 <= gap <= margin, (i, gap, margin)
    assert len(bad) <= max(2, M // 50), len(bad)


@pytest.mark.gpu
def test_greedy_rows_of_a_sampling_launch_equal_lm_head_argmax():
    M, V, K = SHAPES[0]
    x, w, lg, keys, noise = _case(M, V, K)
    it = np.full(M, np.float32(1.0 / 0.7), dtype=np.float32)
    it[::3] = 0.0
    greedy = G.lm_head_argmax(x, w).clone()
    got = G.lm_head_sample(x, w, torch.from_numpy(it).to(DEV), _keys_t(keys))
    assert torch.equal(got[::3], greedy[::3])
    samp = np.ones(M, dtype=bool)
    samp[::3] = False
    exp = (lg * it.astype(np.float64)[:, None] + noise).argmax(axis=1)
    assert (got.cpu().numpy()[samp] == exp[samp]).mean() > 0.95      # (the other rows still sample)
    # unpadded inputs (M floats / M keys) give the same picks as whole-tile ones
    pad = G.row_scale_len(M) - M
    it_p = torch.from_numpy(np.concatenate([it, np.zeros(pad, np.float32)])).to(DEV)
    k_p = _keys_t(np.concatenate([keys, np.zeros((pad, 2), np.uint32)]))
    assert torch.equal(G.lm_head_sample(x, w, it_p, k_p), got)


@pytest.mark.gpu
def test_greedy_rows_resolve_ties_to_the_lowest_column():
    V, d, M = 1024, 256, 256
    x = torch.zeros(M, d, device=DEV)
    w = torch.zeros(V, d, device=DEV)
    x[0, 0] = 1.0
    w[[300, 1000, 700], 0] = 2.0                                     # tie across tiles
    x[1, 1] = 1.0
    w[[515, 513, 777], 1] = 3.0                                      # tie inside one tile (513, 515) and across
    x[2, 2] = -1.0
    w[:, 2] = 1.0
    w[123, 2] = -5.0                                                 # single maximum, negative logits
    x, w = x.to(torch.bfloat16), w.to(torch.bfloat16)
    it = np.full(M, 1.0, dtype=np.float32)
    it[:3] = 0.0
    it[3::3] = 0.0
    keys = S.row_keys(5, np.arange(M))
    got = G.lm_head_sample(x, w, torch.from_numpy(it).to(DEV), _keys_t(keys)).cpu().numpy()
    greedy = G.lm_head_argmax(x, w).cpu().numpy()
    assert got[0] == 300 and got[1] == 513 and got[2] == 123
    assert np.array_equal(got[it == 0], greedy[it == 0]) and (got[3::3] == 0).all()
    # the all-zero rows that sample pick the column of the largest noise term
    rows = np.flatnonzero(it != 0)
    g = S.gumbel(keys[rows], np.arange(V, dtype=np.uint32))
    top2 = np.sort(g, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-3
    assert clear.sum() > 100 and np.array_equal(got[rows][clear], g.argmax(axis=1)[clear])


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1.0, 0.5])
def test_device_draws_follow_softmax(T):
    """4,096 identical rows with distinct keys in one launch: the picks'
    chi-square over the eight heavy tokens + "rest" against softmax(logits /
    T) (of the bf16-rounded logits the kernel sees)."""
    n, K = 4096, 128
    x = torch.zeros(n, K, device=DEV, dtype=torch.bfloat16)
    x[:, 0] = 1.0
    w = torch.zeros(DIST_V, K, device=DEV, dtype=torch.bfloat16)
    w[:, 0] = torch.from_numpy(dist_logits()).to(DEV).to(torch.bfloat16)
    it = torch.full((n,), 1.0 / T, dtype=torch.float32, device=DEV)
    picks = G.lm_head_sample(x, w, it, _keys_t(dist_keys())).cpu().numpy()
    chi = dist_chi2(picks, T, w[:, 0].float().cpu().numpy())
    print(f"T={T}: chi-square {chi:.2f} (bound {CHI2_8})")
    assert chi < CHI2_8


@pytest.mark.gpu
def test_unfused_sample_head_scores_the_library_logits_with_the_same_noise():
    """``HipOps.sample_head`` below ``min_rows`` (the library-GEMM option):
    bf16 logits from ``F.linear``, the device generator's bits, float64
    scores -- the reference sampler over those same logits, row for row."""
    from llm_message_queue_amd.ops.llama_ops import HipOps
    M, V, K = SHAPES[0]
    x, w, _, keys, _ = _case(M, V, K)
    it = np.full(M, np.float32(1.0 / 0.7), dtype=np.float32)
    it[::3] = 0.0
    got = HipOps().sample_head(x, w, torch.from_numpy(it).to(DEV), _keys_t(keys), fused=True, min_rows=M + 1)
    lg = torch.nn.functional.linear(x, w).float().cpu().numpy()
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), S.sample_reference(lg, it, keys))


# --------------------------------------------------------------------------- tiny model end to end
def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(2000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 6).astype(np.int32), gen_tokens=6, **kw)


def _drain(eng, reqs):
    assert len(eng.admit(reqs)) == len(reqs)
    done = {r.req_id: r for r in eng.drain()}
    assert len(done) == len(reqs)
    return done


@pytest.mark.gpu
def test_sampled_request_through_the_hip_engine():
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    cfg = LlamaConfig.tiny()
    eng = BackendEngine(cfg, slots=64, max_ctx=64, token_budget=512, device=DEV, impl="hip")
    alone = _drain(eng, [_req(100, temperature=0.8, seed=7)])[100]
    crowd = _drain(eng, [_req(i) for i in range(40)] + [_req(100, temperature=0.8, seed=7)])
    other = _drain(eng, [_req(100, temperature=0.8, seed=8)])[100]
    torch.cuda.synchronize()
    assert eng.sampled_steps > 0
    assert len(alone.out_tokens) == 6 and np.array_equal(alone.out_tokens, crowd[100].out_tokens)
    assert not np.array_equal(alone.out_tokens, other.out_tokens)

    # the CPU reference engine with the same weights: same tokens up to the
    # first token whose reference score gap is inside the margin
    ref = BackendEngine(cfg, slots=4, max_ctx=64, token_budget=512, device="cpu", impl="ref")
    hm, rm = eng.model, ref.model
    rm.embed, rm.lm_head, rm.final_norm = hm.embed.cpu(), hm.lm_head.cpu(), hm.final_norm.cpu()
    for Lh, Lr in zip(hm.layers, rm.layers):
        for k in Lr:
            Lr[k] = (G.swiglu_unpermute(Lh[k]) if (k == "w_gu" and hm.fused_mlp) else Lh[k]).cpu()
    gaps = []
    inner = rm.ops.sample_head

    def spy(x, w, inv_temp, keys, fused=True, min_rows=256):
        lg = (x.float() @ w.float().t()).double().numpy()
        it = inv_temp[:1].double().numpy()
        kk = keys[:1].contiguous().view(torch.int32).numpy().view(np.uint32)
        sc = lg[:1] * it[:, None] + S.gumbel(kk, np.arange(lg.shape[1], dtype=np.uint32))
        top = np.sort(sc[0])[-2:]
        gaps.append((top[1] - top[0], 1e-3 * np.abs(lg[0]).max() * float(it[0]) + 1e-3))
        return inner(x, w, inv_temp, keys, fused, min_rows)

    rm.ops.sample_head = spy
    want = _drain(ref, [_req(100, temperature=0.8, seed=7)])[100]
    assert len(gaps) == 6
    n = 0
    for (gap, margin), a, b in zip(gaps, alone.out_tokens.tolist(), want.out_tokens.tolist()):
        print(f"token {n}: hip {a} ref {b} gap {gap:.3e} margin {margin:.3e}")
        if gap <= margin:
            break
        assert a == b, (n, a, b, gap, margin)
        n += 1
