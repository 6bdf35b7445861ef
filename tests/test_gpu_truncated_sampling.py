"""Top-k / top-p sampling on the GPU: ``sample_truncated_kernel`` against the
numpy twin on given logits (three vocabulary sizes, a launch above the grid
size, edge rows at the serving vocabulary), the distribution of its draws,
``HipOps.truncated_head`` over exact logits, and a truncating request end to
end through the HIP engine."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as GC
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S
from tests.test_sampling_cpu import DIST_TOP, DIST_V, dist_keys, dist_logits

DEV = "cuda:0"
V_SERVE = 128256
DELTA = 1e-3                       # relative slack on top_p (the device's fp32 mass sums: < 1e-5 relative)
NOISE = 1e-3                       # the noise-arithmetic bound of test_gpu_sampling.py
# chi-square critical value at p = 1e-6, 3 degrees of freedom (scipy.stats.chi2.isf(1e-6, 3))
CHI2_3 = 30.665
TEMPS = (0.25, 0.7, 1.0, 2.0)
TOP_KS = (0, 1, 5, 50, 1000)
TOP_PS = (1.0, 0.1, 0.5, 0.9, 0.999)


def _bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _params(R):
    """Per-row parameters: T cycles with the row, top_k with the row and
    top_p with every fifth row, so every (top_k, top_p) pair occurs."""
    i = np.arange(R)
    it = (1.0 / np.array(TEMPS))[i % 4].astype(np.float32)
    tk = np.array(TOP_KS, dtype=np.int32)[i % 5]
    tp = np.array(TOP_PS, dtype=np.float32)[(i // 5) % 5]
    return it, tk, tp


def _launch(lg: torch.Tensor, V, it, keys, tk, tp) -> np.ndarray:
    """``lg`` bf16 [R][V] on the host -> the kernel's picks; the device rows
    are ld = ceil(V / 8) * 8 long with NaN-free garbage (a huge logit) in the
    padding, which must never be picked."""
    R = lg.shape[0]
    ld = (V + 7) // 8 * 8
    d = torch.full((R, ld), 3.0e38, dtype=torch.bfloat16, device=DEV)
    d[:, :V] = lg.to(DEV)
    got = G.sample_truncated(d, torch.from_numpy(it).to(DEV),
                             torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).to(DEV),
                             torch.from_numpy(tk).to(DEV), torch.from_numpy(tp).to(DEV), vocab=V)
    assert got.dtype == torch.int32 and got.shape == (R,)
    return got.cpu().numpy().astype(np.int64)


def _reference(lg64: np.ndarray, it, keys, tk, tp):
    """Per row: the float64 scores, the twin's pick at top_p, top_p (1 - d)
    and top_p (1 + d), and the untruncated pick."""
    R, V = lg64.shape
    cols = np.arange(V, dtype=np.uint32)
    rows = []
    for r in range(R):
        sc = lg64[r] * float(it[r]) + S.gumbel(keys[r:r + 1], cols)[0]
        sc = np.where(np.isfinite(lg64[r]), sc, -np.inf)
        picks = []
        for f in (1.0, 1.0 - DELTA, 1.0 + DELTA):
            keep = S.truncation_keep(lg64[r], it[r], tk[r], np.float32(tp[r]) * np.float32(f) if tp[r] < 1 else 1.0)
            picks.append(int(np.where(keep, sc, -np.inf).argmax()) if keep.any() else 0)
        rows.append((sc, picks, int(sc.argmax())))
    return rows


def _check(got, ref, max_tolerated):
    """The pass rule: a pick equals the twin's at top_p or at top_p (1 -+ d),
    or the twin's score gap to it is >= 0 and <= 1e-3 + 2^-22 max|score|."""
    tolerated = 0
    for r, (sc, picks, _plain) in enumerate(ref):
        g = int(got[r])
        assert 0 <= g < len(sc), (r, g)
        if g == picks[0]:
            continue
        tolerated += 1
        gap = sc[picks[0]] - sc[g]
        margin = NOISE + 2.0 ** -22 * np.abs(sc[np.isfinite(sc)]).max(initial=0.0)
        print(f"  row {r}: got {g} twin {picks} gap {gap:.3e} margin {margin:.3e}")
        assert g in picks or 0 <= gap <= margin, (r, g, picks, gap, margin)
    assert tolerated <= max_tolerated, tolerated


@functools.lru_cache(maxsize=None)
def _family(V, R):
    """bf16(3 randn) rows from default_rng(0), their parameters and the
    twin's picks, computed once."""
    rng = np.random.default_rng(0)
    lg = _bf16(3.0 * rng.standard_normal((R, V)))
    keys = S.row_keys(np.arange(R, dtype=np.uint64) + np.uint64(500), np.arange(R) % 9)
    it, tk, tp = _params(R)
    ref = _reference(lg.double().numpy(), it, keys, tk, tp)
    return lg, keys, it, tk, tp, ref


@pytest.mark.gpu
@pytest.mark.parametrize("V,R", [(1000, 96), (4099, 96), (V_SERVE, 96), (4099, 300)])
def test_kernel_matches_the_twin(V, R):
    lg, keys, it, tk, tp, ref = _family(V, R)
    got = _launch(lg, V, it, keys, tk, tp)
    changed = np.mean([picks[0] != plain for _sc, picks, plain in ref])
    exact = np.mean([int(got[r]) == ref[r][1][0] for r in range(R)])
    print(f"V={V} R={R}: {exact:.3f} equal the twin, truncation changes {changed:.3f} of the twin's picks")
    assert changed > 0.2
    _check(got, ref, max_tolerated=R * 5 // 100)


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(1)
    V = V_SERVE
    rows, tk, tp = [], [], []

    def add(row, k, p):
        rows.append(row.astype(np.float32))
        tk.append(k)
        tp.append(p)

    shared = -1.0 - np.abs(rng.standard_normal(V))                    # 70,000 columns share the maximum
    shared[rng.permutation(V)[:70000]] = 2.0
    add(shared, 1, 1.0)
    add(shared, 0, 0.5)
    add(shared, 70001, 1.0)                                           # ... and one more group
    last = 3.0 * rng.standard_normal(V)                               # the maximum sits in the last column
    last[V - 1] = 40.0
    add(last, 1, 1.0)
    add(last, 0, 0.9)
    neg = -0.5 - np.abs(3.0 * rng.standard_normal(V))                 # all logits negative
    add(neg, 5, 0.9)
    add(neg, 0, 0.5)
    far = -5.0 - np.abs(rng.standard_normal(V))                       # the 50th largest lies in the second window
    far[[7, 70000, V - 2]] = [1.0, 0.75, 0.5]
    add(far, 50, 1.0)
    add(far, 50, 0.999)
    add(far, 0, 0.9999)
    add(far, 3, 1.0)
    flat = np.full(V, -2.5)                                           # all equal: the argmax of the noise
    add(flat, 1, 1.0)
    add(flat, 0, 0.001)
    nan = 3.0 * rng.standard_normal(V)                                # NaN is never kept, even as "the maximum"
    nan[::3] = np.nan
    add(nan, 2, 1.0)
    add(np.full(V, np.nan), 3, 0.5)                                   # no finite logit: token 0
    lg = _bf16(np.stack(rows))
    R = len(rows)
    keys = S.row_keys(77, np.arange(R))
    it = np.full(R, 1.0, dtype=np.float32)
    tk, tp = np.array(tk, dtype=np.int32), np.array(tp, dtype=np.float32)
    return lg, keys, it, tk, tp, _reference(lg.double().numpy(), it, keys, tk, tp)


@pytest.mark.gpu
def test_edge_rows_at_the_serving_vocabulary():
    lg, keys, it, tk, tp, ref = _edge_rows()
    lg64 = lg.double().numpy()
    # what the cases are meant to be, by the twin
    assert S.truncation_keep(lg64[0], 1.0, 1, 1.0).sum() == 70000
    assert S.truncation_keep(lg64[2], 1.0, 70001, 1.0).sum() > 70000
    assert ref[3][1][0] == V_SERVE - 1 and lg64[5].max() < 0
    k50 = S.truncation_keep(lg64[7], 1.0, 50, 1.0)
    assert k50.sum() >= 50 and lg64[7][k50].min() <= -5.0
    assert ref[11][1][0] == ref[11][2] and ref[14][1][0] == 0
    got = _launch(lg, V_SERVE, it, keys, tk, tp)
    print("edge picks", got.tolist())
    _check(got, ref, max_tolerated=1)
    assert got[3] == V_SERVE - 1 and got[14] == 0 and S.truncation_keep(lg64[13], 1.0, 2, 1.0)[got[13]]
    for r in (0, 1):
        assert lg64[r][got[r]] == 2.0
    # R = 1: every row alone gives the pick it got in the launch of all
    for r in (2, 7, 12):
        one = _launch(lg[r:r + 1], V_SERVE, it[r:r + 1], keys[r:r + 1], tk[r:r + 1], tp[r:r + 1])
        assert one.tolist() == [got[r]]


def _dist_chi2_top(picks, T, logits, n_top):
    lg = np.asarray(logits, dtype=np.float64)[DIST_TOP[:n_top]] / T
    p = np.exp(lg - lg.max())
    p /= p.sum()
    idx = {int(c): i for i, c in enumerate(DIST_TOP[:n_top])}
    cnt = np.bincount([idx[int(c)] for c in picks], minlength=n_top).astype(np.float64)
    e = p * len(picks)
    assert e.min() > 5
    return float(((cnt - e) ** 2 / e).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1.0, 0.5])
def test_truncated_draws_follow_the_renormalised_softmax(T):
    n = 4096
    row = _bf16(dist_logits())
    lg = row.repeat(n, 1)
    it = np.full(n, 1.0 / T, dtype=np.float32)
    ones = np.ones(n, dtype=np.float32)
    picks = _launch(lg, DIST_V, it, dist_keys(), np.full(n, 4, dtype=np.int32), ones)
    assert np.isin(picks, DIST_TOP[:4]).all()
    chi = _dist_chi2_top(picks, T, row.double().numpy(), 4)
    print(f"T={T}: top_k=4 chi-square {chi:.2f} (bound {CHI2_3})")
    assert chi < CHI2_3
    if T == 1.0:
        picks = _launch(lg, DIST_V, it, dist_keys(), np.zeros(n, dtype=np.int32), np.full(n, 0.5, dtype=np.float32))
        assert np.isin(picks, DIST_TOP[:5]).all() and len(set(picks.tolist())) == 5


@pytest.mark.gpu
def test_truncated_head_over_exact_logits_equals_the_reference():
    """x and w over {-1, 0, 1}: the logits are integers, exact in fp32 and in
    bf16, so the store-epilogue GEMM's tensor is the reference's and the picks
    must agree row for row; rows without truncation also equal the fused
    head's (same logits, same noise)."""
    from llm_message_queue_amd.ops.llama_ops import HipOps
    M, N, K = 37, 1024, 256
    c = GC.int_case(M, N, K, 11)
    keys = S.row_keys(np.arange(M, dtype=np.uint64) + np.uint64(31), np.arange(M) % 5)
    it, tk, tp = _params(M)
    x, w = c.x.to(DEV), c.w.to(DEV)
    kd = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)).to(DEV)
    got = HipOps().truncated_head(x, w, torch.from_numpy(it).to(DEV), kd, torch.from_numpy(tk).to(DEV),
                                  torch.from_numpy(tp).to(DEV)).cpu().numpy()
    want = S.sample_truncated_reference(c.ref.numpy(), it, keys, tk, tp)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    plain = (tk == 0) & (tp >= 1)
    assert plain.sum() >= 2
    fused = G.lm_head_sample(x, w, torch.from_numpy(it).to(DEV), kd).cpu().numpy()
    assert np.array_equal(fused[plain], got[plain])
    assert (fused != got).any()                                      # (truncation is not a no-op on tied integer logits)


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
def test_truncating_request_through_the_hip_engine():
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=64, max_ctx=64, token_budget=512, device=DEV, impl="hip")

    def crowd():
        return [_req(i) for i in range(30)] + [_req(30 + i, temperature=0.9, seed=i) for i in range(10)]
    trunc = dict(temperature=0.8, seed=7, top_k=3)
    alone = _drain(eng, [_req(100, **trunc)])[100]
    assert eng.truncated_steps > 0
    n = eng.truncated_steps
    without = _drain(eng, crowd())
    assert eng.truncated_steps == n                                  # (no truncating row: nothing new launched)
    among = _drain(eng, crowd() + [_req(100, **trunc)])
    plain = _drain(eng, [_req(100, temperature=0.8, seed=7)])[100]
    torch.cuda.synchronize()
    assert eng.truncated_steps > n
    assert len(alone.out_tokens) == 6 and np.array_equal(alone.out_tokens, among[100].out_tokens)
    for i in range(40):
        assert np.array_equal(among[i].out_tokens, without[i].out_tokens), i
    assert not np.array_equal(alone.out_tokens, plain.out_tokens)
