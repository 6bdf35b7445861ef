"""Log-probabilities on the GPU: ``logprob_kernel`` against the numpy twin
within the derived bound on given logits (sizes around every loop boundary, a
launch above the block cap, edge rows at the serving vocabulary), the purity
of a row's result, ``HipOps.logprob_head`` over exact logits, the wrapper's
refusals, and a request that asks for log-probabilities end to end through
the HIP engine."""
import functools

import numpy as np
import pytest
import torch

import gemm_cases as GC
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S

DEV = "cuda:0"
V_SERVE = 128256
SENT_LP, SENT_ID = 777.0, -777     # what the outputs hold before the launch
ABOVE_CAP = -1                     # a row count: one above the kernel's block cap (the grid-stride loop)
SHAPES = [(1, 3), (5, 3), (8, 3), (2047, 8), (2049, 8), (16395, 8), (V_SERVE, 4), (1000, ABOVE_CAP)]


def _cap() -> int:
    """The kernel's block cap and alternatives count as the binding exports
    them (``LP_MAX_BLOCKS`` / ``LP_TOP`` of csrc/kernels/logprob_kernels.h)."""
    from llm_message_queue_amd import _native
    k = _native.require_hipops()
    assert k.LP_TOP == S.LP_TOP == G.LP_TOP
    return int(k.LP_MAX_BLOCKS)


def _bf16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _bf16_above(x: float) -> float:
    """The next bf16 number above the bf16 number ``x``."""
    b = int(np.float32(x).view(np.uint32)) >> 16
    b = 0x0001 if (b & 0x7FFF) == 0 else (b - 1 if b & 0x8000 else b + 1)
    return float(np.array([b << 16], dtype=np.uint32).view(np.float32)[0])


def _distinct_top6(row: np.ndarray) -> None:
    """Raise members of the row's top 6 (in place, to bf16 numbers) until no
    two of them are equal: a raised value stays above the 7th."""
    n = min(6, len(row))
    order = np.argsort(-row, kind="stable")[:n]
    for i in range(n - 2, -1, -1):
        if row[order[i]] <= row[order[i + 1]]:
            row[order[i]] = _bf16_above(row[order[i + 1]])


def _launch(lg: torch.Tensor, V: int, tok: np.ndarray):
    """``lg`` bf16 [R][V] on the host -> the kernel's (lp, ids); the device
    rows are ld = ceil(V / 8) * 8 long with a huge logit in the padding, which
    must never count, and the outputs are pre-filled."""
    R = lg.shape[0]
    ld = (V + 7) // 8 * 8
    d = torch.full((R, ld), 3.0e38, dtype=torch.bfloat16, device=DEV)
    d[:, :V] = lg.to(DEV)
    out_lp = torch.full((R, 6), SENT_LP, dtype=torch.float32, device=DEV)
    out_id = torch.full((R, 5), SENT_ID, dtype=torch.int32, device=DEV)
    lp, ids = G.token_logprobs(d, torch.from_numpy(np.asarray(tok, dtype=np.int32)).to(DEV), vocab=V,
                               out_lp=out_lp, out_id=out_id)
    assert lp.shape == (R, 6) and ids.shape == (R, 5) and lp.dtype == torch.float32 and ids.dtype == torch.int32
    return lp.cpu().numpy(), ids.cpu().numpy().astype(np.int64)


def _compare(lp, ids, want_lp, want_ids, bound, what=""):
    """ids exact, -inf exactly where the twin has it, the rest within
    ``bound`` (a number or one per row); returns the worst difference."""
    assert np.array_equal(ids, want_ids), (what, np.flatnonzero((ids != want_ids).any(axis=1))[:8])
    fin = np.isfinite(want_lp)
    assert np.array_equal(np.isfinite(lp), fin) and (lp[~fin] == -np.inf).all(), what
    err = np.where(fin, np.abs(np.where(fin, lp, 0.0).astype(np.float64) - np.where(fin, want_lp, 0.0)), 0.0)
    worst = float(err.max(initial=0.0))
    print(f"{what}: worst |device - twin| {worst:.3e} (bound {np.max(bound):.3e})")
    assert (err <= np.reshape(bound, (-1, 1)) if np.ndim(bound) else err <= bound).all(), (what, worst)
    return worst


def _consistent(lp, ids, tok):
    """Alternatives in non-increasing order; a token that is one of them has
    the same bits in both places."""
    assert (lp[:, 2:] <= lp[:, 1:-1]).all()
    hits = 0
    for r in range(len(lp)):
        for i in np.flatnonzero(ids[r] == tok[r]):
            assert lp[r, 0].view(np.uint32) == lp[r, 1 + i].view(np.uint32), r
            hits += 1
    return hits


@functools.lru_cache(maxsize=None)
def _family(V, R):
    """bf16(3 randn) rows from default_rng(0), no two of a row's top 6 equal
    except in row 1, where a tie at the 5th place is planted (V >= 8); the
    tokens (the most likely, the third, then random ones) and the twin's
    result, computed once."""
    rng = np.random.default_rng(0)
    a = _bf16(3.0 * rng.standard_normal((R, V))).float().numpy()
    for r in range(R):
        _distinct_top6(a[r])
    planted = V >= 8
    if planted:
        order = np.argsort(-a[1], kind="stable")
        a[1, order[5]] = a[1, order[4]]                               # the 6th rises to the 5th: a tie for the last place
    lg = _bf16(a)
    assert np.array_equal(lg.float().numpy(), a)
    for r in range(R):                                                # checked here, so the id comparison needs no exemption
        top = np.sort(a[r])[::-1][:6]
        if planted and r == 1:
            assert top[4] == top[5] and len(set(top[:5].tolist())) == 5
        else:
            assert len(set(top.tolist())) == len(top), r
    tok = rng.integers(0, V, R)
    tok[0] = int(np.argmax(a[0]))
    if R > 2 and V > 2:
        tok[2] = int(np.argsort(-a[2], kind="stable")[2])
    want_lp, want_ids = S.logprob_reference(lg.double().numpy(), tok)
    return lg, tok, want_lp, want_ids


@pytest.mark.gpu
@pytest.mark.parametrize("V,R", SHAPES)
def test_kernel_matches_the_twin(V, R):
    R = _cap() + 1 if R == ABOVE_CAP else R
    lg, tok, want_lp, want_ids = _family(V, R)
    lp, ids = _launch(lg, V, tok)
    _compare(lp, ids, want_lp, want_ids, S.logprob_bound(V), f"V={V} R={R}")
    if V >= 8:                                                        # the planted tie went to the lower column
        a = lg[1].float().numpy()
        tied = np.flatnonzero(a == a[ids[1, 4]])
        assert len(tied) == 2 and ids[1, 4] == tied.min()
    assert _consistent(lp, ids, tok) >= 1
    assert (ids[:, min(V, 5):] == -1).all() and (ids[:, :min(V, 5)] >= 0).all()


@functools.lru_cache(maxsize=None)
def _edge_rows():
    rng = np.random.default_rng(1)
    V = V_SERVE
    rows, tok = [], []

    def add(row, t):
        rows.append(np.asarray(row, dtype=np.float32))
        tok.append(t)

    add(np.full(V, -2.5), 77)                                         # 0: all equal: -log V, alternatives 0..4
    one = np.full(V, np.nan)
    one[1::2] = -np.inf
    one[70001] = 3.0
    add(one, 70001)                                                   # 1: one finite column: lp 0
    add(np.full(V, np.nan), 5)                                        # 2: no candidate at all
    last = 3.0 * rng.standard_normal(V)
    last[V - 1] = 40.0
    add(last, V - 1)                                                  # 3: the maximum only in the last column
    far = -200.0 - np.abs(rng.standard_normal(V))                     # 4, 5: most terms underflow to 0
    far[[7, 70000, V - 2]] = [1.0, 0.75, 0.5]
    add(far, 70000)
    add(far, 12345)                                                   # (a token 200 nats down)
    nan = 3.0 * rng.standard_normal(V)
    nan[::3] = np.nan
    add(nan, 3 * 1000)                                                # 6: the token sits on a NaN column
    add(nan, -1)                                                      # 7, 8, 9: tokens out of range
    add(nan, V)
    add(nan, V + 3)                                                   # (a padding column)
    zeros = np.zeros(V)
    zeros[::2] = -0.0
    add(zeros, 1)                                                     # 10: +0 and -0 are one value
    a = _bf16(np.stack(rows)).float().numpy()
    for r in (3, 6):
        _distinct_top6(a[r])
    lg = _bf16(a)
    tok = np.array(tok, dtype=np.int64)
    want_lp, want_ids = S.logprob_reference(lg.double().numpy(), tok)
    return lg, tok, want_lp, want_ids


@pytest.mark.gpu
def test_edge_rows_at_the_serving_vocabulary():
    lg, tok, want_lp, want_ids = _edge_rows()
    V = V_SERVE
    a = lg.double().numpy()
    # what the cases are meant to be, by the twin
    assert np.allclose(want_lp[0], -np.log(V), atol=1e-12) and want_ids[0].tolist() == [0, 1, 2, 3, 4]
    assert want_lp[1, :2].tolist() == [0.0, 0.0] and want_ids[1].tolist() == [70001, -1, -1, -1, -1]
    assert (want_lp[2] == -np.inf).all() and (want_ids[2] == -1).all()
    assert want_ids[3, 0] == V - 1
    assert a[4].max() - a[4].min() > 104 and want_lp[5, 0] < -200
    assert want_lp[6, 0] == -np.inf and np.isfinite(want_lp[6, 1:]).all()
    assert (want_lp[7:10, 0] == -np.inf).all()
    assert want_ids[10].tolist() == [0, 1, 2, 3, 4]
    lp, ids = _launch(lg, V, tok)
    # the bound for the columns each row compares: the default span covers every probability above 0
    m = np.nanmax(np.where(np.isfinite(a), a, np.nan), axis=1, initial=-np.inf)
    span = [max(128.0, float(m[r] - a[r, tok[r]])) if 0 <= tok[r] < V and np.isfinite(a[r, tok[r]]) else 128.0
            for r in range(len(tok))]
    bound = np.array([S.logprob_bound(V, s) for s in span])
    _compare(lp, ids, want_lp, want_ids, bound, "edge rows")
    _consistent(lp, ids, tok)
    assert lp[1, 0] == 0.0 and lp[10, 0].view(np.uint32) == lp[10, 1].view(np.uint32)


@pytest.mark.gpu
def test_a_rows_result_does_not_depend_on_its_launch():
    V = 16395
    lg, tok, _lp, _ids = _family(V, 8)
    other, otok, _a, _b = _family(2049, 8)
    row, t = lg[3:4], tok[3:4]
    alone = _launch(row, V, t)
    seen = []
    for R, at in ((2, 0), (2, 1), (5, 4), (8, 1), (_cap() + 3, _cap() + 2)):
        fill = lg[torch.arange(R) % 8].clone()
        fill[::2, :2049] = other[0]                                   # (different neighbours from launch to launch)
        toks = np.resize(tok, R)
        fill[at], toks[at] = row[0], t[0]
        lp, ids = _launch(fill, V, toks)
        seen.append((lp[at], ids[at]))
    for lp, ids in seen:
        assert np.array_equal(lp.view(np.uint32), alone[0][0].view(np.uint32)) and np.array_equal(ids, alone[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 1000])
def test_logprob_head_over_exact_logits(N):
    """x and w over {-1, 0, 1}: the logits are integers, exact in fp32 and in
    bf16, so the head's logits are exactly known, from the tile kernel's store
    epilogue (N = 1024) and from the padded ``F.linear`` the tile kernel's
    refusal leads to (N = 1000)."""
    from llm_message_queue_amd.ops.llama_ops import HipOps
    M, K = 37, 256
    c = GC.int_case(M, N, K, 11)
    assert G.supported(M, N, K) == (N == 1024)
    ref = c.ref.numpy()
    tok = np.random.default_rng(3).integers(0, N, M)
    tok[::4] = ref[::4].argmax(axis=1)
    lp, ids = HipOps().logprob_head(c.x.to(DEV), c.w.to(DEV), torch.from_numpy(tok).to(DEV).to(torch.int32))
    want_lp, want_ids = S.logprob_reference(ref, tok)
    span = float((ref.max(axis=1, keepdims=True) - ref).max())
    _compare(lp.cpu().numpy(), ids.cpu().numpy().astype(np.int64), want_lp, want_ids,
             S.logprob_bound(N, max(128.0, span)), f"logprob_head N={N}")
    assert _consistent(lp.cpu().numpy(), ids.cpu().numpy(), tok) >= M // 4


@pytest.mark.gpu
def test_wrapper_refuses_before_any_launch():
    lg = torch.zeros((2, 16), dtype=torch.bfloat16, device=DEV)
    tok = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        G.token_logprobs(lg.float(), tok)
    with pytest.raises(ValueError):
        G.token_logprobs(lg, tok.long())
    with pytest.raises(ValueError):
        G.token_logprobs(lg.cpu(), tok.cpu())
    with pytest.raises(ValueError):
        G.token_logprobs(lg, tok.cpu())
    with pytest.raises(ValueError):
        G.token_logprobs(torch.zeros((2, 12), dtype=torch.bfloat16, device=DEV), tok)
    with pytest.raises(ValueError):
        G.token_logprobs(lg, tok, vocab=17)
    with pytest.raises(ValueError):
        G.token_logprobs(lg, tok, out_lp=torch.zeros((2, 6), dtype=torch.float64, device=DEV))
    lp, ids = G.token_logprobs(lg[:0], tok)                           # no row: no launch, empty results
    assert lp.shape == (0, 6) and ids.shape == (0, 5)


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


def _bits(r):
    return (r.out_tokens.tolist(), r.out_logprobs.view(np.uint32).tolist(), r.out_top_ids.tolist(),
            r.out_top_logprobs.view(np.uint32).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.8, seed=7), dict(temperature=0.8, seed=7, top_k=3)],
                         ids=["greedy", "sampling", "truncating"])
def test_logprob_request_through_the_hip_engine(kw):
    """The log-probabilities are a pure function of the row's logits, and the
    logits are the trunk's: they are the same bits from run to run as long as
    every step takes the same kernels.  A step of at most 64 tokens
    (``token_budget``) runs all its layer GEMMs on the skinny kernel with one
    split-K factor (``ops.gemm.SKINNY_MAX_M``), whoever shares it; a larger
    step moves the gate/up GEMM to the tile kernel, whose other order of
    additions can move a hidden state, and with it a logit, by a bf16 ulp."""
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=64, max_ctx=64, token_budget=64, device=DEV, impl="hip")

    def crowd():
        return [_req(i) for i in range(9)] + [_req(9 + i, temperature=0.9, seed=i) for i in range(3)] \
            + [_req(12 + i, temperature=0.9, seed=i, top_p=0.8) for i in range(3)]
    without = _drain(eng, crowd() + [_req(100, **kw)])
    assert eng.logprob_steps == 0 and without[100].out_logprobs is None
    alone = _drain(eng, [_req(100, logprobs=3, **kw)])[100]
    assert eng.logprob_steps > 0
    among = _drain(eng, crowd() + [_req(100, logprobs=3, **kw)])
    moved = _drain(eng, [_req(200 + i) for i in range(5)] + [_req(100, logprobs=0, **kw)])[100]
    torch.cuda.synchronize()
    assert len(alone.out_tokens) == 6 and alone.out_logprobs.shape == (6,) and alone.out_top_ids.shape == (6, 5)
    assert _bits(alone) == _bits(among[100]) == _bits(moved)
    assert np.array_equal(alone.out_tokens, without[100].out_tokens)
    for i in range(15):
        assert np.array_equal(among[i].out_tokens, without[i].out_tokens), i
        assert among[i].out_logprobs is None
    assert np.isfinite(alone.out_logprobs).all() and (alone.out_logprobs <= 0).all()
    assert (alone.out_top_logprobs[:, 1:] <= alone.out_top_logprobs[:, :-1]).all()
    if not kw:
        # a greedy token is a most likely one (the fused head compares the fp32 accumulators, so among
        # columns whose bf16 logits tie it need not be the lowest: the value is compared, not the id)
        assert np.array_equal(alone.out_top_logprobs[:, 0].view(np.uint32), alone.out_logprobs.view(np.uint32))
