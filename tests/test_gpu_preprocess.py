"""The classifier and summarise kernels (scan_rows, embed_pool, classify_head,
summarise_project, salient_topk) against the exact constructions and the
float64 references of preprocess_cases.py.  Every assertion is an equality or
a bound derived in the docstring of the check it calls.

Run on the MI355X box: ``pytest -m gpu tests/test_gpu_preprocess.py``.
"""
import numpy as np
import pytest
import torch

import preprocess_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(a):
    """uint32 numpy array -> int32 device tensor of the same bits."""
    return _dev(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def k():
    from llm_message_queue_amd import _native
    return _native.require_hipops()


# ----------------------------------------------------------------------------- scan_rows
@pytest.mark.parametrize("stride", PC.SCAN_STRIDES)
@pytest.mark.parametrize("B", PC.SCAN_B)
def test_scan_rows_is_the_integer_prefix_sum(k, B, stride):
    n = PC.scan_counts(B)
    tab = np.full((max(B, 1), stride), -99, dtype=np.int32)
    col = 5 if stride > 1 else 0
    tab[:B, col] = n
    d_tab = _dev(tab)
    row_off = torch.full((B + 2,), PC.PRED_SENTINEL, dtype=torch.int32, device=DEV)
    k.scan_rows(d_tab.data_ptr() + 4 * col, stride, B, row_off.data_ptr(), _stream())
    torch.cuda.synchronize()
    want = np.concatenate([[0], np.cumsum(n.astype(np.int64))]).astype(np.int32)
    got = row_off.cpu().numpy()
    assert np.array_equal(got[:B + 1], want)
    assert got[B + 1] == PC.PRED_SENTINEL


# ----------------------------------------------------------------------------- embed_pool
def _embed(k, c, E, W1t, b1, mode, slack_tiles=3):
    """One embed_pool launch: ``pooled`` [B][H] as numpy, after asserting that
    the NaN rows behind it are untouched.  ``rows_upper`` overshoots the real
    total by ``slack_tiles`` tiles and a bit."""
    B, L, H = c.B, c.L, c.H
    hashes = _u32(c.hashes)
    assert hashes.shape == (B, L) and E.shape[0] == c.V and W1t.shape == (H, PC.D)
    stats = np.full((B, 16), -99, dtype=np.int32)
    stats[:, 5] = c.ntok
    d_stats = _dev(stats)
    row_off = _dev(np.concatenate([[0], np.cumsum(c.ntok)]).astype(np.int32))
    pooled = torch.full((B + 2, H), float("nan"), dtype=torch.float32, device=DEV)
    pooled[:B] = 0
    rows_upper = c.total + slack_tiles * PC.TM + 5
    lds = mode == "lds"
    k.embed_pool(hashes.data_ptr(), L, 0 if lds else row_off.data_ptr(), B, rows_upper, E.data_ptr(), c.V,
                 W1t.data_ptr(), b1.data_ptr(), H, pooled.data_ptr(), _stream(),
                 d_stats.data_ptr() + 4 * 5 if lds else 0, 16 if lds else 0)
    torch.cuda.synchronize()
    out = pooled.cpu().numpy()
    assert np.isnan(out[B:]).all()
    return out[:B]


@pytest.mark.parametrize("mode", ["lds", "global"])
@pytest.mark.parametrize("name,V,H,L", PC.EMBED_CASES, ids=[f"{c[0]}-V{c[1]}-H{c[2]}-L{c[3]}" for c in PC.EMBED_CASES])
def test_embed_pool_exact(k, name, V, H, L, mode):
    """Bit for bit: the in-block scan path and the global row_off path both
    equal the reference, so they equal each other."""
    c = PC.embed_case(name, V, H, L)
    ref = PC.embed_exact_ref(c)
    got = _embed(k, c, c.E.to(DEV), c.W1t.to(DEV), c.b1.to(DEV), mode)
    bad = PC.embed_exact_check(got, ref)
    assert bad == 0, (bad, np.argwhere(PC.bits(got) != PC.bits(ref.main))[:8])
    assert (got[c.ntok == 0] == 0).all()


def test_embed_pool_gelu_probe(k):
    """``pooled`` of the probe is the device's ``gelu_tanh(z)`` alone: finite,
    z or a zero for |z| >= 16, and within ``gelu_bound`` of float64."""
    c = PC.gelu_probe_case()
    for mode in ("lds", "global"):
        got = _embed(k, c, c.E.to(DEV), c.W1t.to(DEV), c.b1.to(DEV), mode)
        need = PC.expf_ulp24_needed(got, c.z)
        ok, worst = PC.gelu_check(got, c.z)
        print(f"PREPROCESS_ULP gelu probe {mode}: worst |err| {worst:.3f} * |z| 2^-24, "
              f"exp error needed {need:.3f} * 2^-24 (allowed {PC.EXPF_ULP24})")
        assert ok, (worst, need)


def _max_parts(ntok):
    """The largest number of tiles a message of the batch spans."""
    off = np.concatenate([[0], np.cumsum(ntok)])
    return max((off[m + 1] - 1) // PC.TM - off[m] // PC.TM + 1 for m in range(len(ntok)) if ntok[m])


_REFS = {}


def _general_ref(name, L, w):
    """A random case under the weights ``w`` with its float64 reference and bound, computed once for both modes."""
    if (name, L) not in _REFS:
        c = PC.with_weights(PC.embed_random_case(name, L, vocab=w.vocab, hidden=w.hidden), w.E, w.W1t, w.b1)
        _REFS[name, L] = (c,) + PC.embed_general_ref(c)
    return _REFS[name, L]


@pytest.fixture(scope="module")
def prod_weights():
    from llm_message_queue_amd.ops.text import ClassifierWeights
    return ClassifierWeights(device=DEV)


@pytest.mark.parametrize("mode", ["lds", "global"])
@pytest.mark.parametrize("name,L", [("straddle", 64), ("parts150", 160), ("zeros_run", 64), ("rand255", 64)])
def test_embed_pool_random_weights_every_element(k, prod_weights, name, L, mode):
    """Production weights: every element of every message inside the bound of ``embed_general_ref``."""
    w = prod_weights
    c, ref, bound = _general_ref(name, L, w)
    got = _embed(k, c, w.E, w.W1t, w.b1, mode)
    ok, worst = PC.embed_general_check(got, ref, bound)
    print(f"PREPROCESS_ULP embed_pool random {name} {mode}: worst err / bound {worst:.3f}, "
          f"largest bound {bound.max():.2e}")
    assert ok, worst
    assert (got[c.ntok == 0] == 0).all()


def test_text_pipeline_pooled_logits_pred_every_message():
    """Production weights through ``TextPipeline.run``: every element of
    ``pooled`` inside the derived bound, and ``pred`` equal to the argmax of
    the float64 product of the kernel's own ``pooled`` wherever its top-two
    margin exceeds twice ``gamma_1024 sum |x||w|`` (``head_general_case``)."""
    from text_cases import _random_texts
    from llm_message_queue_amd.ops.text import TextPipeline
    from llm_message_queue_amd.preprocess import oracle
    from llm_message_queue_amd.utils.config import PreprocessorConfig
    texts = _random_texts(200, seed=11) + ["", "one", "two words"] + ["w " * 200]
    L = 64
    pipe = TextPipeline(PreprocessorConfig(max_tokens=L), device=DEV)
    res = pipe.run(texts, oracle.default_patterns(), classify=True, keep_device=True)
    w = pipe.weights
    ntok = res.stats[:, 5].astype(np.int32)
    assert ntok.max() <= L and (ntok == 0).any() and _max_parts(ntok) >= 2
    c = PC.SimpleNamespace(name="texts", V=w.vocab, H=w.hidden, L=L, B=len(texts), ntok=ntok,
                           hashes=res.hashes.cpu().numpy().view(np.uint32), exact=False, total=int(ntok.sum()))
    ref, bound = PC.embed_general_ref(PC.with_weights(c, w.E, w.W1t, w.b1))
    got = res.pooled.cpu().numpy()
    ok, worst = PC.embed_general_check(got, ref, bound)
    print(f"PREPROCESS_ULP embed_pool texts: worst err / bound {worst:.3f}")
    assert ok, worst
    assert (got[ntok == 0] == 0).all()
    # pred is the argmax of logits the float64 product of the same pooled rows decides
    x64, w64 = got.astype(np.float64), w.W2.double().cpu().numpy()
    lref = x64 @ w64 + w.b2.double().cpu().numpy()
    lbound = PC.gamma(1024) * (np.abs(x64) @ np.abs(w64))
    top = np.sort(lref[:, :4], axis=1)
    decided = (top[:, 3] - top[:, 2]) > 2 * lbound[:, :4].max(axis=1)
    assert decided.mean() > 0.95
    assert np.array_equal(res.pred[decided], (1 + np.argmax(lref[:, :4], axis=1))[decided])


# ----------------------------------------------------------------------------- classify_head
def _head(k, x, W2, b2):
    B, H = x.shape
    logits = torch.full((B + 1, 8), float("nan"), dtype=torch.float32, device=DEV)
    pred = torch.full((B + 1,), PC.PRED_SENTINEL, dtype=torch.int32, device=DEV)
    dx, dw, db = _dev(x), _dev(W2), _dev(b2)
    k.classify_head(dx.data_ptr(), B, H, dw.data_ptr(), db.data_ptr(), logits.data_ptr(), pred.data_ptr(), _stream())
    torch.cuda.synchronize()
    lg, pr = logits.cpu().numpy(), pred.cpu().numpy()
    assert np.isnan(lg[B]).all() and pr[B] == PC.PRED_SENTINEL
    return lg[:B], pr[:B]


@pytest.mark.parametrize("H", PC.HEAD_H)
@pytest.mark.parametrize("B", PC.HEAD_B)
def test_classify_head_exact(k, B, H):
    """All eight logit columns bit for bit, ``pred`` with the lowest tied column."""
    c = PC.head_case(B, H)
    ref = PC.head_exact_ref(c)
    logits, pred = _head(k, c.x, c.W2, c.b2)
    assert PC.same_bits(logits, ref[0]), np.argwhere(logits != ref[0])[:8]
    assert np.array_equal(pred, ref[1]), np.flatnonzero(pred != ref[1])[:8]


@pytest.mark.parametrize("B,H", [(1041, 1024), (1024, 256), (5, 1024)])
def test_classify_head_random(k, B, H):
    c = PC.head_general_case(B, H)
    logits, pred = _head(k, c.x, c.W2, c.b2)
    err = np.abs(logits.astype(np.float64) - c.ref)
    print(f"PREPROCESS_ULP classify_head random B={B} H={H}: worst err / bound {(err / c.bound).max():.4f}, "
          f"{(~c.decided).sum()} of {B} rows undecided")
    assert np.isfinite(logits).all() and (err <= c.bound).all()
    assert np.array_equal(pred[c.decided], c.pred[c.decided])
    assert ((pred >= 1) & (pred <= 4)).all()


@pytest.mark.parametrize("n", [37, 1500])
def test_one_call_path_exact(k, n):
    """Exact weights installed in a ``TextPipeline``: ``pooled`` of the
    text_batch path (reused buffers, run twice) and of the per-launch path
    equal the reference bit for bit; the logits equal a per-launch
    classify_head of the same rows, and the float64 logits wherever those are
    exact (power-of-two token counts); ``pred`` follows."""
    from llm_message_queue_amd.ops.text import ClassifierWeights, TextPipeline
    from llm_message_queue_amd.preprocess import oracle
    from llm_message_queue_amd.utils.config import PreprocessorConfig
    L, V, H = 128, 1024, 1024
    texts = [" ".join(f"w{i}_{j}" for j in range(1 + (i * 7) % 90)) for i in range(n)]
    texts[1], texts[2] = "", "Is this URGENT?"
    pipe = TextPipeline(PreprocessorConfig(max_tokens=L, vocab_buckets=V, hidden_dim=H), device=DEV)
    xw = PC.exact_pipeline_weights(V, H)
    with torch.cuda.stream(pipe.stream):
        w = pipe.weights = ClassifierWeights(vocab=V, hidden=H, device=DEV)
        w.E, w.W1t, w.b1, w.W2, w.b2 = xw.E.to(DEV), xw.W1t.to(DEV), xw.b1.to(DEV), xw.W2.to(DEV), xw.b2.to(DEV)
    pipe.stream.synchronize()
    pats = oracle.default_patterns()
    per = pipe.run(texts, pats, classify=True, keep_device=True, prompt_cap=32)
    ntok = per.stats[:, 5].astype(np.int32)
    c = PC.text_case(xw, per.hashes.cpu().numpy().view(np.uint32), ntok, L)
    ref = PC.embed_exact_ref(c)
    per_pooled = per.pooled.cpu().numpy()
    assert PC.embed_exact_check(per_pooled, ref) == 0
    pow2 = (ntok > 0) & ((ntok & (ntok - 1)) == 0) | (ntok == 0)
    lref, exact = PC.exact_logits(xw, ref.main.astype(np.float64))
    pow2 &= exact
    assert pow2.sum() >= 3 and (~pow2).any()
    pref = (1 + np.argmax(lref[:, :4], axis=1)).astype(np.int32)
    assert np.array_equal(per.pred[pow2], pref[pow2])
    for _ in range(2):                                     # the workspace is reused
        got = pipe.run(texts, pats, classify=True, keep_device=False, prompt_cap=32)
        pooled = pipe._ws["pooled"][:n].clone()
        logits = pipe._ws["logits"][:n].cpu().numpy()
        torch.cuda.synchronize()
        pn = pooled.cpu().numpy()
        assert PC.embed_exact_check(pn, ref) == 0
        lg2 = torch.empty((n, 8), dtype=torch.float32, device=DEV)
        pr2 = torch.empty(n, dtype=torch.int32, device=DEV)
        k.classify_head(pooled.data_ptr(), n, H, w.W2.data_ptr(), w.b2.data_ptr(), lg2.data_ptr(), pr2.data_ptr(),
                        _stream())
        torch.cuda.synchronize()
        assert PC.same_bits(logits, lg2.cpu().numpy()) and np.array_equal(got.pred, pr2.cpu().numpy())
        assert PC.same_bits(logits[pow2], lref[pow2].astype(f32)) and np.array_equal(got.pred[pow2], pref[pow2])
        assert np.array_equal(got.pred, 1 + np.argmax(logits[:, :4], axis=1))
        same = (PC.bits(pn) == PC.bits(per_pooled)).all(axis=1)       # all but a rare three-part message
        assert same.mean() > 0.9 and np.array_equal(got.pred[same], per.pred[same])


# ----------------------------------------------------------------------------- summarise_project
def _project(c):
    from llm_message_queue_amd.ops.summarise import Summariser
    sm = Summariser(dim=PC.SM_DS, hidden=PC.SM_H, alpha=c.alpha, device=DEV)
    sm.Pt = c.Pt.to(DEV)
    pooled = torch.full((c.M + 3, PC.SM_H), float("nan"), dtype=torch.float32, device=DEV)
    pooled[:c.M] = _dev(c.rows)
    state = torch.full((c.C + 1, PC.SM_DS), PC.STATE_SENTINEL, dtype=torch.float32, device=DEV)
    state[:c.C] = _dev(c.state)
    sm.project(pooled, _dev(c.seg), state[:c.C], _dev(c.first))
    torch.cuda.synchronize()
    out = state.cpu().numpy()
    assert (out[c.C] == PC.STATE_SENTINEL).all()
    return out[:c.C]


@pytest.mark.parametrize("alpha", [0.5, 0.75])
@pytest.mark.parametrize("C", PC.SUMMARISE_C)
def test_summarise_project_exact(C, alpha):
    c = PC.summarise_case(C, alpha)
    ref, bound = PC.summarise_ref(c)
    got = _project(c)
    assert PC.summarise_check(got, ref, bound, True)[0], np.argwhere(got != ref.astype(f32))[:8]


@pytest.mark.parametrize("C,alpha", [(17, 0.6), (33, 0.8)])
def test_summarise_project_random(C, alpha):
    c = PC.summarise_random_case(C, alpha)
    ref, bound = PC.summarise_ref(c)
    got = _project(c)
    ok, worst = PC.summarise_check(got, ref, bound, False)
    print(f"PREPROCESS_ULP summarise_project random C={C}: worst err / bound {worst:.3f}, largest bound {bound.max():.2e}")
    assert ok, worst


# ----------------------------------------------------------------------------- salient_topk
@pytest.mark.parametrize("name", PC.SALIENT_CASES)
def test_salient_topk(k, name):
    c = PC.salient_case(name)
    ref = PC.salient_ref(c.hashes, c.ntok, c.seg, c.stop, c.K)
    tab = _dev(c.tab)
    oh = torch.full((c.C + 1, c.K), PC.PRED_SENTINEL, dtype=torch.int32, device=DEV)
    oc = torch.full((c.C + 1, c.K), PC.PRED_SENTINEL, dtype=torch.int32, device=DEV)
    ov = torch.full((c.C + 1,), PC.PRED_SENTINEL, dtype=torch.int32, device=DEV)
    hashes, seg, stop = _u32(c.hashes), _dev(c.seg), _u32(c.stop)
    k.salient_topk(hashes.data_ptr(), c.L, tab.data_ptr() + 4 * c.col, c.stride, seg.data_ptr(), c.C,
                   stop.data_ptr(), len(c.stop), c.K, oh.data_ptr(), oc.data_ptr(), ov.data_ptr(), _stream())
    torch.cuda.synchronize()
    gh, gc, gv = oh.cpu().numpy(), oc.cpu().numpy(), ov.cpu().numpy()
    assert (gh[c.C] == PC.PRED_SENTINEL).all() and (gc[c.C] == PC.PRED_SENTINEL).all() and gv[c.C] == PC.PRED_SENTINEL
    assert np.array_equal(gv[:c.C], ref[2]), (gv, ref[2])
    assert PC.salient_check((gh[:c.C].view(np.uint32), gc[:c.C], gv[:c.C]), ref)


# ----------------------------------------------------------------------------- refused arguments
def test_bad_arguments_are_refused_before_any_launch(k):
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, s = z.data_ptr(), _stream()
    with pytest.raises(ValueError):
        k.scan_rows(p, 0, 4, p, s)                                        # stride 0
    with pytest.raises(ValueError):
        k.embed_pool(p, 4, p, 1, 1, p, 48, p, p, 256, p, s, 0, 0)         # vocab no power of two
    with pytest.raises(ValueError):
        k.embed_pool(p, 4, p, 1, 1, p, 64, p, p, 200, p, s, 0, 0)         # hidden no multiple of 256
    with pytest.raises(ValueError):
        k.embed_pool(p, 4, 0, 1, 1, p, 64, p, p, 256, p, s, 0, 0)         # neither row_off nor ntok_src
    with pytest.raises(ValueError):
        k.classify_head(p, 1, 200, p, p, p, p, s)
    with pytest.raises(ValueError):
        k.summarise_project(p, p, 1, p, 0.5, p, p, 512, 256, s)
    with pytest.raises(ValueError):
        k.salient_topk(p, 4, p, 1, p, 1, p, 0, 65, p, p, p, s)
