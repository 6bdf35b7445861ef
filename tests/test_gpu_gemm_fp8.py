"""The 256x256-tile GEMM over FP8 (e4m3) weight codes (W8A16), on the GPU:
``ops.gemm.gemm_fp8`` / ``gemm_swiglu_fp8`` / ``gemm_residual_fp8``.  From the
smallest launch upward: an exact identity probe (every code in every byte lane
and K slot), bit-equality with the bf16 tile kernel over the decoded weights
(power-of-two scales), the fp32 product's bounds with arbitrary scales,
determinism and containment, the refusals, the model's ``quant`` forwards past
the ``fp8_plan`` thresholds and the engine's ``micro_weights = "fp8"`` mode
with a prefill-carrying micro-forward."""
import functools

import numpy as np
import pytest
import torch

from llm_message_queue_amd import _native
from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import quant as Q

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _table():
    return torch.from_numpy(Q.TABLE).to(DEV)


@functools.lru_cache(maxsize=None)
def _codes(N, K, pow2=False):
    """e4m3 codes [N][K] of Gaussian weights (std 0.02), quantised once per
    shape, and their column scales: the quantiser's power of two times a
    random factor in [0.5, 2) (the kernel takes any fp32 scale), or the power
    of two itself."""
    g = torch.Generator(device=DEV).manual_seed(N + K)
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(torch.bfloat16)
    codes, scale = G.quantize_rows(w)
    if not pow2:
        scale = (scale * (0.5 + 1.5 * torch.rand(N, generator=g, device=DEV))).contiguous()
    return codes, scale


def _rand_q(M, K, N, seed=0, pow2=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    return (x,) + _codes(N, K, pow2)


def _weights(codes, scale):
    return _table()[codes.long()] * scale[:, None]            # fp32 [N][K]


def _row_scale(M, seed):
    """[row_scale_len(M)] in [0.5, 1.5): the kernel reads whole 256-row tiles."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(G.row_scale_len(M), generator=g, device=DEV) + 0.5


def _splits(K):
    """The split_cus values a K takes: whole, and every tile split where the
    kernel can halve K (K % 256 == 0, K >= 512)."""
    return (0, 64) if K % 256 == 0 and K >= 512 else (0,)


def _split_counters():
    live, _ = G._scratch_entry(torch.device("cuda", torch.cuda.current_device()),
                               torch.cuda.current_stream().cuda_stream, "split")
    return live[1] if live else None


# ---------------------------------------------------------------------- 1. identity probe
def _probe_codes(K):
    """[256][K]: row n is a fixed permutation of the 254 finite codes and two
    zeros, rotated by n (and by another 101 in the second K half), so every
    code visits every byte position and every K slot."""
    finite = np.array([c for c in range(256) if c & 0x7F != 0x7F] + [0, 0], dtype=np.int64)
    perm = finite[np.random.default_rng(7).permutation(256)]
    n, k = np.arange(256)[:, None], np.arange(K)[None, :]
    return torch.from_numpy(perm[(k + n + 101 * (k // 256)) % 256].astype(np.uint8)).to(DEV)


def test_identity_probe_is_exact():
    """x = I: out[m][n] is one product decode(codes[n][m]) * col_scale[n] and
    one rounding -- exact by construction."""
    codes = _probe_codes(256)
    cs = (torch.rand(256, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV) * 1.5 + 0.5).contiguous()
    x = torch.eye(256, device=DEV).to(torch.bfloat16)
    out = G.gemm_fp8(x, codes, cs)
    want = (_table()[codes.long()] * cs[:, None]).t().to(torch.bfloat16)
    bad = (out != want).nonzero()
    print("identity probe mismatches:", bad[:8].tolist())
    assert torch.equal(out, want)


@pytest.mark.parametrize("half", [0, 1])
def test_identity_probe_split_k(half):
    """K = 512, both K halves of the split tile: x = [I | 0] and [0 | I]."""
    codes = _probe_codes(512)
    cs = (torch.rand(256, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV) * 1.5 + 0.5).contiguous()
    x = torch.zeros(256, 512, device=DEV, dtype=torch.bfloat16)
    x[:, 256 * half:256 * half + 256] = torch.eye(256, device=DEV).to(torch.bfloat16)
    assert G.split_all(256, 256, 512, 64) == 0
    out = G.gemm_fp8(x, codes, cs, split_cus=64)
    want = (_table()[codes[:, 256 * half:256 * half + 256].long()] * cs[:, None]).t().to(torch.bfloat16)
    assert torch.equal(out, want)
    assert int(_split_counters().abs().sum()) == 0


# ---------------------------------------------------------------------- 2. the bf16 kernel on decoded weights
def _equal_on_decoded(M, N, K, split_cus):
    x, codes, cs = _rand_q(M, K, N, seed=M + N + K, pow2=True)
    w = Q.dequantize(codes, cs)
    r = _row_scale(M, M)
    a = G.gemm_fp8(x, codes, cs, row_scale=r, split_cus=split_cus)
    b = G.gemm(x, w, row_scale=r, split_cus=split_cus)
    assert torch.equal(a, b), "store"
    idx = G.swiglu_perm_index(N // 2, DEV)
    a = G.gemm_swiglu_fp8(x, codes.index_select(0, idx).contiguous(), cs.index_select(0, idx).contiguous(),
                          row_scale=r, split_cus=split_cus)
    b = G.gemm_swiglu(x, w.index_select(0, idx).contiguous(), row_scale=r, split_cus=split_cus)
    assert torch.equal(a, b), "swiglu"
    res = torch.randn(M, N, generator=torch.Generator(device=DEV).manual_seed(K), device=DEV).to(torch.bfloat16)
    a, b = res.clone(), res.clone()
    G.gemm_residual_fp8(x, codes, cs, a, split_cus=split_cus)
    G.gemm_residual(x, w, b, split_cus=split_cus)
    assert torch.equal(a, b), "residual"
    assert not torch.equal(a, res)


@pytest.mark.parametrize("M", [1, 127, 128, 129, 255, 256, 257, 300])
@pytest.mark.parametrize("N,K", [(256, 128), (256, 256), (512, 384), (512, 512), (768, 768)])
def test_equals_the_bf16_tile_kernel_on_decoded_weights(M, N, K):
    """Power-of-two scales: every decoded weight is a bf16 number and a given
    k enters the same MFMA step and operand slot in both kernels, so the three
    epilogues are bit-equal, whole and (K = 512, 768) with every tile split.
    The K values: the drain alone, one loop trip, two trips."""
    assert G.RESID_EPI == G.EPI_RESID_LDS
    for split_cus in _splits(K):
        _equal_on_decoded(M, N, K, split_cus)


def test_equals_the_bf16_tile_kernel_whole_and_split_tiles_mixed():
    """(M, N, split_cus) = (256, 2304, 8): eight whole tiles and one split."""
    assert G.split_all(256, 2304, 512, 8) is None and G.split_plan(256, 2304, 512, 8) == 8
    _equal_on_decoded(256, 2304, 512, 8)


# ---------------------------------------------------------------------- 3. bounds against the fp32 product
@pytest.mark.parametrize("split_cus", [0, 64])
@pytest.mark.parametrize("M", [1, 129, 257, 300])
@pytest.mark.parametrize("N,K", [(512, 512), (1024, 1792)])
def test_matches_fp32(M, N, K, split_cus):
    """Arbitrary column scales and a row scale in [0.5, 1.5): the bounds of
    ``test_gemm.py`` / ``test_gpu_skinny_fp8.py`` for these epilogues."""
    x, codes, cs = _rand_q(M, K, N, seed=3 * M + N + K)
    wf = _weights(codes, cs)
    r = _row_scale(M, M + 1)
    ref = (x.float() * r[:M, None]) @ wf.t()
    out = G.gemm_fp8(x, codes, cs, row_scale=r, split_cus=split_cus)
    err = (out.float() - ref).abs().max().item()
    print(f"store M={M} N={N} K={K} split={split_cus}: err {err:.4g} of max {ref.abs().max().item():.4g}")
    assert err <= 0.01 * ref.abs().max().item() + 1e-3
    res = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    want = res.float() + x.float() @ wf.t()
    got = res.clone()
    G.gemm_residual_fp8(x, codes, cs, got, split_cus=split_cus)
    err = (got.float() - want).abs().max().item()
    print(f"residual: err {err:.4g} of max {want.abs().max().item():.4g}")
    assert err <= 0.01 * want.abs().max().item() + 1e-2
    F = N // 2
    sref = G.swiglu_reference((x.float() * r[:M, None]).to(torch.bfloat16), wf).float()
    idx = G.swiglu_perm_index(F, DEV)
    act = G.gemm_swiglu_fp8(x, codes.index_select(0, idx).contiguous(), cs.index_select(0, idx).contiguous(),
                            row_scale=r, split_cus=split_cus)
    err = (act.float() - sref).abs().max().item()
    print(f"swiglu: err {err:.4g} of max {sref.abs().max().item():.4g}")
    assert err <= 0.02 * sref.abs().max().item() + 1e-3


# ---------------------------------------------------------------------- 4. determinism and containment
@pytest.mark.parametrize("split_cus", [0, 64])
@pytest.mark.parametrize("M", [129, 300])
def test_deterministic_and_contained(M, split_cus):
    """Two residual launches from one start agree; nothing past the [M][N]
    output is written (8 sentinel rows and 256 more elements follow it);
    NaN rows behind x[M:] never reach it; the split counters are left zero."""
    N, K = 512, 512
    _, codes, cs = _rand_q(M, K, N, seed=11)
    xb = torch.full((M + 16, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    xb[:M] = torch.randn(M, K, generator=torch.Generator(device=DEV).manual_seed(M), device=DEV).to(torch.bfloat16)
    x = xb[:M]
    start = torch.randn(M, N, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV).to(torch.bfloat16)
    outs = []
    for _ in range(2):
        buf = torch.full(((M + 8) * N + 256,), 777.0, dtype=torch.bfloat16, device=DEV)
        res = buf[:M * N].view(M, N)
        res.copy_(start)
        G.gemm_residual_fp8(x, codes, cs, res, split_cus=split_cus)
        assert bool((buf[M * N:] == 777.0).all())
        assert bool(torch.isfinite(res.float()).all())
        outs.append(res.clone())
    assert torch.equal(outs[0], outs[1])
    for fn in (G.gemm_fp8, G.gemm_swiglu_fp8):
        Nout = N if fn is G.gemm_fp8 else N // 2
        buf = torch.full(((M + 8) * Nout + 256,), 777.0, dtype=torch.bfloat16, device=DEV)
        out = buf[:M * Nout].view(M, Nout)
        fn(x, codes, cs, out=out, split_cus=split_cus)
        assert bool((buf[M * Nout:] == 777.0).all())
        assert bool(torch.isfinite(out.float()).all())
    if split_cus:
        assert int(_split_counters().abs().sum()) == 0


# ---------------------------------------------------------------------- 5. refusals
def test_refuses_bad_arguments():
    x, codes, cs = _rand_q(4, 512, 256, seed=1)
    out = torch.empty(4, 256, dtype=torch.bfloat16, device=DEV)
    bad = (ValueError, TypeError)
    G.gemm_fp8(x, codes, cs, out=out)
    good = out.clone()
    with pytest.raises(bad):
        G.gemm_fp8(x, codes.view(torch.int8), cs, out=out)                        # dtype
    with pytest.raises(bad):
        G.gemm_fp8(x, codes.t().contiguous().t(), cs, out=out)                    # not contiguous
    pad = torch.zeros(256 * 512 + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(bad):
        G.gemm_fp8(x, pad[1:1 + 256 * 512].view(256, 512), cs, out=out)           # misaligned
    with pytest.raises(bad):
        G.gemm_fp8(x, codes, cs[:128], out=out)                                   # short
    with pytest.raises(bad):
        G.gemm_fp8(x, codes, cs.double(), out=out)
    with pytest.raises(bad):
        G.gemm_fp8(x, codes, cs.cpu(), out=out)
    with pytest.raises(bad):                                                      # N % 256
        G.gemm_fp8(x, codes[:128].contiguous(), cs[:128].contiguous(),
                   out=torch.empty(4, 128, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(bad):                                                      # K % 128
        G.gemm_fp8(x[:, :192].contiguous(), codes[:, :192].contiguous(), cs, out=out)
    with pytest.raises(bad):
        G.gemm_fp8(x, codes, cs, out=torch.empty(4, 512, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(bad):
        G.gemm_swiglu_fp8(x, codes, cs, out=out)                                  # wants [4][128]
    with pytest.raises(bad):
        G.gemm_residual_fp8(x, codes, cs, out, row_scale=torch.ones(256, device=DEV))
    # a split request with K = 384: the launcher refuses the workspace
    k = _native.require_hipops()
    x3, c3 = x[:, :384].contiguous(), codes[:, :384].contiguous()
    ws = torch.empty(512 * 128, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(bad):
        k.gemm_fp8w(x3.data_ptr(), c3.data_ptr(), cs.data_ptr(), out.data_ptr(), 4, 256, 384, G.EPI_STORE, stream, 8,
                    0, 0, ws.data_ptr(), cnt.data_ptr())
    with pytest.raises(bad):                                                      # residual + row scale, natively
        k.gemm_fp8w(x.data_ptr(), codes.data_ptr(), cs.data_ptr(), out.data_ptr(), 4, 256, 512, G.EPI_RESID_LDS,
                    stream, 8, torch.ones(256, device=DEV).data_ptr(), 0, 0, 0)
    with pytest.raises(bad):                                                      # an epilogue it does not have
        k.gemm_fp8w(x.data_ptr(), codes.data_ptr(), cs.data_ptr(), out.data_ptr(), 4, 256, 512, 3, stream, 8,
                    0, 0, 0, 0)
    with pytest.raises(bad):                                                      # null column scales
        k.gemm_fp8w(x.data_ptr(), codes.data_ptr(), 0, out.data_ptr(), 4, 256, 512, G.EPI_STORE, stream, 8,
                    0, 0, 0, 0)
    out.zero_()
    G.gemm_fp8(x, codes, cs, out=out)                                             # a good launch still works
    assert torch.equal(out, good)


# ---------------------------------------------------------------------- 6. the model
THRESHOLD = 65


@pytest.fixture
def low_thresholds(monkeypatch):
    """Every GEMM class on the tile kernel from 65 rows (the lowest legal
    threshold), whatever the measured defaults are; counts the launches."""
    for name in ("FP8_TILE_MIN_M_SMALL", "FP8_TILE_MIN_M_CHIP"):
        monkeypatch.setattr(G, name, {g: THRESHOLD for g in G.FP8_GEMMS})
    counts = {"tile": 0, "skinny_fp8": 0, "bf16": 0}

    def counted(name, kind):
        fn = getattr(G, name)

        def wrapper(*a, **kw):
            counts[kind] += 1
            return fn(*a, **kw)
        monkeypatch.setattr(G, name, wrapper)

    for name in ("gemm_fp8", "gemm_swiglu_fp8", "gemm_residual_fp8"):
        counted(name, "tile")
    counted("skinny_fp8", "skinny_fp8")
    for name in ("gemm", "gemm_swiglu", "gemm_residual", "gemm_residual_rms", "qkv_rope", "skinny"):
        counted(name, "bf16")
    return counts


@functools.lru_cache(maxsize=None)
def _stubs():
    from llm_message_queue_amd.models.llama_stub import QUANT_NAMES, LlamaConfig, LlamaStub
    cfg = LlamaConfig.tiny()
    m = LlamaStub(cfg, slots=8, max_ctx=64, device=DEV, impl="hip", seed=5, small_weights="fp8")
    ref = LlamaStub(cfg, slots=8, max_ctx=64, device=DEV, impl="hip", seed=5)
    for L, Lr in zip(m.layers, ref.layers):
        for k in QUANT_NAMES:
            Lr[k] = Q.dequantize(*L["fp8"][k])
    return cfg, m, ref


@pytest.mark.parametrize("T", [THRESHOLD - 1, THRESHOLD, 300])
def test_quant_forward_takes_the_tile_kernel_from_the_threshold(T, low_thresholds):
    """``hidden(quant=True)`` against a bf16 stub holding the decoded weights
    (the bound of ``test_quant_forward_matches_the_bf16_path_on_decoded_weights``),
    on a CU partition's plan and the whole chip's.  The sampled rows are few,
    so above the threshold the last layer's pruned block runs on the skinny
    kernel while the rest runs on tiles: one forward mixes both."""
    cfg, m, ref = _stubs()
    counts = low_thresholds
    g = torch.Generator(device=DEV).manual_seed(T)
    tok = torch.randint(0, cfg.vocab, (T,), generator=g, device=DEV)
    pos = (torch.arange(T, device=DEV, dtype=torch.int32) % 60).contiguous()
    slot = (torch.arange(T, device=DEV, dtype=torch.int32) // 60).contiguous()
    samp = torch.tensor(sorted(set(list(range(59, T, 60)) + [T - 1])), device=DEV, dtype=torch.long)
    assert samp.numel() < THRESHOLD
    b = ref.hidden(tok, pos, slot, rows=samp, small_cus=64).float()
    for cus in (64, 0):
        for k in counts:
            counts[k] = 0
        a = m.hidden(tok, pos, slot, rows=samp, small_cus=cus, quant=True).float()
        err = (a - b).abs().max().item()
        print(f"T={T} cus={cus}: err {err:.4g} of max {a.abs().max().item():.4g}, launches {counts}")
        assert err <= 0.03 * a.abs().max().item()
        assert counts["bf16"] == 0
        if T < THRESHOLD:
            assert counts["tile"] == 0 and counts["skinny_fp8"] == 4 * cfg.layers
        else:
            # every layer's qkv, and o / gate-up / down of all but the pruned last block
            assert counts["tile"] == cfg.layers + 3 * (cfg.layers - 1)
            assert counts["skinny_fp8"] == 3


# ---------------------------------------------------------------------- 7. the engine
def test_engine_fp8_micro_forward_with_prefill_runs_on_tiles(low_thresholds):
    """``micro_weights = "fp8"`` on the CU partition with four simultaneous
    realtime prompts of 30 tokens: their first micro-forward carries 120 rows
    and takes the tile kernel; every request completes with its token count.
    (No token equality with another path: random weights make argmax ties.)"""
    from llm_message_queue_amd.backend.engine import BackendEngine, Request
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=16, max_ctx=64, token_budget=64, device=torch.device("cuda", 0),
                        impl="hip", seed=3, realtime_mode="micro", micro_slots=4, micro_stream="partition",
                        micro_weights="fp8")
    eng.warm_shapes([1, 8, 64])
    counts = low_thresholds
    counts["tile"] = 0
    rng = np.random.default_rng(4)
    reqs = [Request(req_id=i, prompt=rng.integers(0, 1000, size=30).astype(np.int32), gen_tokens=4, tier=0)
            for i in range(8)]
    got = {}
    pend = list(reqs)
    for _ in range(200):
        if not pend and not eng.active and not eng.queued_steps():
            break
        adm = eng.admit(pend)
        ids = {id(r) for r in adm}
        pend = [r for r in pend if id(r) not in ids]
        eng.launch()
        eng.pump_micro()
        for r in eng.finish(block=True).completed:
            got[r.req_id] = (r.out_tokens.tolist(), r.micro)
    eng.close()
    assert sorted(got) == list(range(8))
    assert all(len(ids) == 4 for ids, _ in got.values())
    assert sum(1 for _, micro in got.values() if micro) >= 4
    assert counts["tile"] > 0
