"""FP8 (e4m3) weights on the skinny GEMM (W8A16), on the GPU: the device
decode and quantiser against the host twin (``ops.quant``), ``skinny_fp8``
against the fp32 product of the decoded weights with the bf16 kernel's
tolerances (every code times a power-of-two scale is exactly a bf16 number,
so the arithmetic is the bf16 kernel's), the pipeline's edges, the model's
``quant`` forwards and the engine's ``micro_weights = "fp8"`` mode."""
import functools

import numpy as np
import pytest
import torch

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
    codes, scale = G.quantize_rows(w)                         # (bit-equal to the twin: its own test)
    if not pow2:
        scale = (scale * (0.5 + 1.5 * torch.rand(N, generator=g, device=DEV))).contiguous()
    return codes, scale


def _rand_q(M, K, N, seed=0, pow2=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    return (x,) + _codes(N, K, pow2)


def _weights(codes, scale):
    return _table()[codes.long()] * scale[:, None]            # fp32 [N][K]


def test_device_decode_is_the_table():
    """Every finite code in every byte position of a word (the other three
    bytes vary) decodes to the table's bf16 bits; the two NaN codes decode to
    a NaN."""
    c = np.arange(256, dtype=np.int64)
    words = np.zeros((4, 256, 4), dtype=np.uint8)
    for p in range(4):
        for j in range(4):
            words[p, :, j] = (c * 7 + 13 * j + p) & 0xFF
        words[p, :, p] = c
    codes = torch.from_numpy(words.reshape(-1)).to(DEV)
    got = G.fp8_decode(codes).cpu().numpy().view(np.uint16)
    want = torch.from_numpy(Q.TABLE)[codes.cpu().long()].to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = (codes.cpu().numpy() & 0x7F) == 0x7F
    bad = np.nonzero((got != want) & ~nan)[0]
    print("decode mismatches:", [(int(codes[i]), hex(got[i]), hex(want[i])) for i in bad[:8]])
    assert bad.size == 0                                      # the 254 finite codes: bit-equal
    # 0x7f / 0xff: a NaN (the payload is the converter's: the device gives
    # 0xffc0, torch's CPU float -> bf16 cast of the table's NaN 0xffff)
    assert nan.sum() == 32 and ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x7F) != 0).all()


@pytest.mark.parametrize("K", [4096, 14336])
def test_device_quantiser_is_the_twin(K):
    g = torch.Generator().manual_seed(K)
    w = (torch.randn(64, K, generator=g) * 0.02).to(torch.bfloat16)
    w[3, 17] = 20.0                                            # one 1000x outlier
    _, s = Q.quantize_rows_e4m3(w[4:5])
    w[5] = (torch.rand(K, generator=g) * 2.0 ** -7 * s[0]).to(torch.bfloat16)   # below 2^-6 * scale of row 4
    w[6] = 0
    w[7] = -w[8]                                               # signs
    w[9, :8] = torch.tensor([448.0, -448.0, 449.0, 2.0 ** -9, -2.0 ** -10, 3 * 2.0 ** -10, 0.0, -0.0])
    codes, scale = Q.quantize_rows_e4m3(w)
    dc, ds = G.quantize_rows(w.to(DEV))
    assert dc.dtype == torch.uint8 and ds.dtype == torch.float32
    assert torch.equal(ds.cpu(), scale)
    assert torch.equal(dc.cpu(), codes)
    with pytest.raises(ValueError):
        G.quantize_rows(torch.full((2, 8), float("inf"), dtype=torch.bfloat16, device=DEV))


@pytest.mark.parametrize("M", [1, 17, 64, 65, 129, 300])
@pytest.mark.parametrize("N,K", [(4096, 4096), (1024, 14336), (6144, 512)])
def test_skinny_fp8_matches_fp32(M, N, K):
    """Store and residual with a row scale and non-power-of-two column
    scales: the bounds of ``test_skinny_gemm_matches_fp32``."""
    x, codes, cs = _rand_q(M, K, N, seed=3 * M + N + K)
    wf = _weights(codes, cs)
    r = torch.rand(M, device=DEV) + 0.5
    ref = (x.float() * r[:, None]) @ wf.t()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    G.skinny_fp8(x, codes, cs, out, G.SK_STORE, row_scale=r, cus=32)
    err = (out.float() - ref).abs().max().item()
    print(f"store M={M} N={N} K={K}: err {err:.4g} of max {ref.abs().max().item():.4g}")
    assert err <= 0.01 * ref.abs().max().item() + 1e-3
    res = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    want = res.float() + x.float() @ wf.t()
    got = res.clone()
    G.skinny_fp8(x, codes, cs, got, G.SK_RESID, cus=32)
    assert (got.float() - want).abs().max().item() <= 0.01 * want.abs().max().item() + 1e-2
    again = res.clone()
    G.skinny_fp8(x, codes, cs, again, G.SK_RESID, cus=32)
    assert torch.equal(got, again)                            # deterministic (partials summed in order)


@pytest.mark.parametrize("M", [3, 64])
def test_skinny_fp8_swiglu_matches_fp32(M):
    """SwiGLU over the permuted codes: gate and up columns each with their
    own scale (the scales permuted with the rows); the bound of
    ``test_skinny_swiglu_matches_fp32``."""
    x, codes, cs = _rand_q(M, 4096, 2 * 1536, seed=40 + M)
    r = torch.rand(M, device=DEV) + 0.5
    ref = G.swiglu_reference((x.float() * r[:, None]).to(torch.bfloat16), _weights(codes, cs)).float()
    idx = G.swiglu_perm_index(1536, DEV)
    out = torch.empty(M, 1536, dtype=torch.bfloat16, device=DEV)
    G.skinny_fp8(x, codes.index_select(0, idx).contiguous(), cs.index_select(0, idx).contiguous(), out,
                 G.SK_SWIGLU, row_scale=r, cus=32)
    assert (out.float() - ref).abs().max().item() <= 0.02 * ref.abs().max().item() + 1e-3


def test_skinny_fp8_equals_the_bf16_kernel_on_decoded_weights():
    """With the quantiser's power-of-two scales the decoded weights are bf16
    numbers: the fp8 path and the bf16 kernel over them differ only by where
    the scale multiplies (an exact power of two), so the outputs are equal."""
    x, codes, cs = _rand_q(40, 4096, 1024, seed=5, pow2=True)
    w = Q.dequantize(codes, cs)
    a = torch.empty(40, 1024, dtype=torch.bfloat16, device=DEV)
    b = torch.empty_like(a)
    G.skinny_fp8(x, codes, cs, a, G.SK_STORE, cus=32)
    G.skinny(x, w, b, G.SK_STORE, cus=32)
    assert torch.equal(a, b)


@pytest.mark.parametrize("M", [m for mt in range(1, 9) for m in (16 * mt - 1, 16 * mt)])
def test_skinny_every_fragment_count_on_both_formats(M):
    """The launcher's dispatch over MT = 1 .. 8 row fragments (M = 16 MT - 1
    and 16 MT), on both weight formats: two column blocks and six pipeline
    steps without split-K, so the three- and the five-stage ring both wrap.
    The fp8 kernel equals the bf16 kernel on the decoded weights (power-of-two
    scales, as above), and that one holds the fp32 product's bound."""
    x, codes, cs = _rand_q(M, 768, 256, seed=M, pow2=True)
    w = Q.dequantize(codes, cs)
    a = torch.empty(M, 256, dtype=torch.bfloat16, device=DEV)
    b = torch.empty_like(a)
    G.skinny_fp8(x, codes, cs, a, G.SK_STORE, cus=32, splits=1)
    G.skinny(x, w, b, G.SK_STORE, cus=32, splits=1)
    assert torch.equal(a, b)
    ref = x.float() @ w.float().t()
    err = (b.float() - ref).abs().max().item()
    print(f"M={M}: err {err:.4g} of max {ref.abs().max().item():.4g}")
    assert err <= 0.01 * ref.abs().max().item() + 1e-3


@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5, 6])
def test_skinny_fp8_pipeline_steps(steps):
    """One 128-column block, 5 rows, K of 1 .. 6 pipeline steps (128 deep):
    the five-stage weight ring below, at and past one wrap (and the bf16
    kernel's three)."""
    K = 128 * steps
    x, codes, cs = _rand_q(5, K, 128, seed=steps)
    ref = x.float() @ _weights(codes, cs).t()
    out = torch.empty(5, 128, dtype=torch.bfloat16, device=DEV)
    G.skinny_fp8(x, codes, cs, out, G.SK_STORE, cus=32, splits=1)
    assert (out.float() - ref).abs().max().item() <= 0.01 * ref.abs().max().item() + 1e-3


@pytest.mark.parametrize("K,S", [(4096, 1), (4096, 8), (14336, 1), (14336, 28)])
def test_skinny_fp8_forced_splits(K, S):
    """No split and the deepest legal one (512-deep splits)."""
    x, codes, cs = _rand_q(17, K, 256, seed=K + S)
    ref = x.float() @ _weights(codes, cs).t()
    out = torch.empty(17, 256, dtype=torch.bfloat16, device=DEV)
    G.skinny_fp8(x, codes, cs, out, G.SK_STORE, cus=32, splits=S)
    assert (out.float() - ref).abs().max().item() <= 0.01 * ref.abs().max().item() + 1e-3


def test_skinny_fp8_refuses_bad_arguments():
    x, codes, cs = _rand_q(4, 256, 128, seed=1)
    out = torch.empty(4, 128, dtype=torch.bfloat16, device=DEV)
    G.skinny_fp8(x, codes, cs, out, G.SK_STORE)
    with pytest.raises(ValueError):                           # K not a multiple of the 128-deep step
        G.skinny_fp8(x[:, :192].contiguous(), codes[:, :192].contiguous(), cs, out, G.SK_STORE)
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes, cs, out, G.SK_STORE, splits=4)  # 256 does not split 4 ways
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes.view(torch.int8), cs, out, G.SK_STORE)
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes.t().contiguous().t(), cs, out, G.SK_STORE)
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes, cs[:64], out, G.SK_STORE)
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes, cs.double(), out, G.SK_STORE)
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes, cs.cpu(), out, G.SK_STORE)
    with pytest.raises(ValueError):
        G.skinny_fp8(x, codes, cs, out[:, :64], G.SK_STORE)


def test_quant_forward_matches_the_bf16_path_on_decoded_weights():
    """The 2-layer 8B-shaped stub: ``hidden(quant=True)`` on a CU partition's
    plan and on the whole chip's against the bf16 small-step path of a stub
    holding the decoded weights -- two routes through the same math."""
    from llm_message_queue_amd.models.llama_stub import QUANT_NAMES, LlamaConfig, LlamaStub
    cfg = LlamaConfig(vocab=32000, dim=4096, layers=2, heads=32, kv_heads=8, ffn=14336)
    m = LlamaStub(cfg, slots=8, max_ctx=64, device=DEV, impl="hip", seed=5, small_weights="fp8")
    ref = LlamaStub(cfg, slots=8, max_ctx=64, device=DEV, impl="hip", seed=5)
    for L, Lr in zip(m.layers, ref.layers):
        for k in QUANT_NAMES:
            assert torch.equal(L[k], Lr[k])
            Lr[k] = Q.dequantize(*L["fp8"][k])
    T = 40
    tok = torch.randint(0, cfg.vocab, (T,), device=DEV)
    pos = torch.arange(T, device=DEV, dtype=torch.int32) % 20
    slot = (torch.arange(T, device=DEV, dtype=torch.int32) // 20)
    samp = torch.tensor([19, 39], device=DEV, dtype=torch.long)
    b = ref.hidden(tok, pos, slot, rows=samp, small_cus=32).float()
    for cus in (32, 0):
        a = m.hidden(tok, pos, slot, rows=samp, small_cus=cus, quant=True).float()
        assert (a - b).abs().max().item() <= 0.03 * a.abs().max().item()
    # a record, not a bar: the quantisation error against the original weights
    o = m.hidden(tok, pos, slot, rows=samp, small_cus=32).float()
    print(f"fp8 vs bf16 weights, 2-layer hidden: max {((a - o).abs().max() / o.abs().max()).item():.4f} of max, "
          f"rms {((a - o).pow(2).mean().sqrt() / o.pow(2).mean().sqrt()).item():.4f}")
    # the whole forward takes the flag, at a row count past the bf16 skinny path's
    T2 = 300
    tok2 = torch.randint(0, cfg.vocab, (T2,), device=DEV)
    pos2 = torch.arange(T2, device=DEV, dtype=torch.int32) % 60
    slot2 = (torch.arange(T2, device=DEV, dtype=torch.int32) // 60)
    samp2 = torch.arange(59, T2, 60, device=DEV, dtype=torch.long)
    a2 = m.hidden(tok2, pos2, slot2, rows=samp2, small_cus=64, quant=True).float()
    b2 = ref.hidden(tok2, pos2, slot2, rows=samp2, small_cus=64).float()
    assert (a2 - b2).abs().max().item() <= 0.03 * a2.abs().max().item()
    assert m.forward(tok2, pos2, slot2, samp2, small_cus=64, quant=True).shape == (5,)


def _engine(mode, **kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=16, max_ctx=64, token_budget=64, device=torch.device("cuda", 0),
                         impl="hip", seed=3, realtime_mode=mode, micro_slots=4, **kw)


def _requests(n=12, seed=0, gen=4):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(seed)
    return [Request(req_id=i, prompt=rng.integers(0, 1000, size=5 + i % 7).astype(np.int32), gen_tokens=gen,
                    tier=i % 3) for i in range(n)]


def _serve(eng, reqs):
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
    return got


def test_fp8_micro_graph_replays_match_eager():
    """``micro_weights = "fp8"`` on the CU partition: decode micro-forwards
    replayed from the captured graphs (which hold the fp8 kernels) give the
    ids of the same micro-forwards launched eagerly."""
    eager = _engine("micro", micro_stream="partition", micro_graph=False, micro_weights="fp8")
    eager.warm_shapes([1, 8, 64])
    a = _serve(eager, _requests(24, seed=9, gen=6))
    eager.close()
    graph = _engine("micro", micro_stream="partition", micro_weights="fp8")
    graph.warm_shapes([1, 8, 64])
    assert graph.micro_graph and graph._mg
    b = _serve(graph, _requests(24, seed=9, gen=6))
    assert graph.micro_graph_steps > 0
    assert sorted(a) == sorted(b) == list(range(24))
    assert {k: v[0] for k, v in a.items()} == {k: v[0] for k, v in b.items()}
    assert sum(v[1] for v in b.values()) >= 4
    graph.close()
