"""FP8 (e4m3) weights for the realtime micro-forwards, on the CPU: the
quantisation contract of ``ops.quant`` (the host twin the device kernels are
held to in ``test_gpu_skinny_fp8.py``), the engine's ``micro_weights`` mode on
the reference ops, and its configuration."""
import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import quant as Q


def _rows():
    """Gaussian rows (std 0.02) of both layer widths, plus the special rows:
    one 1000x outlier, a row entirely below 2^-6 * scale of its neighbour,
    an all-zero row."""
    out = []
    for K in (4096, 14336):
        g = torch.Generator().manual_seed(K)
        w = (torch.randn(16, K, generator=g) * 0.02).to(torch.bfloat16)
        w[3, 17] = 20.0                                        # 1000 x std
        _, s = Q.quantize_rows_e4m3(w[4:5])
        w[5] = (torch.rand(K, generator=g) * 2.0 ** -7 * s[0]).to(torch.bfloat16)   # all below 2^-6 * scale(row 4)
        w[6] = 0
        out.append(w)
    return out


def test_decode_table_is_e4m3fn():
    want = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    nan = np.isnan(want)
    assert nan.tolist() == [c & 0x7F == 0x7F for c in range(256)]
    assert np.array_equal(np.isnan(Q.TABLE), nan)
    assert np.array_equal(Q.TABLE[~nan].view(np.uint32), want[~nan].view(np.uint32))   # (signed zeros too)
    assert np.nanmax(Q.TABLE) == Q.E4M3_MAX


def test_all_finite_codes_times_a_power_of_two_are_bf16():
    codes = torch.arange(256, dtype=torch.uint8).repeat(3, 1)
    scale = torch.tensor([2.0 ** -12, 1.0, 2.0 ** 9])
    d = Q.dequantize(codes, scale)
    exact = torch.from_numpy(Q.TABLE)[None, :] * scale[:, None]
    ok = ~torch.isnan(exact)
    assert torch.equal(d.float()[ok], exact[ok])


@pytest.mark.parametrize("w", _rows(), ids=["k4096", "k14336"])
def test_quantize_contract(w):
    codes, scale = Q.quantize_rows_e4m3(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    m, _ = np.frexp(scale.numpy())
    assert (m == 0.5).all()                                    # powers of two
    assert not ((codes & 0x7F) == 0x7F).any()                  # no NaN code
    deq = Q.dequantize(codes, scale)
    mag = torch.from_numpy(Q.TABLE)[codes.long()].abs()
    top = mag.max(dim=1).values
    zero = w.float().abs().max(dim=1).values == 0
    assert zero.tolist() == [i == 6 for i in range(w.shape[0])]
    assert (scale[zero] == 1).all() and (codes[zero] == 0).all()
    assert ((top[~zero] > 224) & (top[~zero] <= 448)).all()    # the smallest scale that fits
    # every decoded weight is a bf16 number
    assert torch.equal(deq.float().to(torch.bfloat16), deq)
    assert torch.equal(deq.float(), torch.from_numpy(Q.TABLE)[codes.long()] * scale[:, None])
    # the codes are torch's CPU cast of w / scale (round-to-nearest-even)
    assert torch.equal(codes, (w.float() / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8))
    # error: 3 mantissa bits, RNE -> half an ulp = 2^-4 relative in the normal
    # range (|w| >= 2^-6 * scale), half a subnormal step 2^-10 * scale below
    err = (deq.float() - w.float()).abs()
    aw = w.float().abs()
    normal = aw >= 2.0 ** -6 * scale[:, None]
    assert (err[normal] <= 2.0 ** -4 * aw[normal]).all()
    assert (err <= 2.0 ** -10 * scale[:, None])[~normal].all()
    # the row below its neighbour's subnormal range keeps its own scale and precision
    assert scale[5] < scale[4] and normal[5].float().mean() > 0.9
    # the outlier owns its row's scale: the rest of the row is coarser than its neighbours
    assert scale[3] == 2.0 ** -4 and scale[2] == 2.0 ** -12


def test_rne_ties_and_range_match_torch():
    x = torch.cat([torch.linspace(-448, 448, 200001), torch.linspace(-2.0 ** -5, 2.0 ** -5, 200001),
                   torch.from_numpy(Q.TABLE[~np.isnan(Q.TABLE)]),
                   # exact ties between neighbouring codes
                   torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 15 * 2.0 ** -10, 1.0625, 1.1875, 416.0, 432.0])])
    want = x.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(Q.e4m3_rne(x.numpy()), want)


def test_tiny_rows_keep_a_normal_scale_and_nonfinite_is_refused():
    w = torch.tensor([[2.0 ** -130, -2.0 ** -133, 0.0, 0.0]], dtype=torch.float32)
    codes, scale = Q.quantize_rows_e4m3(w)
    assert scale.item() == 2.0 ** -126 and not ((codes & 0x7F) == 0x7F).any()
    with pytest.raises(ValueError):
        Q.quantize_rows_e4m3(torch.tensor([[1.0, float("inf")]]))


# ---------------------------------------------------------------------- engine (reference ops)
def _engine(mode, **kw):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=8, max_ctx=64, token_budget=32, device="cpu", impl="ref", seed=3,
                         realtime_mode=mode, micro_slots=4, **kw)


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


@pytest.fixture(scope="module")
def plain_tokens():
    return _serve(_engine("off"), _requests())


def test_fp8_micro_pool_serves_the_requantised_model(plain_tokens):
    from llm_message_queue_amd.models.llama_stub import QUANT_NAMES
    deq = _engine("off")
    for L in deq.model.layers:
        for k in QUANT_NAMES:
            L[k] = Q.requantized(L[k])
    want = _serve(deq, _requests())
    eng = _engine("micro", micro_weights="fp8")
    got = _serve(eng, _requests())
    assert sorted(got) == sorted(want) == sorted(plain_tokens) == list(range(12))
    micro = [k for k, v in got.items() if v[1]]
    assert micro == [0, 3, 6, 9] and eng.micro_steps >= 4
    for k, (ids, was_micro) in got.items():
        assert len(ids) == 4
        assert ids == (want[k][0] if was_micro else plain_tokens[k][0]), k
    # the mode is not inert: the quantised model answers differently somewhere
    assert any(want[k][0] != plain_tokens[k][0] for k in micro)


def test_fp8_weight_bytes_and_inert_modes(plain_tokens):
    from llm_message_queue_amd.models.llama_stub import QUANT_NAMES, LlamaConfig
    a = _engine("off")
    b = _engine("off", micro_weights="fp8")                    # accepted, inert apart from the memory
    elems = sum(L[k].numel() for L in a.model.layers for k in QUANT_NAMES)
    rows = sum(L[k].shape[0] for L in a.model.layers for k in QUANT_NAMES)
    assert b.weight_bytes - a.weight_bytes == elems + 4 * rows == LlamaConfig.tiny().quant_bytes()
    assert _serve(b, _requests()) == plain_tokens
    # the default mode holds no quantised copy and refuses a quant forward
    assert all("fp8" not in L for L in a.model.layers)
    z = torch.zeros(1, dtype=torch.long)
    with pytest.raises(ValueError):
        a.model.hidden(z, z.int(), z.int(), quant=True)


def test_engine_refuses_bad_micro_weights():
    with pytest.raises(ValueError):
        _engine("micro", micro_weights="x")
    with pytest.raises(ValueError):
        _engine("micro", micro_weights="int4")
    with pytest.raises(ValueError):
        _engine("micro", micro_weights="fp8", micro_gemm="rocblas")
    from llm_message_queue_amd.ops.gemm import SKINNY_CHUNKED_MAX_M
    with pytest.raises(ValueError):
        _engine("micro", micro_weights="fp8", micro_budget=SKINNY_CHUNKED_MAX_M + 1)
    assert _engine("micro", micro_weights="fp8", micro_budget=SKINNY_CHUNKED_MAX_M).micro_weights == "fp8"
    assert _engine("micro").micro_weights == "bf16"


def test_config_validates_micro_weights():
    from llm_message_queue_amd.utils.config import ConfigError, default_config, validate
    cfg = default_config()
    assert cfg.backend.micro_weights == "bf16"
    cfg.backend.micro_weights = "fp8"
    validate(cfg)
    cfg.backend.micro_gemm = "rocblas"
    with pytest.raises(ConfigError):
        validate(cfg)
    cfg.backend.micro_gemm = "hip"
    cfg.backend.micro_weights = "int4"
    with pytest.raises(ConfigError):
        validate(cfg)


def test_serve_engine_builder_passes_micro_weights(monkeypatch):
    import types
    import llm_message_queue_amd.backend.engine as E
    from llm_message_queue_amd.cli import main as M
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    from llm_message_queue_amd.utils.config import default_config
    got = {}

    class FakeEngine:
        def __init__(self, mcfg, **kw):
            got.update(kw)

    monkeypatch.setattr(E, "BackendEngine", FakeEngine)
    monkeypatch.setattr(torch.cuda, "get_device_properties",
                        lambda dev: types.SimpleNamespace(total_memory=64 << 30))
    slots = {}
    for mode in ("bf16", "fp8"):
        cfg = default_config()
        cfg.gpu.slots_per_gpu = 4096
        cfg.gpu.hbm_reserve_gb = 16
        cfg.backend.micro_weights = mode
        M._build_engine(cfg, "llama3-8b", "cpu")
        assert got["micro_weights"] == mode
        slots[mode] = got["slots"]
    # the slot cap sees the FP8 copy: 64 MiB of KV per 512-token slot
    lost = LlamaConfig.llama3_8b().quant_bytes() / (64 << 20)
    assert abs((slots["bf16"] - slots["fp8"]) - lost) <= 1 and lost > 100
