"""Per-request temperature sampling, the parts that need no GPU: the noise
contract's host twin (``ops/sampling.py``; ``csrc/kernels/sample_noise.h``
compiled for the host), the generator's quality, the reference sampler's
distribution, reproducibility through the engine, the descriptor columns and
the API parser."""
import os
import subprocess

import numpy as np
import pytest
import torch

from llm_message_queue_amd.ops import sampling as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# chi-square critical values at p = 1e-6 (scipy.stats.chi2.isf(1e-6, df))
CHI2_255 = 377.078
CHI2_8 = 42.701


# --------------------------------------------------------------------------- noise twin
def test_gumbel_is_finite_at_the_ends_of_the_range():
    g = S.gumbel_from_bits(np.array([0, 1, 2 ** 20, 2 ** 32 - 1], dtype=np.uint32))
    assert np.isfinite(g).all()
    assert abs(g[0] - 22.87) < 0.01 and abs(g[3] + 3.13) < 0.01       # the contract's maximum / minimum
    assert (np.diff(g) < 0).all()                                     # small m is large G


def test_exponential_branches_agree_at_the_switch():
    v = 2.0 ** -12
    a, b = float(S.exponential_series(v)), float(S.exponential_log(v))
    assert abs(a - b) / b < 1e-9
    # the branch the twin takes on either side of the switch
    m = np.array([2 ** 20 - 1, 2 ** 20], dtype=np.uint32)
    vv = (m.astype(np.float64) + 0.5) * 2.0 ** -32
    want = -np.log([S.exponential_series(vv[0]), S.exponential_log(vv[1])])
    assert np.array_equal(S.gumbel_from_bits(m), want)


def test_row_key_is_splitmix64_of_seed_and_token_index():
    def sm64(x):
        x = (x + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return x ^ (x >> 31)
    for seed, g in ((0, 0), (7, 3), (2 ** 63 - 1, 511), (123456789, 0)):
        z = sm64((seed + 0x9E3779B97F4A7C15 * (g + 1)) & (2 ** 64 - 1))
        assert S.row_keys(seed, g).tolist() == [[z & 0xFFFFFFFF, z >> 32]]
    k = S.row_keys(np.array([5, 5, 6], dtype=np.uint64), np.array([0, 1, 0]))
    assert k.shape == (3, 2) and len({tuple(r) for r in k.tolist()}) == 3


def test_header_host_twin_matches_numpy(tmp_path):
    """``sample_noise.h`` compiled for the host: row keys and bits equal the
    numpy twin bit for bit, the float32 Gumbel is within the contract's
    2.4e-4 (+ float32 rounding of G itself) of the float64 one."""
    src = tmp_path / "t.cpp"
    src.write_text(
        '#include <cstdio>\n#include "kernels/sample_noise.h"\n'
        "int main() {\n"
        "  const unsigned long long seeds[3] = {0ull, 7ull, 0x7fffffffffffffffull};\n"
        "  for (int s = 0; s < 3; ++s) for (unsigned g = 0; g < 3; ++g) {\n"
        "    uint32_t k0, k1; llmq::sn_row_key(seeds[s], g, k0, k1);\n"
        "    std::printf(\"K %u %u\\n\", k0, k1);\n"
        "    for (uint32_t n = 0; n < 200; ++n) {\n"
        "      const uint32_t c = n * 641u; const uint32_t m = llmq::sn_bits(k0, k1, c);\n"
        "      std::printf(\"B %u %.9g\\n\", m, (double)llmq::sn_gumbel_from_bits(m)); } }\n"
        "  const uint32_t e[6] = {0u, 1u, 1048575u, 1048576u, 4294967294u, 4294967295u};\n"
        "  for (int i = 0; i < 6; ++i) std::printf(\"B %u %.9g\\n\", e[i], (double)llmq::sn_gumbel_from_bits(e[i]));\n"
        "  return 0; }\n")
    exe = tmp_path / "t"
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{os.path.join(ROOT, 'csrc')}", str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    keys = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("K")]
    want = [tuple(S.row_keys(s, g)[0].tolist()) for s in (0, 7, 2 ** 63 - 1) for g in range(3)]
    assert keys == want
    rows = [ln.split()[1:] for ln in lines if ln.startswith("B")]
    m = np.array([int(r[0]) for r in rows], dtype=np.uint32)
    gdev = np.array([float(r[1]) for r in rows])
    cols = (np.arange(200, dtype=np.uint32) * np.uint32(641))
    bits = S.noise_bits(np.array(want, dtype=np.uint32), cols).reshape(-1)
    assert np.array_equal(m[:len(bits)], bits)
    assert np.isfinite(gdev).all()
    assert np.abs(gdev - S.gumbel_from_bits(m)).max() < 2.4e-4 + 4e-6


# --------------------------------------------------------------------------- generator quality
def _chi2_top_byte(m: np.ndarray) -> float:
    cnt = np.bincount((m >> np.uint32(24)).reshape(-1), minlength=256).astype(np.float64)
    e = m.size / 256.0
    return float(((cnt - e) ** 2 / e).sum())


def _popcount(x: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).reshape(x.size, 32).sum(axis=1)


@pytest.fixture(scope="module")
def bits_by_key():
    """[64 keys][65,536 columns]: 8 seeds x 8 consecutive token indices."""
    seeds = np.repeat(np.array([0, 1, 2, 7, 1 << 32, 123456789, 2 ** 62 + 5, 2 ** 63 - 1], dtype=np.uint64), 8)
    keys = S.row_keys(seeds, np.tile(np.arange(8), 8))
    return S.noise_bits(keys, np.arange(65536, dtype=np.uint32))


@pytest.fixture(scope="module")
def bits_by_gidx():
    """[65,536 consecutive token indices of one seed][6 fixed columns]."""
    keys = S.row_keys(20240229, np.arange(65536))
    return S.noise_bits(keys, np.array([0, 1, 255, 256, 77777, 128255], dtype=np.uint32))


def test_generator_top_byte_is_uniform_over_columns(bits_by_key):
    assert bits_by_key.shape == (64, 65536)
    assert _chi2_top_byte(bits_by_key) < CHI2_255
    for k in range(64):
        assert _chi2_top_byte(bits_by_key[k]) < CHI2_255, k


def test_generator_top_byte_is_uniform_over_token_indices(bits_by_gidx):
    for c in range(bits_by_gidx.shape[1]):
        assert _chi2_top_byte(bits_by_gidx[:, c]) < CHI2_255, c


def test_generator_avalanche(bits_by_key, bits_by_gidx):
    cols = _popcount(bits_by_key[:, 1:] ^ bits_by_key[:, :-1]).mean()
    gidx = _popcount(bits_by_gidx[1:] ^ bits_by_gidx[:-1]).mean()
    assert 14 <= cols <= 18, cols
    assert 14 <= gidx <= 18, gidx


# --------------------------------------------------------------------------- reference sampler distribution
DIST_V = 1024
DIST_TOP = np.array([37, 100, 255, 256, 511, 640, 900, 1023])


def dist_logits() -> np.ndarray:
    """One row: eight tokens hold most of the mass (64 % at T = 1, 99.8 %
    at T = 0.5; the rest still expects ~9 of 4,096 draws there)."""
    lg = np.full(DIST_V, -6.0)
    lg[DIST_TOP] = -0.2 * np.arange(8)
    return lg


def dist_keys() -> np.ndarray:
    return S.row_keys(np.arange(4096, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(99), 0)


def dist_chi2(picks: np.ndarray, T: float, logits: np.ndarray = None) -> float:
    """Chi-square of ``picks`` over the eight tokens + "rest" against
    softmax(logits / T) (``logits``: the row actually sampled, if rounded)."""
    lg = (dist_logits() if logits is None else np.asarray(logits, dtype=np.float64)) / T
    p = np.exp(lg - lg.max())
    p /= p.sum()
    pe = np.append(p[DIST_TOP], 1.0 - p[DIST_TOP].sum())
    idx = np.full(DIST_V, 8)
    idx[DIST_TOP] = np.arange(8)
    cnt = np.bincount(idx[np.asarray(picks)], minlength=9).astype(np.float64)
    e = pe * len(picks)
    assert e.min() > 5
    return float(((cnt - e) ** 2 / e).sum())


@pytest.mark.parametrize("T", [1.0, 0.5])
def test_reference_sampler_draws_from_softmax(T):
    n = 4096
    picks = S.sample_reference(np.tile(dist_logits(), (n, 1)), np.full(n, 1.0 / T, dtype=np.float32), dist_keys())
    assert dist_chi2(picks, T) < CHI2_8


def test_reference_sampler_greedy_rows_are_argmax_with_low_ties():
    lg = np.zeros((3, 64))
    lg[0, [9, 5]] = 2.0
    lg[1, 63] = 1.0
    picks = S.sample_reference(lg, np.zeros(3, dtype=np.float32), S.row_keys(1, [0, 1, 2]))
    assert picks.tolist() == [5, 63, 0]


# --------------------------------------------------------------------------- engine on the CPU
def _engine(slots=32):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    return BackendEngine(LlamaConfig.tiny(), slots=slots, max_ctx=64, token_budget=256, device="cpu", impl="ref")


def _req(i, **kw):
    from llm_message_queue_amd.backend.engine import Request
    rng = np.random.default_rng(1000 + i)
    return Request(req_id=i, prompt=rng.integers(0, 1024, 3 + i % 5).astype(np.int32), gen_tokens=5, **kw)


def _run(reqs, slots=32):
    eng = _engine(slots)
    assert len(eng.admit(reqs)) == len(reqs)
    done = eng.drain()
    assert len(done) == len(reqs)
    return {r.req_id: r for r in done}, eng


@pytest.fixture(scope="module")
def engine_runs():
    others = lambda: [_req(i) for i in range(20)]                      # noqa: E731  (temperature 0)
    alone, e_alone = _run([_req(100, temperature=0.8, seed=7)])
    mixed, e_mixed = _run(others() + [_req(100, temperature=0.8, seed=7)])
    moved, _ = _run([_req(i) for i in range(3)] + [_req(100, temperature=0.8, seed=7)])
    reseed, _ = _run([_req(100, temperature=0.8, seed=8)])
    greedy, e_greedy = _run(others())
    return dict(alone=alone, mixed=mixed, moved=moved, reseed=reseed, greedy=greedy,
                steps=(e_alone.sampled_steps, e_mixed.sampled_steps, e_greedy.sampled_steps))


def test_engine_sampled_request_is_reproducible_across_batches_and_slots(engine_runs):
    a = engine_runs["alone"][100]
    assert a.out_tokens is not None and len(a.out_tokens) == 5
    b, c = engine_runs["mixed"][100], engine_runs["moved"][100]
    assert len({a.slot, b.slot, c.slot}) == 3                            # three different slots
    assert np.array_equal(a.out_tokens, b.out_tokens)
    assert np.array_equal(a.out_tokens, c.out_tokens)
    assert not np.array_equal(a.out_tokens, engine_runs["reseed"][100].out_tokens)
    assert engine_runs["steps"][0] > 0 and engine_runs["steps"][1] > 0 and engine_runs["steps"][2] == 0


def test_engine_greedy_requests_are_untouched_by_a_sampling_neighbour(engine_runs):
    for i in range(20):
        assert np.array_equal(engine_runs["mixed"][i].out_tokens, engine_runs["greedy"][i].out_tokens), i
    # and a sampled request is not its greedy self
    g, _ = _run([_req(100)])
    assert not np.array_equal(g[100].out_tokens, engine_runs["alone"][100].out_tokens)


def test_sim_engine_forward_ignores_sampling_arguments():
    from llm_message_queue_amd.backend.sim_engine import SimEngine
    out = SimEngine._forward(None, None, None, torch.zeros(3), inv_temp=torch.ones(256), keys=torch.zeros(256, 2))
    assert out.shape == (3,)


# --------------------------------------------------------------------------- descriptor, parser, route
def test_descriptor_carries_temperature_and_seed():
    from llm_message_queue_amd.gateway.descriptors import DESC_HDR
    from llm_message_queue_amd.models.message import Message, default_seed
    from tests.test_tier_caps import _gateway
    assert DESC_HDR == 20
    gw = _gateway(True, [0, 0, 0, 0])
    msgs = [Message(id="s0", content="x", metadata={"sampling": {"temperature": 0.7, "seed": 2 ** 63 - 1}}),
            Message(id="s1", content="x", metadata={"sampling": {"temperature": 1.5}}),
            Message(id="s2", content="x"),
            Message(id="s3", content="x", metadata={"sampling": {"temperature": 9}})]
    for i, m in enumerate(msgs):
        m.tier = 2
        m.prompt_ids = np.arange(4, dtype=np.uint32) + i
    buf = np.zeros((len(msgs), DESC_HDR + 8), dtype=np.int32)
    gw._fill_descs(buf, msgs, 1, 8, {})
    reqs = gw._foreign_requests(buf, 8)
    assert [r.temperature for r in reqs] == [float(np.float32(0.7)), 1.5, 0.0, 0.0]
    assert [r.seed for r in reqs] == [2 ** 63 - 1, default_seed("s1"), 0, default_seed("s3")]   # (a greedy seed is unused)
    assert reqs[0].prompt.tolist() == [0, 1, 2, 3] and reqs[3].prompt.tolist() == [3, 4, 5, 6]
    # the effective values are written back for a replay; a bad value falls back to greedy and says so
    assert msgs[1].metadata["sampling"] == {"temperature": 1.5, "seed": default_seed("s1")}
    assert "sampling" not in msgs[2].metadata and "sampling_error" not in msgs[2].metadata
    assert msgs[3].metadata["sampling"]["temperature"] == 0.0 and "temperature" in msgs[3].metadata["sampling_error"]


def test_make_request_fills_the_sampling_fields():
    from llm_message_queue_amd.models.message import Message, default_seed
    from tests.test_tier_caps import _gateway
    gw = _gateway(True, [0, 0, 0, 0])
    m = Message(id="q", content="x", metadata={"sampling": {"temperature": 0.8, "seed": 7}})
    r = gw._make_request(m, 2)
    assert (r.temperature, r.seed) == (0.8, 7)
    m = Message(id="q1", content="x", metadata={"sampling": {"temperature": 0.8}})
    r = gw._make_request(m, 2)
    assert (r.temperature, r.seed) == (0.8, default_seed("q1")) and m.metadata["sampling"]["seed"] == r.seed
    r = gw._make_request(Message(id="q2", content="x"), 2)
    assert (r.temperature, r.seed) == (0.0, 0)                          # (a greedy request's seed is never read)


def test_sampling_parser_ranges():
    from llm_message_queue_amd.models.message import SamplingParseError, default_seed, sampling_from_metadata as p
    assert p({}, "a") == (0.0, default_seed("a")) and p(None, "a") == (0.0, default_seed("a"))
    assert 0 <= default_seed("a") < 2 ** 63 and default_seed("a") != default_seed("b")
    assert p({"sampling": {"temperature": 0}}, "a") == (0.0, default_seed("a"))
    for t in (0.05, 1, 0.8, 2.0):
        assert p({"sampling": {"temperature": t, "seed": 0}}) == (float(t), 0)
    assert p({"sampling": {"temperature": 1.0, "seed": 2 ** 63 - 1}})[1] == 2 ** 63 - 1
    for bad in ({"temperature": 0.049}, {"temperature": 2.01}, {"temperature": 3}, {"temperature": -1},
                {"temperature": "1"}, {"temperature": True}, {"temperature": float("nan")},
                {"temperature": 1.0, "seed": -1}, {"temperature": 1.0, "seed": 2 ** 63},
                {"temperature": 1.0, "seed": 1.5}, {"temperature": 1.0, "seed": "7"}, "hot", [1]):
        with pytest.raises(SamplingParseError):
            p({"sampling": bad}, "a")


def test_post_message_rejects_a_bad_temperature():
    from fastapi.testclient import TestClient
    from llm_message_queue_amd.api.server import create_app
    from llm_message_queue_amd.gateway.app import GatewayApp
    from llm_message_queue_amd.utils.config import default_config
    cfg = default_config()
    cfg.preprocessor.batch_window_us = 200
    app = GatewayApp(cfg, use_gpu=False, simulate_ms=(1, 1, 1, 1))
    try:
        with TestClient(create_app(app)) as c:
            r = c.post("/api/v1/messages", json={"content": "hi", "metadata": {"sampling": {"temperature": 3}}})
            assert r.status_code == 400 and "temperature" in r.text
            r = c.post("/api/v1/messages", json={"content": "hi", "metadata": {"sampling": {"temperature": 0.9,
                                                                                            "seed": 11}}})
            assert r.status_code == 202, r.text
    finally:
        app.stop()
