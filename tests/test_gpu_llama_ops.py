"""rmsnorm, row_rms, silu_mul and rope_kv against float64 references of the
same operations, at every template instantiation, with tail blocks, extreme
rows and sentinel-filled caches; the bounds come from the number formats
(one bf16 rounding, fp32 arithmetic), not from what the kernels return."""
import pytest
import torch

from kernel_checks import BF16_MIN_NORMAL, SENTINEL, _bf16, _rope_ref, sentinel, ulp_distance

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EPS = 1e-5


@pytest.fixture(scope="module")
def hip():
    from llm_message_queue_amd.ops.llama_ops import HipOps
    return HipOps()


def _sentinel(shape):
    return sentinel(shape, DEV)


# ----------------------------------------------------------------------------- rmsnorm
def _norm_rows(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, D, generator=g)
    if T >= 5:
        x[1] = 0.0                    # output exactly zero
        x[2] *= 2.0 ** 40             # sum of squares ~2^93: large, inside fp32
        x[3] *= 2.0 ** -40            # mean square far below eps: the eps branch
    return _bf16(x)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("D", [2048, 4096, 6144, 8192])
def test_rmsnorm_vs_fp64(hip, D, T, residual):
    x = _norm_rows(T, D, seed=D + T)
    g = torch.Generator().manual_seed(7)
    w = _bf16(1 + 0.1 * torch.randn(D, generator=g))
    if residual:
        r = _norm_rows(T, D, seed=D + T + 1)
        # the contract: the fp32 sum rounded to bf16 is the new residual, and the norm is of that
        s = _bf16(x.float() + r.float())
        r_dev = r.to(DEV)
        y = hip.rmsnorm(x.to(DEV), w.to(DEV), EPS, residual=r_dev)
        torch.cuda.synchronize()
        assert torch.equal(r_dev.cpu().view(torch.int16), s.view(torch.int16))
    else:
        s = x
        xd = x.to(DEV)
        y = hip.rmsnorm(xd, w.to(DEV), EPS)
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu().view(torch.int16), x.view(torch.int16))
    sd, wd = s.double(), w.double()
    inv = 1.0 / torch.sqrt((sd * sd).mean(-1, keepdim=True) + EPS)
    ref = sd * inv * wd
    # one bf16 rounding; the second term is a floor for the fp32 rsqrt and reduction
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * wd.abs() * sd.abs().max(-1, keepdim=True).values * inv
    yc = y.cpu()
    err = (yc.double() - ref).abs()
    print(f"LLAMA_ULP rmsnorm D={D} T={T} residual={residual}: {ulp_distance(yc, ref)} ulp")
    assert torch.isfinite(yc.float()).all()
    assert (err <= bound).all(), (err - bound).max().item()
    if T >= 5:
        assert (yc[1].float() == 0).all()
        assert yc[2].float().abs().max() > 1 and yc[3].float().abs().max() > 0


# ----------------------------------------------------------------------------- row_rms
@pytest.mark.parametrize("T", [1, 5, 9])
@pytest.mark.parametrize("D", [512, 2048, 4096])
def test_row_rms_vs_fp64(hip, D, T):
    from llm_message_queue_amd.ops.gemm import row_scale_len
    x = _norm_rows(T, D, seed=3 * D + T)
    r = hip.row_rms(x.to(DEV), EPS)
    torch.cuda.synchronize()
    assert r.dtype == torch.float32 and r.numel() == row_scale_len(T)
    xd = x.double()
    ref = 1.0 / torch.sqrt((xd * xd).mean(-1) + EPS)
    rel = ((r[:T].cpu().double() - ref).abs() / ref).max().item()
    print(f"LLAMA_ULP row_rms D={D} T={T}: rel err {rel:.3e} = {rel / 2 ** -24:.2f} * 2^-24")
    assert rel <= 2.0 ** -20, rel


# ----------------------------------------------------------------------------- silu_mul
GATES = [100.0, -100.0, 88.0, -88.0, 20.0, -20.0, 1e-3, -1e-3, 0.0, -0.0]


def _silu_inputs(T, F, seed):
    """[T, 2F] = [gate | up]: random values, and at the front every special
    gate against up values of both signs."""
    g = torch.Generator().manual_seed(seed)
    gate = 3.0 * torch.randn(T * F, generator=g)
    up = torch.randn(T * F, generator=g)
    n = min(T * F, 4 * len(GATES))
    for i in range(n):
        gate[i] = GATES[i % len(GATES)]
        up[i] = (-1.0) ** (i // len(GATES)) * (1.5 + i / 64)
    return _bf16(torch.cat([gate.view(T, F), up.view(T, F)], dim=1))


@pytest.mark.parametrize("T,F,perm", [(1, 8, False), (3, 136, False), (19, 1024, False), (1, 128, True),
                                      (3, 384, True)])
def test_silu_mul_vs_fp64(hip, T, F, perm):
    assert T * F // 8 < 256 or (T * F // 8) % 256            # one block, or a partly filled last block
    gu = _silu_inputs(T, F, seed=T * F)
    gd, ud = gu[:, :F].double(), gu[:, F:].double()
    ref = gd / (1.0 + torch.exp(-gd)) * ud
    inp = gu
    if perm:
        from llm_message_queue_amd.ops.gemm import swiglu_perm_index
        inp = gu.index_select(1, swiglu_perm_index(F)).contiguous()     # column r holds [gate | up] column idx[r]
    out = _sentinel((T + 1, F))                                         # one row behind the last: never written
    y = hip.silu_mul(inp.to(DEV), out=out[:T], perm=perm)
    torch.cuda.synchronize()
    yc = y.cpu()
    assert (out[T].cpu().view(torch.int16) == SENTINEL).all()
    assert torch.isfinite(yc.float()).all()                             # exp(100) overflows fp32: never NaN
    # one rounding; below the smallest normal a result may lose every bit
    bound = 2.0 ** -8 * ref.abs() + BF16_MIN_NORMAL
    err = (yc.double() - ref).abs()
    normal = ref.abs() >= 2 * BF16_MIN_NORMAL
    print(f"LLAMA_ULP silu_mul T={T} F={F} perm={perm}: "
          f"{ulp_distance(yc[normal], ref[normal]) if normal.any() else 0} ulp")
    assert (err <= bound).all(), (err - bound).max().item()
    big = gd <= -100
    assert (yc[big].float().abs() <= 2.0 ** -133).all()                 # a signed zero or the smallest subnormal


# ----------------------------------------------------------------------------- rope_kv
S, C = 3, 320
TOKENS = [(2, 0), (0, 1), (1, C - 1), (0, 0), (2, C - 1), (1, 1), (0, 17)]          # (slot, pos), shuffled


def _rope_case(Hq, Hkv, tokens, seed, n_slots=S, front=0, back=0):
    """qkv, tables and sentinel-filled caches with ``front`` / ``back`` extra
    slots and table rows around what the op is told about."""
    from llm_message_queue_amd.ops.llama_ops import rope_tables
    g = torch.Generator().manual_seed(seed)
    T = len(tokens)
    qkv = _bf16(torch.randn(T, (Hq + 2 * Hkv) * 128, generator=g))
    cos, sin = rope_tables(C + 8 * (front + back))
    kfull = _sentinel((n_slots + front + back, Hkv, C, 128))
    vfull = _sentinel((n_slots + front + back, Hkv, C, 128))
    return dict(qkv=qkv, cos=cos, sin=sin, kfull=kfull, vfull=vfull, kc=kfull[front:front + n_slots],
                vc=vfull[front:front + n_slots], cos_v=cos[8 * front:], sin_v=sin[8 * front:],
                slot=torch.tensor([s for s, _ in tokens], dtype=torch.int32),
                pos=torch.tensor([p for _, p in tokens], dtype=torch.int32))


def _rope_check(d, Hq, Hkv, q, valid, front=0):
    """q rows and written K rows of the ``valid`` tokens within the bound, V
    rows bit-equal to the input, every other cache row and every q row of a
    dropped token still the sentinel."""
    T = d["qkv"].shape[0]
    x = d["qkv"].double().view(T, Hq + 2 * Hkv, 128)
    tab = 8 * front
    cos = torch.stack([d["cos"][tab + int(p)] if v else d["cos"][0] for p, v in zip(d["pos"], valid)]).double()
    sin = torch.stack([d["sin"][tab + int(p)] if v else d["sin"][0] for p, v in zip(d["pos"], valid)]).double()
    qref, qb = _rope_ref(x[:, :Hq], cos, sin)
    kref, kb = _rope_ref(x[:, Hq:Hq + Hkv], cos, sin)
    qc = q.cpu().view(T, Hq, 128)
    kf, vf = d["kfull"].cpu(), d["vfull"].cpu()
    touched = torch.zeros(kf.shape[0], C, dtype=torch.bool)
    worst = 0
    for t in range(T):
        if not valid[t]:
            assert (qc[t].view(torch.int16) == SENTINEL).all(), f"dropped token {t} wrote q"
            continue
        s, p = front + int(d["slot"][t]), int(d["pos"][t])
        touched[s, p] = True
        assert ((qc[t].double() - qref[t]).abs() <= qb[t]).all(), f"q of token {t}"
        assert ((kf[s, :, p].double() - kref[t]).abs() <= kb[t]).all(), f"k of token {t}"
        assert torch.equal(vf[s, :, p].view(torch.int16), d["qkv"].view(T, -1, 128)[t, Hq + Hkv:].view(torch.int16))
        worst = max(worst, ulp_distance(qc[t], qref[t]), ulp_distance(kf[s, :, p], kref[t]))
    rest = ~touched[:, None, :].expand(-1, Hkv, -1)
    assert (kf.view(torch.int16)[rest] == SENTINEL).all(), "a K row that no token addresses changed"
    assert (vf.view(torch.int16)[rest] == SENTINEL).all(), "a V row that no token addresses changed"
    return worst


@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (16, 4), (36, 9), (32, 8)])
def test_rope_kv_vs_fp64(hip, Hq, Hkv):
    d = _rope_case(Hq, Hkv, TOKENS, seed=Hq)
    q = hip.rope_kv(d["qkv"].to(DEV), d["pos"].to(DEV), d["slot"].to(DEV), d["cos_v"].to(DEV), d["sin_v"].to(DEV),
                    Hq, Hkv, d["kc"], d["vc"])
    torch.cuda.synchronize()
    worst = _rope_check(d, Hq, Hkv, q, [True] * len(TOKENS))
    print(f"LLAMA_ULP rope_kv Hq={Hq} Hkv={Hkv}: {worst} ulp")


def test_rope_kv_drops_out_of_range_tokens(hip):
    """One cache slot and 8 table rows in front of and behind what the op is
    told about: whatever a missing guard would touch belongs to this test."""
    Hq, Hkv = 16, 4
    bad = {1: (S, 5), 3: (-1, 5), 5: (1, C), 6: (1, -1), 8: (0, C + 3), 9: (2, -8)}       # row: (slot, pos)
    good = iter(TOKENS)
    tokens = [bad[i] if i in bad else next(good) for i in range(11)]
    d = _rope_case(Hq, Hkv, tokens, seed=5, front=1, back=1)
    cos_d, sin_d = d["cos"].to(DEV), d["sin"].to(DEV)
    q_out = _sentinel((len(tokens), Hq * 128))
    assert d["kc"].is_contiguous() and d["kc"].shape[0] == S
    hip.rope_kv(d["qkv"].to(DEV), d["pos"].to(DEV), d["slot"].to(DEV), cos_d[8:], sin_d[8:], Hq, Hkv, d["kc"],
                d["vc"], q_out=q_out)
    torch.cuda.synchronize()
    _rope_check(d, Hq, Hkv, q_out, [i not in bad for i in range(len(tokens))], front=1)
