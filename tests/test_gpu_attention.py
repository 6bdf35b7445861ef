"""The four attention kernels (per-token, segment MFMA with 32- and 64-key
blocks, decode, and the mixed launch) against the fp64 reference of
tests/attention_cases.py: probes whose result is one known V row (needle,
ladder), the mean of two (twins), or a spread softmax, all through bounds
derived from the number formats; untouched output rows, the descriptor
guards, NaN beyond the context, and the wrappers' argument checks."""
import pytest
import torch

import attention_cases as AC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 0x5A5A          # bf16 1.5e16: an unwritten covered row fails every bound
PAD = 16                   # rows in front of and behind q / out in the guard tests


@pytest.fixture(scope="module")
def hip():
    from llm_message_queue_amd.ops.llama_ops import HipOps
    return HipOps()


_DEV_CACHE = {}


def _dev(case):
    """The case's tensors on the device (uploaded once, never written)."""
    k = id(case)
    if k not in _DEV_CACHE:
        e = case.edge
        cov = e.covered.nonzero().flatten()
        _DEV_CACHE[k] = dict(
            case=case, q=case.q.to(DEV), kc=case.kc.to(DEV), vc=case.vc.to(DEV),
            tiles=torch.from_numpy(e.tiles).to(DEV), cov=cov.to(DEV), q_cov=case.q[cov].contiguous().to(DEV),
            pos_cov=e.pos[cov].to(torch.int32).to(DEV), slot_cov=e.slot[cov].to(torch.int32).to(DEV))
    return _DEV_CACHE[k]


def _sentinel(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def run_path(hip, path, case, kc=None, vc=None):
    """Output [T, Hq * 128] of ``case`` under ``path``, on a sentinel-filled
    tensor.  The per-token kernel has no notion of an uncovered row: it gets
    the covered rows only."""
    d = _dev(case)
    cfg = AC.PATHS[path]
    kc = d["kc"] if kc is None else kc
    vc = d["vc"] if vc is None else vc
    out = _sentinel(d["q"].shape)
    if cfg["api"] == "token":
        o = hip.attention(d["q_cov"], kc, vc, d["pos_cov"], d["slot_cov"], case.Hq, case.Hkv, case.scale)
        out[d["cov"]] = o
    else:
        n_dec = case.edge.n_dec if cfg["dec"] else 0
        hip.attention_tiles(d["q"], kc, vc, d["tiles"], case.Hq, case.Hkv, case.scale, out=out, n_dec=n_dec,
                            seg_keys=cfg["seg_keys"], mixed=cfg["mixed"])
        if cfg["mixed"]:     # one launch == the two separate launches, bit for bit
            sep = _sentinel(d["q"].shape)
            hip.attention_tiles(d["q"], kc, vc, d["tiles"], case.Hq, case.Hkv, case.scale, out=sep, n_dec=n_dec,
                                seg_keys=cfg["seg_keys"], mixed=False)
            assert torch.equal(out.view(torch.int16), sep.view(torch.int16)), f"{path}: mixed != separate launches"
    torch.cuda.synchronize()
    return out.cpu()


def check(case, path, out):
    """Every covered element inside the path's bound of the fp64 reference;
    every uncovered row still the sentinel."""
    e = case.edge
    ref, A, _ = case.ref()
    o = out.double().view(e.T, case.Hq, AC.HD)
    raw = out.view(torch.int16).view(e.T, -1)
    assert (raw[~e.covered] == SENTINEL).all(), f"{path}/{case.name}: a row of no tile was written"
    err = (o - ref).abs()
    bnd = AC.row_bound(path, e, ref, A)
    m = e.covered
    ratio = (err[m] / A[m]).max().item()
    on_dec = m & e.dec_row if AC.PATHS[path].get("dec") else torch.zeros_like(m)
    for kind, rows in (("decode kernel", on_dec), ("token kernel" if path == "token" else "segment kernel", m & ~on_dec)):
        if rows.any():
            r = (err[rows] / A[rows]).max().item()
            print(f"ATTN_RATIO {path} {case.name} Hkv={case.Hkv} Hq={case.Hq} {kind}: max err/A = {r:.3e} "
                  f"= {r / 2 ** -7:.3f} * 2^-7")
    bad = ((err > bnd) | ~torch.isfinite(o)) & m[:, None, None]
    if bad.any():
        t, h, dd = [int(x) for x in bad.nonzero()[0]]
        G = case.Hq // case.Hkv
        p, s = int(e.pos[t]), int(e.slot[t])
        near = AC.nearest_key(o[t, h], case.vc, s, h // G)
        want = "" if case.target is None else f" expected key {int(case.target[t, h])}" + (
            "" if case.target2 is None else f"+{int(case.target2[t, h])}")
        raise AssertionError(
            f"{path}/{case.name}: row {t} (slot {s}, pos {p}, {'decode' if e.dec_row[t] else 'prefill'} tile) "
            f"head {h} dim {dd}:{want}; nearest V row is key {near}; out {o[t, h, dd].item():.6g} ref "
            f"{ref[t, h, dd].item():.6g} err {err[t, h, dd].item():.3e} > bound {bnd[t, h, dd].item():.3e}; "
            f"{int(bad.sum())} elements over, worst err/A {ratio:.3e}")


ALL_PATHS = list(AC.PATHS)
TILE_PATHS = [p for p in ALL_PATHS if p != "token"]


# ----------------------------------------------------------------------------- probes
@pytest.mark.parametrize("path", ALL_PATHS)
def test_needle(hip, path):
    case = AC.needle()
    check(case, path, run_path(hip, path, case))


@pytest.mark.parametrize("path", ALL_PATHS)
def test_needle_every_key_of_a_128_context(hip, path):
    case = AC.needle(sweep=True)
    check(case, path, run_path(hip, path, case))


@pytest.mark.parametrize("a", [8, 2])
@pytest.mark.parametrize("path", ALL_PATHS)
def test_ladder(hip, path, a):
    case = AC.ladder(a)
    check(case, path, run_path(hip, path, case))


@pytest.mark.parametrize("path", ALL_PATHS)
def test_twins(hip, path):
    case = AC.twins()
    check(case, path, run_path(hip, path, case))


@pytest.mark.parametrize("sigma", [0.5, 2, 4])
@pytest.mark.parametrize("path", ALL_PATHS)
def test_spread(hip, path, sigma):
    case = AC.spread(sigma)
    check(case, path, run_path(hip, path, case))


# ----------------------------------------------------------------------------- GQA shapes
@pytest.mark.parametrize("probe", ["needle", "ladder"])
@pytest.mark.parametrize("Hkv,group", [(1, 1), (1, 2), (1, 4), (3, 1), (3, 2), (3, 4)])
def test_per_token_gqa_groups(hip, probe, Hkv, group):
    case = AC.needle(Hkv, group) if probe == "needle" else AC.ladder(8, Hkv, group)
    check(case, "token", run_path(hip, "token", case))


@pytest.mark.parametrize("probe", ["needle", "ladder", "spread"])
@pytest.mark.parametrize("Hkv", [1, 8])          # Hkv = 2 is every other test of this file
@pytest.mark.parametrize("path", TILE_PATHS)
def test_tiles_kv_heads(hip, path, Hkv, probe):
    """Hkv = 8 is the serving shape; with Hkv = 1 the 14 decode items are no
    multiple of the decode kernel's 4 per block (the item >= n_items exit)."""
    case = {"needle": lambda: AC.needle(Hkv), "ladder": lambda: AC.ladder(8, Hkv),
            "spread": lambda: AC.spread(2, Hkv)}[probe]()
    assert Hkv != 1 or (case.edge.n_dec * Hkv) % 4 != 0
    check(case, path, run_path(hip, path, case))


# ----------------------------------------------------------------------------- NaN beyond the context
@pytest.mark.parametrize("path", ALL_PATHS)
def test_nan_tail_is_never_loaded(hip, path):
    """Cache rows at or after a slot's last used position hold NaN patterns:
    the output is the same bits as with a clean tail (and correct)."""
    case = AC.needle(ctx_limit=129)
    e = case.edge
    d = _dev(case)
    clean = run_path(hip, path, case)
    check(case, path, clean)
    kc, vc = d["kc"].clone(), d["vc"].clone()
    used = [int((e.tiles[e.tiles[:, 2] == s][:, 3] + e.tiles[e.tiles[:, 2] == s][:, 1]).max())
            for s in range(AC.N_SLOTS)]
    assert any(u % 32 for u in used) and max(used) < AC.MAX_CTX       # NaN begins inside a key block
    for s, u in enumerate(used):
        kc[s, :, u:].view(torch.int16).fill_(0x7FC0)                   # quiet NaN
        vc[s, :, u:].view(torch.int16).fill_(-1)                       # 0xFFFF: NaN with every bit set
        kc[s, :, u].view(torch.int16).fill_(0x7F81)                    # signalling NaN right behind the context
    out = run_path(hip, path, case, kc=kc, vc=vc)
    assert torch.equal(out.view(torch.int16), clean.view(torch.int16))


# ----------------------------------------------------------------------------- descriptor guards
class _Guarded:
    """Spread inputs inside padded allocations, so that every address a
    missing guard would touch belongs to this test: one cache slot in front
    of and behind the N_SLOTS the ops are told about, PAD rows in front of and
    behind q and out."""

    def __init__(self, Hkv=2):
        self.case = c = AC.spread(2, Hkv)
        S = AC.N_SLOTS
        g = torch.Generator().manual_seed(77)
        self.kfull = torch.randn(S + 2, Hkv, AC.MAX_CTX, AC.HD, generator=g).to(torch.bfloat16).to(DEV)
        self.vfull = torch.randn(S + 2, Hkv, AC.MAX_CTX, AC.HD, generator=g).to(torch.bfloat16).to(DEV)
        self.kfull[1:S + 1] = c.kc.to(DEV)
        self.vfull[1:S + 1] = c.vc.to(DEV)
        self.kc, self.vc = self.kfull[1:S + 1], self.vfull[1:S + 1]
        assert self.kc.is_contiguous() and self.kc.shape[0] == S
        T = c.edge.T
        self.qfull = torch.randn(T + 2 * PAD, c.Hq * AC.HD, generator=g).to(torch.bfloat16).to(DEV)
        self.qfull[PAD:PAD + T] = c.q.to(DEV)
        self.q = self.qfull[PAD:PAD + T]
        self.ofull = _sentinel(self.qfull.shape)
        self.out = self.ofull[PAD:PAD + T]

    def check(self, path, valid_rows):
        """Rows of ``valid_rows`` are correct, every other byte of the padded
        output is still the sentinel."""
        c, e = self.case, self.case.edge
        torch.cuda.synchronize()
        ref, A, _ = c.ref()
        full = self.ofull.cpu()
        raw = full.view(torch.int16)
        keep = torch.ones(full.shape[0], dtype=torch.bool)
        keep[PAD + valid_rows] = False
        assert (raw[keep] == SENTINEL).all(), f"{path}: a dropped descriptor wrote output rows " \
            f"{(raw[keep] != SENTINEL).any(dim=1).nonzero().flatten().tolist()} (padded numbering)"
        o = full[PAD:PAD + e.T].double().view(e.T, c.Hq, AC.HD)
        bnd = AC.row_bound(path, e, ref, A)
        assert ((o - ref).abs()[valid_rows] <= bnd[valid_rows]).all(), f"{path}: a valid row next to a dropped one"


def test_guard_per_token(hip):
    g = _Guarded()
    c, e = g.case, g.case.edge
    S, C = AC.N_SLOTS, AC.MAX_CTX
    pos, slot = e.pos.clone(), e.slot.clone()
    rows = e.covered.nonzero().flatten()
    # (row, pos, slot): each lands inside the padded caches if it were used
    bad = [(rows[0], 5, S), (rows[3], 5, -1), (rows[5], C, 1), (rows[8], -1, 2), (rows[11], -7, 2),
           (rows[14], C + 40, 0)]
    for r, p, s in bad:
        pos[r], slot[r] = p, s
    for r in (~e.covered).nonzero().flatten():           # rows of no tile: dropped the same way
        pos[r], slot[r] = -1, 1
    hip.attention(g.q, g.kc, g.vc, pos.to(torch.int32).to(DEV), slot.to(torch.int32).to(DEV), c.Hq, c.Hkv, c.scale,
                  out=g.out)
    valid = e.covered.clone()
    valid[torch.stack([r for r, _, _ in bad])] = False
    g.check("token", valid.nonzero().flatten())


def _bad_tiles(e, dec):
    """The edge set's tile list with some descriptors made invalid; returns
    (tiles, rows that stay valid).  Decode tiles: slot, position and row
    guards; segment tiles: slot, n, position and row-range guards."""
    S, C, T = AC.N_SLOTS, AC.MAX_CTX, e.T
    t = e.tiles.copy()
    hit = []

    def put(i, **kw):
        hit.append(i)
        for k, v in kw.items():
            t[i, "row n slot pos".split().index(k)] = v

    if dec:
        put(0, slot=S)
        put(2, slot=-1)
        put(4, pos=C)
        put(5, pos=-1)
        put(7, pos=-9)
        put(9, row=-1)
        put(10, row=T)
        put(12, row=T + PAD - 1)
    b = e.n_dec
    put(b + 0, slot=S)
    put(b + 1, slot=-1)
    put(b + 2, n=0)
    put(b + 3, n=17)                      # rows row .. row+16 stay inside the padded q
    put(b + 4, n=-3)
    put(b + 5, pos=-1)
    put(b + 6, pos=C - 15)                # pos + n = max_ctx + 1
    put(b + 7, pos=C)
    put(b + 8, row=-1)
    put(b + 9, row=T - 15)                # row + n = T + 1
    put(b + 10, row=T)
    assert e.tiles[b + 6, 1] == 16 and e.tiles[b + 9, 1] == 16, "these two need 16-row tiles"
    valid = torch.zeros(T, dtype=torch.bool)
    for i, (r0, n, _, _) in enumerate(e.tiles.tolist()):
        if i not in hit:
            valid[r0:r0 + n] = True
    return torch.from_numpy(t).to(DEV), valid.nonzero().flatten()


@pytest.mark.parametrize("path", TILE_PATHS)
def test_guard_tiles(hip, path):
    g = _Guarded()
    c, e = g.case, g.case.edge
    cfg = AC.PATHS[path]
    tiles, valid = _bad_tiles(e, cfg["dec"])
    hip.attention_tiles(g.q, g.kc, g.vc, tiles, c.Hq, c.Hkv, c.scale, out=g.out, n_dec=e.n_dec if cfg["dec"] else 0,
                        seg_keys=cfg["seg_keys"], mixed=cfg["mixed"])
    g.check(path, valid)


# ----------------------------------------------------------------------------- wrapper argument checks
def test_wrappers_reject_what_the_kernels_would_misread(hip):
    c = AC.spread(2)
    d = _dev(c)
    q, kc, vc, tiles = d["q_cov"], d["kc"], d["vc"], d["tiles"]
    pos, slot = d["pos_cov"], d["slot_cov"]
    a = (c.Hq, c.Hkv, c.scale)
    T = q.shape[0]

    def token(**kw):
        args = dict(q=q, kc=kc, vc=vc, pos=pos, slot=slot)
        args.update(kw)
        out = args.pop("out", None)
        return hip.attention(args["q"], args["kc"], args["vc"], args["pos"], args["slot"], *a, out=out)

    def tiled(**kw):
        args = dict(q=d["q"], kc=kc, vc=vc, tiles=tiles)
        args.update(kw)
        out = args.pop("out", None)
        return hip.attention_tiles(args["q"], args["kc"], args["vc"], args["tiles"], *a, out=out)

    kc_t = kc.transpose(1, 2)                                  # right numel, not contiguous
    common = [
        (TypeError, dict(kc=kc.float())), (TypeError, dict(vc=vc.to(torch.float16))),
        (ValueError, dict(kc=kc_t, vc=vc.transpose(1, 2))),
        (ValueError, dict(kc=kc[:, :1].contiguous())),         # Hkv mismatch
        (ValueError, dict(vc=vc[:-1])),                        # vc shape != kc shape
        (ValueError, dict(kc=kc.view(AC.N_SLOTS, c.Hkv, -1, 64), vc=vc.view(AC.N_SLOTS, c.Hkv, -1, 64))),
        (ValueError, dict(kc=kc.view(-1, AC.MAX_CTX, AC.HD), vc=vc.view(-1, AC.MAX_CTX, AC.HD))),
        (ValueError, dict(kc=kc.cpu(), vc=vc.cpu())),
        (TypeError, dict(q=q.float())),
    ]
    for exc, kw in common:
        with pytest.raises(exc):
            token(**kw)
        with pytest.raises(exc):
            tiled(**{k: (d["q"].float() if k == "q" else v) for k, v in kw.items()})
    for exc, kw in [
        (TypeError, dict(pos=pos.long())), (TypeError, dict(slot=slot.long())),
        (ValueError, dict(pos=torch.stack([pos, pos], 1)[:, 0])), (ValueError, dict(slot=slot[:-1])),
        (ValueError, dict(pos=pos.cpu())), (ValueError, dict(slot=slot.cpu())),
        (TypeError, dict(out=torch.empty_like(q, dtype=torch.float32))),
        (ValueError, dict(out=torch.empty_like(q)[:-1])),
        (ValueError, dict(out=torch.empty_like(q).cpu())),
        (ValueError, dict(out=torch.empty(T, 2 * q.shape[1], dtype=q.dtype, device=DEV)[:, :q.shape[1]])),
        (ValueError, dict(q=q.view(T, c.Hq, AC.HD))),
    ]:
        with pytest.raises(exc):
            token(**kw)
    for exc, kw in [
        (ValueError, dict(tiles=tiles.cpu())), (ValueError, dict(tiles=tiles.long())),
        (ValueError, dict(tiles=tiles.t().contiguous().t())),
        (TypeError, dict(out=torch.empty_like(d["q"], dtype=torch.float16))),
        (ValueError, dict(out=torch.empty_like(d["q"])[:-1])),
        (ValueError, dict(out=torch.empty_like(d["q"]).cpu())),
    ]:
        with pytest.raises(exc):
            tiled(**kw)
    # an int64 pos used to be read as int32 pairs; the int32 form still runs
    o = token()
    torch.cuda.synchronize()
    assert o.shape == q.shape
