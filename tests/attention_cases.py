"""Shared attention probes for the attention tests (the HIP kernels and the
CPU construction checks): one edge set of decode contexts and prefill tiles,
input builders whose fp64 result is known by construction (needle, ladder,
twin needles) or spread over many keys, the fp64 reference and the derived
error bounds.  Plain torch on the CPU; nothing here touches a GPU."""
import functools

import numpy as np
import torch

from llm_message_queue_amd.ops.llama_ops import make_tiles

HD = 128
MAX_CTX = 320
N_SLOTS = 4
SCALE = 128 ** -0.5
U = 2.0 ** -8                      # bf16 unit roundoff used by the bounds

# ctx = pos + 1.  8 | 9: the decode kernel's 8-key pass; 32 | 33 and 64 | 65: its
# 32-key load group and 64-key block (and the segment kernel's key blocks)
DEC_CTX = (1, 2, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 320)
# (pos0, n).  (24,16), (56,16), (120,16) straddle a 32- or 64-key block edge:
# their earlier rows have no live key in the last block.  (304,16) ends at MAX_CTX
PREFILL = ((0, 1), (0, 2), (0, 15), (0, 16), (24, 16), (31, 2), (56, 16), (63, 2), (120, 16), (304, 16))
LONG_SEG = (40, 33)                # cut into tiles by make_tiles
EDGE_KEYS = (15, 16, 31, 32, 63, 64, 127, 128)
TWIN_PAIRS = ((31, 32), (32, 31), (63, 64), (64, 63), (5, 70), (70, 5), (20, 40), (40, 20), (3, 100), (40, 50))

# kernel paths: api, decode tiles on the decode kernel, one mixed launch, keys per segment block
PATHS = {
    "token": dict(api="token"),
    "seg32": dict(api="tiles", dec=False, mixed=False, seg_keys=32),
    "seg64": dict(api="tiles", dec=False, mixed=False, seg_keys=64),
    "dec+seg": dict(api="tiles", dec=True, mixed=False, seg_keys=32),
    "mixed32": dict(api="tiles", dec=True, mixed=True, seg_keys=32),
    "mixed64": dict(api="tiles", dec=True, mixed=True, seg_keys=64),
}


class EdgeSet:
    """tiles int32 [n, 4] = (first row, n, slot, first position), decode
    (1-token) tiles first; per-row ``pos`` / ``slot`` (-1 / 0 on a row that no
    tile covers) and the ``covered`` mask."""

    def __init__(self, tiles, n_dec, T):
        self.tiles = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 4)
        self.n_dec = int(n_dec)
        self.T = int(T)
        self.pos, self.slot = expand_tiles(self.tiles, self.T)
        self.covered = self.pos >= 0
        self.dec_row = torch.zeros(self.T, dtype=torch.bool)
        self.dec_row[torch.from_numpy(self.tiles[:self.n_dec, 0]).long()] = True


def expand_tiles(tiles, T):
    """Per-row (pos, slot) of a tile list, the way RefOps.attention_tiles
    expands it; rows of no tile get pos -1."""
    pos = torch.full((T,), -1, dtype=torch.long)
    slot = torch.zeros(T, dtype=torch.long)
    for r0, n, sl, p0 in np.asarray(tiles).tolist():
        assert (pos[r0:r0 + n] < 0).all(), "tiles overlap"
        pos[r0:r0 + n] = torch.arange(p0, p0 + n)
        slot[r0:r0 + n] = sl
    return pos, slot


@functools.lru_cache(maxsize=None)
def edge_set(ctx_limit=MAX_CTX):
    """The shared edge set (``ctx_limit``: only tiles whose context ends at or
    before it).  Segments take their token rows in a shuffled order, so rows
    are not in tile or slot order; row 0, one row after every sixth segment and
    the last two rows belong to no tile."""
    segs = [(c - 1, 1) for c in DEC_CTX] + list(PREFILL) + [LONG_SEG]
    n_dec_all = len(DEC_CTX)
    keep = [i for i, (p0, n) in enumerate(segs) if p0 + n <= ctx_limit]
    n_dec = sum(1 for i in keep if i < n_dec_all)
    segs = [segs[i] for i in keep]
    m = next(m for m in (7, 11, 13, 17, 19, 23) if np.gcd(m, len(segs)) == 1)
    order = [(i * m + 3) % len(segs) for i in range(len(segs))]
    start, row = {}, 1
    for k, i in enumerate(order):
        start[i] = row
        row += segs[i][1]
        if k % 6 == 5:
            row += 1
    T = row + 2
    idx = range(len(segs))
    tiles = make_tiles([start[i] for i in idx], [segs[i][1] for i in idx], [i % N_SLOTS for i in idx],
                       [segs[i][0] for i in idx])
    assert (tiles[:n_dec, 1] == 1).all()
    return EdgeSet(tiles, n_dec, T)


@functools.lru_cache(maxsize=None)
def sweep_set():
    """One slot, context 128: 16 decode rows at position 127 and one 16-row
    prefill tile at 112..127, so 8 heads x 16 rows can address every key."""
    tiles = [(r, 1, 1, 127) for r in range(16)] + [(16, 16, 1, 112)]
    return EdgeSet(np.asarray(tiles), 16, 33)


# ----------------------------------------------------------------------------- inputs
def v_code(S, Hkv, C=MAX_CTX):
    """V[slot, g, key, d]: non-zero integers in [-31, 31] (exact in bf16) from
    a fixed hash, so two keys of a head agree in about 1 dim in 62."""
    s, g, k, d = np.ogrid[:S, :Hkv, :C, :HD]
    M = np.uint64(0xFFFFFFFF)
    x = (k.astype(np.uint64) * np.uint64(0x9E3779B1) + d.astype(np.uint64) * np.uint64(0x85EBCA6B)
         + g.astype(np.uint64) * np.uint64(0xC2B2AE35) + s.astype(np.uint64) * np.uint64(0x27D4EB2F)) & M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & M
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & M
    x ^= x >> np.uint64(15)
    m = (x % np.uint64(62)).astype(np.int64)
    v = np.where(m < 31, m - 31, m - 30)
    return torch.from_numpy(v).to(torch.bfloat16)


def sign_keys(S, Hkv, seed, C=MAX_CTX):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (S, Hkv, C, HD), generator=g) * 2 - 1).to(torch.bfloat16)


class Case:
    def __init__(self, name, edge, Hq, Hkv, q, kc, vc, target=None, target2=None, scale=SCALE):
        self.name, self.edge, self.Hq, self.Hkv, self.scale = name, edge, Hq, Hkv, scale
        self.q, self.kc, self.vc = q.contiguous(), kc.contiguous(), vc.contiguous()
        self.target, self.target2 = target, target2
        self._ref = None

    def ref(self):
        """(ref, A, weights) of ``reference``, computed once."""
        if self._ref is None:
            e = self.edge
            self._ref = reference(self.q, self.kc, self.vc, e.pos, e.slot, self.Hq, self.Hkv, self.scale)
        return self._ref


def _filler_q(T, Hq, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, Hq, HD, generator=g).to(torch.bfloat16)


def needle_targets(edge, Hq, Hkv):
    """target[row, head]: heads cycle through the row's own position, key 0,
    every visible block-edge key and a few interior keys; the heads of a group
    (consecutive entries) disagree whenever the row sees enough keys."""
    tgt = torch.full((edge.T, Hq), -1, dtype=torch.long)
    rank = 0
    for t in range(edge.T):
        p = int(edge.pos[t])
        if p < 0:
            continue
        cand = []
        for c in [p, 0] + [e for e in EDGE_KEYS if e <= p] + [p // 2, p - 1, p // 3, 1]:
            if 0 <= c <= p and c not in cand:
                cand.append(c)
        must = len({p, 0, *[e for e in EDGE_KEYS if e <= p]})   # own position, key 0, visible edges
        if must <= Hq:
            cand = cand[:Hq]                                # then every one of them is some head's target
        for h in range(Hq):
            tgt[t, h] = cand[(rank * 3 + h) % len(cand)]
        rank += 1
    return tgt


def _gather_k(kc, edge, tgt, Hq, Hkv):
    """K[slot[row], head's kv head, tgt[row, head]] as float [T, Hq, 128]
    (zero where tgt < 0)."""
    G = Hq // Hkv
    g = (torch.arange(Hq) // G)[None, :].expand(edge.T, Hq)
    s = edge.slot[:, None].expand(edge.T, Hq)
    k = kc.float()[s, g, tgt.clamp(min=0)]
    return torch.where((tgt >= 0)[..., None], k, torch.zeros(()))


@functools.lru_cache(maxsize=None)
def needle(Hkv=2, group=4, sweep=False, ctx_limit=MAX_CTX):
    """Probe 1: q = 4 K[target]; the reference is V[target]."""
    Hq = Hkv * group
    if sweep:
        assert Hq == 8
        edge = sweep_set()
        tgt = (torch.arange(edge.T)[:, None] % 16) * 8 + torch.arange(8)[None, :]
        tgt[~edge.covered] = -1
    else:
        edge = edge_set(ctx_limit)
        tgt = needle_targets(edge, Hq, Hkv)
    kc, vc = sign_keys(N_SLOTS, Hkv, seed=11), v_code(N_SLOTS, Hkv)
    q = 4.0 * _gather_k(kc, edge, tgt, Hq, Hkv)
    q = torch.where(edge.covered[:, None, None], q, _filler_q(edge.T, Hq, 12).float())
    return Case("needle", edge, Hq, Hkv, q.to(torch.bfloat16).reshape(edge.T, Hq * HD), kc, vc, target=tgt)


@functools.lru_cache(maxsize=None)
def ladder(a=8, Hkv=2, group=4):
    """Probe 2: the score grows with the key position (32 a scale per step)
    over the WHOLE cache, so every key a row must not see beats every key it
    may see; the reference is V[own position] (a = 8) or a geometric mix of the
    last few keys (a = 2)."""
    Hq = Hkv * group
    edge = edge_set()
    p = torch.arange(MAX_CTX)
    krow = torch.zeros(MAX_CTX, HD)
    krow[:, 0:32] = (p // 16)[:, None].float()
    krow[:, 32:64] = (p % 16)[:, None].float()
    kc = krow.to(torch.bfloat16)[None, None].expand(N_SLOTS, Hkv, MAX_CTX, HD).contiguous()
    qrow = torch.zeros(HD)
    qrow[0:32] = 16.0 * a
    qrow[32:64] = float(a)
    q = qrow.to(torch.bfloat16)[None, None].expand(edge.T, Hq, HD).reshape(edge.T, Hq * HD)
    tgt = edge.pos[:, None].expand(edge.T, Hq).clone()
    return Case(f"ladder{a}", edge, Hq, Hkv, q, kc, v_code(N_SLOTS, Hkv), target=tgt)


@functools.lru_cache(maxsize=None)
def twins(Hkv=2, group=4):
    """Probe 3: q = 4 (K[t1] + K[t2]): both keys score exactly the same; the
    reference is (V[t1] + V[t2]) / 2.  Pairs sit on either side of key 32 and
    of key 64 (a later block ties the running max) and inside one block."""
    Hq = Hkv * group
    edge = edge_set()
    t1 = torch.full((edge.T, Hq), -1, dtype=torch.long)
    t2 = t1.clone()
    rank = 0
    for t in range(edge.T):
        p = int(edge.pos[t])
        if p < 0:
            continue
        pairs = [pr for pr in TWIN_PAIRS if max(pr) <= p] or [(0, p)]
        for h in range(Hq):
            t1[t, h], t2[t, h] = pairs[(rank + h) % len(pairs)]
        rank += 1
    kc, vc = sign_keys(N_SLOTS, Hkv, seed=21), v_code(N_SLOTS, Hkv)
    q = 4.0 * (_gather_k(kc, edge, t1, Hq, Hkv) + _gather_k(kc, edge, t2, Hq, Hkv))
    q = torch.where(edge.covered[:, None, None], q, _filler_q(edge.T, Hq, 22).float())
    return Case("twins", edge, Hq, Hkv, q.to(torch.bfloat16).reshape(edge.T, Hq * HD), kc, vc, target=t1, target2=t2)


@functools.lru_cache(maxsize=None)
def spread(sigma=0.5, Hkv=2, group=4):
    """Probe 4: unit-variance random K and V, q ~ sigma N(0, 1)."""
    Hq = Hkv * group
    edge = edge_set()
    g = torch.Generator().manual_seed(31 + int(sigma * 8) + 100 * Hkv)
    kc = torch.randn(N_SLOTS, Hkv, MAX_CTX, HD, generator=g).to(torch.bfloat16)
    vc = torch.randn(N_SLOTS, Hkv, MAX_CTX, HD, generator=g).to(torch.bfloat16)
    q = (sigma * torch.randn(edge.T, Hq * HD, generator=g)).to(torch.bfloat16)
    return Case(f"spread{sigma}", edge, Hq, Hkv, q, kc, vc)


# ----------------------------------------------------------------------------- reference
def _rows(q, kc, vc, pos, slot, Hq, Hkv, scale):
    """Per covered row: (t, scores [Hq, n], V [Hq, n, 128]) in float64."""
    G = Hq // Hkv
    qd = q.double().view(q.shape[0], Hq, HD)
    for t in range(q.shape[0]):
        n = int(pos[t]) + 1
        if n < 1:
            continue
        K = kc[int(slot[t]), :, :n].double().repeat_interleave(G, dim=0)
        V = vc[int(slot[t]), :, :n].double().repeat_interleave(G, dim=0)
        yield t, torch.einsum("hd,hnd->hn", qd[t], K) * scale, V


def reference(q, kc, vc, pos, slot, Hq, Hkv, scale):
    """float64 attention of the bf16 input values.  Returns (ref [T, Hq, 128],
    A [T, Hq, 128] = sum_j p_j |v_jd|, weights [T, Hq, max_ctx]); rows with
    pos < 0 are zero."""
    T, C = q.shape[0], kc.shape[2]
    ref = torch.zeros(T, Hq, HD, dtype=torch.float64)
    A = torch.zeros_like(ref)
    W = torch.zeros(T, Hq, C, dtype=torch.float64)
    for t, sc, V in _rows(q, kc, vc, pos, slot, Hq, Hkv, scale):
        p = torch.softmax(sc, dim=-1)
        ref[t] = torch.einsum("hn,hnd->hd", p, V)
        A[t] = torch.einsum("hn,hnd->hd", p, V.abs())
        W[t, :, :p.shape[1]] = p
    return ref, A, W


def _bf16(x):
    return x.float().to(torch.bfloat16).double()


def emulate_segment(q, kc, vc, pos, slot, Hq, Hkv, scale):
    """What a correct segment kernel computes, up to its fp32 arithmetic: P
    rounded to bf16 before P V, the row sum taken of the unrounded p, one
    bf16 rounding of the output."""
    out = torch.zeros(q.shape[0], Hq, HD, dtype=torch.float64)
    for t, sc, V in _rows(q, kc, vc, pos, slot, Hq, Hkv, scale):
        p = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        out[t] = _bf16(torch.einsum("hn,hnd->hd", _bf16(p), V) / p.sum(-1, keepdim=True))
    return out


# ----------------------------------------------------------------------------- bounds
def seg_bound(ref, A):
    """Segment kernel: P in bf16 (u A) + one output rounding (u |ref| <= u A);
    the extra quarter covers fp32 accumulation over <= 320 keys (~2^-16 A) and
    the exp2 / score error (~2^-13 A)."""
    return 1.25 * 2.0 ** -7 * A


def fp32_bound(ref, A):
    """Per-token and decode kernels: P stays fp32; one output rounding."""
    return U * ref.abs() + 2.0 ** -11 * A


def row_bound(path, edge, ref, A):
    """The bound of every output element under ``path``: decode rows run the
    fp32 decode kernel where the path sends them there."""
    cfg = PATHS[path]
    if cfg["api"] == "token":
        return fp32_bound(ref, A)
    b = seg_bound(ref, A)
    if cfg["dec"]:
        b = torch.where(edge.dec_row[:, None, None], fp32_bound(ref, A), b)
    return b


def nearest_key(out_row, vc, slot, g, ctx=MAX_CTX):
    """The key whose V row is nearest to ``out_row`` [128] (what a wrong
    index or swizzle read instead)."""
    d = (vc[slot, g, :ctx].double() - out_row.double()[None, :]).abs().sum(-1)
    return int(d.argmin())
