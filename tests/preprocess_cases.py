"""Constructions, plain references and comparisons for the classifier and
summarise kernels (the GPU tests in test_gpu_preprocess.py, the construction
and fault checks in test_preprocess_cases_cpu.py).

The exact cases keep every intermediate an integer far below 2^24, so fp32
arithmetic is exact in any order and the kernels' outputs are fixed bit for
bit: ``E`` over {-8, 0, 8}, ``W1t`` over {-1, 0, 1} and ``b1`` in multiples of
8 make every pre-activation a multiple of 8, where the kernel's tanh-GELU is
``max(z, 0)`` exactly (``gelu_f32`` below shows it, also with a 1 % error in
the exponential); integer ``pooled`` / ``W2`` / ``b2`` fix the logits; rows
``base_c + d_m`` with ``sum d_m = 0`` fix a conversation's bf16 mean.  Only the
mean's ``sum * fl(1 / n)`` rounds, and that is emulated in fp32.  The general
cases carry per-element bounds built from the data.  Every reference takes a
``fault`` name and then computes what a kernel with that single defect would;
the CPU tests assert that each comparison rejects it.  numpy and torch on the
CPU; nothing here touches a GPU."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import torch

f32 = np.float32
U = 2.0 ** -24                     # fp32 unit roundoff
TM, D = 64, 256                    # embed_pool: rows per tile, embedding dim
K0, K1 = float(f32(0.7978845608028654)), float(f32(0.044715))   # the kernel's fp32 constants
GELU_LIPSCHITZ = 1.13              # max |d/dz tanh-GELU| = 1.1289 (at z = 1.5)
GELU_F32_ULP24 = 1.83              # fp32 evaluation with an exact exp vs float64, in |z| 2^-24
# worst |device gelu_tanh(z) - float64| over the GELU probe on an MI355X, in |z| 2^-24 (at z = 4.2428; the fp32
# emulation with an exact exponential gives the same value there), and the exponential's relative error, in 2^-24,
# that an allowance of twice that worst case amounts to (see gelu_bound; docs/development.md records the measurement)
GELU_PROBE_WORST_ULP24 = 1.633
EXPF_ULP24 = (2 * GELU_PROBE_WORST_ULP24 - GELU_F32_ULP24) / 0.25
SAL_TABLE, SAL_MAX_STOP = 2048, 128
SAL_MULT = 2654435761
PRED_SENTINEL = -777


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error of n fp32 roundings in a row."""
    return n * U / (1.0 - n * U)


def bf16(a):
    """float64 / float32 array -> bf16 torch tensor (round to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def is_bf16(a64):
    return np.array_equal(bf16(a64).double().numpy(), np.asarray(a64, dtype=np.float64), equal_nan=True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, ref):
    """fp32 arrays equal bit for bit (NaN patterns and the sign of zero included)."""
    return got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


# ----------------------------------------------------------------------------- GELU
def gelu64(z):
    z = np.asarray(z, dtype=np.float64)
    return 0.5 * z * (1.0 + np.tanh(K0 * (z + K1 * z * z * z)))


def gelu_f32(x, exp_rel=0.0):
    """The kernel's ``gelu_tanh`` step by step in fp32, with a correctly
    rounded exponential scaled by ``1 + exp_rel``."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = f32(K0) * (x + f32(K1) * x * x * x)
        e = (np.exp((f32(2) * y).astype(np.float64)) * (1.0 + exp_rel)).astype(f32)
        t = f32(1) - f32(2) / (e + f32(1))
        return f32(0.5) * x * (f32(1) + t)


def gelu_bound(z, expf_ulp24=EXPF_ULP24):
    """|device gelu_tanh(z) - gelu64(z)| <= (1.83 + 0.25 eps) |z| 2^-24.

    1.83 |z| 2^-24 is the distance of the fp32 evaluation with a correctly
    rounded exponential from float64 (400 000 points in [-7, 7]; outside, fp32
    gives z or 0 exactly and float64 is within |z| 2^-24 of that).  The device
    adds the error of ``__expf``: with e = exp(2y), t = 1 - 2 / (e + 1) moves by
    2 e / (e + 1)^2 * eps <= eps / 2 for a relative error eps of e, and the
    result 0.5 z (1 + t) by at most 0.25 |z| eps.  eps has two parts.  The
    argument scaling u = fl(2y * log2 e) carries one rounding and the rounded
    constant, |du| <= 1.6 |u| 2^-24, i.e. a relative error 1.6 |2y| 2^-24 of
    exp2(u); where the result is sensitive, (1 - t^2) |2y| <= 0.9, so this part
    acts like eps <= 1.5 * 2^-24.  The hardware exp2's accuracy is not stated in
    the project's guides, so the device is measured instead: over the probe
    its worst deviation from float64 is 1.633 |z| 2^-24, no more than the fp32
    evaluation's own 1.83 (``expf_ulp24_needed`` is negative: the exponential's
    error does not show).  Twice the measured worst case is allowed,
    3.266 |z| 2^-24, which in the formula above is eps = EXPF_ULP24 = 5.74 * 2^-24:
    room for the argument scaling and a hardware exp2 good to two fp32 ulps."""
    return (GELU_F32_ULP24 + 0.25 * expf_ulp24) * np.abs(z) * U


@functools.lru_cache(maxsize=None)
def gelu_probe_case():
    """One-token messages whose ``E`` row has one non-zero element e_r (k = 0),
    ``W1t[c][0] = +-1`` and a fine ladder of biases: ``pooled[r][c]`` is the
    device's ``gelu_tanh(z)`` alone, ``z = fl(e_r w_c + b1_c)`` (one fp32 add of
    an exact product).  63 x 256 points: [-12, 12] densely, and +-32 .. +-1e30."""
    V, H, L = 64, 256, 4
    e = np.concatenate([np.linspace(-11.75, 11.75, 55), [32.0, -32.0, 1000.0, -1000.0, 1e10, -1e10, 1e30, -1e30]])
    e = bf16(e).double().numpy()
    B = len(e)
    assert B == V - 1
    E = np.zeros((V, D))
    E[0] = np.nan                                      # row 0: no token hashes to it
    E[1:, 0] = e
    W = np.zeros((H, D))
    W[:, 0] = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    b1 = np.linspace(-0.25, 0.25, H).astype(f32)
    hashes = np.full((B, L), 0, dtype=np.uint32)
    hashes[:, 0] = np.arange(1, V, dtype=np.uint32) + np.uint32(V) * np.arange(B, dtype=np.uint32) * 977
    z = (np.outer(e, W[:, 0]).astype(f32) + b1[None, :]).astype(f32)
    return SimpleNamespace(V=V, H=H, L=L, B=B, E=bf16(E), W1t=bf16(W), b1=torch.from_numpy(b1),
                           hashes=hashes, ntok=np.ones(B, dtype=np.int32), total=B, z=z)


def gelu_check(got, z, expf_ulp24=EXPF_ULP24):
    """(ok, worst): every value finite, within ``gelu_bound`` of float64, and
    for |z| >= 16 exactly z or a zero; ``worst`` is max |got - ref| / (|z| 2^-24)."""
    got64, z64 = got.astype(np.float64), z.astype(np.float64)
    if not np.isfinite(got).all():
        return False, float("inf")
    err = np.abs(got64 - gelu64(z64))
    big = np.abs(z64) >= 16
    exact = np.where(z64 > 0, got64 == z64, got64 == 0.0)
    nz = z64 != 0
    worst = float((err[nz] / (np.abs(z64[nz]) * U)).max())
    ok = bool((err <= gelu_bound(z64, expf_ulp24)).all() and exact[big].all() and (got64[~nz] == 0).all())
    return ok, worst


def expf_ulp24_needed(got, z):
    """The exponential's relative error (units of 2^-24) that explains the
    probe's worst deviation: max (err / |z| - 1.83 * 2^-24) / 0.25."""
    z64 = z.astype(np.float64)
    nz = (z64 != 0) & (np.abs(z64) < 16)
    err = np.abs(got.astype(np.float64) - gelu64(z64))
    return float(((err[nz] / (np.abs(z64[nz]) * U) - GELU_F32_ULP24) / 0.25).max())


# ----------------------------------------------------------------------------- embed_pool
def token_pattern(name, L):
    """Token counts per message that put messages where the tiling can go wrong."""
    p = {
        "inside": [5, 1, 17, 30, 3],                                   # one tile, 56 rows
        "edge63": [30, 34, 64, 10, 60, 2],                             # ends on row 63, starts on row 64, a straddler
        "straddle": [50, 40, 64, 64, 20, 27, 33],                      # two-part messages, power-of-two and not
        "parts66": [63, 66, 7],                                        # starts on row 63: 1 + 64 + 1 rows
        "parts128": [63, 128, 1],                                      # three parts, power-of-two count
        "parts150": [63, 150, 44],                                     # four parts; 257 rows: a last tile of 1 row
        "tail1": [64, 1],
        "tail63": [64, 20, 43],
        "zeros_edges": [0, 0, 0, 9, 55, 0, 12, 64, 0, 0, 0, 0, 0],     # leading, inner and trailing empty messages
        "zeros_run": [7] + [0] * 70 + [60, 3] + [0] * 66 + [64, 0, 0, 5],  # > 64 messages inside one tile
    }[name]
    assert max(p) <= L
    return np.asarray(p, dtype=np.int32)


def random_counts(B, L, seed):
    g = np.random.default_rng(seed)
    n = g.integers(1, L + 1, B)
    n[g.random(B) < 0.2] = 0
    if B >= 3:
        n[B // 2] = L
    return n.astype(np.int32)


def one_token_counts(B=5000):
    """One token per message (64 messages per tile, three levels of the 64-ary
    search) with empty runs: leading, longer than a window, trailing."""
    n = np.ones(B, dtype=np.int32)
    n[:3] = 0
    n[100:230] = 0
    n[1000:1065] = 0
    n[3000:3002] = 0
    n[B - 100:] = 0
    return n


# (name, V, H, L): every V, H (1, 2, 4 column-chunk blocks per tile) and L; B = 1 .. 513 cross the 256-wide in-block scan
EMBED_CASES = (
    ("inside", 64, 256, 64), ("edge63", 1024, 512, 64), ("straddle", 64, 1024, 64), ("parts66", 1024, 256, 160),
    ("parts128", 64, 512, 160), ("parts150", 1024, 1024, 160), ("tail1", 64, 256, 64), ("tail63", 1024, 256, 160),
    ("zeros_edges", 64, 512, 64), ("zeros_run", 1024, 256, 64),
    ("rand1", 64, 256, 64), ("rand3", 1024, 512, 160), ("rand255", 64, 256, 64), ("rand256", 1024, 1024, 64),
    ("rand257", 64, 512, 160), ("rand513", 1024, 256, 64), ("ones5000", 64, 256, 64),
)


def _counts(name, L):
    if name.startswith("rand"):
        return random_counts(int(name[4:]), L, seed=int(name[4:]))
    if name.startswith("ones"):
        return one_token_counts(int(name[4:]))
    return token_pattern(name, L)


def _hashes(ntok, L, V, g, poison):
    """[B][L] uint32 token hashes: random high bits, buckets anywhere but 0 and
    ``poison``; every slot past a message's count hashes to ``poison``."""
    B = len(ntok)
    bucket = g.integers(1, V - 1, (B, L)).astype(np.uint32)
    bucket[bucket >= poison] += 1                                         # 1 .. V-1 without poison
    h = (g.integers(0, 2 ** 32 // V, (B, L)).astype(np.uint32) * np.uint32(V)) | bucket
    h[np.arange(L)[None, :] >= ntok[:, None]] = np.uint32(poison + 5 * V)
    return h


@functools.lru_cache(maxsize=None)
def embed_case(name, V, H, L, seed=0):
    """The exact case: see the module docstring.  ``E`` row 0 is NaN (read for
    the rows a tile lacks, never to be used) and row ``poison`` is 1024
    throughout (behind every message's last token)."""
    g = np.random.default_rng(seed + 1000 * H + V)
    ntok = _counts(name, L)
    poison = V // 2 + 3
    E = g.integers(-1, 2, (V, D)).astype(np.float64) * 8.0
    E[0] = np.nan
    E[poison] = 1024.0
    W = g.integers(-1, 2, (H, D)).astype(np.float64)
    b1 = g.integers(-8, 9, H).astype(np.float64) * 8.0
    c = SimpleNamespace(name=name, V=V, H=H, L=L, B=len(ntok), ntok=ntok, poison=poison, E64=E, W64=W, b64=b1,
                        E=bf16(E), W1t=bf16(W), b1=torch.from_numpy(b1.astype(f32)),
                        hashes=_hashes(ntok, L, V, g, poison), exact=True, total=int(ntok.sum()))
    assert is_bf16(E) and is_bf16(W)
    return c


@functools.lru_cache(maxsize=None)
def exact_pipeline_weights(V, H, seed=3):
    """Exact classifier weights for a whole ``TextPipeline`` (tokens hash to any
    bucket: no NaN row, no poison): E, W1t, b1 as in ``embed_case``, ``W2`` over
    [-3, 3] and an integer ``b2``."""
    g = np.random.default_rng(seed)
    E = g.integers(-1, 2, (V, D)).astype(np.float64) * 8.0
    W = g.integers(-1, 2, (H, D)).astype(np.float64)
    b1 = g.integers(-8, 9, H).astype(np.float64) * 8.0
    W2 = g.integers(-3, 4, (H, 8)).astype(np.float64)
    b2 = g.integers(-5, 6, 8).astype(np.float64)
    return SimpleNamespace(V=V, H=H, E64=E, W64=W, b64=b1, W2_64=W2, b2_64=b2, E=bf16(E), W1t=bf16(W),
                           b1=torch.from_numpy(b1.astype(f32)), W2=torch.from_numpy(W2.astype(f32)),
                           b2=torch.from_numpy(b2.astype(f32)))


def text_case(w, hashes, ntok, L):
    """An exact embed case from a pipeline's own token hashes [B][L] and counts."""
    return SimpleNamespace(name="text", V=w.V, H=w.H, L=L, B=len(ntok), ntok=np.asarray(ntok, dtype=np.int32),
                           hashes=np.ascontiguousarray(hashes, dtype=np.uint32), E64=w.E64, W64=w.W64, b64=w.b64,
                           exact=True, total=int(np.sum(ntok)))


def exact_logits(w, pooled64):
    """float64 logits of exactly representable ``pooled`` rows (multiples of
    1/8: sums of multiples of 8 over a power-of-two count up to 64) and whether
    each row's every partial sum is exact in fp32: sum |x||w| + |b2| < 2^21."""
    mag = np.abs(pooled64) @ np.abs(w.W2_64) + np.abs(w.b2_64)
    return pooled64 @ w.W2_64 + w.b2_64, (mag < 2 ** 21).all(axis=1)


@functools.lru_cache(maxsize=None)
def embed_random_case(name, L, seed=0, vocab=65536, hidden=1024):
    """Token counts of ``name`` with random hashes, for weights given later
    (the production ``ClassifierWeights``)."""
    g = np.random.default_rng(seed + 77)
    ntok = _counts(name, L)
    B = len(ntok)
    h = g.integers(0, 2 ** 32, (B, L), dtype=np.uint64).astype(np.uint32)
    return SimpleNamespace(name=name, V=vocab, H=hidden, L=L, B=B, ntok=ntok, hashes=h, exact=False,
                           total=int(ntok.sum()))


def with_weights(c, E, W1t, b1):
    """``c`` with the float64 copies of bf16 / fp32 weight tensors."""
    c = SimpleNamespace(**vars(c))
    c.E64, c.W64, c.b64 = E.double().cpu().numpy(), W1t.double().cpu().numpy(), b1.double().cpu().numpy()
    return c


def _embed_rows(c, fault=None):
    """Per token row: the owning message and the float64 pre-activations
    (and sum |a||b| for the general bound)."""
    ntok, B = c.ntok.astype(np.int64), c.B
    own = np.repeat(np.arange(B), ntok)
    row_off = np.concatenate([[0], np.cumsum(ntok)])
    tok = np.arange(len(own)) - row_off[own]
    if fault == "token_off_by_one":
        tok = np.minimum(tok + 1, c.L - 1)
    mask = (c.V // 2 - 1) if fault == "half_mask" else c.V - 1
    X = c.E64[c.hashes[own, tok] & np.uint32(mask)]
    W = c.W64
    if fault == "swap_w1t_cols":
        W = W.copy()
        W[:, [3, 200]] = W[:, [200, 3]]
    if fault == "drop_k_chunk":
        W = W.copy()
        W[:, 40:48] = 0.0
    b = np.zeros_like(c.b64) if fault == "no_bias" else c.b64
    if fault == "boundary_row":            # the first row of a message, inside a tile, pooled into the message before it
        r = next(r for r in range(1, len(own)) if own[r] != own[r - 1] and r % TM)
        own = own.copy()
        own[r] = own[r - 1]
    return own, X, W, b


def embed_exact_ref(c, fault=None):
    """What ``embed_pool`` must write for an exact case: ``main`` [B][H] fp32
    and, for the messages of three or more tile parts whose count is no power of
    two, ``alts[m]``: the results of every order in which the parts can be added.

    Per (tile, message) part the row sum is an exact integer; the part's
    contribution is ``fl(sum * fl(1 / n))`` and the contributions meet in
    ``pooled`` by fp32 adds (one or two parts: order-free)."""
    assert c.exact
    own, X, W, b = _embed_rows(c, fault)
    z = X @ W.T + b
    if fault is None:
        assert np.array_equal(z, np.round(z / 8) * 8) and np.abs(z).max() < 2 ** 24 / TM
    hid = np.maximum(z, 0.0)                                              # GELU == ReLU on multiples of 8
    R = len(own)
    main = np.zeros((c.B, c.H), dtype=f32)
    if R == 0:
        return SimpleNamespace(main=main, alts={})
    r = np.arange(R)
    starts = np.flatnonzero((r % TM == 0) | (own != np.concatenate([[-1], own[:-1]])))
    part = np.add.reduceat(hid, starts, axis=0)
    assert fault is not None or np.abs(part).max() < 2 ** 24
    seg_msg = own[starts]
    seg_rows = np.diff(np.concatenate([starts, [R]]))
    n = seg_rows if fault == "tile_rows_mean" else c.ntok[seg_msg]
    inv = f32(1) / n.astype(f32)
    contrib = part.astype(f32) * inv[:, None]
    nparts = np.bincount(seg_msg, minlength=c.B)
    keep = np.ones(len(starts), dtype=bool)
    if fault in ("drop_part", "store_second"):
        for m in np.flatnonzero(nparts >= 2):
            s = np.flatnonzero(seg_msg == m)
            keep[s[1] if fault == "drop_part" else s[0]] = False          # stored, not added: the first part is lost
            if fault == "drop_part":
                break
    np.add.at(main, seg_msg[keep], contrib[keep])
    alts = {}
    for m in np.flatnonzero(nparts >= 3):
        s = np.flatnonzero((seg_msg == m) & keep)
        if c.ntok[m] & (c.ntok[m] - 1) == 0 or len(s) < 3:
            continue
        rows = []
        for perm in itertools.permutations(s):
            acc = np.zeros(c.H, dtype=f32)
            for i in perm:
                acc = acc + contrib[i]
            rows.append(acc)
        alts[int(m)] = np.unique(np.stack(rows), axis=0)
    return SimpleNamespace(main=main, alts=alts)


def embed_exact_check(got, ref):
    """Number of elements of ``got`` [B][H] that are not, bit for bit, a value the reference allows."""
    gb = bits(got)
    ok = gb == bits(ref.main)
    for m, a in ref.alts.items():
        ok[m] = (gb[m][None, :] == bits(a)).any(0)
    return int((~ok).sum())


def embed_general_ref(c, fault=None):
    """float64 ``pooled`` and its per-element bound for arbitrary weights.

    Per row: the MFMA chain and the bias add are at most 257 fp32 roundings
    of partial sums bounded by S = sum |a||b| + |b1|, so |dz| <= gamma_257 S;
    GELU carries that on with its Lipschitz constant 1.13 and adds
    ``gelu_bound(|z| + dz)``.  Per message: n rows are summed, scaled by
    fl(1 / n) (two roundings) and up to three parts added: gamma_(n+4) mean |g|."""
    own, X, W, b = _embed_rows(c, fault)
    ref = np.zeros((c.B, c.H))
    bound = np.zeros((c.B, c.H))
    if len(own) == 0:
        return ref, bound
    z = X @ W.T + b
    dz = gamma(D + 1) * (np.abs(X) @ np.abs(W).T + np.abs(b))
    g = gelu64(z)
    gb = GELU_LIPSCHITZ * dz + gelu_bound(np.abs(z) + dz)
    msgs = np.flatnonzero(np.bincount(own, minlength=c.B))
    starts = np.flatnonzero(own != np.concatenate([[-1], own[:-1]]))
    n = np.bincount(own, minlength=c.B)[msgs].astype(np.float64)[:, None]
    ref[msgs] = np.add.reduceat(g, starts, axis=0) / n
    bound[msgs] = np.add.reduceat(gb, starts, axis=0) / n + gamma(n + 4) * np.add.reduceat(np.abs(g), starts, axis=0) / n
    return ref, bound


def embed_general_check(got, ref, bound):
    """(ok, worst err / bound); rows of empty messages must be exactly zero."""
    err = np.abs(got.astype(np.float64) - ref)
    if not np.isfinite(got).all():
        return False, float("inf")
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    return bool((err <= bound).all()), worst


# ----------------------------------------------------------------------------- classify_head
HEAD_H = (256, 1024)
HEAD_B = (1, 3, 4, 5, 1024, 1025, 1026, 1027, 1028, 1041)   # one message per wave up to 1024, four above
# target logits of the planted rows: four-way tie; the maximum shared by columns 0 and 3; a two-way tie of 1 and 2;
# the largest logit in columns 4..7; a two-way tie of 0 and 1 under a larger column 6
HEAD_PLANTS = ((7, 7, 7, 7, 0, 0, 0, 0), (9, 1, 2, 9, -3, 4, 5, 6), (1, 4, 4, 2, 0, 1, 2, 3),
               (1, 2, 3, 0, 50, 60, 70, 80), (5, 5, 1, 0, 2, 2, 9, 2))


@functools.lru_cache(maxsize=None)
def head_case(B, H, seed=0):
    """Integer ``pooled`` [-4, 4], ``W2`` [-3, 3] and ``b2`` [-5, 5].  The first
    eight hidden units feed one logit each (``W2[:8] = I``), so a row's logits
    are set to any integers through ``pooled[row][:8]``: the first and the last
    rows of the batch get HEAD_PLANTS."""
    g = np.random.default_rng(seed + B * 7 + H)
    x = g.integers(-4, 5, (B, H)).astype(np.float64)
    W2 = g.integers(-3, 4, (H, 8)).astype(np.float64)
    W2[:8] = np.eye(8)
    b2 = g.integers(-5, 6, 8).astype(np.float64)
    planted = {}
    for rows in (range(len(HEAD_PLANTS)), (B - 1 - i for i in range(len(HEAD_PLANTS)))):
        for t, row in zip(HEAD_PLANTS, rows):
            if 0 <= row < B and row not in planted:
                planted[row] = t
    for row, t in planted.items():
        x[row, :8] += np.asarray(t, dtype=np.float64) - (x[row] @ W2 + b2)
    logits = x @ W2 + b2
    for row, t in planted.items():
        assert np.array_equal(logits[row], np.asarray(t, dtype=np.float64))
    assert np.abs(x).max() * 3 * H < 2 ** 24
    return SimpleNamespace(B=B, H=H, x=x.astype(f32), W2=W2.astype(f32), b2=b2.astype(f32), planted=planted)


def head_exact_ref(c, fault=None):
    """(logits [B][8] fp32, pred [B] int32): exact integers; the lowest of tied columns 0..3 wins."""
    W2 = c.W2.astype(np.float64)
    if fault == "swap_w2_cols":
        W2 = W2[:, [0, 2, 1, 3, 4, 5, 6, 7]]
    logits = c.x.astype(np.float64) @ W2 + c.b2.astype(np.float64)
    if fault == "shift_in_wave":            # message m of a four-message wave takes message m + 1's partial sums
        src = np.arange(c.B)
        src[(src % 4 != 3) & (src + 1 < c.B)] += 1
        logits = logits[src]
    first4 = logits[:, :4]
    if fault == "tie_high":
        pred = 4 - np.argmax(first4[:, ::-1], axis=1)
    else:
        pred = 1 + np.argmax(first4, axis=1)
    return logits.astype(f32), pred.astype(np.int32)


def head_check(logits, pred, ref):
    return same_bits(logits, ref[0]) and np.array_equal(pred, ref[1])


HEAD_GENERAL_SEED = 5


@functools.lru_cache(maxsize=None)
def head_general_case(B, H, seed=HEAD_GENERAL_SEED):
    """Random fp32 data.  ``bound = gamma_1024 * sum |x||w|``: a logit is
    H / 64 multiply-adds per lane, six shuffle adds and the bias add -- far
    fewer than 1024 roundings (about 24), each of a partial sum below
    sum |x||w| + |b2| with |b2| below sum |x||w| here.  ``decided``: rows whose top-two margin among
    columns 0..3 exceeds twice the bound, where ``pred`` is asserted."""
    g = np.random.default_rng(seed + B + H)
    x = (g.standard_normal((B, H)) * 0.3).astype(f32)
    W2 = (g.standard_normal((H, 8)) / H ** 0.5).astype(f32)
    b2 = (g.standard_normal(8) * 0.05).astype(f32)
    x64, w64 = x.astype(np.float64), W2.astype(np.float64)
    ref = x64 @ w64 + b2.astype(np.float64)
    mag = np.abs(x64) @ np.abs(w64)
    assert (np.abs(b2).max() <= mag).all()
    bound = gamma(1024) * mag
    top = np.sort(ref[:, :4], axis=1)
    decided = (top[:, 3] - top[:, 2]) > 2 * bound[:, :4].max(axis=1)
    return SimpleNamespace(B=B, H=H, x=x, W2=W2, b2=b2, ref=ref, bound=bound, decided=decided,
                           pred=(1 + np.argmax(ref[:, :4], axis=1)).astype(np.int32))


# ----------------------------------------------------------------------------- scan_rows
SCAN_B = (0, 1, 1023, 1024, 1025, 2049)
SCAN_STRIDES = (1, 16)


def scan_counts(B, seed=0):
    """Counts with zeros and one large value; the total stays below 2^31."""
    g = np.random.default_rng(seed + B)
    n = g.integers(0, 200, B).astype(np.int32)
    n[g.random(B) < 0.3] = 0
    if B:
        n[B // 3] = 1 << 29
    assert int(n.astype(np.int64).sum()) < 2 ** 31
    return n


# ----------------------------------------------------------------------------- summarise_project
SM_H, SM_DS, SM_ROWS = 1024, 256, 16
SUMMARISE_C = (1, 15, 16, 17, 33)
STATE_SENTINEL = -12345.0


def summarise_counts(C):
    """Messages per conversation: 1, 2, 16, 17 and 40 (the 16-row mean loop
    crosses rounds inside a conversation), empty ones, and for C > 32 a whole
    empty row block (conversations 16..31) between two non-empty ones."""
    cyc = (1, 2, 16, 0, 17, 40, 3, 0, 0, 5)
    n = np.asarray([cyc[c % len(cyc)] for c in range(C)], dtype=np.int32)
    if C > 32:
        n[16:32] = 0
    return n


@functools.lru_cache(maxsize=None)
def summarise_case(C, alpha, seed=0):
    """The exact case: ``pooled`` rows ``base_c + d_m`` (integers, the d_m of a
    conversation sum to zero), ``Pt`` over {-1, 0, 1}, integer ``state``; alpha
    0.5 or 0.75.  fl(n base fl(1 / n)) is within an fp32 ulp of base, so its bf16
    rounding is base; projection and EMA are then exact."""
    g = np.random.default_rng(seed + 31 * C)
    counts = summarise_counts(C)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    M = int(seg[-1])
    base = g.integers(-8, 9, (C, SM_H)).astype(np.float64)
    rows = np.zeros((M, SM_H))
    for c in range(C):
        n = int(counts[c])
        if n:
            d = g.integers(-16, 17, (n, SM_H)).astype(np.float64)
            d[-1] = -d[:-1].sum(0)
            rows[seg[c]:seg[c + 1]] = base[c] + d
            assert (rows[seg[c]:seg[c + 1]].sum(0) == n * base[c]).all()
    Pt = g.integers(-1, 2, (SM_DS, SM_H)).astype(np.float64)
    state = g.integers(-50, 51, (C, SM_DS)).astype(np.float64)
    first = (g.random(C) < 0.4).astype(np.int32)
    if C >= 15:
        first[0], first[1] = 1, 0
    assert is_bf16(base) and np.abs(rows).max() * 40 < 2 ** 24
    return SimpleNamespace(C=C, alpha=alpha, counts=counts, seg=seg, M=M, rows=rows.astype(f32), Pt64=Pt, Pt=bf16(Pt),
                           state=state.astype(f32), first=first, exact=True)


@functools.lru_cache(maxsize=None)
def summarise_random_case(C, alpha, seed=0):
    g = np.random.default_rng(seed + 17 * C)
    counts = summarise_counts(C)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    M = int(seg[-1])
    rows = g.standard_normal((M, SM_H)).astype(f32)
    Pt = bf16(g.standard_normal((SM_DS, SM_H)) / SM_H ** 0.5)
    state = g.standard_normal((C, SM_DS)).astype(f32)
    first = (g.random(C) < 0.4).astype(np.int32)
    return SimpleNamespace(C=C, alpha=alpha, counts=counts, seg=seg, M=M, rows=rows, Pt64=Pt.double().numpy(), Pt=Pt,
                           state=state, first=first, exact=False)


def _bf16_step(a):
    """Spacing of bf16 at |a| (float64 array)."""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -126))) - 7)


def summarise_ref(c, fault=None):
    """(state' [C][DS] float64, bound): mean in float64 -> bf16 -> Pt . mean ->
    ``first ? proj : alpha state + (1 - alpha) proj`` with the fp32 alpha.

    The kernel rounds its fp32 mean to bf16; that mean is within
    gamma_(n+2) mean |x| of the float64 one, so the two roundings differ, by one
    bf16 step, only where the float64 mean lies that close to a rounding
    boundary: the bound counts |Pt_k| ulp_bf16(mean_k) for those k alone (never
    more than the sum over all k), plus gamma_1028 sum |Pt_k||mean_k| for the
    MFMA chain and the K-quarter adds, scaled by 1 - alpha in the EMA, plus three
    roundings of the EMA's own terms.  An exact case has bound 0."""
    C, a = c.C, float(f32(c.alpha))
    b = float(f32(1) - f32(c.alpha))
    if fault == "swap_alpha":
        a, b = b, a
    rows = c.rows.astype(np.float64)
    mean = np.zeros((C, SM_H))
    dmean = np.zeros((C, SM_H))
    for i in range(C):
        lo, hi = int(c.seg[i]), int(c.seg[i + 1])
        if hi > lo:
            mean[i] = rows[lo:hi].mean(0)
            dmean[i] = gamma(hi - lo + 2) * np.abs(rows[lo:hi]).mean(0)
        elif fault == "empty_mean_stale" and i > 0:
            mean[i] = mean[i - 1]
    mb = bf16(mean).double().numpy()
    step = _bf16_step(np.abs(mean) + dmean)
    # distance of the float64 mean from the nearest bf16 rounding boundary (the midpoints of the grid)
    frac = np.abs(mean) / step
    to_mid = np.abs(frac - np.floor(frac) - 0.5) * step
    flips = (to_mid <= dmean) & (dmean > 0)
    P = c.Pt64
    if fault == "drop_k_quarter":
        P = P.copy()
        P[:, 256:512] = 0.0
    proj = mb @ P.T
    perr = (step * flips) @ np.abs(c.Pt64).T + gamma(SM_H + 4) * (np.abs(mb) @ np.abs(c.Pt64).T)
    old = c.state.astype(np.float64)
    ema = a * old + b * proj
    first = np.zeros(C, dtype=bool) if fault == "ignore_first" else c.first.astype(bool)
    out = np.where(first[:, None], proj, ema)
    bound = np.where(first[:, None], perr, abs(b) * perr + 3 * U * (np.abs(a * old) + np.abs(b * proj)))
    if fault == "swap_rows" and C >= 2:
        out = out.copy()
        out[[0, C - 1]] = out[[C - 1, 0]]
    if c.exact:                                        # the fp32 mean rounds to base_c: nothing to allow
        bound = np.zeros_like(bound)
    return out, bound


def summarise_check(got, ref, bound, exact):
    """(ok, worst err / bound); an exact case compares bit for bit."""
    if exact:
        return same_bits(got, ref.astype(f32)), 0.0
    if not np.isfinite(got).all():
        return False, float("inf")
    err = np.abs(got.astype(np.float64) - ref)
    return bool((err <= bound).all()), float((err / np.maximum(bound, 1e-300)).max())


# ----------------------------------------------------------------------------- salient_topk
def salient_ref(hashes, ntok, seg, stop, K, fault=None):
    """Per conversation the top K of (count desc, first occurrence asc) over
    its tokens that are not stop words, hash 0 folded into 1 after the stop
    test; zero-filled past the distinct tokens.  Returns (hash [C][K] uint32,
    count [C][K] int32, overflow [C] int32); a conversation of more than 2048
    distinct tokens is flagged and its rows are not to be compared."""
    C = len(seg) - 1
    stop = set(int(s) for s in stop)
    oh = np.zeros((C, K), dtype=np.uint32)
    oc = np.zeros((C, K), dtype=np.int32)
    ov = np.zeros(C, dtype=np.int32)
    for c in range(C):
        cnt, first, i = {}, {}, 0
        hi = int(seg[c + 1]) + (1 if fault == "segment_off_by_one" and seg[c + 1] < len(ntok) else 0)
        for m in range(int(seg[c]), hi):
            for t in hashes[m, :int(ntok[m])].tolist():
                i += 1
                if t in stop and fault != "count_stop":
                    continue
                if t == 0 and fault != "no_fold":
                    t = 1
                cnt[t] = cnt.get(t, 0) + 1
                first.setdefault(t, i)
        if len(cnt) > SAL_TABLE:
            ov[c] = 1
            continue
        key = (lambda kv: (-kv[1], kv[0])) if fault == "tie_by_hash" else (lambda kv: (-kv[1], first[kv[0]]))
        for k, (h, n) in enumerate(sorted(cnt.items(), key=key)[:K]):
            oh[c, k], oc[c, k] = h, n
    return oh, oc, ov


def salient_check(got, ref):
    gh, gc, gv = got
    rh, rc, rv = ref
    if not np.array_equal(np.asarray(gv, dtype=np.int32), rv):
        return False
    keep = rv == 0
    return np.array_equal(np.asarray(gh, dtype=np.uint32)[keep], rh[keep]) and np.array_equal(np.asarray(gc)[keep], rc[keep])


def colliding_keys(home, count):
    """``count`` distinct non-zero hashes whose table slot (h * SAL_MULT) & 2047 is ``home``."""
    inv = pow(SAL_MULT, -1, 2 ** 32)
    keys = [(inv * (home + SAL_TABLE * j)) % 2 ** 32 for j in range(1, count + 1)]
    assert all(k and (k * SAL_MULT) % 2 ** 32 % SAL_TABLE == home for k in keys) and len(set(keys)) == count
    return keys


def _pack_messages(msgs, L, stride, stride_col=5):
    """Token lists -> hashes [M][L] uint32 (0xDEAD past the count) and the
    counts, alone (stride 1) or as column ``stride_col`` of an [M][stride] table."""
    M = len(msgs)
    h = np.full((max(M, 1), L), 0xDEAD, dtype=np.uint32)
    tab = np.full((max(M, 1), stride), -99, dtype=np.int32)
    col = 0 if stride == 1 else stride_col
    for m, t in enumerate(msgs):
        assert len(t) <= L
        h[m, :len(t)] = t
        tab[m, col] = len(t)
    return h, tab, col


@functools.lru_cache(maxsize=None)
def salient_case(name):
    """Named cases; each has hashes, the count table (``ntok = tab[:, col]``,
    row stride ``stride``), ``seg``, ``stop`` and ``K``."""
    g = np.random.default_rng(sum(map(ord, name.split("_")[0])))   # one data set per family
    L, stride, K = 8, 1, 5
    stop = [3, 4]
    convs = []                                        # conversations: lists of messages (token lists)

    def msgs(n, alphabet, lmax=L, empty=0.25):
        out = []
        for _ in range(n):
            k = 0 if g.random() < empty else int(g.integers(1, lmax + 1))
            out.append([int(x) for x in g.choice(alphabet, k)])
        return out

    if name in ("paths", "paths_stride16", "paths_k1", "paths_k64"):
        # sequential path (300 messages) beside the flat path at its limit (256) and just past it (257);
        # tokens 0 and 1 both present (0 folds into 1), stop words, an empty conversation, a single message
        alpha = list(range(0, 40))
        convs = [msgs(300, alpha), msgs(256, alpha), [], msgs(257, alpha), [[0, 1, 0, 7]], msgs(3, alpha)]
        stride = 16 if name == "paths_stride16" else 1
        K = {"paths_k1": 1, "paths_k64": 64}.get(name, 5)          # 64 > the 38 distinct tokens: zero-filled
    elif name in ("stop128", "stop129"):
        n = int(name[4:])                                          # 128: the LDS copy; 129: read from global memory
        stop = [1000 + 3 * i for i in range(n)]
        alpha = stop[::7] + stop[-2:] + list(range(1, 30))
        convs = [msgs(40, alpha, empty=0.1), msgs(3, alpha)]
    elif name in ("distinct2048", "distinct2049"):
        n = int(name[8:])
        L = 128
        toks = [int(x) for x in g.permutation(np.arange(5, 5 + n))]    # n distinct tokens, none a stop word
        toks += toks[100:110] + toks[100:103] + [3, 4]                 # repeats give a top-K; stop words take no slot
        convs = [[toks[i:i + L] for i in range(0, len(toks), L)], [[9, 9, 8]]]
    elif name == "probe_chain":
        # 40 keys with home slot 2040: the chain runs over the table's end into slots 0..31
        keys = colliding_keys(2040, 40)
        L = 64
        toks = keys + keys[10:20] + keys[35:] + keys[38:]
        convs = [[toks[:L], toks[L:]], [keys[:3]]]
    else:
        raise KeyError(name)
    flat = [m for cv in convs for m in cv]
    seg = np.concatenate([[0], np.cumsum([len(cv) for cv in convs])]).astype(np.int32)
    h, tab, col = _pack_messages(flat, L, stride)
    return SimpleNamespace(name=name, hashes=h, tab=tab, col=col, stride=stride, ntok=tab[:, col].copy(), seg=seg,
                           stop=np.asarray(stop, dtype=np.uint32), K=K, L=L, C=len(convs))


SALIENT_CASES = ("paths", "paths_stride16", "paths_k1", "paths_k64", "stop128", "stop129", "distinct2048",
                 "distinct2049", "probe_chain")
