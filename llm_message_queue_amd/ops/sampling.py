"""Host twin of the LM head's sampling noise (``csrc/kernels/sample_noise.h``
holds the contract and the device code).

Temperature sampling is ``argmax_n(logit_n / T + G_n)`` with i.i.d. standard
Gumbel ``G_n`` -- an exact draw from ``softmax(logits / T)``.  ``G_n`` is a
pure function of (request seed, index of the generated token, vocabulary
column), so a request's tokens are reproducible whatever step, row, batch or
GPU computed them.  The integer part (row keys, bits) equals the device's
bit for bit; the Gumbel values are the same two-branch formula in float64.

Top-k / top-p: :func:`truncation_keep` and :func:`sample_truncated_reference`
are the twin of ``csrc/kernels/sample_truncate_kernels.h`` (the selection
over whole groups of equal bf16 logits, then the same draw over what is kept).

Log-probabilities: :func:`logprob_reference` is the float64 twin of
``csrc/kernels/logprob_kernels.h`` and :func:`logprob_bound` the bound on the
device's distance from it, derived there.

Penalties: :func:`penalise_reference` is the bit-exact twin of the edit in
``csrc/kernels/penalty_kernels.h`` (over bf16 bit patterns, so padding and
non-finite values compare too), :func:`penalised_pick_reference` that of its
greedy pick.

Allow-lists and biases: :func:`logit_edit_reference` is the bit-exact twin of
``csrc/kernels/logit_edit_kernels.h``; ``min_p`` is one more keep rule of
:func:`truncation_keep`, evaluated in float32 exactly as the device does.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
SERIES_BELOW = 2.0 ** -12            # E = v + v*v/2 + v*v*v/3 below, -log(1 - v) from here on


def fmix32(h) -> np.ndarray:
    """The murmur3 finaliser over uint32 arrays."""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def splitmix64(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64) + np.uint64(GOLDEN)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def row_keys(seed, gidx) -> np.ndarray:
    """uint32 [n][2] = (k0, k1) of generated token ``gidx`` (its index within
    the request) under ``seed``; both broadcast."""
    with np.errstate(over="ignore"):
        s = np.asarray(seed, dtype=np.uint64)
        g = np.asarray(gidx, dtype=np.int64).astype(np.uint64)
        z = np.atleast_1d(splitmix64(s + np.uint64(GOLDEN) * (g + np.uint64(1))))
    out = np.empty((len(z), 2), dtype=np.uint32)
    out[:, 0] = (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out[:, 1] = (z >> np.uint64(32)).astype(np.uint32)
    return out


def noise_bits(keys, cols) -> np.ndarray:
    """uint32 [n_keys][n_cols]: ``m = fmix32(fmix32(n ^ k0) + k1)``."""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    n = np.asarray(cols, dtype=np.uint32).reshape(1, -1)
    with np.errstate(over="ignore"):
        return fmix32(fmix32(n ^ keys[:, 0:1]) + keys[:, 1:2])


def exponential_series(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return v * (1.0 + v * (0.5 + v / 3.0))


def exponential_log(v) -> np.ndarray:
    return -np.log(1.0 - np.asarray(v, dtype=np.float64))


def gumbel_from_bits(m) -> np.ndarray:
    """float64 standard Gumbel of the bits ``m``: ``v = (m + 0.5) * 2^-32``,
    ``E = -log1p(-v)`` by the contract's two branches, ``G = -log(E)``."""
    v = (np.asarray(m, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32
    small = v < SERIES_BELOW
    e = np.where(small, exponential_series(v), exponential_log(np.where(small, 0.5, v)))
    return -np.log(e)


def gumbel(keys, cols) -> np.ndarray:
    return gumbel_from_bits(noise_bits(keys, cols))


def inv_temperature(temperature) -> np.ndarray:
    """float32 1 / T, 0 for a greedy row (T <= 0)."""
    t = np.asarray(temperature, dtype=np.float64)
    return np.where(t > 0, 1.0 / np.where(t > 0, t, 1.0), 0.0).astype(np.float32)


def min_p_log(min_p) -> np.ndarray:
    """float32 ``log(permille / 1000)`` of ``min_p`` rounded to thousandths:
    what the truncated sampler takes as ``log_min_p``.  -inf (off) for a value
    that rounds to 0 permille, 0.0 for 1.0."""
    pm = np.rint(np.clip(np.nan_to_num(np.asarray(min_p, dtype=np.float64)), 0.0, 1.0) * 1000.0)
    with np.errstate(divide="ignore"):
        return np.log(pm / 1000.0).astype(np.float32)


def truncation_keep(logits_bf16, inv_temp, top_k, top_p, min_p=None, log_min_p=None) -> np.ndarray:
    """bool [V]: the columns top-k, top-p and then min-p keep of one row of bf16 logits
    (an array of bf16-representable values), in float64 -- the twin of the
    selection in ``csrc/kernels/sample_truncate_kernels.h``, which holds the
    contract.  The distinct finite values in descending order are groups with
    their counts; top-k keeps a group iff fewer than ``top_k`` columns lie in
    the groups before it (0: off), top-p a group top-k kept iff the mass
    ``count * exp((value - max) * inv_temp)`` of the kept groups before it is
    below ``top_p`` times their total (>= 1: off); the first group always
    stays.  A NaN or infinite logit is never kept.  ``log_min_p`` (float32,
    what the kernel takes; or ``min_p``, a ratio converted by
    :func:`min_p_log`; None or -inf: off): a column of value ``v`` stays iff
    ``fl(fl(v - max) * inv_temp) >= log_min_p``, both operations in float32 as
    on the device, so this rule is exact."""
    if log_min_p is None and min_p is not None:
        log_min_p = min_p_log(min_p)
    v = np.asarray(logits_bf16, dtype=np.float64).reshape(-1)
    fin = np.isfinite(v)
    if not fin.any():
        return np.zeros(v.shape, dtype=bool)
    vals, counts = np.unique(v[fin], return_counts=True)          # (-0 and +0 are one value)
    vals, counts = vals[::-1], counts[::-1].astype(np.int64)
    keep = np.ones(len(vals), dtype=bool)
    if int(top_k) > 0:
        keep = np.cumsum(counts) - counts < int(top_k)
    tp = float(np.float32(top_p))
    if tp < 1.0:
        mass = np.where(keep, counts * np.exp((vals - vals[0]) * float(np.float32(inv_temp))), 0.0)
        keep &= np.cumsum(mass) - mass < tp * mass.sum()
    keep[0] = True
    kept = fin & (v >= vals[keep].min())
    if log_min_p is not None and not np.float32(log_min_p) == np.float32(-np.inf):
        with np.errstate(all="ignore"):
            d = np.where(fin, v, vals[0]).astype(np.float32) - np.float32(vals[0])
            kept &= d * np.float32(inv_temp) >= np.float32(log_min_p)
    return kept


def sample_truncated_reference(logits, inv_temp, keys, top_k, top_p, min_p=None, log_min_p=None) -> np.ndarray:
    """The reference of the truncated sampler: int32 [R] picks over bf16
    ``logits`` [R][V], per row the argmax of ``logit * inv_temp + G`` over the
    columns :func:`truncation_keep` keeps (float64 scores, ties to the lower
    column; 0 for a row that keeps nothing).  ``top_k`` / ``top_p`` /
    ``log_min_p`` (or ``min_p``, a ratio): per row or one value for all."""
    if log_min_p is None and min_p is not None:
        log_min_p = min_p_log(min_p)
    lg = np.asarray(logits, dtype=np.float64)
    R, V = lg.shape
    it = np.broadcast_to(np.asarray(inv_temp, dtype=np.float32), (R,))
    tk = np.broadcast_to(np.asarray(top_k, dtype=np.int64), (R,))
    tp = np.broadcast_to(np.asarray(top_p, dtype=np.float32), (R,))
    lm = None if log_min_p is None else np.broadcast_to(np.asarray(log_min_p, dtype=np.float32), (R,))
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    cols = np.arange(V, dtype=np.uint32)
    out = np.zeros(R, dtype=np.int32)
    for r in range(R):
        keep = truncation_keep(lg[r], it[r], tk[r], tp[r], log_min_p=None if lm is None else lm[r])
        if keep.any():
            sc = np.where(keep, lg[r], 0.0) * float(it[r]) + gumbel(keys[r:r + 1], cols)[0]
            out[r] = np.where(keep, sc, -np.inf).argmax()
    return out


# alternatives a row: the package's one copy of csrc/kernels/logprob_kernels.h's LP_TOP (the parser's
# upper limit, the engine's buffers and the K_LOGP stream all take it from here)
LP_TOP = 5


def logprob_reference(logits, tok) -> tuple:
    """The twin of ``csrc/kernels/logprob_kernels.h``, which holds the
    contract, in float64: ``(lp float64 [L][1 + LP_TOP], ids int64
    [L][LP_TOP])`` over bf16 ``logits`` [L][V] (an array of bf16-representable
    values) and the chosen tokens ``tok`` [L].  Per row the candidates are the
    finite columns, ``lp(n) = (l[n] - m) - log(sum exp(l - m))`` with ``m``
    their maximum; ``lp[:, 0]`` is the token's (-inf for a token outside [0,
    V) or on a column that is no candidate), ``lp[:, 1:]`` those of the LP_TOP
    largest candidates ``ids`` (ties to the lower column; -1 / -inf where the
    row has fewer)."""
    lg = np.asarray(logits, dtype=np.float64)
    L, V = lg.shape
    tok = np.broadcast_to(np.asarray(tok, dtype=np.int64), (L,))
    lp = np.full((L, 1 + LP_TOP), -np.inf, dtype=np.float64)
    ids = np.full((L, LP_TOP), -1, dtype=np.int64)
    for r in range(L):
        fin = np.isfinite(lg[r])
        if not fin.any():
            continue
        m = lg[r][fin].max()
        d = np.where(fin, lg[r], m) - m
        logz = np.log(np.exp(d[fin]).sum())
        cand = np.flatnonzero(fin)
        order = cand[np.argsort(-lg[r][cand], kind="stable")[:LP_TOP]]     # (stable: a tie keeps the lower column)
        ids[r, :len(order)] = order
        lp[r, 1:1 + len(order)] = d[order] - logz
        t = int(tok[r])
        if 0 <= t < V and fin[t]:
            lp[r, 0] = d[t] - logz
    return lp, ids


def logprob_bound(V: int, span: float = 128.0) -> float:
    """The bound on ``|device - twin|`` of a log-probability, in nats, for a
    row of ``V`` columns and a column within ``span`` of the row's maximum
    (``|l - m| <= span``; an fp32 ``exp`` is 0 from 104 on, so the default
    covers every column with a probability above 0).  The derivation, term by
    term from the kernel's order of operations, is in
    ``csrc/kernels/logprob_kernels.h``."""
    import math
    u = 2.0 ** -24
    logv = math.log(max(int(V), 2))
    depth = 8 * ((int(V) + 2047) // 2048) + 8         # a thread's columns, 6 shuffle levels, 2 for the waves
    rho = math.expm1((logv + 2.0 + depth) * math.log1p(u)) + int(V) * 2.0 ** -126
    return (-math.log1p(-rho)                         # log Z' against log Z
            + 2.0 * u * (logv + rho)                  # logf, 1 ulp
            + span * u                                # d = fl(l - m)
            + (span + logv + 1.0) * u)                # lp = fl(d - log Z)


def sample_reference(logits, inv_temp, keys) -> np.ndarray:
    """The reference sampler: int32 [M] picks over ``logits`` [M][V]
    (float64 scores; a row with ``inv_temp == 0`` is the plain argmax, ties
    to the lower column)."""
    lg = np.asarray(logits, dtype=np.float64)
    it = np.asarray(inv_temp, dtype=np.float32).astype(np.float64).reshape(-1)
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1, 2)
    M, V = lg.shape
    out = np.empty(M, dtype=np.int32)
    cols = np.arange(V, dtype=np.uint32)
    for i in range(0, M, 64):                       # (noise in row chunks: [64][V] float64)
        j = min(M, i + 64)
        g = gumbel(keys[i:j], cols)
        sc = np.where(it[i:j, None] != 0, lg[i:j] * it[i:j, None] + g, lg[i:j])
        out[i:j] = sc.argmax(axis=1)
    return out


# history entries a row: the package's one copy of csrc/kernels/penalty_kernels.h's PEN_HIST_MAX (the engine
# checks its max_ctx against it)
PEN_HIST_MAX = 4096


def bf16_bits(x) -> np.ndarray:
    """float32 values -> bf16 bit patterns (uint16), round to nearest even; a
    NaN becomes 0x7fc0, an overflow an infinity (``pen_bf16``)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where((u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000), np.uint16(0x7FC0), r)


def bf16_values(bits) -> np.ndarray:
    """bf16 bit patterns (uint16) -> their float32 values."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _f32_nearest_even(q) -> np.float32:
    """The float32 nearest to the non-zero rational ``q``, ties to even
    (denormals and overflow included)."""
    neg, a = q < 0, abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if a < Fraction(2) ** e:
        e -= 1                                       # 2^e <= a < 2^(e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    m, rem = divmod(a, ulp)
    m = int(m)
    if rem * 2 > ulp or (rem * 2 == ulp and (m & 1)):
        m += 1
    v = float(m * ulp)                               # (exact in float64; above the float32 range it becomes inf)
    with np.errstate(over="ignore"):
        return np.float32(-v if neg else v)


def _fma_f32(a: np.float32, c: int, x: np.float32) -> np.float32:
    """``fma(a, float(c), x)`` in float32 with one rounding (``a`` finite,
    ``c`` a small non-negative integer)."""
    if not np.isfinite(x):
        return x
    q = Fraction(float(a)) * int(c) + Fraction(float(x))
    if q != 0:
        return _f32_nearest_even(q)
    p_neg = bool(np.signbit(a))                      # (the product's sign: c >= 0)
    both_zero = (float(a) == 0.0 or int(c) == 0) and float(x) == 0.0
    return np.float32(-0.0) if (both_zero and p_neg and np.signbit(x)) else np.float32(0.0)


def penalise_reference(bits, vocab: int, h, n_p: int, pp, fp, rp) -> np.ndarray:
    """The twin of the edit in ``csrc/kernels/penalty_kernels.h``, which holds
    the contract, bit for bit: one row of bf16 bit patterns ``bits`` (uint16
    [ld], columns ``vocab .. ld`` padding) under the history ``h`` (ids, the
    first ``n_p`` prompt tokens, the rest generated) and the float32
    parameters; returns the edited copy.  Per distinct id in [0, vocab):
    ``x = x > 0 ? x / rp : x * rp`` if ``rp != 1``, ``x = fma(-fp, c_gen,
    x)``, ``x -= pp`` if ``c_gen > 0``, each rounded once in float32, then
    bf16 by round-to-nearest-even."""
    out = np.array(bits, dtype=np.uint16).reshape(-1)
    h = np.asarray(h, dtype=np.int64).reshape(-1)
    pp, fp, rp = np.float32(pp), np.float32(fp), np.float32(rp)
    n_p = min(max(int(n_p), 0), len(h))
    with np.errstate(all="ignore"):
        for t in np.unique(h):
            if not 0 <= t < int(vocab):
                continue
            c_gen = int(np.count_nonzero(h[n_p:] == t))
            x = bf16_values(out[t:t + 1])[0]
            if rp != np.float32(1.0):
                x = np.float32(x / rp) if x > 0 else np.float32(x * rp)
            x = _fma_f32(-fp, c_gen, x)
            if c_gen > 0:
                x = np.float32(x - pp)
            out[t] = bf16_bits(np.array([x], dtype=np.float32))[0]
    return out


def penalise_rows_reference(bits, vocab: int, hist, spans, params) -> np.ndarray:
    """:func:`penalise_reference` over rows [R][ld] the way the device reads
    its histories: ``hist`` int32 [slots][stride], ``spans`` [R][4] = (slot,
    from, split, end), ``params`` float32 [R][3] = (pp, fp, rp); spans are
    clamped to the table as the kernel clamps them."""
    out = np.array(bits, dtype=np.uint16)
    hist = np.asarray(hist)
    stride = hist.shape[1]
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 4)
    params = np.asarray(params, dtype=np.float32).reshape(-1, 3)
    for r in range(out.shape[0]):
        s, a, m, b = (int(v) for v in spans[r])
        if not 0 <= s < hist.shape[0]:
            continue
        a = min(max(a, 0), stride)
        b = min(min(max(b, a), stride), a + min(stride, PEN_HIST_MAX))
        m = min(max(m, a), b)
        out[r] = penalise_reference(out[r], vocab, hist[s, a:b], m - a, *params[r])
    return out


def penalised_pick_reference(bits, vocab: int) -> np.ndarray:
    """The twin of ``penalised_argmax_kernel``: int32 [R], per row of bf16 bit
    patterns [R][ld] the argmax over the finite columns < ``vocab``, ties to
    the lower column, 0 for a row with none."""
    v = bf16_values(np.asarray(bits, dtype=np.uint16).reshape(len(bits), -1)[:, :int(vocab)]).astype(np.float64)
    v = np.where(np.isfinite(v), v, -np.inf)
    return np.where(np.isfinite(v.max(axis=1)), v.argmax(axis=1), 0).astype(np.int32)


# entries a list: the package's one copy of csrc/kernels/logit_edit_kernels.h's LE_MAX (the parser's cap, the
# engine's staging and the K_HIST extension all take it from here)
LE_MAX = 64


def logit_edit_reference(bits, vocab: int, ids, vals, spans) -> np.ndarray:
    """The twin of ``csrc/kernels/logit_edit_kernels.h``, which holds the
    contract, bit for bit: rows of bf16 bit patterns ``bits`` (uint16 [R][ld],
    columns ``vocab .. ld`` padding) under the flat lists ``ids`` (int32 [N])
    and ``vals`` (float32 [N]) and the per-row ``spans`` [R][4] = (allow_off,
    n_allow, bias_off, n_bias); returns the edited copy.  An offset is clamped
    into [0, N], a count into [0, min(LE_MAX, N - offset)].  With an allow
    list every column < ``vocab`` outside it becomes 0xff80; then each bias
    entry whose id is in [0, vocab), the first of its id, adds its value in
    float32 (one rounding) and rounds to bf16 by nearest-even."""
    out = np.array(bits, dtype=np.uint16)
    out = out.reshape(1, -1) if out.ndim == 1 else out
    V = int(vocab)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals, dtype=np.float32).reshape(-1)
    N = min(len(ids), len(vals))
    spans = np.asarray(spans, dtype=np.int64).reshape(-1, 4)
    for r in range(out.shape[0]):
        a_off, n_a, b_off, n_b = (int(x) for x in spans[r])
        a_off, b_off = min(max(a_off, 0), N), min(max(b_off, 0), N)
        n_a = min(max(n_a, 0), LE_MAX, N - a_off)
        n_b = min(max(n_b, 0), LE_MAX, N - b_off)
        if n_a > 0:
            al = ids[a_off:a_off + n_a]
            mask = np.ones(V, dtype=bool)
            mask[al[(al >= 0) & (al < V)]] = False
            out[r, :V][mask] = 0xFF80
        seen = set()
        for i in range(n_b):
            t = int(ids[b_off + i])
            if not 0 <= t < V or t in seen:
                continue
            seen.add(t)
            with np.errstate(all="ignore"):
                x = np.float32(bf16_values(out[r, t:t + 1])[0] + vals[b_off + i])
            out[r, t] = bf16_bits(np.array([x], dtype=np.float32))[0]
    return out


# the package's one copy of csrc/kernels/stop_kernels.h's constants (the parser's caps, the engine's staging and the
# extension stream all take them from here)
STOP_ENTRIES = 8
STOP_LEN = 8
STOP_ROW_WORDS = 6
STOP_ENT_WORDS = 1 + STOP_LEN


def stop_table(entries) -> np.ndarray:
    """Stop entries (sequences of token ids, each of 1..STOP_LEN) as rows of
    the packed entry table int32 [n][STOP_ENT_WORDS] = (length, the tokens,
    oldest first, zero padded)."""
    out = np.zeros((len(entries), STOP_ENT_WORDS), dtype=np.int32)
    for i, e in enumerate(entries):
        e = np.asarray(e, dtype=np.int64).reshape(-1)
        if not 1 <= len(e) <= STOP_LEN:
            raise ValueError(f"a stop entry holds 1..{STOP_LEN} tokens")
        out[i, 0] = len(e)
        out[i, 1:1 + len(e)] = np.where((e >= 0) & (e < 1 << 31), e, -1)
    return out


def stop_match_reference(tok, hist, rows, ent) -> np.ndarray:
    """The twin of ``csrc/kernels/stop_kernels.h``, which holds the contract
    (all integer: exact): int32 [R], per row the lowest stop entry that equals
    the tail of ``hist[slot][gen_from:end] + [tok[r]]``, or -1.  ``tok`` int32
    [R]; ``hist`` int32 [slots][stride] or None; ``rows`` int32 [R][6] =
    (slot, gen_from, end, min_tokens, ent_off, n_ent); ``ent`` int32
    [N][1 + STOP_LEN] = (length, tokens oldest first).  Spans and entry ranges
    are clamped as the kernel clamps them; a slot outside the table leaves
    only ``tok[r]`` to compare; an entry whose length is outside 1..STOP_LEN
    is ignored."""
    tok = np.asarray(tok, dtype=np.int32).reshape(-1)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, STOP_ROW_WORDS)
    ent = np.asarray(ent, dtype=np.int32).reshape(-1, STOP_ENT_WORDS)
    N = len(ent)
    n_slots, stride = (0, 0) if hist is None else np.asarray(hist).shape
    out = np.full(len(tok), -1, dtype=np.int32)
    for r in range(len(tok)):
        slot, a, b, min_tokens, off, cnt = (int(v) for v in rows[r])
        a = min(max(a, 0), stride)
        b = min(max(b, a), stride)
        w = [int(x) for x in hist[slot][a:b]] if 0 <= slot < n_slots else []
        w.append(int(tok[r]))
        if len(w) < min_tokens:
            continue
        off = min(max(off, 0), N)
        cnt = min(max(cnt, 0), STOP_ENTRIES, N - off)
        for k in range(cnt):
            n = int(ent[off + k, 0])
            if 1 <= n <= STOP_LEN and n <= len(w) and w[len(w) - n:] == [int(x) for x in ent[off + k, 1:1 + n]]:
                out[r] = k
                break
    return out
