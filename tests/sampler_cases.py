"""Exact kept-set cases for the top-k / top-p select of the truncated sampler
(the GPU tests in test_gpu_sampler_exact.py and the construction checks in
test_sampler_cases_cpu.py; ``csrc/kernels/sample_truncate_kernels.h`` holds
the contract and ``ops.sampling.truncation_keep`` is its float64 twin).

A case is one row of bf16 logits with ``inv_temp``, ``top_k`` and ``top_p``
whose kept set is known group by group: a few planted groups of equal values
at chosen window offsets below the row's maximum, over a filler of candidates
so far below that no draw can reach them.  The draw among the kept columns is
decided by noise the host knows in float64, so each case carries row keys that
were searched, over ``S.row_keys(seed, 0)``, to decide it clearly:

  edge    the twin's pick lies in the LOWEST kept group and wins among the
          kept columns by >= CLEAR.  A kernel that drops that group picks
          another column under this key.
  trap    a column of the NEXT group below the cut would win by >= CLEAR if it
          were kept, and the twin's own winner is clear by >= CLEAR.  A kernel
          that keeps one group too many picks the trap under this key.
  plain   a clear winner in a group above the lowest kept one.

CLEAR = 0.05 is the project's margin for "the device's fp32 scores cannot
change the winner": 50 times the noise-arithmetic bound of 1e-3.  The expected
pick is the twin's, always, and the comparison on the device is equality.

Top-p sums fp32 masses on the device and float64 masses in the twin, so a
top-p case is admitted only if the twin's kept set is the same at ``top_p (1 -
DELTA)``, ``top_p`` and ``top_p (1 + DELTA)`` (DELTA = 1e-3; the device's sums
are within 1e-5 relative).  That is a condition on the inputs, asserted by the
builder, not a tolerance on the result.  Top-k is integer arithmetic and needs
none.

Every builder asserts on the twin that the case is what it claims: the kept
set, the value of the lowest kept group and of the next group below it, their
window offsets (``st_key`` is transcribed here), and that no column outside
the few "live" ones can come within CLEAR of a winner under any key.

Plain numpy on the CPU; nothing here touches a GPU."""
import functools
import time
from types import SimpleNamespace

import numpy as np

from llm_message_queue_amd.ops import sampling as S

ST_WIN = 32768                       # keys a window (sample_truncate_kernels.h)
ST_CHUNK = 128                       # keys a thread scans
DELTA = 1e-3                         # relative slack on top_p under which a top-p case's kept set must not move
CLEAR = 0.05                         # float64 score gap that decides a draw on the device too
# the Gumbel of sample_noise.h: v = (m + 0.5) 2^-32 lies in [2^-33, 1 - 2^-33], G = -log(-log1p(-v))
G_MAX, G_MIN = 22.9, -3.2
REACH = G_MAX - G_MIN + 2 * CLEAR    # a column this far (in score) below the maximum never wins or comes close
KEY_ZERO = 0x8000                    # +0 and -0
KEY_TOP, KEY_BOTTOM = 65407, 128     # the largest and the lowest finite bf16
NAN_BITS = (0x7FC0, 0x7F80, 0xFF80, 0xFFC1, 0x7FFF)                   # NaN, +inf, -inf, NaN, NaN: never candidates
SUB_POS, SUB_NEG, ZERO_POS, ZERO_NEG = 0x0001, 0x8001, 0x0000, 0x8000
TOP_FINITE, LOW_FINITE = 0x7F7F, 0xFF7F
SEARCH_BATCH = 512
SEARCH_BUDGET = 40000

SEARCH_SECONDS = [0.0]               # host time spent in the witness search (reported by the tests)


# ----------------------------------------------------------------------------- the key of a bf16 value
def st_key(bits) -> np.ndarray:
    """``st_key`` of the kernel over uint16 bit patterns: ascending with the
    value, -1 for NaN / inf, -0 on the key of +0."""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    k = np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)
    k = np.where(k == 0x7FFF, KEY_ZERO, k)
    return np.where((b & 0x7F80) == 0x7F80, -1, k)


def key_bits(key: int) -> int:
    """``st_value``: the bit pattern of a key (key 32,768 gives +0; 32,767 is no key)."""
    key = int(key)
    assert 0 <= key <= 0xFFFF and key != 0x7FFF
    return (key & 0x7FFF) if key & 0x8000 else (~key & 0xFFFF)


def bits_of(x) -> int:
    """The bit pattern of a value that is a bf16 number."""
    b = S.bf16_bits(np.array([x], dtype=np.float32))
    assert S.bf16_values(b)[0] == np.float32(x), x
    return int(b[0])


def bits_at(max_bits: int, offset: int) -> int:
    """The bit pattern ``offset`` keys below ``max_bits``."""
    return key_bits(int(st_key(max_bits)) - offset)


def offset_of(max_bits: int, bits: int) -> int:
    return int(st_key(max_bits)) - int(st_key(bits))


def values64(bits) -> np.ndarray:
    with np.errstate(invalid="ignore"):                                 # (a signalling NaN widens to a quiet one)
        return S.bf16_values(np.asarray(bits, dtype=np.uint16)).astype(np.float64)


# ----------------------------------------------------------------------------- building one case
def _scale(top_p, f):
    """top_p (1 + f) as the existing GPU tests compute it."""
    return np.float32(top_p) * np.float32(1.0 + f)


def _groups_of(row64):
    fin = np.isfinite(row64)
    vals, counts = np.unique(row64[fin], return_counts=True)
    return vals[::-1], counts[::-1].astype(np.int64)


def top_p_between(row64, inv_temp, top_k, edge_value) -> np.float32:
    """The top_p whose target lies in the middle of the group ``edge_value``:
    that group is the last one top-p keeps, by half its mass on either side."""
    vals, counts = _groups_of(row64)
    keep = np.ones(len(vals), dtype=bool) if top_k <= 0 else np.cumsum(counts) - counts < top_k
    mass = np.where(keep, counts * np.exp((vals - vals[0]) * float(np.float32(inv_temp))), 0.0)
    i = int(np.flatnonzero(vals == edge_value)[0])
    assert keep[i] and mass[i] > 0
    return np.float32((np.cumsum(mass)[i] - 0.5 * mass[i]) / mass.sum())


def _search(c, n_edge, n_trap, n_plain, budget):
    """Row keys over seeds ``c.seed0 + i``: ``n_edge`` keys that make a column
    of the edge group the clear winner, ``n_trap`` under which a column of the
    trap group would win clearly if kept (both spread evenly over the group's
    columns), and ``n_plain`` keys with a clear winner in an upper group.  Only the live columns need their noise: the others are out of
    reach under any key (asserted by the builder)."""
    t0 = time.perf_counter()
    live = c.live
    base = c.row64[live] * float(c.inv_temp)
    kept = c.keep[live]
    is_edge, is_trap = np.isin(live, c.edge_cols), np.isin(live, c.trap_cols)
    wide = kept | is_trap
    edges, traps, plains = [], [], []
    need_e = n_edge if len(c.edge_cols) else 0
    need_t = n_trap if len(c.trap_cols) else 0
    need_p = n_plain if (kept & ~is_edge).any() else 0
    cap_e = -(-need_e // max(len(c.edge_cols), 1))                      # keys a column
    cap_t = -(-need_t // max(len(c.trap_cols), 1))

    def top2(sc, mask):
        m = np.where(mask, sc, -np.inf)
        win = m.argmax(axis=1)
        if mask.sum() == 1:
            return win, np.full(len(sc), np.inf)
        part = np.partition(m, -2, axis=1)
        return win, part[:, -1] - part[:, -2]

    seeds = 0
    while seeds < budget and (len(edges) < need_e or len(traps) < need_t or len(plains) < need_p):
        ids = np.arange(seeds, seeds + SEARCH_BATCH, dtype=np.uint64) + np.uint64(c.seed0)
        keys = S.row_keys(ids, 0)
        sc = base[None, :] + S.gumbel(keys, live.astype(np.uint32))
        win, gap = top2(sc, kept)
        wwin, wgap = top2(sc, wide)
        clear = gap >= CLEAR
        for i in np.flatnonzero(clear):
            col = int(live[win[i]])
            tcol = int(live[wwin[i]])
            if is_edge[win[i]] and len(edges) < need_e and sum(e[0] == col for e in edges) < cap_e:
                edges.append((col, keys[i]))
            elif not is_edge[win[i]] and len(plains) < need_p and col not in [p[0] for p in plains]:
                plains.append((col, keys[i]))
            if is_trap[wwin[i]] and wgap[i] >= CLEAR and len(traps) < need_t and sum(e[0] == tcol for e in traps) < cap_t:
                traps.append((tcol, keys[i], col))
        seeds += SEARCH_BATCH
    SEARCH_SECONDS[0] += time.perf_counter() - t0
    assert len(edges) == need_e and len(traps) == need_t and len(plains) == need_p, \
        (c.name, c.V, "witness search", len(edges), need_e, len(traps), need_t, len(plains), need_p)
    c.seeds_used = seeds
    c.keys, c.wants, c.kinds, c.trap_wins = [], [], [], []
    for col, key in edges:
        c.keys.append(key), c.wants.append(col), c.kinds.append("edge"), c.trap_wins.append(-1)
    for tcol, key, col in traps:
        c.keys.append(key), c.wants.append(col), c.kinds.append("trap"), c.trap_wins.append(tcol)
    for col, key in plains:
        c.keys.append(key), c.wants.append(col), c.kinds.append("plain"), c.trap_wins.append(-1)


def build_case(name, cls, V, index, groups, inv_temp, top_k=0, top_p=1.0, *, cut, p_cut=None, filler="low",
               cols=None, edge_off=None, trap_off=None, all_cols=False, n_edge=2, n_trap=2, n_plain=1,
               budget=SEARCH_BUDGET):
    """``groups``: the planted groups in descending order, each ``(bit
    patterns, count)`` -- the patterns are dealt to the group's columns in
    turn, so a group may mix +0 and -0.  ``cut``: the index of the lowest
    group the row keeps (None: every candidate is kept); the next one is the
    trap.  ``p_cut``: take the top_p that cuts in the middle of that group
    (:func:`top_p_between`) instead of ``top_p``.  ``filler``: "low" --
    candidates in [-1000, -200], far below every planted value -- or "nan" --
    no candidate at all (NaN and infinities).  ``cols``: the planted columns
    group by group (default: drawn from default_rng(index)).  ``edge_off`` /
    ``trap_off``: the claimed window offsets of the lowest kept group and of
    the trap below the row's maximum."""
    rng = np.random.default_rng(1000 + index)
    if filler == "low":
        bits = S.bf16_bits(-(200.0 + 800.0 * rng.random(V)).astype(np.float32))
    else:
        bits = np.array(NAN_BITS, dtype=np.uint16)[rng.integers(0, len(NAN_BITS), V)]
    counts = [n for _b, n in groups]
    if cols is None:
        perm = rng.permutation(V)[:sum(counts)]
        cols = [perm[sum(counts[:g]):sum(counts[:g + 1])] for g in range(len(groups))]
    cols = [np.sort(np.asarray(cg, dtype=np.int64)) for cg in cols]
    flat = np.concatenate(cols)
    assert [len(cg) for cg in cols] == counts and len(set(flat.tolist())) == len(flat) and flat.min() >= 0 and flat.max() < V
    for (pat, n), cg in zip(groups, cols):
        bits[cg] = np.resize(np.asarray(pat, dtype=np.uint16), n)
    row64 = values64(bits)
    gvals = [float(values64([pat[0]])[0]) for pat, _n in groups]
    assert all(a > b for a, b in zip(gvals, gvals[1:])), (name, gvals)       # descending, distinct (+0 == -0)
    for (pat, _n), v in zip(groups, gvals):
        assert (values64(pat) == v).all(), (name, pat)
    fin = np.isfinite(row64)
    planted = np.zeros(V, dtype=bool)
    planted[flat] = True
    assert row64[fin].max() == gvals[0]

    c = SimpleNamespace(name=name, cls=cls, V=V, bits=bits, row64=row64, inv_temp=np.float32(inv_temp), top_k=int(top_k),
                        groups=cols, group_values=gvals, seed0=1000003 * (index + 1))
    c.top_p = top_p_between(row64, c.inv_temp, c.top_k, gvals[p_cut]) if p_cut is not None else np.float32(top_p)
    c.keep = S.truncation_keep(row64, c.inv_temp, c.top_k, c.top_p)
    if c.top_p < 1:
        for f in (-DELTA, DELTA):                                       # the admission condition of a top-p case
            assert np.array_equal(S.truncation_keep(row64, c.inv_temp, c.top_k, _scale(c.top_p, f)), c.keep), (name, f)
    # the kept set is the planted groups down to ``cut`` (or every candidate)
    want = fin.copy() if cut is None else np.isin(np.arange(V), np.concatenate(cols[:cut + 1]))
    assert np.array_equal(c.keep, want), (name, int(c.keep.sum()), int(want.sum()))
    vals, _counts = _groups_of(row64)
    low = row64[c.keep].min()
    below = vals[vals < low]
    c.kmax = int(st_key(bits[fin]).max())
    assert c.kmax == int(st_key(groups[0][0][0]))
    # the live columns: every other one is out of reach of a winner under any key
    c.live = np.flatnonzero(fin & ((gvals[0] - row64) * float(c.inv_temp) <= REACH))
    assert 0 < len(c.live) <= 64 and planted[c.live].all(), (name, len(c.live))
    edge_g = len(groups) - 1 if cut is None else cut
    c.edge_cols = cols[edge_g] if gvals[edge_g] == low and np.isin(cols[edge_g], c.live).all() else np.zeros(0, dtype=np.int64)
    assert cut is None or len(c.edge_cols), name
    c.trap_cols = np.zeros(0, dtype=np.int64)
    c.edge_off = offset_of(groups[0][0][0], groups[edge_g][0][0]) if gvals[edge_g] == low else None
    c.trap_off = None
    if cut is not None and cut + 1 < len(groups):
        assert len(below) and below[0] == gvals[cut + 1], name              # the trap is the very next group of the row
        c.trap_off = offset_of(groups[0][0][0], groups[cut + 1][0][0])
        if n_trap:
            c.trap_cols = cols[cut + 1]
            assert np.isin(c.trap_cols, c.live).all(), name
    else:
        assert cut is None and not len(below), name                        # no trap group: everything is kept
    assert edge_off is None or c.edge_off == edge_off, (name, c.edge_off, edge_off)
    assert trap_off is None or c.trap_off == trap_off, (name, c.trap_off, trap_off)
    c.edge_window = None if c.edge_off is None else c.edge_off // ST_WIN
    c.trap_window = None if c.trap_off is None else c.trap_off // ST_WIN
    # the two mutants a wrong select would produce: one group more, one group fewer
    c.more = c.keep.copy()
    c.more[c.trap_cols] = True
    c.fewer = c.keep.copy()
    if edge_g > 0:
        c.fewer[c.edge_cols] = False
    _search(c, len(c.edge_cols) if all_cols else n_edge, len(c.trap_cols) if all_cols else n_trap, n_plain, budget)
    return c


# ----------------------------------------------------------------------------- the cases
M_BITS = 0x407F                      # 3.984375: the last key of its binade, so window offset 128 n is a binade edge


def _b(x):
    return [bits_of(x)]


def _cut_groups(edge_off, trap_off):
    """The maximum, a group half way down, the lowest kept group and the trap
    at the given offsets, and one more group below."""
    return [([M_BITS], 1), ([bits_at(M_BITS, edge_off // 2)], 2), ([bits_at(M_BITS, edge_off)], 2),
            ([bits_at(M_BITS, trap_off)], 2), ([bits_at(M_BITS, trap_off + 37)], 2)]


# (class, lowest kept offset, trap offset): cuts against the chunk, wave and window boundaries of the scan
CUTS = (("chunk_127", 127, 128), ("chunk_128", 128, 129), ("mid_chunk_511", 511, 512), ("mid_chunk_512", 512, 513),
        ("wave_8191", 8191, 8192), ("window_32767", 32767, 32768), ("window_32768", 32768, 32769))
TWO_WINDOWS = [([M_BITS], 1), (_b(3.0), 2), (_b(2.0), 2), (_b(-1.0), 2), (_b(-1.25), 2), (_b(-1.5), 2), (_b(-1.75), 2)]
TIES = [([M_BITS], 2), (_b(3.0), 2), (_b(2.0), 3), (_b(1.0), 2)]
NEGATIVE = [(_b(-0.5), 1), (_b(-0.75), 2), (_b(-1.0), 2), (_b(-1.5), 2), (_b(-2.0), 2)]
ZEROS = [(_b(0.5), 1), ([SUB_POS], 2), ([ZERO_POS, ZERO_NEG], 4), ([SUB_NEG], 2), (_b(-0.5), 2)]
SUBNORMAL_MAX = [([0x0002], 2), ([SUB_POS], 2), ([ZERO_NEG, ZERO_POS], 2), ([SUB_NEG], 2), (_b(-0.5), 2)]
EXTREME = [([TOP_FINITE], 1), (_b(1.0), 2), (_b(-1.0), 2), ([LOW_FINITE], 1)]
HOT = [(_b(4.0), 1), (_b(3.984375), 1), (_b(3.96875), 2), (_b(3.0), 2), (_b(-2.0), 2)]

# classes that must show an edge witness / a trap in every launch of all cases
EDGE_CLASSES = tuple(c for c, _e, _t in CUTS) + (
    "tie_k_minus_1", "tie_straddle", "tie_dropped", "tie_k1", "all_kept", "negative", "top_p_second_window",
    "k_second_p_first", "k_second_p_second", "k_second", "top_p_near_1", "top_p_tiny", "zero_boundary", "zero_trap",
    "subnormal_max", "inv_temp_20", "columns")
TRAP_CLASSES = tuple(c for c in EDGE_CLASSES if c not in ("all_kept", "inv_temp_20"))
SERVING_CLASSES = ("window_32767", "window_32768", "subnormal_max", "zero_boundary", "k_second_p_first")


def special_columns(V):
    """Two disjoint sets of columns at the ends of the row, on both sides of
    the first 16-byte vector boundary and (V % 8 != 0) in the last, partial
    vector."""
    part = V - V % 8 if V % 8 > 1 else V - 9
    return [0, 8, V - 1], [7, part, 16]


def _specs(V):
    s = []

    def add(name, cls, groups, it, top_k=0, top_p=1.0, **kw):
        s.append((name, cls, groups, it, top_k, top_p, kw))

    for i, (cls, e, t) in enumerate(CUTS):
        it = 0.25 if e > 4000 else 0.5
        # 3 columns above the lowest kept group of 2: top_k = 4 straddles it, top_k = 5 ends on it
        add(cls + "/top_k", cls, _cut_groups(e, t), it, top_k=4 + i % 2, cut=2, edge_off=e, trap_off=t)
        add(cls + "/top_p", cls, _cut_groups(e, t), it, p_cut=2, cut=2, edge_off=e, trap_off=t)
    # tie arithmetic at the cut: 2 + 2 columns above the boundary group of 3
    add("tie/before=k-1", "tie_k_minus_1", TIES, 0.5, top_k=5, cut=2)
    add("tie/straddle", "tie_straddle", TIES, 0.5, top_k=6, cut=2)
    add("tie/before=k", "tie_dropped", TIES, 0.5, top_k=4, cut=1)
    add("tie/k=1", "tie_k1", [([M_BITS], 3)] + TIES[1:], 0.5, top_k=1, cut=0, n_edge=3)
    # the window loop
    add("all_kept/nan_inf", "all_kept", TWO_WINDOWS, 0.25, top_k=V + 7, cut=None, filler="nan")
    add("negative/top_k", "negative", NEGATIVE, 0.5, top_k=4, cut=2)
    add("negative/top_p", "negative", NEGATIVE, 0.5, p_cut=2, cut=2)
    add("negative/both", "negative", NEGATIVE, 0.5, top_k=6, p_cut=1, cut=1)
    add("top_p/second_window", "top_p_second_window", TWO_WINDOWS, 0.25, p_cut=4, cut=4)
    add("top_k_second/top_p_first", "k_second_p_first", TWO_WINDOWS, 0.25, top_k=8, p_cut=1, cut=1)
    add("top_k_second/top_p_second", "k_second_p_second", TWO_WINDOWS, 0.25, top_k=8, p_cut=3, cut=3)
    add("top_k_second", "k_second", TWO_WINDOWS, 0.25, top_k=8, cut=4)
    add("top_p_near_1", "top_p_near_1", TWO_WINDOWS, 0.25, top_k=8, top_p=0.999, cut=4)
    add("top_p_tiny", "top_p_tiny", TWO_WINDOWS, 0.25, top_p=0.01, cut=0)
    # the key mapping: -0 is +0 (key 32,767 is never used, so the negative subnormal is two keys below the zeros)
    z = offset_of(ZEROS[0][0][0], ZERO_POS)
    add("zero/boundary/top_k", "zero_boundary", ZEROS, 0.5, top_k=4, cut=2, edge_off=z, trap_off=z + 2, all_cols=True)
    add("zero/boundary/top_p", "zero_boundary", ZEROS, 0.5, p_cut=2, cut=2, edge_off=z, trap_off=z + 2, all_cols=True)
    add("zero/trap/top_k", "zero_trap", ZEROS, 0.5, top_k=3, cut=1, edge_off=z - 1, trap_off=z, all_cols=True)
    add("zero/trap/top_p", "zero_trap", ZEROS, 0.5, p_cut=1, cut=1, edge_off=z - 1, trap_off=z, all_cols=True)
    add("subnormal_max/top_k", "subnormal_max", SUBNORMAL_MAX, 0.5, top_k=3, cut=1, edge_off=1, trap_off=2, all_cols=True)
    add("subnormal_max/top_p", "subnormal_max", SUBNORMAL_MAX, 0.5, p_cut=1, cut=1, edge_off=1, trap_off=2, all_cols=True)
    # the whole key range: no key can decide such a row but for the maximum, so these carry plain keys only
    add("extreme/top_k", "extreme", EXTREME, 0.25, top_k=2 ** 31 - 1, cut=None)
    add("extreme/top_p", "extreme", EXTREME, 0.25, top_k=2 ** 31 - 1, top_p=0.9, cut=0, n_trap=0)
    # inv_temp = 20: exp(-120) is 0 in fp32.  Stability under DELTA leaves the groups below the cut at most 1e-6 of
    # the mass, so no key within reach makes the trap win: edge and plain witnesses only
    add("inv_temp_20", "inv_temp_20", HOT, 20.0, top_p=0.999, cut=2, n_trap=0)
    # columns: the ends of the row, a vector boundary, the last partial vector
    a, b = special_columns(V)
    g = _cut_groups(127, 128)
    for i, (ec, tc) in enumerate(((a, b), (b, a))):
        cols = [[V // 2], [V // 2 + 1, V // 3], ec, tc, [V // 3 + 8, V // 3 + 9, V // 3 + 10][:2]]
        gg = [g[0], g[1], (g[2][0], 3), (g[3][0], 3), g[4]]
        add(f"columns/{i}/top_k", "columns", gg, 0.5, top_k=5, cut=2, cols=cols, all_cols=True)
        add(f"columns/{i}/top_p", "columns", gg, 0.5, p_cut=2, cut=2, cols=cols, all_cols=True)
    return s


@functools.lru_cache(maxsize=None)
def cases(V, classes=None):
    """Every case at vocabulary ``V`` (of the classes named, if any), built once."""
    out = []
    for index, (name, cls, groups, it, top_k, top_p, kw) in enumerate(_specs(V)):
        if classes is None or cls in classes:
            out.append(build_case(name, cls, V, index, groups, it, top_k, top_p, **kw))
    return tuple(out)


def witness_rows(cs):
    """One row a witness over the cases ``cs``: ``(bits uint16 [R][V], inv_temp,
    keys uint32 [R][2], top_k, top_p, wants, (case, kind) a row)``."""
    bits, it, keys, tk, tp, wants, tags = [], [], [], [], [], [], []
    for c in cs:
        for key, want, kind in zip(c.keys, c.wants, c.kinds):
            bits.append(c.bits), it.append(c.inv_temp), keys.append(key), tk.append(c.top_k), tp.append(c.top_p)
            wants.append(int(want)), tags.append((c, kind))
    return (np.stack(bits), np.array(it, dtype=np.float32), np.stack(keys).astype(np.uint32),
            np.array(tk, dtype=np.int32), np.array(tp, dtype=np.float32), wants, tags)


def tally(tags):
    """{class: [edge witnesses, traps, plain keys]} of the rows of :func:`witness_rows`."""
    out = {}
    for c, kind in tags:
        out.setdefault(c.cls, [0, 0, 0])[("edge", "trap", "plain").index(kind)] += 1
    return out


def check_coverage(tags, V, classes=None):
    """A launch of the rows ``tags`` describes holds an edge witness and a
    trap for every boundary class (of ``classes``, if given), at least two of
    each a case wherever the group can win a draw, and -- with all classes --
    witnesses and traps at the ends of the row, on both sides of a vector
    boundary and in the last partial vector."""
    t = tally(tags)
    for cls in EDGE_CLASSES:
        if classes is None or cls in classes:
            assert t.get(cls, [0, 0, 0])[0] >= 1, (cls, "no edge witness")
    for cls in TRAP_CLASSES:
        if classes is None or cls in classes:
            assert t.get(cls, [0, 0, 0])[1] >= 1, (cls, "no trap")
    for c in {id(c): c for c, _kind in tags}.values():
        assert c.kinds.count("edge") >= (2 if len(c.edge_cols) else 0), c.name
        assert c.kinds.count("trap") >= (2 if len(c.trap_cols) else 0), c.name
    if classes is None:
        a, b = special_columns(V)
        for kind in ("edge", "trap"):
            seen = set()
            for c in {id(c): c for c, _kind in tags}.values():
                seen |= {int(w if kind == "edge" else tw) for w, tw, k in zip(c.wants, c.trap_wins, c.kinds) if k == kind}
            assert set(a) | set(b) <= seen, (kind, sorted((set(a) | set(b)) - seen))
            assert V % 8 == 0 or any(col >= V - V % 8 for col in seen), kind
