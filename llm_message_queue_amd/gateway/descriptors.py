"""Fixed-width int32 rows the ranks exchange in every tick's all_to_all
(``parallel.comm``): request descriptors a router hands to another GPU,
completion / failure / abort records owed back to the origin router, KV
migration orders and cancels.  int64 fields travel as (lo, hi) int32 pairs.
The reference has no inter-service transport at all: its binaries do not
share queues."""
from __future__ import annotations

import numpy as np

from ..ops.sampling import LE_MAX as EXT_LIST_MAX, LP_TOP   # (entries an extension list; alternatives a row)
from ..ops.sampling import STOP_ENTRIES, STOP_LEN

# --------------------------------------------------------------------------- descriptors
K_DISPATCH, K_DONE, K_FAIL = 1, 2, 3     # K_FAIL: an evacuating backend hands a request back
K_MIGRATE = 4       # [kind, conv lo/hi, dest]: to a conversation's home GPU -- send its KV to dest this tick
# a backend aborted a request in flight: its processing deadline passed /
# its origin cancelled it (completion-record layout, owed like K_DONE)
K_TIMEOUT, K_CANCELLED = 5, 6
# K_FAIL's admitted field: the backend failed while running the request
# (the origin retries with backoff) / it never ran there (requeued as is)
FAIL_UNTOUCHED, FAIL_FAILED = 0, 1
K_CANCEL = 7        # [kind, handle lo/hi, origin]: origin -> the GPU running its request: abort it
# origin -> the GPU it dispatched a dialog turn to, one tick after the
# K_DISPATCH row: the dialog's real token history for a non-resident replay,
# HIST_SPAN tokens a row in the payload columns: [kind, handle lo/hi, origin,
# offset, ..., n (col 10), ..., history length (col 14), prefix length (col 15)];
# the payload is the compressed-context prefix (N5 salient tokens) then the history
K_HIST = 8
# completion records (K_DONE) carry the turn's generated token ids in the
# payload columns, their count in col 10 (dialog turns: the origin's history;
# requests dispatched with FINISH: their ``generation`` record), and in col 11
# how the generation ended (``pack_finish``; 0: not reported)
DESC_HDR = 20       # [kind, handle lo/hi, origin, tier, arrival lo/hi, enq lo/hi, gen, plen, flags, conv lo/hi,
#                    dialog history length, decision - enq (us), processing timeout (ms),
#                    sampling temperature (float32 bits), sampling seed lo/hi];
#                    tier = tier | presence, frequency, repetition penalties << 4 (``pack_penalties``)
#                           | EXTENSION; gen = the request's own count (the configured one, or its ``max_tokens``)
#                           | min_p permille << 16 (``pack_gen``) | FINISH;
#                    flags = (home GPU + 1) | KV_MIGRATE | DIALOG_TURN | top_k << 10 | top_p permille << 20
#                            | LOGPROBS
KV_MIGRATE = 1 << 8     # descriptor flag: hold the turn until its KV arrives from the home GPU
DIALOG_TURN = 1 << 9    # descriptor flag: a conversation turn -- its generated ids go back with K_DONE
# the sampling truncation of a request with a temperature, 10 bits each of the
# flags column: top_k (0 = off, <= 1023) in bits 10-19, top_p in thousandths
# in bits 20-29 (0 or 1000 = off).  A request without truncation leaves both
# zero.  The engine's float is float32(permille / 1000) on every GPU.
TOPK_SHIFT, TOPP_SHIFT, TRUNC_MASK = 10, 20, 0x3FF


def pack_truncation(top_k: int, top_p: float) -> int:
    """The flags-column bits of ``(top_k, top_p)`` (0: no truncation)."""
    pm = int(round(float(top_p) * 1000.0))
    pm = 0 if not 0 < pm < 1000 else pm
    return (min(max(int(top_k), 0), TRUNC_MASK) << TOPK_SHIFT) | (pm << TOPP_SHIFT)


def unpack_truncation(flags: int) -> tuple:
    """``(top_k, top_p)`` of a flags column value."""
    pm = (int(flags) >> TOPP_SHIFT) & TRUNC_MASK
    return (int(flags) >> TOPK_SHIFT) & TRUNC_MASK, (pm / 1000.0 if 0 < pm < 1000 else 1.0)


# descriptor flag: score the request's tokens (``Request.logprobs``).  Only the
# flag travels: the serving GPU always returns all alternatives and the origin,
# which knows the message's n, trims
LOGPROBS = 1 << 30
# the penalties of a request, in hundredths above the tier (1..4, bits 0-3) of
# a K_DISPATCH row's tier column: presence in bits 4-12 and frequency in bits
# 13-21 (signed 9 bits, -200..200), repetition - 100 in bits 22-29 (signed 8
# bits, -50..100).  A request without penalties leaves them zero.  The
# engine's floats are float32(hundredths / 100) on every GPU.
TIER_MASK = 0xF
PRES_SHIFT, FREQ_SHIFT, REP_SHIFT = 4, 13, 22


def _hundredths(v: float, lo: int, hi: int, off: int) -> int:
    h = int(round(float(v) * 100.0)) if np.isfinite(v) else off
    return h if lo <= h <= hi else off


def pack_penalties(presence: float, frequency: float, repetition: float) -> int:
    """The tier-column bits of the three penalties (0: none)."""
    return ((_hundredths(presence, -200, 200, 0) & 0x1FF) << PRES_SHIFT) \
        | ((_hundredths(frequency, -200, 200, 0) & 0x1FF) << FREQ_SHIFT) \
        | (((_hundredths(repetition, 50, 200, 100) - 100) & 0xFF) << REP_SHIFT)


def unpack_penalties(col: int) -> tuple:
    """``(tier, presence, frequency, repetition)`` of a tier column value."""
    def signed(v, bits):
        return v - (1 << bits) if v >> (bits - 1) else v
    c = int(col)
    if c < 0:                                        # (a message dispatched without a tier: nothing is packed)
        return c, 0.0, 0.0, 1.0
    return (c & TIER_MASK, signed((c >> PRES_SHIFT) & 0x1FF, 9) / 100.0, signed((c >> FREQ_SHIFT) & 0x1FF, 9) / 100.0,
            (signed((c >> REP_SHIFT) & 0xFF, 8) + 100) / 100.0)
# bit 30 of the tier column: the request has an extension stream -- its
# ``allowed_token_ids`` and ``logit_bias`` lists -- that follows one tick later
# as the third section (prefix, history, extension) of its K_HIST stream; the
# serving GPU holds the request until it has arrived.  Every K_HIST row carries
# the extension's length in col 16 (0: none).  ``unpack_penalties`` reads bits
# 0-29 and is blind to it.
EXTENSION = 1 << 30
GEN_MASK = 0xFFFF       # col 9: tokens to generate (<= 4,096: the engine's largest ``max_ctx``) | min_p permille << 16
MIN_P_SHIFT = 16


def pack_gen(gen: int, min_p: float = 0.0) -> int:
    """Col 9 of a K_DISPATCH row: ``gen`` and ``min_p`` as permille above it
    (0: off; a value outside [0, 1] is off)."""
    pm = int(round(float(min_p) * 1000.0)) if np.isfinite(min_p) else 0
    return (min(max(int(gen), 0), GEN_MASK)) | ((pm if 0 <= pm <= 1000 else 0) << MIN_P_SHIFT)


def unpack_gen(col: int) -> tuple:
    """``(gen, min_p)`` of a col 9 value."""
    c = int(col)
    if c < 0:
        return c, 0.0
    pm = (c >> MIN_P_SHIFT) & 0x3FF
    return c & GEN_MASK, (pm / 1000.0 if pm <= 1000 else 0.0)


# bit 26 of col 9 (above min_p's 10 bits): the request named a stop key
# (``max_tokens``, ``min_tokens``, ``stop_token_ids``, ``stop_sequences``) -- the
# serving GPU sends its generated ids home in its K_DONE payload, as a dialog
# turn's, and how it ended in col 11
FINISH = 1 << 26
FIN_LENGTH, FIN_STOP = 1, 2     # col 11 of a K_DONE row: 0 none, 1 "length", 2 + the matched entry's index "stop"


def pack_finish(finish_reason: str, stop_entry: int = -1) -> int:
    """Col 11 of a K_DONE row."""
    if finish_reason == "stop" and 0 <= int(stop_entry) < STOP_ENTRIES:
        return FIN_STOP + int(stop_entry)
    return FIN_LENGTH if finish_reason in ("length", "stop") else 0


def unpack_finish(col: int) -> tuple:
    """``(finish_reason, stop_entry)`` of a K_DONE row's col 11 (``("", -1)``:
    not reported)."""
    c = int(col)
    if FIN_STOP <= c < FIN_STOP + STOP_ENTRIES:
        return "stop", c - FIN_STOP
    return ("length", -1) if c == FIN_LENGTH else ("", -1)


def pack_stop_section(ext, min_tokens: int, entries) -> np.ndarray:
    """The extension stream ``ext`` (``pack_extension`` words, possibly none)
    with the stop section behind it: ``[n_entries, min_tokens, the entries'
    lengths..., their tokens...]``.  A request without entries gets ``ext``
    back unchanged (``min_tokens`` filters stops and means nothing without
    one); one without lists gets the two zero counts of empty first sections
    in front."""
    ents = [np.asarray(e, dtype=np.int32).reshape(-1) for e in (entries or ())]
    ents = [e for e in ents if 1 <= len(e) <= STOP_LEN][:STOP_ENTRIES]
    ext = np.asarray(ext, dtype=np.int32).reshape(-1)
    if not ents:
        return ext
    head = ext if len(ext) else np.zeros(2, dtype=np.int32)
    return np.concatenate([head, [len(ents), max(0, int(min_tokens))], [len(e) for e in ents]] + ents).astype(np.int32)


def unpack_stop_section(words) -> tuple:
    """``(min_tokens, entries)`` of the stop section behind the first two
    sections of an extension stream (``(0, [])``: none); counts and lengths
    that leave the stream or their ranges end the list there."""
    w = np.asarray(words, dtype=np.int32).reshape(-1)
    if not len(w):
        return 0, []
    na = min(max(int(w[0]), 0), EXT_LIST_MAX, len(w) - 1)
    rest = w[1 + na:]
    nb = min(max(int(rest[0]), 0), EXT_LIST_MAX, (len(rest) - 1) // 2) if len(rest) else 0
    st = rest[1 + 2 * nb:]
    if len(st) < 2:
        return 0, []
    n = min(max(int(st[0]), 0), STOP_ENTRIES, len(st) - 2)
    lens, toks, out = st[2:2 + n].tolist(), st[2 + n:], []
    for ln in lens:
        if not 1 <= ln <= STOP_LEN or ln > len(toks):
            break
        out.append(toks[:ln].copy())
        toks = toks[ln:]
    return max(0, int(st[1])), out




def pack_extension(allowed, bias_ids, bias_vals) -> np.ndarray:
    """The extension stream of a request, int32 words ``[n_allow, allow
    ids..., n_bias, bias ids..., bias float32 bits...]``; no words at all for
    a request with neither list.  A list is cut at ``EXT_LIST_MAX`` entries."""
    al = np.asarray(allowed if allowed is not None else (), dtype=np.int32).reshape(-1)[:EXT_LIST_MAX]
    bi = np.asarray(bias_ids if bias_ids is not None else (), dtype=np.int32).reshape(-1)[:EXT_LIST_MAX]
    bv = np.asarray(bias_vals if bias_vals is not None else (), dtype=np.float32).reshape(-1)[:len(bi)]
    bi = bi[:len(bv)]
    if not len(al) and not len(bi):
        return np.zeros(0, dtype=np.int32)
    return np.concatenate([[len(al)], al, [len(bi)], bi, bv.view(np.int32)]).astype(np.int32)


def unpack_extension(words) -> tuple:
    """``(allowed int32, bias ids int32, bias values float32)`` of an
    extension stream; counts that leave the stream are clamped to it."""
    w = np.asarray(words, dtype=np.int32).reshape(-1)
    none = np.zeros(0, dtype=np.int32)
    if not len(w):
        return none, none, np.zeros(0, dtype=np.float32)
    na = min(max(int(w[0]), 0), EXT_LIST_MAX, len(w) - 1)
    al = w[1:1 + na].copy()
    rest = w[1 + na:]
    nb = min(max(int(rest[0]), 0), EXT_LIST_MAX, (len(rest) - 1) // 2) if len(rest) else 0
    return al, rest[1:1 + nb].copy(), rest[1 + nb:1 + 2 * nb].copy().view(np.float32)


# serving GPU -> origin, ahead of the request's K_DONE (same FIFO): the
# log-probabilities of a request dispatched with LOGPROBS, LP_WORDS int32 a
# generated token -- id, lp (float32 bits), 5 alternative ids, their 5 lps --
# as one stream cut into rows of at most ``cap`` payload words: [kind, handle
# lo/hi, origin, offset (col 4), words of this row lo/hi, words in all (col 7)
# lo/hi, -, words of this row (col 10)]
K_LOGP = 9
LP_WORDS = 2 + 2 * LP_TOP


def pack_logprob_stream(tokens, lp, top_ids, top_lp) -> np.ndarray:
    """The int32 stream of a request's log-probability results (LP_WORDS a
    token; floats as their bits)."""
    n = len(tokens)
    st = np.empty((n, LP_WORDS), dtype=np.int32)
    st[:, 0] = np.asarray(tokens, dtype=np.int32)
    st[:, 1] = np.ascontiguousarray(lp, dtype=np.float32).view(np.int32)
    st[:, 2:2 + LP_TOP] = np.asarray(top_ids, dtype=np.int32).reshape(n, LP_TOP)
    st[:, 2 + LP_TOP:] = np.ascontiguousarray(top_lp, dtype=np.float32).view(np.int32).reshape(n, LP_TOP)
    return st.reshape(-1)


def unpack_logprob_stream(stream: np.ndarray) -> tuple:
    """``(tokens int32 [n], lp float32 [n], top_ids int32 [n][5], top_lp
    float32 [n][5])`` of a stream of :func:`pack_logprob_stream`."""
    st = np.ascontiguousarray(stream, dtype=np.int32).reshape(-1, LP_WORDS)
    return (st[:, 0].copy(), st[:, 1].copy().view(np.float32), st[:, 2:2 + LP_TOP].copy(),
            np.ascontiguousarray(st[:, 2 + LP_TOP:]).view(np.float32))


def logprob_chunks(total: int, cap: int) -> list:
    """``(offset, words)`` of the K_LOGP rows that carry a stream of
    ``total`` words, ``cap`` payload words a row."""
    return [(off, min(cap, total - off)) for off in range(0, total, cap)]


def fill_logprob_row(row: np.ndarray, stream: np.ndarray, off: int, n: int) -> None:
    """Words ``off .. off + n`` of ``stream`` into the K_LOGP row ``row``."""
    row[10] = n
    row[DESC_HDR:DESC_HDR + n] = stream[off:off + n]


def take_logprob_rows(parts: dict, src: int, rows: np.ndarray) -> None:
    """K_LOGP rows from ``src`` into ``parts``: (source, handle) -> the
    stream so far (whole once every row of it has arrived; rows may come in
    several exchanges)."""
    for h, off, n, total, row in zip(_get64(rows, 1).tolist(), rows[:, 4].tolist(), rows[:, 10].tolist(),
                                     rows[:, 7].tolist(), rows):
        buf = parts.get((src, h))
        if buf is None or len(buf) != total:
            buf = parts[(src, h)] = np.zeros(total, dtype=np.int32)
        buf[off:off + n] = row[DESC_HDR:DESC_HDR + n]


def conv_key(conversation_id: str) -> int:
    """63-bit key of a conversation id (KV residency / affinity)."""
    if not conversation_id:
        return -1
    import hashlib
    return int.from_bytes(hashlib.blake2b(conversation_id.encode(), digest_size=8).digest(), "little") >> 1


def _put64(buf: np.ndarray, col: int, vals) -> None:
    """Store int64 ``vals`` into int32 columns (col, col + 1) = (lo, hi) of
    ``buf`` [n][width] (little-endian: an int64 viewed as two int32s)."""
    buf[:, col:col + 2] = np.asarray(vals, dtype=np.int64).reshape(-1, 1).view(np.int32)


def _get64(buf: np.ndarray, col: int) -> np.ndarray:
    """int64 from int32 columns (col, col + 1) = (lo, hi) of ``buf`` [n][width]."""
    return np.ascontiguousarray(buf[:, col:col + 2]).view(np.int64).reshape(-1)
