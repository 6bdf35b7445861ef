"""Fixed-width int32 rows the ranks exchange in every tick's all_to_all
(``parallel.comm``): request descriptors a router hands to another GPU,
completion / failure / abort records owed back to the origin router, KV
migration orders and cancels.  int64 fields travel as (lo, hi) int32 pairs.
The reference has no inter-service transport at all: its binaries do not
share queues."""
from __future__ import annotations

import numpy as np

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
# payload columns, their count in col 10 (dialog turns: the origin's history)
DESC_HDR = 20       # [kind, handle lo/hi, origin, tier, arrival lo/hi, enq lo/hi, gen, plen, flags, conv lo/hi,
#                    dialog history length, decision - enq (us), processing timeout (ms),
#                    sampling temperature (float32 bits), sampling seed lo/hi];
#                    flags = (home GPU + 1) | KV_MIGRATE | DIALOG_TURN | top_k << 10 | top_p permille << 20
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
