"""Domain objects: priorities, messages, conversations (component C1).

Parity notes (reference `pkg/models/message.go`):
  * ``Priority`` is a plain int where LOWER is more urgent: realtime=1, high=2,
    normal=3, low=4 (`message.go:15-22`).  ``priority_name`` reproduces
    ``Priority.String()`` (`message.go:24-37`), which maps every other value to
    ``"unknown"``.
  * JSON priority is emitted as an int.  On input we ALSO accept the strings the
    reference docs use (`README.md:180-186`, `docs/api.md:55-66`) -- the Go code
    rejects them with a 400 (defect D4 in SURVEY.md §8).
  * ``new_message`` defaults MaxRetries=3 / Timeout=30 s (`message.go:76-91`).
    REST-bound messages in the reference get Timeout=0 (defect D16); here the
    timeout always defaults to 30 s.
"""
from __future__ import annotations

import datetime as _dt
import itertools
import math
import re
import time
import uuid
from typing import Any, Dict, List, Optional

# --------------------------------------------------------------------------- priority
PRIORITY_REALTIME = 1
PRIORITY_HIGH = 2
PRIORITY_NORMAL = 3
PRIORITY_LOW = 4
PRIORITY_LEVELS = (PRIORITY_REALTIME, PRIORITY_HIGH, PRIORITY_NORMAL, PRIORITY_LOW)
LEVEL_NAMES = ("realtime", "high", "normal", "low")

_NAME_BY_PRIO = {1: "realtime", 2: "high", 3: "normal", 4: "low"}
_PRIO_BY_NAME = {
    "realtime": 1, "urgent": 1,  # "urgent" is the docs' realtime alias
    "high": 2, "normal": 3, "medium": 3, "low": 4,
}


class Priority(int):
    """Integer priority with the reference's ``String()`` naming.

    Subclassing int keeps arithmetic/comparison/JSON behaviour identical to the
    Go ``type Priority int``.
    """

    REALTIME = PRIORITY_REALTIME
    HIGH = PRIORITY_HIGH
    NORMAL = PRIORITY_NORMAL
    LOW = PRIORITY_LOW

    def __str__(self) -> str:  # Priority.String()
        return priority_name(int(self))

    def __repr__(self) -> str:
        return f"Priority({int(self)}:{priority_name(int(self))})"


def priority_name(p: int) -> str:
    """``Priority.String()`` -- queue names used everywhere as ``fmt.Sprint(p)``."""
    return _NAME_BY_PRIO.get(int(p), "unknown")


class PriorityParseError(ValueError):
    pass


_ASCII_WS = " \t\n\r\x0b\x0c"
_INT_TEXT = re.compile(r"[+-]?[0-9]+\Z")


def parse_priority(value: Any, default: int = 0) -> int:
    """Accept an integral number 0..4 (0 = let the preprocessor decide), a
    decimal string of one, or a level name (case-insensitive, ASCII-trimmed;
    ``urgent`` = realtime, ``medium`` = normal).  Anything else raises.  The
    C++ front door applies the same rule (``csrc/ingress/http_ingress.cpp:
    priority_from_string``), so both front doors accept and assign alike."""
    if value is None:
        return default
    if isinstance(value, bool):
        raise PriorityParseError(f"invalid priority {value!r}")
    if isinstance(value, float):
        if not math.isfinite(value) or value != int(value):
            raise PriorityParseError(f"invalid priority {value!r}")
        value = int(value)
    if isinstance(value, int):
        if not 0 <= value <= PRIORITY_LOW:
            raise PriorityParseError(f"invalid priority {value!r}")
        return int(value)
    if isinstance(value, str):
        s = value.strip(_ASCII_WS).lower()
        if s in _PRIO_BY_NAME:
            return _PRIO_BY_NAME[s]
        if _INT_TEXT.match(s) and len(s.lstrip("+-").lstrip("0")) <= 1:
            return parse_priority(int(s))
        raise PriorityParseError(f"invalid priority {value!r}")
    raise PriorityParseError(f"invalid priority {value!r}")


def level_priority_from_name(name: str) -> Optional[int]:
    """Map ``realtime|high|normal|low`` (any case) to its int, else None."""
    return {"realtime": 1, "high": 2, "normal": 3, "low": 4}.get(str(name).lower())


# --------------------------------------------------------------------------- enums
class MessageStatus:
    PENDING = "pending"
    PROCESSING = "processing"
    COMPLETED = "completed"
    FAILED = "failed"
    TIMEOUT = "timeout"
    CANCELLED = "cancelled"      # DELETE /api/v1/messages/{id} aborted it in flight
    ALL = ("pending", "processing", "completed", "failed", "timeout", "cancelled")


class ConversationState:
    ACTIVE = "active"
    INACTIVE = "inactive"
    COMPLETED = "completed"
    ARCHIVED = "archived"
    ALL = ("active", "inactive", "completed", "archived")


class ConversationNotFound(KeyError):
    """``ErrConversationNotFound`` (`message.go:11-13`)."""

    def __str__(self) -> str:  # KeyError quotes its arg; keep the Go text
        return "conversation not found"


# --------------------------------------------------------------------------- time helpers
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)
GO_ZERO_TIME = "0001-01-01T00:00:00Z"
DEFAULT_TIMEOUT_NS = 30 * 1_000_000_000
DEFAULT_MAX_RETRIES = 3


def now_ns() -> int:
    return time.time_ns()


def format_time(ns: Optional[int]) -> Optional[str]:
    """RFC3339Nano in UTC (Go's ``time.Time`` JSON encoding)."""
    if ns is None:
        return None
    if ns == 0:
        return GO_ZERO_TIME
    sec, rem = divmod(int(ns), 1_000_000_000)
    t = _dt.datetime.fromtimestamp(sec, tz=_dt.timezone.utc)
    frac = f".{rem:09d}".rstrip("0") if rem else ""
    if frac == ".":
        frac = ""
    return t.strftime("%Y-%m-%dT%H:%M:%S") + frac + "Z"


def parse_time(value: Any) -> Optional[int]:
    """Parse RFC3339 / epoch-ns into ns since epoch; None passes through."""
    if value is None or value == "":
        return None
    if isinstance(value, (int, float)):
        return int(value)
    s = str(value).strip()
    if s.startswith("0001-01-01"):
        return 0
    frac_ns = 0
    main = s
    tz = "+00:00"
    if s.endswith("Z"):
        main = s[:-1]
    else:
        for sep in ("+", "-"):
            idx = s.rfind(sep)
            if idx > 10:
                main, tz = s[:idx], s[idx:]
                break
    if "." in main:
        main, frac = main.split(".", 1)
        frac_ns = int((frac + "000000000")[:9])
    t = _dt.datetime.fromisoformat(main + tz)
    return int((t - _EPOCH).total_seconds()) * 1_000_000_000 + frac_ns


# --------------------------------------------------------------------------- message
_handle_counter = itertools.count(1)


class Message:
    """A queued LLM request (`message.go:58-74`).

    ``handle`` is a process-local integer id used by the native queue core
    (the C++ rings carry handles, never Python objects).
    """

    __slots__ = (
        "id", "conversation_id", "user_id", "content", "priority", "status",
        "queue_name", "retry_count", "max_retries", "timeout", "created_at",
        "updated_at", "scheduled_at", "completed_at", "metadata", "handle",
        "enqueued_at", "dispatched_at", "arrival_ns", "prompt_ids", "endpoint_id", "tier", "pin_key",
        "ingest_ns", "popped_ns", "recv_ns", "lc",
    )

    def __init__(self, id: str = "", conversation_id: str = "", user_id: str = "",
                 content: str = "", priority: int = 0, status: str = MessageStatus.PENDING,
                 queue_name: str = "", retry_count: int = 0,
                 max_retries: int = DEFAULT_MAX_RETRIES, timeout: int = DEFAULT_TIMEOUT_NS,
                 created_at: int = 0, updated_at: int = 0,
                 scheduled_at: Optional[int] = None, completed_at: Optional[int] = None,
                 metadata: Optional[Dict[str, Any]] = None):
        self.id = id
        self.conversation_id = conversation_id
        self.user_id = user_id
        self.content = content
        self.priority = int(priority)
        self.status = status
        self.queue_name = queue_name
        self.retry_count = int(retry_count)
        self.max_retries = int(max_retries)
        self.timeout = int(timeout)
        self.created_at = int(created_at)
        self.updated_at = int(updated_at)
        self.scheduled_at = scheduled_at
        self.completed_at = completed_at
        self.metadata = metadata if metadata is not None else {}
        self.handle = next(_handle_counter)
        self.enqueued_at = 0      # ns, set by the queue on push
        self.dispatched_at = 0    # ns, set by the dispatcher
        self.arrival_ns = 0       # ns, set by ingress (request received)
        self.prompt_ids = None    # token ids from the GPU tokenizer (backend prompt)
        self.endpoint_id = ""     # backend chosen at dispatch
        self.tier = -1            # tier index at dispatch
        self.pin_key = -1         # (home GPU, tier) the queued message is counted under (gateway pins)
        self.ingest_ns = 0        # ns, taken from the gateway inbox into a preprocess batch
        self.popped_ns = 0        # ns, popped from its queue by a dispatch decision
        self.recv_ns = 0          # ns, handed to this process's gateway (Gateway.submit)
        self.lc = 0               # lifecycle state at the origin router (gateway.request_table)

    # -- JSON ------------------------------------------------------------------
    def to_dict(self) -> Dict[str, Any]:
        return {
            "id": self.id,
            "conversation_id": self.conversation_id,
            "user_id": self.user_id,
            "content": self.content,
            "priority": int(self.priority),
            "status": self.status,
            "queue_name": self.queue_name,
            "retry_count": self.retry_count,
            "max_retries": self.max_retries,
            "timeout": self.timeout,
            "created_at": format_time(self.created_at),
            "updated_at": format_time(self.updated_at),
            "scheduled_at": format_time(self.scheduled_at),
            "completed_at": format_time(self.completed_at),
            "metadata": self.metadata,
        }

    @classmethod
    def from_dict(cls, d: Dict[str, Any], *, default_timeout_ns: int = DEFAULT_TIMEOUT_NS) -> "Message":
        """Bind a JSON body.  Raises ``PriorityParseError``/``ValueError`` on bad input."""
        if not isinstance(d, dict):
            raise ValueError("message body must be a JSON object")
        md = d.get("metadata")
        if md is not None and not isinstance(md, dict):
            raise ValueError("metadata must be an object")
        timeout = d.get("timeout")
        if timeout in (None, 0):
            timeout = default_timeout_ns
        elif isinstance(timeout, str):
            from ..utils.duration import parse_duration_ns
            timeout = parse_duration_ns(timeout)
        max_retries = d.get("max_retries")
        m = cls(
            id=str(d.get("id") or ""),
            conversation_id=str(d.get("conversation_id") or ""),
            user_id=str(d.get("user_id") or ""),
            content=str(d.get("content") or ""),
            priority=parse_priority(d.get("priority"), 0),
            status=str(d.get("status") or MessageStatus.PENDING),
            queue_name=str(d.get("queue_name") or ""),
            retry_count=int(d.get("retry_count") or 0),
            max_retries=DEFAULT_MAX_RETRIES if max_retries in (None, 0) else int(max_retries),
            timeout=int(timeout),
            created_at=parse_time(d.get("created_at")) or 0,
            updated_at=parse_time(d.get("updated_at")) or 0,
            scheduled_at=parse_time(d.get("scheduled_at")),
            completed_at=parse_time(d.get("completed_at")),
            metadata=dict(md) if md else {},
        )
        return m

    def copy(self) -> "Message":
        m = Message(self.id, self.conversation_id, self.user_id, self.content, self.priority,
                    self.status, self.queue_name, self.retry_count, self.max_retries,
                    self.timeout, self.created_at, self.updated_at, self.scheduled_at,
                    self.completed_at, dict(self.metadata))
        return m

    def __repr__(self) -> str:
        return (f"Message(id={self.id!r}, prio={self.priority}, queue={self.queue_name!r}, "
                f"status={self.status!r}, retry={self.retry_count})")


def new_message(conversation_id: str, user_id: str, content: str, priority: int) -> Message:
    """``NewMessage`` (`message.go:76-91`)."""
    t = now_ns()
    return Message(id=str(uuid.uuid4()), conversation_id=conversation_id, user_id=user_id,
                   content=content, priority=priority, status=MessageStatus.PENDING,
                   retry_count=0, max_retries=DEFAULT_MAX_RETRIES, timeout=DEFAULT_TIMEOUT_NS,
                   created_at=t, updated_at=t, metadata={})


# --------------------------------------------------------------------------- sampling parameters
TEMPERATURE_MIN, TEMPERATURE_MAX = 0.05, 2.0


class SamplingParseError(ValueError):
    pass


def default_seed(message_id: str) -> int:
    """63-bit seed of a message that names none: a hash of its id, so every
    retry / replay of the message draws the same tokens."""
    import hashlib
    return int.from_bytes(hashlib.blake2b((message_id or "").encode(), digest_size=8).digest(), "little") >> 1


def sampling_from_metadata(md: Any, message_id: str = "") -> tuple:
    """``(temperature, seed)`` of a message's ``metadata.sampling`` object.

    ``temperature``: 0 (greedy, the default) or a number in [0.05, 2.0].
    ``seed``: an integer in [0, 2^63); without one, ``default_seed(message_id)``.
    ``top_k`` / ``top_p`` of the same object: :func:`truncation_from_metadata`;
    its penalties: :func:`penalties_from_metadata`.
    Raises ``SamplingParseError`` on anything else."""
    sp = md.get("sampling") if isinstance(md, dict) else None
    if sp is None:
        return 0.0, default_seed(message_id)
    if not isinstance(sp, dict):
        raise SamplingParseError("sampling must be an object")
    t = sp.get("temperature", 0.0)
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t):
        raise SamplingParseError("sampling.temperature must be a number")
    t = float(t)
    if t != 0.0 and not (TEMPERATURE_MIN <= t <= TEMPERATURE_MAX):
        raise SamplingParseError(f"sampling.temperature must be 0 or in [{TEMPERATURE_MIN}, {TEMPERATURE_MAX}]")
    seed = sp.get("seed")
    if seed is None:
        seed = default_seed(message_id)
    elif isinstance(seed, bool) or not isinstance(seed, int) or not (0 <= seed < (1 << 63)):
        raise SamplingParseError("sampling.seed must be an integer in [0, 2^63)")
    return t, int(seed)


TOP_K_MAX = 1023                     # (10 bits of the dispatch descriptor's flags column)


def truncation_from_metadata(md: Any) -> tuple:
    """``(top_k, top_p)`` of a message's ``metadata.sampling`` object.

    ``top_k``: an integer, 0 (off, the default) or 1..1023.  ``top_p``: a
    number in (0, 1], rounded to thousandths (so at least 0.001 after
    rounding); 1.0 (the default) is off.  Both take effect only with a
    ``temperature`` > 0.  Raises ``SamplingParseError`` on anything else."""
    sp = md.get("sampling") if isinstance(md, dict) else None
    if sp is None:
        return 0, 1.0
    if not isinstance(sp, dict):
        raise SamplingParseError("sampling must be an object")
    k = sp.get("top_k", 0)
    if isinstance(k, bool) or not isinstance(k, int) or not (0 <= k <= TOP_K_MAX):
        raise SamplingParseError(f"sampling.top_k must be an integer, 0 or in [1, {TOP_K_MAX}]")
    p = sp.get("top_p", 1.0)
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not math.isfinite(p):
        raise SamplingParseError("sampling.top_p must be a number")
    permille = int(round(float(p) * 1000.0))
    if not (0.0 < p <= 1.0) or permille < 1:
        raise SamplingParseError("sampling.top_p must be in (0, 1] and at least 0.001")
    return int(k), permille / 1000.0


from ..ops.sampling import LP_TOP as LOGPROBS_MAX  # noqa: E402  (the alternatives the kernel reports)


def logprobs_from_metadata(md: Any) -> int:
    """``logprobs`` of a message's ``metadata.sampling`` object: -1 (off, the
    default: the key is absent) or an integer ``n`` in 0..5 -- return every
    generated token with its log-probability and, for ``n`` > 0, the ``n``
    most likely tokens at each position.  It works with or without a
    ``temperature``.  Raises ``SamplingParseError`` on anything else."""
    sp = md.get("sampling") if isinstance(md, dict) else None
    if sp is None:
        return -1
    if not isinstance(sp, dict):
        raise SamplingParseError("sampling must be an object")
    if "logprobs" not in sp:
        return -1
    n = sp["logprobs"]
    if isinstance(n, bool) or not isinstance(n, int) or not (0 <= n <= LOGPROBS_MAX):
        raise SamplingParseError(f"sampling.logprobs must be an integer in [0, {LOGPROBS_MAX}]")
    return int(n)


# the penalty keys of ``metadata.sampling``: (lowest, highest, the value that is off)
PENALTY_KEYS = {"presence_penalty": (-2.0, 2.0, 0.0), "frequency_penalty": (-2.0, 2.0, 0.0),
                "repetition_penalty": (0.5, 2.0, 1.0)}


def penalty_from_metadata(md: Any, key: str) -> float:
    """One of ``presence_penalty`` / ``frequency_penalty`` /
    ``repetition_penalty`` of a message's ``metadata.sampling`` object,
    rounded to hundredths; the key's off value where it is absent.  Raises
    ``SamplingParseError`` on anything but a number in the key's range."""
    lo, hi, off = PENALTY_KEYS[key]
    sp = md.get("sampling") if isinstance(md, dict) else None
    if sp is None:
        return off
    if not isinstance(sp, dict):
        raise SamplingParseError("sampling must be an object")
    if key not in sp:
        return off
    v = sp[key]
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not (lo <= v <= hi):
        raise SamplingParseError(f"sampling.{key} must be a number in [{lo}, {hi}]")
    return int(round(float(v) * 100.0)) / 100.0


def penalties_from_metadata(md: Any) -> tuple:
    """``(presence_penalty, frequency_penalty, repetition_penalty)`` of a
    message's ``metadata.sampling`` object: numbers in [-2, 2], [-2, 2] and
    [0.5, 2], rounded to hundredths; 0, 0 and 1.0 (the defaults) are off.
    They work with or without a ``temperature`` and apply before it
    (``csrc/kernels/penalty_kernels.h``): presence and frequency over the
    tokens generated so far, repetition over those and the message's own
    prompt.  Raises ``SamplingParseError`` on anything else."""
    return tuple(penalty_from_metadata(md, k) for k in PENALTY_KEYS)


from ..ops.sampling import LE_MAX as EDIT_LIST_MAX  # noqa: E402  (entries the edit kernel takes a list)
LOGIT_BIAS_MAX = 100.0
TOKEN_ID_END = 1 << 31


def _sampling_object(md: Any):
    sp = md.get("sampling") if isinstance(md, dict) else None
    if sp is not None and not isinstance(sp, dict):
        raise SamplingParseError("sampling must be an object")
    return sp


def min_p_from_metadata(md: Any) -> float:
    """``min_p`` of a message's ``metadata.sampling`` object: a number in [0,
    1], rounded to thousandths; 0 (the default, and any value that rounds to
    it) is off.  It takes effect only with a ``temperature`` > 0: a token
    stays eligible iff its probability is at least ``min_p`` times the most
    likely token's.  Raises ``SamplingParseError`` on anything else."""
    sp = _sampling_object(md)
    if sp is None or "min_p" not in sp:
        return 0.0
    v = sp["min_p"]
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not (0.0 <= v <= 1.0):
        raise SamplingParseError("sampling.min_p must be a number in [0, 1]")
    return int(round(float(v) * 1000.0)) / 1000.0


def _token_id(x: Any, what: str) -> int:
    if isinstance(x, bool) or not isinstance(x, int) or not (0 <= x < TOKEN_ID_END):
        raise SamplingParseError(f"sampling.{what} must be integers in [0, 2^31)")
    return int(x)


def logit_bias_from_metadata(md: Any) -> tuple:
    """``logit_bias`` of a message's ``metadata.sampling`` object: ``(ids
    int32 [n], values float32 [n])``, n <= 64, in the object's order and
    without the entries whose value is 0; two empty arrays where the key is
    absent.  The object maps a token id -- a JSON key, so the integer's
    canonical decimal string: no sign, no leading zero -- in [0, 2^31) to a
    number in [-100, 100] that is added to the token's logit as
    ``float32(value)``, with or without a ``temperature``.  Raises
    ``SamplingParseError`` on anything else."""
    import numpy as np
    sp = _sampling_object(md)
    ids, vals = [], []
    if sp is not None and "logit_bias" in sp:
        lb = sp["logit_bias"]
        if not isinstance(lb, dict) or len(lb) > EDIT_LIST_MAX:
            raise SamplingParseError(f"sampling.logit_bias must be an object of at most {EDIT_LIST_MAX} entries")
        for k, v in lb.items():
            # (at most the 10 digits of 2^31 - 1 before any conversion: int() itself refuses very long strings
            #  with a plain ValueError)
            if not isinstance(k, str) or not 0 < len(k) <= 10 or not k.isascii() or not k.isdigit() \
                    or k != str(int(k)):
                raise SamplingParseError("sampling.logit_bias keys must be token ids in canonical decimal form")
            t = _token_id(int(k), "logit_bias keys")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) \
                    or not (-LOGIT_BIAS_MAX <= v <= LOGIT_BIAS_MAX):
                raise SamplingParseError(f"sampling.logit_bias values must be numbers in [-{LOGIT_BIAS_MAX:g}, "
                                         f"{LOGIT_BIAS_MAX:g}]")
            if np.float32(v) != 0:
                ids.append(t)
                vals.append(v)
    return np.asarray(ids, dtype=np.int32), np.asarray(vals, dtype=np.float32)


def allowed_from_metadata(md: Any):
    """``allowed_token_ids`` of a message's ``metadata.sampling`` object: an
    int32 array of 1..64 distinct token ids in [0, 2^31), the only tokens
    that can be picked or drawn, greedy or sampling; an empty array where
    the key is absent.  Raises ``SamplingParseError`` on anything else."""
    import numpy as np
    sp = _sampling_object(md)
    if sp is None or "allowed_token_ids" not in sp:
        return np.zeros(0, dtype=np.int32)
    al = sp["allowed_token_ids"]
    if not isinstance(al, (list, tuple)) or not (1 <= len(al) <= EDIT_LIST_MAX):
        raise SamplingParseError(f"sampling.allowed_token_ids must be a list of 1 to {EDIT_LIST_MAX} token ids")
    ids = [_token_id(x, "allowed_token_ids") for x in al]
    if len(set(ids)) != len(ids):
        raise SamplingParseError("sampling.allowed_token_ids must be distinct")
    return np.asarray(ids, dtype=np.int32)


def eligibility_from_metadata(md: Any) -> tuple:
    """``(min_p, logit_bias, allowed_token_ids)`` of a message's
    ``metadata.sampling`` object (:func:`min_p_from_metadata`,
    :func:`logit_bias_from_metadata`, :func:`allowed_from_metadata`).  Order
    of the whole object: penalties, ``allowed_token_ids``, ``logit_bias``,
    temperature, ``top_k``, ``top_p``, ``min_p``, then the draw."""
    return min_p_from_metadata(md), logit_bias_from_metadata(md), allowed_from_metadata(md)


from ..ops.sampling import STOP_ENTRIES, STOP_LEN  # noqa: E402  (entries a request, tokens an entry: the stop kernel's)
STOP_KEYS = ("max_tokens", "min_tokens", "stop_token_ids", "stop_sequences")


def _count(sp, key: str, lo: int, hi, default: int) -> int:
    if sp is None or key not in sp:
        return default
    v = sp[key]
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise SamplingParseError(f"sampling.{key} must be an integer in [{lo}, {hi}]" if hi is not None
                                 else f"sampling.{key} must be an integer, at least {lo}")
    return int(v)


def max_tokens_from_metadata(md: Any, gen_tokens: int = 0) -> int:
    """``max_tokens`` of a message's ``metadata.sampling`` object: an integer
    in [1, ``gen_tokens``], the configured count (``backend.gen_tokens``),
    which stays the default and the cap; 0 where the key is absent.  With
    ``gen_tokens`` 0 (the caller knows no configured count) any integer >= 1
    passes.  Raises ``SamplingParseError`` on anything else."""
    return _count(_sampling_object(md), "max_tokens", 1, int(gen_tokens) if gen_tokens > 0 else None, 0)


def min_tokens_from_metadata(md: Any, cap: int = 0) -> int:
    """``min_tokens`` of a message's ``metadata.sampling`` object: an integer
    in [0, ``cap``] (the request's ``max_tokens``, else the configured count;
    0: no cap known), default 0.  Raises ``SamplingParseError`` on anything
    else."""
    return _count(_sampling_object(md), "min_tokens", 0, int(cap) if cap > 0 else None, 0)


def stop_token_ids_from_metadata(md: Any) -> list:
    """``stop_token_ids`` of a message's ``metadata.sampling`` object: a list
    of 1..8 distinct token ids in [0, 2^31), in the order given; empty where
    the key is absent.  Raises ``SamplingParseError`` on anything else."""
    sp = _sampling_object(md)
    if sp is None or "stop_token_ids" not in sp:
        return []
    st = sp["stop_token_ids"]
    if not isinstance(st, (list, tuple)) or not (1 <= len(st) <= STOP_ENTRIES):
        raise SamplingParseError(f"sampling.stop_token_ids must be a list of 1 to {STOP_ENTRIES} token ids")
    ids = [_token_id(x, "stop_token_ids") for x in st]
    if len(set(ids)) != len(ids):
        raise SamplingParseError("sampling.stop_token_ids must be distinct")
    return ids


def stop_sequences_from_metadata(md: Any) -> list:
    """``stop_sequences`` of a message's ``metadata.sampling`` object: a list
    of 1..8 lists of 1..8 token ids in [0, 2^31) each; empty where the key is
    absent.  Raises ``SamplingParseError`` on anything else."""
    sp = _sampling_object(md)
    if sp is None or "stop_sequences" not in sp:
        return []
    sq = sp["stop_sequences"]
    if not isinstance(sq, (list, tuple)) or not (1 <= len(sq) <= STOP_ENTRIES):
        raise SamplingParseError(f"sampling.stop_sequences must be a list of 1 to {STOP_ENTRIES} lists")
    out = []
    for e in sq:
        if not isinstance(e, (list, tuple)) or not (1 <= len(e) <= STOP_LEN):
            raise SamplingParseError(f"sampling.stop_sequences entries must be lists of 1 to {STOP_LEN} token ids")
        out.append([_token_id(x, "stop_sequences") for x in e])
    return out


def stop_entries(stop_token_ids: list, stop_sequences: list) -> list:
    """The stop entries in entry order: the stop tokens in the order given,
    each an entry of one token, then the sequences; at most 8 together, else
    ``SamplingParseError``."""
    out = [[t] for t in stop_token_ids] + list(stop_sequences)
    if len(out) > STOP_ENTRIES:
        raise SamplingParseError(f"sampling.stop_token_ids and stop_sequences hold at most {STOP_ENTRIES} "
                                 "entries together")
    return out


def stop_entries_from_metadata(md: Any) -> list:
    """The stop entries of a message's ``metadata.sampling`` object
    (:func:`stop_token_ids_from_metadata`, :func:`stop_sequences_from_metadata`,
    :func:`stop_entries`).  Raises ``SamplingParseError`` on a bad value."""
    return stop_entries(stop_token_ids_from_metadata(md), stop_sequences_from_metadata(md))


def stop_from_metadata(md: Any, gen_tokens: int = 0) -> tuple:
    """``(max_tokens, min_tokens, entries, n_stop_tokens)`` of a message's
    ``metadata.sampling`` object (:func:`max_tokens_from_metadata`,
    :func:`stop_entries_from_metadata`; the first ``n_stop_tokens`` entries
    are its ``stop_token_ids``).  ``min_tokens``: an integer in [0,
    ``max_tokens``] (the configured count where ``max_tokens`` is absent),
    default 0 -- a stop that would end the generation with fewer tokens is
    ignored.  It filters the stop decision; it masks no logit, and none of
    the four keys changes a token that is drawn.  Raises
    ``SamplingParseError`` on anything else."""
    sp = _sampling_object(md)
    mx = max_tokens_from_metadata(md, gen_tokens)
    mn = min_tokens_from_metadata(md, mx or gen_tokens)
    ent = stop_entries_from_metadata(md)
    n_tok = len(sp["stop_token_ids"]) if (sp is not None and "stop_token_ids" in sp) else 0
    return mx, mn, ent, n_tok


def finish_record(tokens, finish_reason: str, stop_reason=None) -> Dict[str, Any]:
    """``metadata.generation`` of a completed message that named a stop key
    (``max_tokens``, ``min_tokens``, ``stop_token_ids``, ``stop_sequences``):
    the generated tokens, ``finish_reason`` ("stop" or "length") and, for a
    stop, the matched entry (an int for a stop token, a list for a sequence)."""
    out = {"tokens": [int(t) for t in tokens], "finish_reason": str(finish_reason)}
    if finish_reason == "stop" and stop_reason is not None:
        out["stop_reason"] = stop_reason
    return out


def generation_record(tokens, token_logprobs, top_ids, top_logprobs, n: int) -> Dict[str, Any]:
    """``metadata.generation`` of a completed message that asked for
    ``logprobs = n``: the generated tokens, their log-probabilities and, for
    ``n`` > 0, the ``n`` most likely tokens of each position (fewer where the
    distribution had fewer).  A non-finite value is written as None (JSON
    ``null``)."""
    def num(x):
        x = float(x)
        return x if math.isfinite(x) else None

    out = {"tokens": [int(t) for t in tokens], "token_logprobs": [num(x) for x in token_logprobs]}
    if n > 0:
        out["top_logprobs"] = [[{"token": int(i), "logprob": num(x)} for i, x in zip(ids[:n], lps[:n]) if i >= 0]
                               for ids, lps in zip(top_ids, top_logprobs)]
    return out


# --------------------------------------------------------------------------- conversation
class Conversation:
    """`message.go:93-109`, plus the summary state produced by the
    ``context_summarise`` kernel (N5)."""

    __slots__ = (
        "id", "user_id", "title", "context", "status", "state", "priority",
        "message_count", "last_activity", "last_active_time", "created_at",
        "updated_at", "completed_at", "messages", "metadata", "summary_vec",
        "summary_tokens", "evicted_count", "home_gpu",
    )

    def __init__(self, id: str, user_id: str = "", *, created_at: Optional[int] = None,
                 state: str = ConversationState.ACTIVE, metadata: Optional[Dict[str, Any]] = None):
        t = now_ns() if created_at is None else created_at
        self.id = id
        self.user_id = user_id
        self.title = ""
        self.context = ""
        self.status = ""
        self.state = state
        self.priority = 0
        self.message_count = 0
        self.last_activity = t
        self.last_active_time = t
        self.created_at = t
        self.updated_at = t
        self.completed_at = 0
        self.messages: List[Message] = []
        self.metadata: Dict[str, Any] = metadata if metadata is not None else {}
        self.summary_vec = None        # list[float] | None  (N5 output)
        self.summary_tokens: List[int] = []  # salient token hashes (N5 output)
        self.evicted_count = 0
        self.home_gpu = -1             # KV-residency hint (sticky routing)

    def to_dict(self, include_messages: bool = True) -> Dict[str, Any]:
        d = {
            "id": self.id,
            "user_id": self.user_id,
            "title": self.title,
            "context": self.context,
            "status": self.status,
            "state": self.state,
            "priority": int(self.priority),
            "message_count": self.message_count,
            "last_activity": format_time(self.last_activity),
            "last_active_time": format_time(self.last_active_time),
            "created_at": format_time(self.created_at),
            "updated_at": format_time(self.updated_at),
            "completed_at": format_time(self.completed_at),
            "messages": [m.to_dict() for m in self.messages] if include_messages else [],
            "metadata": self.metadata,
        }
        if self.summary_tokens or self.summary_vec is not None:
            d["summary"] = {"evicted_messages": self.evicted_count,
                            "salient_tokens": list(self.summary_tokens)}
        if self.home_gpu >= 0:
            d["home_gpu"] = self.home_gpu
        return d

    @classmethod
    def from_dict(cls, d: Dict[str, Any]) -> "Conversation":
        c = cls(str(d.get("id", "")), str(d.get("user_id", "")),
                created_at=parse_time(d.get("created_at")) or 0,
                state=str(d.get("state") or ConversationState.ACTIVE),
                metadata=dict(d.get("metadata") or {}))
        c.title = str(d.get("title") or "")
        c.context = str(d.get("context") or "")
        c.status = str(d.get("status") or "")
        c.priority = int(d.get("priority") or 0)
        c.message_count = int(d.get("message_count") or 0)
        c.last_activity = parse_time(d.get("last_activity")) or 0
        c.last_active_time = parse_time(d.get("last_active_time")) or 0
        c.updated_at = parse_time(d.get("updated_at")) or 0
        c.completed_at = parse_time(d.get("completed_at")) or 0
        c.messages = [Message.from_dict(m) for m in (d.get("messages") or [])]
        s = d.get("summary") or {}
        c.evicted_count = int(s.get("evicted_messages", 0))
        c.summary_tokens = list(s.get("salient_tokens", []))
        c.home_gpu = int(d.get("home_gpu", -1))
        return c


class QueueStats:
    """Per-named-queue counters (`queue.go:60-68`).  Always returned as a copy
    (the reference returns its live pointer -- defect D22)."""

    __slots__ = ("pending_count", "processing_count", "completed_count", "failed_count",
                 "total_wait_time", "total_process_time", "last_update")

    def __init__(self, pending_count=0, processing_count=0, completed_count=0, failed_count=0,
                 total_wait_time=0, total_process_time=0, last_update=0):
        self.pending_count = pending_count
        self.processing_count = processing_count
        self.completed_count = completed_count
        self.failed_count = failed_count
        self.total_wait_time = total_wait_time
        self.total_process_time = total_process_time
        self.last_update = last_update

    def to_dict(self) -> Dict[str, Any]:
        return {
            "PendingCount": self.pending_count,
            "ProcessingCount": self.processing_count,
            "CompletedCount": self.completed_count,
            "FailedCount": self.failed_count,
            "TotalWaitTime": self.total_wait_time,
            "TotalProcessTime": self.total_process_time,
            "LastUpdate": format_time(self.last_update),
        }

    def __repr__(self) -> str:
        return (f"QueueStats(pending={self.pending_count}, processing={self.processing_count}, "
                f"completed={self.completed_count}, failed={self.failed_count})")
