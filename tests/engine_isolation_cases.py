"""Scenario, driver and poisoner of the engine isolation tests
(``test_engine_isolation_cpu.py``, ``test_gpu_engine_isolation.py``).

One deterministic schedule is served twice by ``BackendEngine``.  In the
second run, before every launch of either pool, every byte the engine's own
bookkeeping says no live row may read is overwritten: KV positions at or past
a slot's context, device-history positions outside a penalty / stop window,
the kernels' ``torch.empty`` scratch, and the host pins of the step about to
launch.  The two runs must agree bit for bit; there is no tolerance.

The host schedule does not depend on GPU timing: the serving driver only ever
waits blockingly (``launch`` reaping the oldest step once ``max_inflight`` are
queued, ``finish(block=True)`` on every third iteration), and the micro driver
blocks on every step, so every launch sees the same host state in every run.

What a launch may read (``Poisoner._windows``; the engine lines they encode
are named in ``test_gpu_engine_isolation.py``'s docstring):

  KV, slot s    active: ``s_pref[s] + max(s_gen[s] - 1, 0)`` positions
                parked (``conv_lru[s_conv[s]] == s``): ``s_cached[s]``
                otherwise: none
  history, s    active with ``s_pen[s]`` or ``s_shist[s]``: ``[lo, valid)``,
                ``lo = s_pfrom[s]`` if penalised else ``s_plen[s]``
                otherwise: none

Every poison value keeps a stray read a wrong value, never a bad address: NaN
bit patterns or finite floats for floating data, ids inside the vocabulary for
token data.
"""
import functools
import hashlib
from typing import NamedTuple, Optional

import numpy as np
import torch

SLOTS, MAX_CTX, MICRO_SLOTS = 8, 64, 4
VOCAB = 1024
SEED = 5
FINISH_EVERY = 3                 # the serving driver reaps everything on every third iteration
# penalty strengths at which a history id moved by one position changes a pick
STRONG = dict(presence_penalty=1.2, frequency_penalty=0.6, repetition_penalty=1.5)
DEFAULT_ID = 1                   # history poison of a slot whose clean run has no token to aim at
PIN_ID = 2                       # stale "sampled id" of a result pin
K_QNAN, K_SNAN, V_NAN = 0x7FC0, 0x7F81, -1        # bf16 bit patterns (V: 0xFFFF), as in test_gpu_attention.py
CLASSES = ("kv", "hist", "scratch", "pins")
COUNTERS = ("total_tokens", "completed_tokens", "completed_total", "stopped_total", "stop_dropped_rows",
            "kv_reused_tokens", "cancelled_total", "expired_total", "step_id", "micro_id", "micro_steps",
            "micro_graph_steps", "sampled_steps", "truncated_steps", "logprob_steps", "penalised_steps",
            "edited_steps", "stop_steps")
FIELDS = ("out_tokens", "out_logprobs", "out_top_ids", "out_top_logprobs")

I32 = lambda v: np.asarray(v, dtype=np.int32)      # noqa: E731
F32 = lambda v: np.asarray(v, dtype=np.float32)    # noqa: E731


class Spec(NamedTuple):
    rid: int
    at: int                      # the driver iteration from which the request is ready
    n: int                       # prompt tokens
    gen: int
    kw: dict
    after: int = -1              # ready only once this request's completion was delivered (a dialog's next turn)
    stop_ids: Optional[tuple] = None   # (a, b): stop on its own generated ids a..b-1 of the discovery run
    one_token: bool = False      # ... as a one-token stop: the last of those ids that it has not generated before


# ----------------------------------------------------------------------------- scenarios
# Serving (slots 8, token_budget 24, max_inflight 2).  Iteration 0 admits six
# requests whose prompts (36 tokens) spill over the budget; 6 and 7 run long
# and are expired / cancelled with steps in flight; the two stop requests are
# admitted together at iteration 2, so they sample generated id 4 in step 6,
# reaped at launch 8 with step 7 (their next rows) already queued.
CANCEL_RID, CANCEL_AT = 7, 4
EXPIRE_RID, EXPIRE_AT = 6, 5
STOP_RIDS = (4, 5)
DIALOG = (14, 15, 16, 17)        # conversation 7: three resident turns, then one that overflows max_ctx
LONG_RID = 8                     # a prompt longer than the token budget
SERVING = (
    Spec(0, 0, 4, 5, {}),
    Spec(1, 0, 9, 8, dict(logprobs=2)),
    Spec(2, 0, 5, 6, dict(temperature=0.8, seed=11)),
    Spec(3, 0, 7, 7, dict(temperature=0.9, seed=12, top_k=5, top_p=0.9, logprobs=0)),
    Spec(6, 0, 6, 24, dict(timeout_ns=3600 * 10 ** 9, **STRONG)),
    Spec(7, 0, 5, 24, dict(temperature=0.7, seed=19)),
    Spec(4, 2, 3, 12, dict(finish=True), stop_ids=(2, 5), one_token=True),
    Spec(5, 2, 6, 12, dict(temperature=0.7, seed=18, min_tokens=3, finish=True, **STRONG), stop_ids=(2, 5)),
    Spec(8, 3, 37, 4, dict(temperature=0.7, seed=13, min_p=0.25)),
    Spec(9, 3, 6, 7, dict(presence_penalty=1.2)),
    Spec(10, 3, 8, 6, dict(temperature=1.1, seed=14, frequency_penalty=0.6, top_k=8, min_p=0.05)),
    Spec(11, 3, 5, 8, dict(repetition_penalty=1.5)),
    Spec(12, 4, 4, 4, dict(allowed=I32([3, 5, 7, 9]))),
    Spec(13, 4, 6, 5, dict(logit_bias=(I32([10, 2000000]), F32([2.0, -3.0])), presence_penalty=0.2,
                           temperature=0.6, seed=15)),
    Spec(18, 9, 5, 16, dict(**STRONG)),
    Spec(19, 9, 2, 14, dict(temperature=0.8, seed=17, top_p=0.8, allowed=I32([1, 2, 30, 40, 50]),
                            logit_bias=(I32([2]), F32([1.5])))),
    Spec(14, 12, 6, 5, dict(conv=7)),
    Spec(15, 12, 5, 6, dict(conv=7, **STRONG), after=14),
    Spec(16, 12, 4, 5, dict(conv=7, logprobs=1), after=15),
    Spec(17, 12, 30, 8, dict(conv=7), after=16),
    Spec(20, 14, 5, 7, {}),
)
# Micro (slots 8 + 4, token_budget 32): plain realtime requests (tier 0) whose
# decode steps replay graphs once the realtime request with options (eager:
# penalty, stop, logprobs) has stopped, later ones that take the freed micro
# slots, and a serving-pool crowd (tier 2) next to them
MICRO_STOP_RID = 3
MICRO = (
    Spec(0, 0, 5, 10, dict(tier=0)),
    Spec(1, 0, 7, 10, dict(tier=0)),
    Spec(2, 0, 6, 9, dict(tier=0)),
    Spec(3, 0, 6, 8, dict(tier=0, logprobs=1, finish=True, **STRONG), stop_ids=(1, 3)),
    Spec(4, 0, 40, 4, dict(tier=2)),
    Spec(5, 0, 6, 6, dict(tier=2, temperature=0.8, seed=21, top_k=6)),
    Spec(6, 0, 5, 7, dict(tier=2, **STRONG)),
    Spec(7, 1, 4, 5, dict(tier=2, logprobs=2)),
    Spec(8, 2, 5, 6, dict(tier=0)),
    Spec(9, 2, 3, 7, dict(tier=0)),
    Spec(10, 2, 7, 5, dict(tier=2, temperature=0.9, seed=22, repetition_penalty=1.5)),
    Spec(11, 3, 6, 4, dict(tier=2)),
)
SCENARIOS = {"serving": SERVING, "micro": MICRO}


def _prompt(rid: int, n: int) -> np.ndarray:
    return np.random.default_rng(900 + rid).integers(0, VOCAB, n).astype(np.int32)


def stop_entries(spec: Spec, ids) -> list:
    """The stop entries of ``spec`` from the ids its request generated in
    the discovery run."""
    a, b = spec.stop_ids
    ids = [int(x) for x in ids]
    assert len(ids) >= b, (spec.rid, ids)
    if not spec.one_token:
        return [ids[a:b]]
    fresh = [j for j in range(a, b) if ids[j] not in ids[:j]]
    assert fresh, (spec.rid, ids)
    return [[ids[fresh[-1]]]]


def _requests(scenario: str, stops):
    """``stops``: rid -> entries (None: the discovery run, nobody stops)."""
    from llm_message_queue_amd.backend.engine import Request
    out = []
    for sp in SCENARIOS[scenario]:
        kw = dict(sp.kw)
        if sp.stop_ids is not None and stops is not None:
            kw["stop"] = stops[sp.rid]
        out.append((sp, Request(req_id=sp.rid, prompt=_prompt(sp.rid, sp.n), gen_tokens=sp.gen, **kw)))
    return out


# ----------------------------------------------------------------------------- poisoner
class Poisoner:
    """Wraps ``eng._launch_pool``: before every launch of a pool, the
    overwrites of ``classes`` on that pool's stream, over that pool's slots.
    Records per launch what the windows were and what was written, and for
    every sampled row (request, generated index) -> the launch that drew it.

    ``aim``: rid -> the clean run's ``out_tokens``; a slot's history poison
    is the id its request sampled at generated index ``s_gen[s]`` there, the
    one the row is about to pick.  The controls move a window edge into live
    data: ``kv_shift`` / ``hist_hi_shift`` -1 start the poison one position
    early (active slots), ``hist_lo_shift`` +1 ends the front poison one
    position late."""

    def __init__(self, eng, classes=(), aim=None, kv_shift: int = 0, hist_lo_shift: int = 0,
                 hist_hi_shift: int = 0):
        self.eng = eng
        self.classes = frozenset(classes)
        assert self.classes <= set(CLASSES), classes
        self.aim = aim or {}
        self.kv_shift, self.hist_lo_shift, self.hist_hi_shift = kv_shift, hist_lo_shift, hist_hi_shift
        self.launches = []
        self.drawn = {}                  # (rid, generated index) -> launch number
        self.zeroed = set()              # (scratch user, spec index) allocated with torch.zeros
        self.used = set()                # scratch users this engine's forwards called for
        self._inner = eng._launch_pool
        eng._launch_pool = self._launch_pool
        self._G = self._scratch_inner = None
        if eng.cuda and eng.impl == "hip":
            from llm_message_queue_amd.ops import gemm as G
            self._G, self._scratch_inner = G, G._scratch
            G._scratch = self._scratch

    def close(self):
        if self._G is not None:
            self._G._scratch = self._scratch_inner

    def _scratch(self, device, stream, name, *specs):
        self.used.add(name)
        for i, sp in enumerate(specs):
            if sp[2] is torch.zeros:
                self.zeroed.add((name, i))
        return self._scratch_inner(device, stream, name, *specs)

    # -- what the bookkeeping says
    def _windows(self, a: int, b: int):
        """Per slot of [a, b): KV positions valid before the next launch,
        and the history window [lo, hi) it may read (empty: lo = hi = 0)."""
        e = self.eng
        sl = slice(a, b)
        act = e.s_active[sl]
        valid = np.where(act, e.s_pref[sl] + np.maximum(e.s_gen[sl] - 1, 0), 0)
        for conv, s in e.conv_lru.items():
            if a <= s < b and e.s_conv[s] == conv and not e.s_active[s]:
                valid[s - a] = e.s_cached[s]
        reads = act & (e.s_pen[sl] | e.s_shist[sl])
        lo = np.where(reads, np.where(e.s_pen[sl], e.s_pfrom[sl], e.s_plen[sl]), 0)
        hi = np.where(reads, valid, 0)
        return act, valid.astype(np.int64), lo.astype(np.int64), hi.astype(np.int64)

    def _ids(self, a: int, b: int) -> np.ndarray:
        e = self.eng
        ids = np.full(b - a, DEFAULT_ID, dtype=np.int32)
        for s in range(a, b):
            r = e.active.get(s)
            t = self.aim.get(r.req_id) if r is not None else None
            if t is not None and e.s_gen[s] < len(t):
                ids[s - a] = t[e.s_gen[s]]
        return ids

    # -- the overwrites
    def _poison_kv(self, a, b, act, valid):
        e, dev = self.eng, self.eng.device
        start = np.where(act, np.maximum(valid + self.kv_shift, 0), valid)[:, None]
        pos = np.arange(e.max_ctx)[None, :]
        mask = torch.from_numpy(pos >= start).to(dev)[:, None, :, None]
        pat = torch.from_numpy(np.where(pos == start, K_SNAN, K_QNAN).astype(np.int16)).to(dev)[:, None, :, None]
        for kc, vc in zip(e.model.kcache, e.model.vcache):
            k = kc[a:b].view(torch.int16)
            k.copy_(torch.where(mask, pat, k))
            vc[a:b].view(torch.int16).masked_fill_(mask, V_NAN)
        return [int((pos >= start).sum())] * len(e.model.kcache)

    def _poison_hist(self, a, b, lo, hi):
        e = self.eng
        if e.d_hist is None:
            return None
        pos = np.arange(e.max_ctx)[None, :]
        keep = (pos >= (lo + self.hist_lo_shift)[:, None]) & (pos < (hi + self.hist_hi_shift)[:, None]) \
            & (hi > lo)[:, None]
        mask = torch.from_numpy(~keep).to(e.device)
        ids = torch.from_numpy(self._ids(a, b)).to(e.device)[:, None]
        h = e.d_hist[a:b]
        h.copy_(torch.where(mask, ids, h))
        return int((~keep).sum())

    def _poison_scratch(self):
        """Every live ``torch.empty`` floating scratch tensor of the current
        stream: the dtype's largest finite value.  Returns the users hit."""
        hit = set()
        if self._G is None:
            return hit
        handle = torch.cuda.current_stream(self.eng.device).cuda_stream
        for (_, _, stream, user), (live, _) in self._G._SCRATCH.items():
            if stream != handle:
                continue
            for i, t in enumerate(live):
                if (user, i) not in self.zeroed and t.is_floating_point() and t.device == self.eng.device:
                    t.fill_(torch.finfo(t.dtype).max)
                    hit.add(user)
        return hit

    def _poison_pins(self, micro: bool):
        e = self.eng
        sid = e.micro_id if micro else e.step_id
        pins = e._pins_m if micro else e._pins
        k = sid % len(pins)
        (e._out_pins_m if micro else e._out_pins)[k].fill_(PIN_ID)
        lp, ids = (e._lp_pins_m if micro else e._lp_pins)[k]
        lp.fill_(float("nan"))
        ids.zero_()
        stop = e._stop_pins_m if micro else e._stop_pins
        if stop is not None:
            stop[k].zero_()              # flag 0: "entry 0 matched"

    def _launch_pool(self, micro: bool):
        e = self.eng
        a, b = (e.slots, e.slots + e.micro_slots) if micro else (0, e.slots)
        act, valid, lo, hi = self._windows(a, b)
        rec = {"n": len(self.launches), "micro": bool(micro), "sid": int(e.micro_id if micro else e.step_id),
               "valid": valid, "lo": lo, "hi": hi, "kv": None, "hist": None, "scratch": set(),
               "hist_exists": e.d_hist is not None}
        if self.classes:
            if not e.cuda:
                ctx = _Null()
            elif micro:
                ctx = torch.cuda.stream(e.rt_stream) if e.rt_stream is not None else _Null()
            else:
                ctx = e.stream_ctx()
            with ctx:
                if "kv" in self.classes:
                    rec["kv"] = self._poison_kv(a, b, act, valid)
                if "hist" in self.classes:
                    rec["hist"] = self._poison_hist(a, b, lo, hi)
                if "scratch" in self.classes:
                    rec["scratch"] = self._poison_scratch()
            if "pins" in self.classes:
                self._poison_pins(micro)
        who = {s: r.req_id for s, r in e.active.items() if a <= s < b}
        # prompts this launch goes on with in the middle: rid -> the position its chunk starts at
        rec["resumed"] = {rid: int(e.s_pref[s]) for s, rid in who.items()
                          if e.active[s].reused < e.s_pref[s] < e.s_plen[s]}
        q = e._qm if micro else e._q
        before = (e.micro_id if micro else e.step_id)
        ran = self._inner(micro)
        if ran:
            f = q[-1]
            assert f.step == before
            rec["n_pre"] = int(f.n_pre)
            live = e.s_active[a:b]
            rec["partial"] = bool((live & (e.s_pref[a:b] > 0) & (e.s_pref[a:b] < e.s_plen[a:b])).any())
            for s, g in zip(f.samp_slots.tolist(), f.gidx.tolist()):
                self.drawn[(who[s], int(g))] = (rec["n"], int(s))
            self.launches.append(rec)
        return ran


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ----------------------------------------------------------------------------- driver
class Run(NamedTuple):
    done: dict                   # rid -> the compared fields of a completed request
    counters: dict
    launches: list
    drawn: dict
    notes: dict                  # what the counter assertions need beyond the counters
    hidden: list                 # per launch the sha256 of the rows handed to the head (``capture_hidden``)
    scratch_used: frozenset = frozenset()      # scratch users the run's forwards called for (HIP)
    scratch_hit: frozenset = frozenset()       # ... of which a tensor was poisoned


def _fields(r, step: int) -> dict:
    d = {k: (None if getattr(r, k) is None else np.ascontiguousarray(getattr(r, k)).tobytes()) for k in FIELDS}
    d.update(finish_reason=r.finish_reason, stop_entry=int(r.stop_entry), generated=int(r.generated),
             reused=int(r.reused), step=step, tokens=None if r.out_tokens is None else r.out_tokens.copy(),
             slot=int(r.slot), micro=bool(r.micro))
    return d


def _engine(scenario, impl, device, micro_stream):
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    if scenario == "serving":
        return BackendEngine(LlamaConfig.tiny(), slots=SLOTS, max_ctx=MAX_CTX, token_budget=24, device=device,
                             impl=impl, max_inflight=2, seed=SEED)
    return BackendEngine(LlamaConfig.tiny(), slots=SLOTS, max_ctx=MAX_CTX, token_budget=32, device=device, impl=impl,
                         seed=SEED, realtime_mode="micro", micro_slots=MICRO_SLOTS, micro_stream=micro_stream)


def run(scenario: str, impl: str = "ref", device: str = "cpu", micro_stream: str = "partition", stops=None,
        classes=(), aim=None, capture_hidden: bool = False, **shifts) -> Run:
    """Serve ``scenario`` once on a fresh engine."""
    saved = None
    if impl == "hip":
        from llm_message_queue_amd.ops import gemm as G
        saved = dict(G.EFFECTIVE_CUS)        # (a CU-partitioned engine shrinks it for every later model)
    eng = _engine(scenario, impl, device, micro_stream)
    poi = Poisoner(eng, classes, aim, **shifts)
    hidden = []
    if scenario == "micro" and eng.cuda:
        # graphs on (the warm-up forwards do not go through ``_launch_pool``: nothing is poisoned under
        # them, and the poisoner sees which scratch users the captured forwards call)
        eng.warm_shapes([1, 8, 32])
        assert eng.micro_graph and eng._mg
    if capture_hidden:
        inner = eng.model.hidden

        def spy(*a, **k):
            h = inner(*a, **k)
            hidden.append(hashlib.sha256(h.detach().float().cpu().numpy().tobytes()).hexdigest())
            return h
        eng.model.hidden = spy
    try:
        return _serve(eng, poi, scenario, stops, hidden)
    finally:
        poi.close()
        eng.close()
        if saved is not None:
            G.EFFECTIVE_CUS.clear()
            G.EFFECTIVE_CUS.update(saved)


def _serve(eng, poi, scenario, stops, hidden) -> Run:
    serving = scenario == "serving"
    pend = _requests(scenario, stops)
    total = len(pend)
    done, notes = {}, {"aborted": {}, "inflight_at_abort": {}, "launches_at_abort": {}}

    def collect(res, it):
        for r in res.completed:
            assert r.req_id not in done
            done[r.req_id] = _fields(r, it)

    for it in range(200):
        if not pend and not eng.active and not eng.queued_steps():
            break
        # a dialog's turn first: its parked KV is what an admission with no free slot evicts
        ready = sorted((x for x in pend if x[0].at <= it and (x[0].after < 0 or x[0].after in done)),
                       key=lambda x: x[0].after < 0)
        if ready:
            got = {id(r) for r in eng.admit([r for _, r in ready])}
            pend = [x for x in pend if id(x[1]) not in got]
        if serving and it == CANCEL_AT:
            notes["inflight_at_abort"]["cancel"] = len(eng._q)
            notes["launches_at_abort"]["cancel"] = len(poi.launches)
            out = eng.cancel([CANCEL_RID])
            notes["aborted"]["cancel"] = [(r.req_id, r.slot) for r in out]
        if serving and it == EXPIRE_AT:
            notes["inflight_at_abort"]["expire"] = len(eng._q)
            notes["launches_at_abort"]["expire"] = len(poi.launches)
            out = eng.expire(now_ns=1 << 62)
            notes["aborted"]["expire"] = [(r.req_id, r.slot) for r in out]
        eng.launch()
        if not serving:
            eng.pump_micro()
            collect(eng.finish(block=True), it)
        elif it % FINISH_EVERY == FINISH_EVERY - 1:
            collect(eng.finish(block=True), it)
    collect(eng.finish(block=True), it)
    assert not pend and not eng.active and not eng.queued_steps()
    assert len(done) == total - (2 if serving else 0), sorted(done)
    hit = set().union(*(L["scratch"] for L in poi.launches)) & poi.used
    return Run(done, {k: int(getattr(eng, k)) for k in COUNTERS}, poi.launches, poi.drawn, notes, hidden,
               frozenset(poi.used), frozenset(hit))


# ----------------------------------------------------------------------------- shared runs
@functools.lru_cache(maxsize=None)
def discovered_stops(scenario: str, impl: str = "ref", device: str = "cpu", micro_stream: str = "partition"):
    """The scenario's stop entries, from a run in which nobody stops."""
    d = run(scenario, impl, device, micro_stream, stops=None)
    return {sp.rid: stop_entries(sp, d.done[sp.rid]["tokens"]) for sp in SCENARIOS[scenario]
            if sp.stop_ids is not None}


@functools.lru_cache(maxsize=None)
def clean(scenario: str, impl: str = "ref", device: str = "cpu", micro_stream: str = "partition",
          which: str = "A") -> Run:
    """Clean run ``which`` ("A", "B": two runs of the same thing), computed
    once and shared by the tests that compare with it."""
    return run(scenario, impl, device, micro_stream, stops=discovered_stops(scenario, impl, device, micro_stream))


def poisoned(scenario: str, impl: str = "ref", device: str = "cpu", micro_stream: str = "partition",
             classes=CLASSES, **shifts) -> Run:
    a = clean(scenario, impl, device, micro_stream)
    return run(scenario, impl, device, micro_stream, stops=discovered_stops(scenario, impl, device, micro_stream),
               classes=classes, aim={rid: d["tokens"] for rid, d in a.done.items()}, **shifts)


# ----------------------------------------------------------------------------- comparison
_COMPARED = FIELDS + ("finish_reason", "stop_entry", "generated", "reused", "step")


def changed(a: Run, b: Run) -> list:
    """The requests whose compared fields differ between two runs."""
    return sorted(rid for rid in set(a.done) | set(b.done)
                  if rid not in a.done or rid not in b.done
                  or any(a.done[rid][k] != b.done[rid][k] for k in _COMPARED))


def describe(a: Run, b: Run) -> str:
    """'' if ``b`` equals ``a`` bit for bit, else the first request and
    generated index that differ, the launch of ``b`` that drew that token,
    its slot and the slot's windows there."""
    bad = changed(a, b)
    cnt = {k: (a.counters[k], b.counters[k]) for k in COUNTERS if a.counters[k] != b.counters[k]}
    if not bad and not cnt:
        return ""
    msg = [f"requests that differ: {bad}; counters (clean, other): {cnt}"]
    for rid in bad[:1]:
        x, y = a.done.get(rid), b.done.get(rid)
        if x is None or y is None:
            msg.append(f"request {rid} completed in only one run")
            break
        msg.append(f"request {rid}: " + ", ".join(f"{k} {x[k]!r} -> {y[k]!r}" for k in _COMPARED[len(FIELDS):]
                                                   if x[k] != y[k]))
        ta, tb = x["tokens"], y["tokens"]
        n = min(len(ta), len(tb))
        diff = np.flatnonzero(ta[:n] != tb[:n])
        gi = int(diff[0]) if len(diff) else n
        msg.append(f"first differing generated index {gi}: clean {ta.tolist()} other {tb.tolist()}")
        if len(diff) == 0 and len(ta) == len(tb):
            which = [k for k in FIELDS if x[k] != y[k]]
            msg.append(f"tokens equal; differing fields {which}")
            gi = 0
        at = b.drawn.get((rid, gi))
        if at is not None:
            n_l, s = at
            L = b.launches[n_l]
            i = s - (SLOTS if L["micro"] else 0)
            msg.append(f"drawn by launch {n_l} ({'micro' if L['micro'] else 'serving'} step {L['sid']}) in slot {s}: "
                       f"valid {int(L['valid'][i])}, history window [{int(L['lo'][i])}, {int(L['hi'][i])})")
    return "\n".join(msg)


def first_hidden_difference(scenario, impl, device, micro_stream="partition") -> str:
    """Two more clean runs with the rows every launch hands to the head
    hashed: the first launch at which they differ (a nondeterministic op in
    the trunk), for the message of a failed precondition."""
    st = discovered_stops(scenario, impl, device, micro_stream)
    x = run(scenario, impl, device, micro_stream, stops=st, capture_hidden=True)
    y = run(scenario, impl, device, micro_stream, stops=st, capture_hidden=True)
    for i, (p, q) in enumerate(zip(x.hidden, y.hidden)):
        if p != q:
            L = x.launches[i] if i < len(x.launches) else {}
            return f"hidden rows first differ at forward {i} (micro: {L.get('micro')}, step {L.get('sid')})"
    return "hidden rows agree in two further runs"


# ----------------------------------------------------------------------------- what the scenario must cover
def check_serving_coverage(a: Run) -> None:
    """The serving scenario still produces every case it is for (clean run)."""
    c, done = a.counters, a.done
    assert any(L["n_pre"] > 0 and L["partial"] for L in a.launches if not L["micro"])
    # the prompt longer than the token budget goes on at a position that is no multiple of 16
    assert any(L["resumed"].get(LONG_RID, 0) % 16 for L in a.launches), [L["resumed"] for L in a.launches]
    assert c["cancelled_total"] == 1 and c["expired_total"] == 1, c
    for what, rid in (("cancel", CANCEL_RID), ("expire", EXPIRE_RID)):
        (got, slot), = a.notes["aborted"][what]
        assert got == rid and a.notes["inflight_at_abort"][what] > 0, a.notes
        assert rid not in done
        # the slot is taken again by a request admitted after the abort
        assert any(d["slot"] == slot and a.drawn[(r, 0)][0] >= a.notes["launches_at_abort"][what]
                   for r, d in done.items()), (what, slot)
    t1, t2, t3, t4 = (done[r] for r in DIALOG)
    assert c["kv_reused_tokens"] > 0 and t1["reused"] == 0 and t2["reused"] > 0 and t3["reused"] > t2["reused"]
    assert t4["reused"] == 0 and t4["slot"] == t3["slot"]          # parked, and restarted: the context is full
    assert t3["out_logprobs"] is not None
    for k in ("sampled_steps", "truncated_steps", "logprob_steps", "penalised_steps", "edited_steps", "stop_steps"):
        assert c[k] > 0, (k, c)
    assert c["stopped_total"] == 2 and c["stop_dropped_rows"] > 0, c
    assert sorted(r for r, d in done.items() if d["finish_reason"] == "stop") == sorted(STOP_RIDS)
    sp = {s.rid: s for s in SERVING}
    for rid in STOP_RIDS:
        assert done[rid]["generated"] < sp[rid].gen and done[rid]["stop_entry"] == 0


def check_micro_coverage(a: Run, graphs: bool) -> None:
    c, done = a.counters, a.done
    assert c["micro_steps"] > 0 and any(not L["micro"] for L in a.launches), c
    if graphs:
        assert c["micro_graph_steps"] > 0, c
    m = done[MICRO_STOP_RID]
    assert m["micro"] and m["finish_reason"] == "stop" and m["out_logprobs"] is not None, m
    assert c["stopped_total"] == 1 and c["penalised_steps"] > 0 and c["logprob_steps"] > 0, c
    assert sum(d["micro"] for d in done.values()) >= 5             # the micro slots are taken again
    assert sum(not d["micro"] for d in done.values()) >= 5         # the serving-pool crowd
    assert any(L["n_pre"] > 0 and L["partial"] for L in a.launches if not L["micro"])


def check_poison_counts(p: Run, classes) -> None:
    """Every launch of the poisoned run wrote what it was meant to."""
    assert p.launches
    seen = False
    for L in p.launches:
        if "kv" in classes:
            assert L["kv"] and all(n >= 1 for n in L["kv"]), L
        if "hist" in classes:
            assert (L["hist"] is not None) == L["hist_exists"], L
            assert not L["hist_exists"] or L["hist"] >= 1, L
            seen |= L["hist_exists"]
    assert seen or "hist" not in classes
