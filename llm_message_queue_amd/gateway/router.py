"""The gateway data path: ingress micro-batcher -> GPU preprocess -> native
4-tier queue -> dispatcher -> GPU backends (one per process/GPU).

This is what the reference's monolith was meant to do but does not (its
level queues are never created and its workers never started, SURVEY.md D1,
D2): ``POST /api/v1/messages`` -> ``Preprocessor.ProcessMessage`` ->
``QueueManager.PushMessage`` (`api/handlers.go:160-219`) -> ``Worker`` tick ->
``LoadBalancer.GetEndpoint`` (`worker.go:109-188`, `load_balancer.go:234`).

MI355X design:
  * ingress is micro-batched per tick; the whole batch is preprocessed by one
    fused HIP launch chain (text_analyze + MFMA classifier);
  * the queue is the C++ bucket queue with per-level locks; the dispatcher pops
    with strict priority + aging + per-tier in-flight caps (``pop_tiers``);
  * dispatch is slot-bounded: a request is dispatched when a backend batch
    slot is free for it (no unbounded backend-side queue), so
    enqueue->dispatch latency is the honest gateway metric;
  * with >1 GPU, each process is router + backend; per tick the ranks
    all_gather their load vectors over the node-local shared-memory control
    plane (``parallel.comm.ShmComm``; KV migration rides the RCCL data group),
    compute the same plan
    (``parallel.planner``), and move request descriptors / completion records
    with one all_to_all (``parallel.comm``).
"""
from __future__ import annotations

import collections
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..backend.engine import BackendEngine, Request
from ..models.message import (PENALTY_KEYS, STOP_KEYS, Message, MessageStatus, SamplingParseError, allowed_from_metadata,
                              finish_record, generation_record, logit_bias_from_metadata, logprobs_from_metadata,
                              max_tokens_from_metadata, min_p_from_metadata, min_tokens_from_metadata,
                              penalty_from_metadata, stop_entries, stop_sequences_from_metadata,
                              stop_token_ids_from_metadata,
                              priority_name, sampling_from_metadata, truncation_from_metadata)
from ..parallel import planner
from ..parallel.comm import Comm, SoloComm
from ..queue.core import QueueError
from ..queue.manager import QueueManager, QueueManagerConfig
from ..utils.logging import get_logger

NS = 1_000_000_000

from .descriptors import (DESC_HDR, FAIL_UNTOUCHED, GEN_MASK, K_CANCEL, K_CANCELLED, K_DISPATCH, K_DONE,  # noqa: F401
                          K_FAIL, K_MIGRATE, K_TIMEOUT, KV_MIGRATE, _get64, _put64, conv_key, pack_finish)
from .latency import (PATHS, P_LANE, P_OWN, P_PLAN_LOCAL, P_PLAN_REMOTE, STAGES, LatencyRecorder,  # noqa: F401
                      StageRecorder, _hbin, hist_percentile)
from .gateway_admission import OwnAdmissionMixin
from .gateway_affinity import AffinityMixin
from .gateway_exchange import ExchangeMixin
from .gateway_failure import FailureMixin
from .gateway_resources import ResourceMixin
from .request_table import INBOX, NONE, PREPROCESS, QUEUED, RequestTable


class Gateway(ExchangeMixin, FailureMixin, AffinityMixin, ResourceMixin, OwnAdmissionMixin):
    """One rank's router + backend driver.  Split by concern (VERDICT r4
    weak #9): this class holds the tick (ingest -> launch -> reap -> dispatch)
    and local dispatch; ``gateway_exchange`` the multi-rank load exchange,
    plan and descriptor all_to_all; ``gateway_failure`` the shedding / timeout /
    cancel / retry / health paths, ``gateway_affinity`` conversation homes,
    pins and KV migration, ``gateway_resources`` the balancer / HBM /
    ResourceScheduler view, ``gateway_admission`` own-GPU admission between
    collectives.

    Thread ownership.  The serve loop (``tick``, under ``_tick_lock``) owns
    every field.  Other threads enter through a handful of methods only:
      * ``submit`` (ring / HTTP ingest threads) -> ``_inbox`` under ``_inbox_lock``;
      * ``request_cancel`` (API / peer threads) -> ``_cancel_req`` under ``_cancel_lock``;
      * ``_retry_ready`` (the DelayedQueue thread) -> ``_retry_due`` under ``_retry_lock``;
      * ``set_healthy`` (telemetry / API) takes ``_tick_lock``, i.e. waits for the tick;
      * ``_pin(m, -1)`` via ``qm.on_remove`` (API / peer deletes) -> ``_pin_lock``;
      * read-only counters / stats (``counters``, ``pending``, histograms)."""
    def __init__(self, cfg, *, preprocessor=None, engine: Optional[BackendEngine] = None,
                 comm: Optional[Comm] = None, load_balancer=None, metrics=None, state_manager=None,
                 use_gpu_preprocess: Optional[bool] = None, prompt_cap: Optional[int] = None,
                 gen_tokens: Optional[int] = None, name: str = "gateway",
                 queue_manager: Optional[QueueManager] = None, dead_letter=None):
        from ..preprocess.preprocessor import Preprocessor
        self.cfg = cfg
        self.log = get_logger("gateway")
        self.comm = comm or SoloComm()
        self.rank, self.world = self.comm.rank, self.comm.world
        if self.world > planner.MAX_WORLD:
            raise ValueError(f"world size {self.world} > {planner.MAX_WORLD}")
        self.pre = preprocessor or Preprocessor(cfg.preprocessor)
        self.use_gpu_pre = use_gpu_preprocess
        self.engine = engine
        self.lb = load_balancer
        self.state_manager = state_manager
        self.prompt_cap = int(prompt_cap if prompt_cap is not None else cfg.backend.prompt_tokens)
        self.gen_tokens = int(gen_tokens if gen_tokens is not None else cfg.backend.gen_tokens)
        if not 0 <= self.gen_tokens <= GEN_MASK:      # (col 9 of a dispatch row carries min_p above it)
            raise ValueError(f"gen_tokens {self.gen_tokens} exceeds the dispatch row's {GEN_MASK}")
        q = cfg.queue
        self.qm = queue_manager or QueueManager(QueueManagerConfig(
            default_max_size=q.default_max_size, monitor_interval=q.monitor_interval,
            cleanup_interval=q.cleanup_interval, max_retention_period=q.max_retention_period,
            enable_metrics=q.enable_metrics and metrics is not None, enable_auto_scaling=q.enable_auto_scaling,
            scaling_thresholds=dict(q.scaling_thresholds)), name=name, metrics=metrics)
        levels = sorted(q.levels, key=lambda lv: lv.priority)
        self.tiers = [lv.name for lv in levels]
        self.tier_prio = [lv.priority for lv in levels]
        self.tier_of_queue = {n: i for i, n in enumerate(self.tiers)}
        self.aging_ns = [lv.max_wait_time if q.enable_aging else 0 for lv in levels]
        la = int(getattr(q, "lifo_after", 0))
        self.lifo_ns = ([la if la > 0 else int(lv.max_wait_time) for lv in levels]
                        if getattr(q, "adaptive_lifo", False) else None)
        self.max_conc = self._tier_caps([lv.max_concurrent for lv in levels],
                                        bool(getattr(q, "priority_monotone_caps", True)))
        for n in self.tiers:                          # D1: the level queues exist
            self.qm.create_queue(n)
        # every request's lifecycle state and the in-flight maps (one owner:
        # gateway.request_table)
        self.table = RequestTable()
        # a queued message removed other than by dispatch (admin delete,
        # peer dequeue, retention cleanup) releases its (home GPU, tier) pin
        # and leaves the lifecycle
        self.qm.on_remove.append(self._queue_removed)
        self.metrics = metrics
        self._inbox: List[Message] = []
        self._inbox_lock = threading.Lock()
        self._pre_pending = None        # outstanding asynchronous preprocess batch (ingest_async)
        self.inflight_by_tier = np.zeros(len(self.tiers), dtype=np.int64)
        # queued requests per (home GPU, tier): KV-residency pins (planner L_PIN)
        self.pinned = np.zeros((self.world, planner.NTIERS), dtype=np.int64)
        self._away: set = set()        # handles of queued turns pinned to another GPU
        self._pin_lock = threading.Lock()
        # multi-GPU placement follows loadbalancer.algorithm (planner.PlanState;
        # identical on every rank, advanced identically by every plan)
        self.plan_state = planner.PlanState(strategy=str(getattr(cfg.loadbalancer, "algorithm", "")))
        self.resources = None          # optional ResourceScheduler: per-GPU usage from the load exchange
        self._parked_eps: Dict[str, object] = {}   # GPU endpoints the resource scheduler parked
        self._res_next_ns = 0
        # ResourceScheduler cadence: heartbeats / loads / backlog from the
        # tick's load vectors at most this often (gpu.rebalance_interval_ms)
        self.res_interval_ns = int(max(1, getattr(cfg.gpu, "rebalance_interval_ms", 100)) * 1_000_000)
        self.hbm_fn = None             # optional () -> (used MiB, total MiB) of this rank's GPU
        self._hbm_cache = (0, 0, 0)    # (used, total, refreshed at ns)
        self._rt_ewma_us = 0.0         # service time (admit -> done) EWMA of this GPU
        self._err_ewma = 0.0           # backend error EWMA of this GPU
        self.epoch = 0                 # KV migrations completed by this rank
        self.loads = None              # last all-gathered load matrix
        # KV migration (N11): a turn placed away from its (alive) home GPU
        # moves the dialog's KV there instead of replaying the dialog
        self.kv_migrate = bool(getattr(cfg.gpu, "kv_migration", True))
        # conversation affinity in multi-GPU placement (pins); off = every
        # turn is placed by the strategy alone.  ``rehome_every_turn``
        # (bench/migrate_bench.py): a turn goes to any GPU but its home --
        # the worst case of rebalancing, for measuring migration vs replay
        self.affinity = True
        self.rehome_every_turn = False
        # orders (conv, home, dest) decided this tick; their K_MIGRATE rows go
        # to the home GPUs in the next tick's all_to_all (counts announced in
        # that tick's load vector), when home and dest both execute them
        self._mig_out: List[Tuple[int, int, int]] = []
        self._await_kv: Dict[int, List[Tuple[Request, int]]] = {}   # conv -> [(held turn, home GPU)]
        # held turns whose KV transfer is in flight on the device (RCCL)
        self._await_import: Dict[int, List[Tuple[Request, int]]] = {}
        self.migrator = None
        if self.world > 1 and engine is not None and self.kv_migrate and hasattr(engine, "model"):
            from ..parallel.migration import KVMigrator
            self.migrator = KVMigrator(engine.model, self.comm)
            self.comm.warm_data_plane()
        self.local: Dict[int, Message] = self.table.local        # handle -> msg dispatched to my engine
        self.remote_out: Dict[int, Message] = self.table.remote_out  # handle -> msg sent to another rank
        self.foreign: Dict[int, Tuple[int, int, int]] = {}  # my engine req id -> (origin, handle, tier)
        self._done_owed: Dict[int, List[Tuple[int, int, int, int]]] = {r: [] for r in range(self.world)}
        self._done_pub: List[int] = [0] * self.world      # records of _done_owed announced this tick
        # generated ids of the dialog turns, and of the requests that named a stop key, in _done_owed
        # (origin -> handle -> (ids, the K_DONE row's finish column))
        self._done_tok: Dict[int, Dict[int, tuple]] = {r: {} for r in range(self.world)}
        # log-probability streams of the K_LOGP rows in _done_owed (origin -> handle -> int32 stream),
        # and the chunks received for my own requests ((source, handle) -> stream so far)
        self._done_lp: Dict[int, Dict[int, np.ndarray]] = {r: {} for r in range(self.world)}
        self._lp_parts: Dict[Tuple[int, int], np.ndarray] = {}
        # dialog histories owed to the GPUs this router dispatched turns to
        # (sent one tick later as K_HIST rows, counted in that tick's load vector)
        # entries: (handle, prefix, history, extension words)
        self._hist_out: Dict[int, List[Tuple[int, np.ndarray, np.ndarray, np.ndarray]]] = {}
        self._hist_pub: Dict[int, List[Tuple[int, np.ndarray, np.ndarray, np.ndarray]]] = {}
        # foreign turns that must replay their dialog, waiting for its history: (origin, handle) -> Request
        self._await_hist: Dict[Tuple[int, int], Request] = {}
        # every foreign turn a K_HIST is still expected for (also KV-held ones) and the lengths seen
        self._hist_wait: Dict[Tuple[int, int], Request] = {}
        self._hist_len: Dict[Tuple[int, int], Tuple[int, int]] = {}
        self.rec = LatencyRecorder(len(self.tiers))
        self.rec_stage = StageRecorder(len(self.tiers))
        self.counters = {"submitted": 0, "rejected": 0, "dispatched": 0, "completed": 0, "ticks": 0,
                         "remote_sent": 0, "remote_recv": 0, "evacuated": 0, "handed_back": 0, "expired": 0,
                         "overcommit": 0, "kv_migrated": 0, "kv_migrate_replays": 0, "realtime_local": 0,
                         "extra_steps": 0, "extra_admitted": 0, "retried": 0, "retry_exhausted": 0,
                         "inflight_timeout": 0, "cancelled": 0, "dialog_ids_real": 0, "dialog_ids_placeholder": 0,
                         "hist_tokens_sent": 0, "hist_tokens_recv": 0}
        # In-flight processing timeout: the reference runs every message under
        # context.WithTimeout(msg.Timeout) and retries / dead-letters it on
        # expiry (`internal/priorityqueue/worker.go:162-188, 202-239`).  Here a
        # request's attempt gets ``Message.timeout`` (30 s default, D16) from
        # its admission into a GPU slot; the engine aborts it past that (slot
        # freed for the next admission) and it takes the retry path.
        # ``queue.inflight_timeout`` off: admitted requests always run out.
        self.inflight_timeout = bool(getattr(q, "inflight_timeout", True))
        self._expire_next_ns = 0
        # cancellation of a request in flight (DELETE /api/v1/messages/{id}):
        # API / peer threads queue (message, Future); the serve loop aborts it
        # on its own GPU or sends K_CANCEL to the GPU running it
        self._cancel_lock = threading.Lock()
        self._cancel_req: List[Tuple[Message, object]] = []
        self._cancel_out: Dict[int, List[int]] = {}     # dest GPU -> handles to abort there
        self._cancel_pub: Dict[int, List[int]] = {}     # ... announced in this tick's load vector
        # overload shedding (expire_queued) -> dead-letter queue
        self.shed_expired = bool(getattr(q, "shed_expired", True))
        # realtime lane (tier 0 admitted past the step's prefill headroom and
        # prefilled first): queue.realtime_lane, default on
        self.realtime_lane = bool(getattr(q, "realtime_lane", True))
        self.extra_steps = bool(getattr(cfg.gpu, "extra_steps", True))
        self.dead_letter = dead_letter
        self.on_expire = None       # optional callback(msg)
        # Retry policy for requests a backend failure handed back (evacuation,
        # K_FAIL): with a DelayedQueue attached (``attach_retry_queue``) they
        # wait out an exponential backoff (queue.retry) before re-entering
        # their tier, and go to the dead-letter queue once retries are
        # exhausted -- the reference's intended retry path (`worker.go:202-239`,
        # SURVEY D15), here on the GPU gateway.  Without one they re-enter
        # their tier at once (the round-3 behaviour).
        self.retry_queue = None
        self.retry_backoff = None
        self._retry_due: List[Message] = []
        self._retry_lock = threading.Lock()
        # failure detection: a backend error (HIP error / OOM), the telemetry
        # poller (ECC, amd-smi gone) or an operator marks this GPU unhealthy;
        # it then takes no new work, its in-flight requests are re-routed and
        # conversations homed on it are re-homed wherever they land next
        self.healthy = True
        self.health_reason = ""
        # coordinated shutdown: a stopping rank flags it in its load vector and
        # every rank leaves its serve loop after the same tick (each tick is a
        # collective, so ranks must stop together)
        self.stopping = False
        self.peers_stopping = False
        self.cluster_idle = False     # every rank idle at the last load exchange
        self._tick_lock = threading.RLock()     # set_healthy from a telemetry thread waits for the tick
        self.unhealthy_peers: set = set()
        self.excluded_peers: set = set()    # parked / operator-excluded GPUs (balancer view)
        self._gpu_eps_seen: set = set()     # GPU endpoints this rank's balancer has registered
        self.on_complete = None     # optional callback(msg)
        self.tracer = None          # optional utils.tracing.RequestTracer
        self.rec_done = LatencyRecorder(len(self.tiers))   # arrival -> completion (end to end)
        # conversation KV residency: turns of a dialog go to the GPU that holds
        # its KV (conv_home) and prefill only their new tokens there
        import collections
        self.kv_residency = True
        self.conv_home: "collections.OrderedDict[str, int]" = collections.OrderedDict()
        self.conv_hist: "collections.OrderedDict[str, np.ndarray]" = collections.OrderedDict()
        self.max_dialogs = 200_000
        self.history_cap = int(getattr(cfg.backend, "max_ctx", 512))
        self._done_buf: List[Tuple[int, int, int]] = []
        self._last_ingest_ns = 0
        self.host_ns = np.zeros(5, dtype=np.int64)   # per-phase host time (host_profile)
        self.ingest_ns = np.zeros(3, dtype=np.int64)  # [preprocess ns, queue push ns, messages]
        self._ticks0 = 0
        self._next_req = 1 << 40
        # lock-step attribution: host time each multi-rank tick spends inside
        # its control-plane collectives (load all_gather + descriptor
        # all_to_all) -- the wait for the slowest rank plus the exchange
        self.coll_wait_ns: "collections.deque[int]" = collections.deque(maxlen=1 << 16)
        self._pump = None               # the current tick's arrival feed (collective overlap loops)
        # Own-arrival reservation (multi-rank): each tick a router holds back,
        # from the capacity it publishes, what its own arrivals are expected
        # to need until the plan is applied -- the EWMA of its enqueues during
        # a tick's collective waits (all tiers -> prefill headroom; tier 0 x 2
        # -> lane slots).  It
        # admits arrivals into that reserve while it waits at the collectives,
        # so the plan, which only sees what was queued when the loads were
        # published, never stalls fresh local arrivals for a whole tick.
        self._enq_tick = [0, 0]         # enqueued during this tick's collective waits (all, tier 0)
        self._enq_ewma = [0.0, 0.0]
        self._in_wait = False
        self._reserve = [0, 0]          # [headroom admits, lane slots] left this tick
        # per-tier depth this rank published and not yet popped its grant of:
        # own admissions in the wait must leave at least that much queued
        self._pub_depth: Optional[List[int]] = None
        self.own_reserve = True
        # Holding back prefill HEADROOM as well (all tiers) was measured worse:
        # a faster GPU's unused reserve is lost to the plan that tick, so a
        # slower GPU's backlog (its low tier) waits for aging instead of
        # moving (profiles/r4_sim8_own_admission.jsonl).  Lane slots (tier 0)
        # are plentiful, so holding them back costs the plan nothing.
        self.reserve_headroom = False

    # ------------------------------------------------------------------ ingress
    def submit(self, msgs: Sequence[Message]) -> None:
        now = time.monotonic_ns()
        for m in msgs:
            m.recv_ns = now
            m.lc = INBOX                    # (not visible to any other thread before the inbox)
            if not m.arrival_ns:
                m.arrival_ns = now
        with self._inbox_lock:
            self._inbox.extend(msgs)
        self.counters["submitted"] += len(msgs)

    def ingest(self) -> List[Tuple[Message, Optional[QueueError]]]:
        """Synchronous ingest: finish any outstanding preprocess batch, then
        preprocess + enqueue everything in the inbox."""
        out = self._finish_pending(block=True)
        batch = self._take_inbox()
        if not batch:
            return out
        t0 = time.perf_counter_ns()
        g0 = self.pre.stats.get("gpu_batches", 0)
        self.pre.process_batch(batch, use_gpu=self.use_gpu_pre, prompt_cap=self.prompt_cap)
        dt = time.perf_counter_ns() - t0
        self.ingest_ns[0] += dt
        self._observe_preprocess(g0, dt, "sync_batch")
        return out + self._enqueue(batch)

    def _observe_preprocess(self, gpu_batches_before: int, host_ns: int, stage: str) -> None:
        """llm_preprocess_kernel_seconds{stage}: ``gpu_batch`` = a GPU batch
        from launch to its results on the host; ``stage`` = the host time of
        the call (a whole synchronous batch, or the decode of a finished one)."""
        if self.metrics is None:
            return
        ps = self.metrics.preprocess_seconds
        if self.pre.stats.get("gpu_batches", 0) != gpu_batches_before:
            ps.labels("gpu_batch").observe(self.pre.stats["last_gpu_ms"] / 1e3)
        ps.labels(stage).observe(host_ns / 1e9)

    def ingest_async(self) -> bool:
        """Overlapped ingest (GPU preprocess only): enqueue the outstanding
        batch if its kernels finished, and launch the inbox as the next batch
        without waiting for it.  The preprocess chain queues behind the
        forward's GEMMs for CUs; the host keeps ingesting and dispatching
        meanwhile.  True if anything was done."""
        if not self.use_gpu_pre:
            return bool(self.ingest())
        did = False
        if self._pre_pending is not None:
            if not self.pre.batch_ready(self._pre_pending):
                return False
            did = bool(self._finish_pending(block=True))
        batch = self._take_inbox()
        if batch:
            t0 = time.perf_counter_ns()
            self._pre_pending = self.pre.begin_batch(batch, prompt_cap=self.prompt_cap)
            self.ingest_ns[0] += time.perf_counter_ns() - t0
            did = True
        return did

    # Largest preprocess batch per ingest.  Under an ingest overload the inbox
    # grows faster than it drains; taking all of it at once makes each tick
    # (and with it every dispatch round) as long as the backlog, so served
    # throughput collapsed as the offered rate rose (null backend: 130k/s
    # served at 130k offered, 24k at 200k).  Bounded batches keep ticks short
    # and throughput at capacity; the rest waits in the inbox, oldest first.
    MAX_INGEST_BATCH = 8192

    def _take_inbox(self) -> list:
        with self._inbox_lock:
            if len(self._inbox) <= self.MAX_INGEST_BATCH:
                batch, self._inbox = self._inbox, []
            else:
                batch = self._inbox[:self.MAX_INGEST_BATCH]
                del self._inbox[:self.MAX_INGEST_BATCH]
        now = time.monotonic_ns()
        for m in batch:
            m.ingest_ns = now
        self.table.move_many(batch, PREPROCESS)
        return batch

    def preprocessing(self) -> int:
        """Messages inside an outstanding preprocess batch."""
        return len(self._pre_pending["msgs"]) if self._pre_pending is not None else 0

    def _finish_pending(self, block: bool) -> List[Tuple[Message, Optional[QueueError]]]:
        tok = self._pre_pending
        if tok is None or (not block and not self.pre.batch_ready(tok)):
            return []
        self._pre_pending = None
        t0 = time.perf_counter_ns()
        g0 = self.pre.stats.get("gpu_batches", 0)
        self.pre.end_batch(tok)
        dt = time.perf_counter_ns() - t0
        self.ingest_ns[0] += dt
        self._observe_preprocess(g0, dt, "host_finish")
        return self._enqueue(tok["msgs"])

    def _enqueue(self, batch) -> List[Tuple[Message, Optional[QueueError]]]:
        t1 = time.perf_counter_ns()
        batch, dead, _ = self.table.split_cancelled(batch)
        for m in dead:                      # cancelled while being preprocessed: never queued
            self._finish_cancel(m)
        for m in batch:
            if not m.queue_name:
                m.queue_name = priority_name(m.priority)
        self.table.move_many(batch, QUEUED)
        errs = self.qm.push_routed(batch)
        self.ingest_ns[1] += time.perf_counter_ns() - t1
        self.ingest_ns[2] += len(batch)
        out = []
        t0name = self.tiers[0] if self.tiers else None
        wait = self._in_wait
        for m, e in zip(batch, errs):
            if e is None and wait:                # enqueued while waiting at a collective
                self._enq_tick[0] += 1
                if m.queue_name == t0name:
                    self._enq_tick[1] += 1
            if e is None and self.world > 1:
                self._pin(m, +1)
            if e is not None:
                m.status = MessageStatus.FAILED
                self.table.move(m, NONE)
                self.counters["rejected"] += 1
                if self.metrics:
                    self.metrics.requests_rejected.labels(e.code).inc()
            out.append((m, e))
        return out

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _tier_caps(caps: List[int], monotone: bool) -> List[int]:
        """In-flight cap per tier (most urgent first; <= 0 = no cap).
        ``monotone``: a tier's cap is at least every less urgent tier's, so a
        cap can never make an urgent request wait while a less urgent one is
        admitted (``queue.priority_monotone_caps``)."""
        if not monotone:
            return list(caps)
        out, run = [], 0
        for c in reversed(caps):                      # least urgent first
            run = -1 if (c <= 0 or run < 0) else max(run, c)
            out.append(run)
        return out[::-1]

    def _budgets(self) -> List[int]:
        return [(-1 if c <= 0 else max(0, int(c - self.inflight_by_tier[i])))
                for i, c in enumerate(self.max_conc)]

    def _queue_state(self):
        depth, age = [], []
        now = time.monotonic_ns()
        for n in self.tiers:
            depth.append(self.qm.size(n))
            try:
                head = self.qm.peek_message(n)
                age.append(max(0, (now - head.enqueued_at) // 1000))
            except QueueError:
                age.append(0)
        b = self._budgets()
        depth = [d if bb < 0 else min(d, bb) for d, bb in zip(depth, b)]
        return depth, age

    def _make_request(self, m: Message, tier: int) -> Request:
        prompt = m.prompt_ids if m.prompt_ids is not None else np.zeros(1, dtype=np.uint32)
        p = np.asarray(prompt, dtype=np.uint32).astype(np.int64).astype(np.int32) \
            if len(prompt) else np.zeros(1, dtype=np.int32)
        ck = conv_key(m.conversation_id) if self.kv_residency else -1
        hist, pre = self._dialog_context(m)
        temp, seed, top_k, top_p, logprobs, pens, (min_p, bias, allowed), (max_tokens, min_tokens, stops, finish) = \
            self._sampling(m, self.gen_tokens)
        return Request(req_id=m.handle, prompt=p, gen_tokens=max_tokens or self.gen_tokens, tier=tier, meta=m, conv=ck,
                       min_tokens=min_tokens, stop=stops or None, finish=finish,
                       history=hist, prefix=pre, timeout_ns=self._timeout_ns(m), temperature=temp, seed=seed,
                       top_k=top_k, top_p=top_p, logprobs=logprobs, presence_penalty=pens[0],
                       frequency_penalty=pens[1], repetition_penalty=pens[2], min_p=min_p,
                       logit_bias=bias if len(bias[0]) else None, allowed=allowed if len(allowed) else None)

    _NO_STOP = (0, 0, [], False)
    _NO_ELIGIBILITY = (0.0, (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)), np.zeros(0, dtype=np.int32))

    @staticmethod
    def _sampling(m: Message, gen_tokens: int = 0) -> tuple:
        """The message's effective ``(temperature, seed, top_k, top_p,
        logprobs, (presence, frequency, repetition penalty), (min_p,
        (logit_bias ids, values), allowed_token_ids), (max_tokens, min_tokens,
        stop entries, finish))``
        (``metadata.sampling``), lenient: this path also serves
        messages no route validated (the native ingress), so a bad
        temperature or seed falls back to greedy, a bad ``top_k`` / ``top_p``
        turns the truncation off, a bad ``logprobs`` turns the
        log-probabilities off (-1), a bad penalty turns that penalty off, a
        bad ``min_p`` / ``logit_bias`` / ``allowed_token_ids`` turns that key
        off, and each is reported in
        ``metadata["sampling_error"]``.  A message that asked for sampling
        gets the effective values written back, so a client can replay it:
        ``top_k`` / ``top_p`` only where they are active (with a temperature,
        and not off; ``min_p`` likewise), a penalty only where it is not
        off (greedy or not), ``logit_bias`` (its non-zero entries) and
        ``allowed_token_ids`` only where they are in effect (greedy or not),
        and ``logprobs`` only where the message named it, so a
        message that named none of them keeps exactly ``{"temperature",
        "seed"}``.  The stop keys (``models.message.stop_from_metadata``;
        ``gen_tokens`` is the configured count, the cap of ``max_tokens``):
        a bad ``max_tokens``, ``min_tokens``, ``stop_token_ids`` or
        ``stop_sequences`` turns that key off and leaves the others in effect
        (the two lists both, where only their total is too long); ``max_tokens`` is 0 where the configured count holds.
        Written back: ``max_tokens`` where named, ``min_tokens`` where above
        0, the lists where not empty.  ``finish``: one of them is in effect,
        so the message gets a ``finish_reason``."""
        md = m.metadata
        if not md or "sampling" not in md:
            # greedy (the default traffic): the seed is never read
            return 0.0, 0, 0, 1.0, -1, (0.0, 0.0, 1.0), Gateway._NO_ELIGIBILITY, Gateway._NO_STOP
        try:
            temp, seed = sampling_from_metadata(md, m.id)
        except SamplingParseError as e:
            md["sampling_error"] = str(e)
            temp, seed = 0.0, sampling_from_metadata(None, m.id)[1]
        try:
            top_k, top_p = truncation_from_metadata(md)
        except SamplingParseError as e:
            md["sampling_error"] = "; ".join(x for x in (md.get("sampling_error"), str(e)) if x)
            top_k, top_p = 0, 1.0
        try:
            logprobs = logprobs_from_metadata(md)
        except SamplingParseError as e:
            md["sampling_error"] = "; ".join(x for x in (md.get("sampling_error"), str(e)) if x)
            logprobs = -1
        pens = []
        for key, (_lo, _hi, off) in PENALTY_KEYS.items():
            try:
                pens.append(penalty_from_metadata(md, key))
            except SamplingParseError as e:
                md["sampling_error"] = "; ".join(x for x in (md.get("sampling_error"), str(e)) if x)
                pens.append(off)
        elig = []
        for parse, off in zip((min_p_from_metadata, logit_bias_from_metadata, allowed_from_metadata),
                              Gateway._NO_ELIGIBILITY):
            try:
                elig.append(parse(md))
            except SamplingParseError as e:
                md["sampling_error"] = "; ".join(x for x in (md.get("sampling_error"), str(e)) if x)
                elig.append(off)
        min_p, bias, allowed = elig
        if temp <= 0:
            top_k, top_p, min_p = 0, 1.0, 0.0     # (accepted, without effect)
        eff = {"temperature": temp, "seed": seed}
        if top_k > 0:
            eff["top_k"] = top_k
        if top_p < 1.0:
            eff["top_p"] = top_p
        if logprobs >= 0:
            eff["logprobs"] = logprobs
        for (key, (_lo, _hi, off)), v in zip(PENALTY_KEYS.items(), pens):
            if v != off:
                eff[key] = v
        if min_p > 0:
            eff["min_p"] = min_p
        if len(bias[0]):
            eff["logit_bias"] = {str(int(t)): float(v) for t, v in zip(*bias)}
        if len(allowed):
            eff["allowed_token_ids"] = [int(t) for t in allowed]
        stop = Gateway._NO_STOP
        sp = md["sampling"]
        if isinstance(sp, dict) and any(k in sp for k in STOP_KEYS):
            def lenient(parse, off):
                try:
                    return parse()
                except SamplingParseError as e:
                    md["sampling_error"] = "; ".join(x for x in (md.get("sampling_error"), str(e)) if x)
                    return off

            mx = lenient(lambda: max_tokens_from_metadata(md, gen_tokens), 0)
            # each list on its own: a bad one leaves the other in effect; both off where only their total is too long
            st = lenient(lambda: stop_token_ids_from_metadata(md), [])
            sq = lenient(lambda: stop_sequences_from_metadata(md), [])
            ent = lenient(lambda: stop_entries(st, sq), [])
            mn = lenient(lambda: min_tokens_from_metadata(md, mx or gen_tokens), 0)   # (against the effective max_tokens)
            n_tok = len(st) if ent else 0
            if mx > 0:
                eff["max_tokens"] = mx
            if mn > 0:
                eff["min_tokens"] = mn
            if n_tok:
                eff["stop_token_ids"] = [int(e[0]) for e in ent[:n_tok]]
            if len(ent) > n_tok:
                eff["stop_sequences"] = [[int(t) for t in e] for e in ent[n_tok:]]
            stop = (mx, mn, ent, bool(mx > 0 or mn > 0 or ent))
        md["sampling"] = eff
        return temp, seed, top_k, top_p, logprobs, tuple(pens), (min_p, bias, allowed), stop

    @staticmethod
    def _attach_finish(m: Message, tokens, finish_reason: str, stop_entry: int) -> None:
        """``finish_reason`` (and ``stop_reason``, the matched entry: an int
        for a stop token, a list for a sequence) into ``metadata.generation``
        of a message that named a stop key, next to the log-probability
        fields where the message asked for those too (cut to the same
        length), else with the generated tokens alone."""
        if tokens is None or not finish_reason or not isinstance(m.metadata, dict):
            return
        sp = m.metadata.get("sampling")
        reason = None
        if finish_reason == "stop" and isinstance(sp, dict) and stop_entry >= 0:
            st, sq = sp.get("stop_token_ids") or [], sp.get("stop_sequences") or []
            reason = st[stop_entry] if stop_entry < len(st) else \
                (list(sq[stop_entry - len(st)]) if stop_entry - len(st) < len(sq) else None)
        rec = finish_record(tokens, finish_reason, reason)
        gen = m.metadata.get("generation")
        if isinstance(gen, dict) and "token_logprobs" in gen:
            n = len(rec["tokens"])
            for k in ("tokens", "token_logprobs", "top_logprobs"):
                if k in gen:
                    gen[k] = gen[k][:n]
            gen.update({k: v for k, v in rec.items() if k != "tokens"})
        else:
            m.metadata["generation"] = rec

    @staticmethod
    def _attach_generation(m: Message, tokens, lp, top_ids, top_lp) -> None:
        """``metadata.generation`` of a message that asked for
        log-probabilities, from its last attempt's results, trimmed to its
        own ``n`` (nothing for a message that did not ask, or an engine that
        ran no model)."""
        sp = m.metadata.get("sampling") if isinstance(m.metadata, dict) else None
        n = sp.get("logprobs") if isinstance(sp, dict) else None
        if tokens is None or lp is None or isinstance(n, bool) or not isinstance(n, int) or n < 0:
            return
        k = min(len(tokens), len(lp))
        m.metadata["generation"] = generation_record(tokens[:k], lp[:k], top_ids[:k], top_lp[:k], n)

    def _timeout_ns(self, m: Message) -> int:
        return int(m.timeout) if (self.inflight_timeout and m.timeout and m.timeout > 0) else 0

    def _popped(self, msgs: Sequence[Message], tier_idx) -> None:
        """A dispatch decision took ``msgs`` out of their queues: stamp it and
        record the stages before it (inbox, preprocess, queue wait)."""
        if not len(msgs):
            return
        now = time.monotonic_ns()
        n = len(msgs)
        a = np.empty((4, n), dtype=np.int64)
        for k, m in enumerate(msgs):
            m.popped_ns = now
            a[0, k] = m.arrival_ns or m.recv_ns or m.ingest_ns or m.enqueued_at
            a[1, k] = m.recv_ns or a[0, k]
            a[2, k] = m.ingest_ns or a[1, k]
            a[3, k] = m.enqueued_at or a[2, k]
        t = np.asarray(tier_idx, dtype=np.int64)[:n]
        rs = self.rec_stage
        rs.record(0, t, a[1] - a[0])
        rs.record(1, t, a[2] - a[1])
        rs.record(2, t, a[3] - a[2])
        rs.record(3, t, now - a[3])

    def _record(self, tiers, arrival, enq, now, decided=None, path: int = -1):
        tiers = np.asarray(tiers, dtype=np.int64)
        if decided is not None and len(tiers):
            self.rec_stage.record(4, tiers, now - np.asarray(decided, dtype=np.int64))
        if path >= 0:
            self.rec_stage.count(path, tiers.tolist())
        self.rec.record(tiers, now - np.asarray(arrival, dtype=np.int64), now - np.asarray(enq, dtype=np.int64))
        if self.metrics is not None:
            for t, a in zip(tiers, np.asarray(enq)):
                self.metrics.dispatch_latency.labels(self.tiers[int(t)]).observe((now - int(a)) / 1e9)

    # ------------------------------------------------------------------ dispatch
    def dispatch(self) -> int:
        if self.shed_expired:
            self.expire_queued()
        if self.world == 1:
            if self.resources is not None and self.engine is not None and time.monotonic_ns() >= self._res_next_ns:
                self._observe_loads(self._my_load()[None, :])
            return self._dispatch_local()
        return self._dispatch_global()

    def _dispatch_local(self) -> int:
        if self.engine is None or not self.healthy:
            return 0
        free = self.engine.admit_capacity()
        msgs, tier_idx = [], np.zeros(0, dtype=np.int32)
        if free > 0:
            msgs, tier_idx, enq = self.qm.pop_tiers(self.tiers, free, self.aging_ns, self._budgets(),
                                                    self.lifo_ns)
            self._popped(msgs, tier_idx)
            msgs, tier_idx = self._drop_cancelled(msgs, tier_idx)
        n_head = len(msgs)
        lane = self._lane_budget(len(msgs), int((np.asarray(tier_idx) == 0).sum()))
        if lane > 0:
            # realtime lane: tier-0 requests the step's prefill headroom could
            # not take are admitted into any free slot; the engine prefills
            # them first in the next step (engine.fast_tiers)
            b = [0] * len(self.tiers)
            b[0] = lane
            m2, t2, _ = self.qm.pop_tiers(self.tiers, lane, [0] * len(self.tiers), b, None)
            if m2:
                self._popped(m2, t2)
                m2, t2 = self._drop_cancelled(m2, t2)
                msgs = list(msgs) + list(m2)
                tier_idx = np.concatenate([np.asarray(tier_idx, dtype=np.int64), np.asarray(t2, dtype=np.int64)])
        lane_ids = {id(m) for m in msgs[n_head:]}
        if not msgs:
            return 0
        if self.shed_expired:     # expired requests behind a live tier head
            now = time.monotonic_ns()
            dead = [i for i, m in enumerate(msgs) if self._expired(m, now)]
            if dead:
                self._shed([msgs[i] for i in dead])
                keep = np.ones(len(msgs), dtype=bool)
                keep[dead] = False
                msgs = [m for m, k in zip(msgs, keep) if k]
                tier_idx = np.asarray(tier_idx)[keep]
        reqs = []
        for m, t in zip(msgs, tier_idx):
            t = int(t)
            m.tier = t
            if self.lb is not None:
                ep = self.lb.get_endpoint(m, m.conversation_id)
                m.endpoint_id = ep.id
            reqs.append(self._make_request(m, t))
        admitted = self.engine.admit(reqs)
        now = time.monotonic_ns()
        for r in admitted:
            m = r.meta
            m.dispatched_at = now
            m.status = MessageStatus.PROCESSING
            self.table.to_local(m)
            self.inflight_by_tier[r.tier] += 1
        if self.lb is not None and admitted:
            for r in admitted:
                self.lb.mark_admitted(r.meta.endpoint_id)
        n_lane = sum(1 for r in admitted if id(r.meta) in lane_ids)
        if n_lane:
            self.rec_stage.count(P_LANE, [r.tier for r in admitted if id(r.meta) in lane_ids])
        self.rec_stage.count(P_PLAN_LOCAL, [r.tier for r in admitted if id(r.meta) not in lane_ids])
        self._record([r.tier for r in admitted], [r.meta.arrival_ns for r in admitted],
                     [r.meta.enqueued_at for r in admitted], now, [r.meta.popped_ns for r in admitted])
        if len(admitted) < len(reqs):    # cannot happen (free slots were counted); requeue defensively
            got = {id(r) for r in admitted}
            for r in reqs:
                if id(r) not in got:
                    self._requeue(r.meta)
        self.counters["dispatched"] += len(admitted)
        return len(admitted)

    # ------------------------------------------------------------------ backend step
    def _complete(self, m: Message, process_ns: int) -> None:
        self.table.end(m)
        m.status = MessageStatus.COMPLETED
        m.completed_at = time.time_ns()
        if self.tracer is not None:
            self.tracer.request(m)
        if m.arrival_ns:
            # stamped now (the response exists on this router from here), not
            # at the tick's flush: realtime micro-forwards complete mid-tick
            self._done_buf.append((m.tier, m.arrival_ns, m.enqueued_at or m.arrival_ns, time.monotonic_ns()))
        self.qm.complete_message(m.queue_name, m.id, process_ns, m.priority)
        if self.lb is not None and m.endpoint_id:
            self.lb.release_endpoint(m.endpoint_id, process_ns, False)
        self.counters["completed"] += 1
        if self.on_complete is not None:
            self.on_complete(m)

    def step_backend(self):
        """Synchronous backend step (launch + finish)."""
        if self.engine is None:
            return None
        self.engine.launch()
        return self.finish_backend(block=True)

    def finish_backend(self, block: bool = False):
        """Reap finished backend steps (non-blocking by default: the engine
        bounds its own run-ahead) and complete their requests."""
        if self.engine is None:
            return None
        res = self.engine.finish(block=block)
        self._on_results(res)
        return res

    def _finish_micro(self) -> bool:
        """Realtime micro-forwards (``backend.realtime_mode = micro``): launch
        the next ones and complete the requests the finished ones served at
        once -- they finish every few ms, well inside a serving step, so
        their completion is not held back to the tick's reap."""
        eng = self.engine
        if eng is None or not getattr(eng, "micro", False):
            return False
        n = eng.pump_micro()
        res = eng.finish_micro()
        self._on_results(res)
        return bool(n or res.completed or res.first_tokens)

    def _on_results(self, res) -> None:
        if res.completed:
            # this GPU's service-time EWMA (alpha 0.1 per completion, as the
            # reference's ReleaseEndpoint): published in the load vector for
            # the adaptive strategy on every rank
            st = np.fromiter((r.done_ns - r.admitted_ns for r in res.completed), dtype=np.float64)
            a = 1.0 - 0.9 ** len(st)
            self._rt_ewma_us = (1 - a) * self._rt_ewma_us + a * float(st.mean()) / 1e3 \
                if self._rt_ewma_us > 0 else float(st.mean()) / 1e3
            self._err_ewma *= 0.9 ** len(st)
        for r in res.completed:
            if isinstance(r.meta, Message):
                m = r.meta
                self.local.pop(m.handle, None)
                if 0 <= r.tier < len(self.inflight_by_tier):
                    self.inflight_by_tier[r.tier] -= 1
                if self.table.cancelled(m):     # cancelled after its last token was launched
                    self._finish_cancel(m, r.done_ns - r.admitted_ns, dispatched=True)
                    continue
                self._remember_dialog(m, self.rank, r.out_tokens, int(getattr(r, "generated", 0)))
                self._attach_generation(m, r.out_tokens, getattr(r, "out_logprobs", None),
                                        getattr(r, "out_top_ids", None), getattr(r, "out_top_logprobs", None))
                if getattr(r, "finish", False) and getattr(self.engine, "runs_model", False):
                    self._attach_finish(m, r.out_tokens, r.finish_reason, r.stop_entry)
                self._complete(m, r.done_ns - r.admitted_ns)
            else:
                origin, handle, tier = self.foreign.pop(r.req_id)
                if getattr(r, "out_logprobs", None) is not None and r.out_tokens is not None:
                    self._owe_logprobs(origin, handle, r)     # (ahead of the K_DONE: FIFO)
                self._done_owed[origin].append((handle, tier, r.admitted_ns, r.done_ns, K_DONE))
                fin = getattr(r, "finish", False) and getattr(self.engine, "runs_model", False)
                # a dialog turn, or a request that named a stop key: its ids go home
                if (r.conv >= 0 or r.dialog or fin) and r.out_tokens is not None:
                    self._done_tok[origin][handle] = (r.out_tokens,
                                                      pack_finish(r.finish_reason, r.stop_entry) if fin else 0)

    def tick(self, pump=None):
        """One serving tick, pipelined so host work overlaps the forward:
        launch the backend forward (async) -> ingest + GPU preprocess on a
        side stream -> collect the forward (completions free slots) ->
        dispatch queued requests into free slots for the next forward.

        ``pump`` (optional callable) feeds new arrivals; while the launch
        waits for the GPU (its run-ahead queue is full) the gateway calls it
        and ingests -- and, on a single rank, dispatches -- so requests are
        enqueued and admitted while the forward runs instead of at the next
        tick boundary.  (Multi-rank dispatch is a collective and stays once
        per tick.)"""
        with self._tick_lock:
            return self._tick(pump)

    WAIT_INGEST_NS = 8_000_000      # min spacing of ingest batches while the GPU is busy
    WAIT_INGEST_MSGS = 512          # ... unless this many arrived

    def _while_waiting(self, pump, admit: bool = True) -> bool:
        """Work done while the engine waits for the GPU (or, ``admit`` off,
        while this rank waits for its peers at a collective); True if any.
        Arrivals are preprocessed in batches (every WAIT_INGEST_NS or
        WAIT_INGEST_MSGS): each GPU preprocess batch is a fixed chain of
        small kernels, so tiny batches would cost GPU time the forward needs
        (the CPU twin has no such fixed cost: it takes the inbox every time).
        With ``admit`` the enqueued requests are admitted into this GPU's
        free slots at once (one rank: the dispatcher; several: own-GPU
        admission between collectives, ``_dispatch_own``)."""
        if pump is not None:
            pump()
        micro = self._finish_micro()
        now = time.monotonic_ns()
        if self._pre_pending is not None and self.pre.batch_ready(self._pre_pending):
            # a finished preprocess batch is enqueued (and dispatched) at once
            self._finish_pending(block=True)
            if admit:
                self._admit_between()
            return True
        if not self._inbox:
            return micro
        if self.use_gpu_pre and len(self._inbox) < self.WAIT_INGEST_MSGS \
                and now - self._last_ingest_ns < self.WAIT_INGEST_NS:
            return micro
        self._last_ingest_ns = now
        did = self.ingest_async()
        if admit:
            did = self._admit_between() > 0 or did
        return did

    def quiesce(self, pump=None, poll_s: float = 0.0002) -> None:
        """Wait until no forward step is queued on the GPU, ingesting (and on
        one rank dispatching) arrivals from ``pump`` meanwhile, then reap the
        finished steps.  A following ``torch.cuda.synchronize`` returns at
        once, so a synchronisation point (bench window edges) does not stall
        live arrivals behind up to ``max_inflight`` forwards."""
        with self._tick_lock:
            eng = self.engine
            if eng is None:
                return
            while eng.queued_steps():
                if not eng.poll_one() and not self._while_waiting(pump):
                    time.sleep(poll_s)
            self._finish_pending(block=True)      # no preprocess kernels left on the GPU either
            self.finish_backend()

    def _tick(self, pump=None):
        self._pump = pump
        self._process_cancels()
        self._drain_retries()
        self._expire_inflight()
        res = None
        pc = time.perf_counter_ns
        ht = self.host_ns
        t0 = pc()
        if self.engine is not None and self.healthy:
            try:
                self.engine.launch(wait_cb=lambda: self._while_waiting(pump))
                t1 = pc()
                if self.engine.queued_steps():
                    self.ingest_async()          # the GPU is busy: do not wait for the preprocess chain
                else:
                    self.ingest()
                t2 = pc()
                res = self.finish_backend()
                t3 = pc()
                ht[0] += t1 - t0
                ht[1] += t2 - t1
                ht[2] += t3 - t2
                t0 = t3
            except RuntimeError as e:           # HIP error / OOM from the backend
                self._set_healthy(False, f"backend error: {e}")
        if res is None:
            if pump is not None:
                pump()
            self.ingest()
        t4 = pc()
        n = self.dispatch()
        self._finish_micro()                 # realtime requests just admitted start at once
        ht[3] += pc() - t4
        ht[4] += t4 - t0 if res is None else 0
        self.counters["ticks"] += 1
        self.flush_latency()
        return n, res

    def reset_latency(self) -> None:
        """Fresh latency windows: arrival -> dispatch, stages, end to end, and
        the per-tick host / collective profile."""
        self.flush_latency()
        self.rec.reset()
        self.rec_stage.reset()
        self.rec_done.reset()
        self.host_profile(reset=True)
        self.lockstep_stats(reset=True)

    def flush_latency(self) -> None:
        """Move buffered completion timestamps into the e2e histogram."""
        if self._done_buf:
            a = np.asarray(self._done_buf, dtype=np.int64)
            self._done_buf = []
            tiers = np.clip(a[:, 0], 0, len(self.tiers) - 1)
            self.rec_done.record(tiers, a[:, 3] - a[:, 1], a[:, 3] - a[:, 2])

    def host_profile(self, reset: bool = False) -> Dict[str, float]:
        """Mean host milliseconds per tick in each phase (launch includes any
        wait for the GPU when the engine's run-ahead queue is full)."""
        n = max(1, self.counters["ticks"] - self._ticks0)
        out = {k: round(float(v) / n / 1e6, 3) for k, v in
               zip(("launch", "ingest", "finish", "dispatch", "ingest_idle"), self.host_ns)}
        nm = max(1, int(self.ingest_ns[2]))
        out["ingest_msgs_per_tick"] = round(float(self.ingest_ns[2]) / n, 1)
        out["preprocess_us_per_msg"] = round(float(self.ingest_ns[0]) / nm / 1e3, 2)
        out["queue_push_us_per_msg"] = round(float(self.ingest_ns[1]) / nm / 1e3, 2)
        if reset:
            self.host_ns[:] = 0
            self.ingest_ns[:] = 0
            self._ticks0 = self.counters["ticks"]
        return out

    def lockstep_stats(self, reset: bool = False) -> Dict[str, float]:
        """Per-tick control-plane collective time of this rank (ms): the
        wait for the slowest peer plus the exchange itself."""
        w = np.asarray(self.coll_wait_ns, dtype=np.float64) / 1e6
        out = {"ticks": int(w.size),
               "p50_ms": round(float(np.percentile(w, 50)), 4) if w.size else 0.0,
               "p99_ms": round(float(np.percentile(w, 99)), 4) if w.size else 0.0,
               "max_ms": round(float(w.max()), 4) if w.size else 0.0,
               "mean_ms": round(float(w.mean()), 4) if w.size else 0.0}
        if reset:
            self.coll_wait_ns.clear()
        return out

    def request_stop(self) -> None:
        self.stopping = True
        if self.world == 1:
            self.peers_stopping = True

    def pending(self) -> int:
        return self.qm.total_pending()

    def inbox_size(self) -> int:
        """Submitted, not yet ingested (preprocessed + queued)."""
        with self._inbox_lock:
            return len(self._inbox)

    def drop_pending(self) -> int:
        self._finish_pending(block=True)
        n = 0
        for t in self.tiers:
            n += self.qm.size(t)
            for m in self.qm.mlq.messages(t):
                self._pin(m, -1)
                self.table.end(m)
            self.qm.mlq.clear(t)
        with self._inbox_lock:
            n += len(self._inbox)
            for m in self._inbox:
                self.table.end(m)
            self._inbox = []
        return n

    # ------------------------------------------------------------------ lifecycle helpers
    def _queue_removed(self, m: Message) -> None:
        """``qm.on_remove`` (API / peer threads): a queued message taken out
        other than by dispatch leaves the lifecycle (its pin is released)."""
        self._pin(m, -1)
        if m.lc == QUEUED:
            m.lc = NONE

    def _drop_cancelled(self, msgs, tier_idx):
        """Popped messages with a cancel pending end here instead of being
        dispatched; returns the rest (and their tier indices)."""
        if not self.table.tomb or not len(msgs):
            return msgs, tier_idx
        live, dead, t = self.table.split_cancelled(msgs, list(np.asarray(tier_idx).tolist()))
        for m in dead:
            self._pin(m, -1)
            self._finish_cancel(m, dispatched=True)        # (popped: its processing count is open)
        return live, np.asarray(t, dtype=np.int64)
