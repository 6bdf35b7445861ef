"""GPU backend engine: continuous batching over fixed batch slots (N12 + N9).

One engine per GPU process.  ``admit`` places dispatched requests into free
slots; ``launch`` enqueues ONE model forward over a token batch made of
  * one decode token for every slot that is generating, then
  * chunked-prefill tokens of admitted prompts, up to ``token_budget``;
and returns immediately.  The pipeline is fully asynchronous:
  * a decode token's id is the previous step's greedy output, which stays on
    the device -- the next step gathers it there (``index_select``), so the
    host never waits for token values;
  * completions are deterministic (greedy decode always yields a token), so
    a request's slot is freed at launch of its last step and can be re-admitted
    into the NEXT step (same-stream ordering keeps its KV rows safe) -- except
    a request ended by a stop token or stop sequence, which is known only
    when its step is reaped and completes there (``_reap_stops``);
  * at most ``max_inflight`` (2) steps are queued on the GPU; ``finish`` reaps
    finished steps (blocking only when the queue is full), so host work of the
    next tick overlaps the current forward and the GPU never idles between
    steps.
The slot census of every step is written by the ``slot_census`` kernel into
the node-shared load page (zero-copy for routers, N9).

Reference: the reference has no model backend -- its workers call a
``ProcessFunc`` (`internal/priorityqueue/worker.go:162-189`) that
`cmd/server/main.go:172-193` (`startWorkers`) stubs out; this engine is what a
dispatched request runs on instead.

Request cost model (README/bench): prompt = the message's tokens from the
GPU tokenizer (capped), generation = ``gen_tokens`` greedy tokens, all 32
layers of the stub, never skipped.
"""
from __future__ import annotations

import collections
import math
import time
from dataclasses import dataclass
from typing import Deque, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..models.llama_stub import LlamaConfig, LlamaStub, LogitEdit, Penalise, Stops, Truncate
from ..ops.gemm import SKINNY_CHUNKED_MAX_M, row_scale_len
from ..ops.sampling import (LE_MAX, LP_TOP, PEN_HIST_MAX, STOP_ENT_WORDS, STOP_ENTRIES, STOP_LEN, STOP_ROW_WORDS,
                            inv_temperature, min_p_log, row_keys)


@dataclass
class Request:
    req_id: int
    prompt: np.ndarray            # int32 token ids
    gen_tokens: int
    tier: int = 2
    slot: int = -1
    prefilled: int = 0
    generated: int = 0
    admitted_ns: int = 0
    first_token_ns: int = 0
    done_ns: int = 0
    meta: object = None
    out_idx: int = -1             # row of the previous step's output holding my last token
    out_step: int = -1
    conv: int = -1                # conversation key: its KV stays resident in the slot between turns
    reused: int = 0               # context tokens served from the resident KV (not re-prefilled)
    history: Optional[np.ndarray] = None   # earlier dialog tokens, prefilled only if not resident
    # compressed context of an evicted window (N5 salient tokens), prepended
    # to a non-resident replay ahead of ``history``; never part of a resident KV
    prefix: Optional[np.ndarray] = None
    timeout_ns: int = 0           # processing timeout of this attempt (0: none); the deadline starts at admission
    deadline_ns: int = 0          # admitted_ns + timeout_ns (monotonic), set by ``admit``
    micro: bool = False           # served by the realtime micro-forwards (``realtime_mode="micro"``)
    aborted: bool = False         # this attempt was aborted (timeout / cancel / evacuation)
    # the greedy token ids this attempt generated, read back from the device
    # with the step that sampled them (set when the request completes)
    out_tokens: Optional[np.ndarray] = None
    # a conversation turn dispatched by another router: its ``out_tokens``
    # go back with the completion record even when ``conv`` is -1 (no KV
    # residency), so the origin's dialog history holds the real ids
    dialog: bool = False
    # sampling: 0 = greedy, else tokens are drawn from softmax(logits /
    # temperature) with noise that is a pure function of (seed, index of the
    # generated token, vocabulary column) -- ``ops.sampling``.  With a
    # temperature, ``top_k`` > 0 / ``top_p`` < 1 truncate the distribution
    # first (``csrc/kernels/sample_truncate_kernels.h``); a greedy request
    # ignores both
    temperature: float = 0.0
    seed: int = 0
    top_k: int = 0
    top_p: float = 1.0
    # log-probabilities (``csrc/kernels/logprob_kernels.h``): -1 = off, 0..5 =
    # score every generated token, greedy or sampled (the engine always reads
    # back all 5 alternatives; the caller trims to its n).  The results, one
    # row per generated token, are set with ``out_tokens``
    logprobs: int = -1
    out_logprobs: Optional[np.ndarray] = None       # float32 [generated]
    out_top_ids: Optional[np.ndarray] = None        # int32 [generated][5] (-1: no such alternative)
    out_top_logprobs: Optional[np.ndarray] = None   # float32 [generated][5]
    # penalties (``csrc/kernels/penalty_kernels.h``), greedy or sampling,
    # applied before temperature and truncation: presence / frequency over the
    # tokens this attempt generated, repetition over those and the message's
    # own prompt (0 / 0 / 1: off).  Earlier turns of a dialog, resident or
    # replayed, are outside the window
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    repetition_penalty: float = 1.0
    # which tokens are eligible.  ``allowed`` (int32 ids, at most 64) and
    # ``logit_bias`` (int32 ids, float32 values, at most 64) edit the logits
    # after the penalties and before the temperature, greedy or sampling
    # (``csrc/kernels/logit_edit_kernels.h``); an id outside the vocabulary is
    # ignored.  ``min_p`` (0: off) is one more truncation rule of a sampling
    # request, after ``top_p``; a greedy request ignores it
    min_p: float = 0.0
    logit_bias: Optional[Tuple[np.ndarray, np.ndarray]] = None
    allowed: Optional[np.ndarray] = None
    # when to stop (``csrc/kernels/stop_kernels.h``).  ``max_tokens`` (0: the
    # configured count) caps ``gen_tokens`` at admission; ``stop`` is the
    # request's stop entries, each a sequence of 1..8 token ids (a stop token
    # is an entry of one), compared with the tail of what this attempt has
    # generated after every token; a match that would end the generation with
    # fewer than ``min_tokens`` tokens is ignored.  None of them changes a
    # token.  ``finish`` asks for the outcome to be reported; the engine sets
    # ``finish_reason`` ("stop" / "length") and, for a stop, ``stop_entry``
    # (the matched entry's index) with ``generated`` when the request completes
    max_tokens: int = 0
    min_tokens: int = 0
    stop: Optional[list] = None
    finish: bool = False
    finish_reason: str = ""
    stop_entry: int = -1
    seq_key: int = 0              # its slot's admission key (unique per admission: names this attempt to queued steps)


@dataclass
class StepResult:
    tokens: int
    prefill_tokens: int
    decode_tokens: int
    completed: List[Request]
    first_tokens: List[Request]
    elapsed_ms: float


class _blas:
    """torch's library-GEMM backend for a block (``cublas`` = rocBLAS on ROCm,
    ``cublaslt`` = hipBLASLt), restored after it (the serve loop is one thread)."""

    def __init__(self, lib: str):
        self.lib = lib

    def __enter__(self):
        self.prev = torch.backends.cuda.preferred_blas_library()
        torch.backends.cuda.preferred_blas_library(self.lib)
        return self

    def __exit__(self, *exc):
        torch.backends.cuda.preferred_blas_library(self.prev)
        return False


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _Staging:
    """The layout of one step's int32 staging buffer: the blocks in the
    order given, each ``(name, words)`` or ``(name, words, align)`` -- a
    block that is not empty starts on a multiple of ``align`` words, the
    words skipped before it zero.  ``host`` and ``dev`` give the same block
    of the host buffer (numpy) and of its device copy ``dbuf`` (torch), as
    int32 or (``f32``) float32, in the shape asked for."""

    def __init__(self, *blocks):
        self.at = {}
        n, pads = 0, []
        for name, words, *align in blocks:
            if words and align and n % align[0]:
                pads.append((n, n + align[0] - n % align[0]))
                n = pads[-1][1]
            self.at[name] = (n, n + words)
            n += words
        self.buf = np.empty(n, dtype=np.int32)
        for a, b in pads:
            self.buf[a:b] = 0
        self.dbuf = None

    def host(self, name: str, shape=None, f32: bool = False) -> np.ndarray:
        a, b = self.at[name]
        v = self.buf[a:b].view(np.float32) if f32 else self.buf[a:b]
        return v if shape is None else v.reshape(shape)

    def dev(self, name: str, shape=None, f32: bool = False) -> torch.Tensor:
        a, b = self.at[name]
        v = self.dbuf[a:b].view(torch.float32) if f32 else self.dbuf[a:b]
        return v if shape is None else v.view(shape)


class BackendHung(Exception):
    """A forward step has not completed on the GPU within the engine's
    ``step_timeout_s``.  Not a RuntimeError on purpose: a recoverable
    backend error (HIP error, OOM) evacuates this GPU and keeps serving, but
    a step that never completes leaves nothing to evacuate to -- the work
    queued behind it waits forever -- so the process must end (the serve
    loop treats it like ``PeerLost``) and the launcher restarts the job."""


@dataclass
class _Inflight:
    step: int
    event: object
    T: int
    n_pre: int
    n_dec: int
    completed: List[Request]
    firsts: List[Request]
    t0: float
    out: object                   # device tensor of sampled tokens (kept alive for the next gather)
    t0_ns: int = 0                # monotonic launch time (tracing)
    ev_start: object = None       # timing event before the forward (``time_steps``)
    micro: bool = False           # a realtime micro-forward (``_qm``), not a serving step
    samp_slots: object = None     # int64 [S]: the slot each sampled row belongs to
    gidx: object = None           # int64 [S]: which generated token of its request each row is
    host_out: object = None       # pinned int32 [>= S]: the sampled ids, copied back behind the forward
    lp_rows: object = None        # int64 [L]: the sampled rows scored by ``logprob_head`` (None: none)
    host_lp: object = None        # pinned (float32 [>= L][6], int32 [>= L][5]): their results, copied back likewise
    stop_rows: object = None      # int64 [R]: the sampled rows that have stop entries (None: none)
    host_stop: object = None      # pinned int32 [>= R]: their matched entry (-1: none), copied back likewise
    stop_reqs: object = None      # (their requests, their slots' admission keys), as the launch saw them


class BackendEngine:
    MICRO_GRAPH_BUCKETS = (8, 16, 32, 64)
    runs_model = True             # False: an engine that runs no model ignores a request's penalties
    scores_logprobs = True        # False: an engine that runs no model leaves ``Request.out_logprobs`` None

    def __init__(self, model_cfg: LlamaConfig, slots: int = 256, max_ctx: int = 512,
                 token_budget: int = 2048, device="cuda", impl: str = "hip", seed: int = 0,
                 page=None, gpu_index: int = 0, max_inflight: int = 2, residual_in_gemm: bool = True,
                 split_qkv: bool = False, fused_mlp=None, fused_qkv=None, row_scale_norm: bool = True,
                 fused_head=None, fused_resid=None, prune_last: bool = True, step_timeout_s: float = 60.0,
                 realtime_step_tokens: int = 0, fused_rms=None, realtime_mode: str = "",
                 micro_slots: int = 96, micro_budget: int = 512, micro_inflight: int = 1,
                 micro_stream: str = "partition", micro_cus: int = 64, micro_gemm: str = "hip",
                 library_gemm: bool = False, micro_graph: bool = True, micro_weights: str = "bf16"):
        self.cfg = model_cfg
        # a queued forward older than this raises BackendHung (0 = wait forever)
        self.step_timeout_s = float(step_timeout_s)
        self.slots = slots
        self.max_ctx = max_ctx
        # every generating slot gets its decode token each step (the on-device
        # token gather reads the previous step's output only)
        self.token_budget = max(token_budget, slots)
        # How realtime requests (tier < fast_tiers) are served
        # (``backend.realtime_mode``; docs/performance.md "Realtime modes"):
        #   "off"   -- in the serving steps like everyone else (prefilled first);
        #   "cap"   -- the step cap (``backend.realtime_step_tokens``): while a
        #              realtime request is in the batch a step carries at most
        #              that many tokens (never fewer than its decode rows), so
        #              its 4 forwards finish sooner -- at the price of the
        #              smaller steps' GEMM efficiency for everyone in them
        #              (profiles/r5_step_budget_sweep_1gpu.jsonl);
        #   "micro" -- realtime micro-forwards: realtime requests take slots of
        #              a separate pool (``micro_slots``) that only small
        #              forwards over those slots touch, launched back to back
        #              on their own stream (``micro_stream``: "high" = a
        #              high-priority HIP stream next to the serving stream,
        #              "same" = the serving stream) while the big steps run.
        # An empty mode follows ``realtime_step_tokens`` (> 0: "cap").
        self.rt_step_tokens = int(realtime_step_tokens)
        mode = realtime_mode or ("cap" if self.rt_step_tokens > 0 else "off")
        if max_ctx > PEN_HIST_MAX:
            raise ValueError(f"max_ctx {max_ctx} exceeds the penalty kernel's history of {PEN_HIST_MAX} tokens")
        if mode not in ("off", "cap", "micro"):
            raise ValueError(f"realtime_mode must be off / cap / micro, not {mode!r}")
        if mode != "cap":
            self.rt_step_tokens = 0
        self.realtime_mode = mode
        self.micro = mode == "micro"
        self.micro_slots = int(micro_slots) if self.micro else 0
        if self.micro and self.micro_slots < 1:
            raise ValueError("realtime_mode micro needs micro_slots >= 1")
        self.micro_budget = max(int(micro_budget), self.micro_slots + 1)
        self.micro_inflight = max(1, int(micro_inflight))
        self.device = torch.device(device)
        self.cuda = self.device.type == "cuda"
        # decode-only micro-forwards (<= 64 rows) replay HIP graphs captured
        # at warm-up, one per row bucket (``MICRO_GRAPH_BUCKETS``): a
        # micro-forward is ~350 kernel launches the serve loop's host thread
        # would otherwise issue one by one between pumping arrivals.  The
        # padding rows of a bucket run on a scratch slot past the micro pool.
        self.micro_graph = bool(micro_graph) and self.micro and self.cuda and impl == "hip" \
            and micro_stream in ("high", "partition")
        self.scratch_slot = slots + self.micro_slots if self.micro_graph else -1
        # KV slots: serving pool, then the micro pool (+ the graphs' scratch slot)
        self.n_all = slots + self.micro_slots + (1 if self.micro_graph else 0)
        self.async_device = self.cuda          # forwards run asynchronously (a GPU stream)
        self.rt_stream = None
        self.main_stream = None          # (partition: the serving steps' CU-masked stream)
        self.micro_cus = 0
        if self.micro and micro_stream not in ("high", "same", "partition"):
            raise ValueError(f"micro_stream must be high / same / partition, not {micro_stream!r}")
        if self.micro and self.cuda and micro_stream == "high":
            self.rt_stream = torch.cuda.Stream(self.device, priority=torch.cuda.Stream.priority_range()[1])
        elif self.micro and self.cuda and micro_stream == "partition":
            # the chip split in two CU partitions: the micro-forwards own
            # ``micro_cus`` CUs, the serving steps the rest (their GEMM tile
            # plans size waves for that count), so neither waits for the
            # other's kernels to drain (docs/performance.md "Realtime modes")
            from .cu_partition import partition_streams
            self.micro_cus = int(micro_cus)
            self.main_stream, self.rt_stream, big_cus = partition_streams(self.device, self.micro_cus)
            from ..ops import gemm as _G
            _G.EFFECTIVE_CUS[self.device.index if self.device.index is not None else 0] = big_cus
            # serving steps of whole waves on the remaining CUs: 16 row tiles
            # per 256 CUs (4,096 tokens on the chip, 3,072 on 192 CUs --
            # profiles/r6_token_budget_sweep_1gpu.jsonl, r6_realtime_modes.md)
            self.token_budget = max(min(self.token_budget, 16 * big_cus), slots)
        self.micro_stream = micro_stream if self.micro else ""
        # the micro-forwards' GEMMs on a CU partition: "hip" = the hand-written
        # kernels (split-K small steps), "rocblas" = the library through
        # rocBLAS (classic, non-persistent kernels: safe on a CU mask, unlike
        # hipBLASLt's stream-K grids sized for the whole chip)
        if micro_gemm not in ("hip", "rocblas"):
            raise ValueError(f"micro_gemm must be hip / rocblas, not {micro_gemm!r}")
        self.micro_gemm = micro_gemm
        # the layer weights the micro-forwards read: "bf16" = the serving
        # pool's, "fp8" = an e4m3 copy with one scale a row (W8A16: half the
        # bytes a micro-forward streams; ops.quant, ops.gemm.skinny_fp8 / gemm_fp8).  A
        # request of the micro pool then sees the quantised model in all its
        # forwards, eager or graph-replayed, so its tokens differ from the
        # serving pool's (``Request.micro`` tells which pool served it).
        # Without micro-forwards the mode only costs the copy's memory.
        if micro_weights not in ("bf16", "fp8"):
            raise ValueError(f"micro_weights must be bf16 / fp8, not {micro_weights!r}")
        if micro_weights == "fp8" and micro_gemm == "rocblas":
            raise ValueError("micro_weights fp8 needs micro_gemm hip (the library has no W8A16 kernel)")
        if micro_weights == "fp8" and self.micro and self.micro_budget > SKINNY_CHUNKED_MAX_M:
            raise ValueError(f"micro_weights fp8: micro_budget {self.micro_budget} exceeds the fp8 kernel's "
                             f"{SKINNY_CHUNKED_MAX_M} rows")
        self.micro_weights = micro_weights
        if self.micro_cus and micro_gemm == "rocblas":
            import os
            # rocBLAS may hand some GEMMs to hipBLASLt on gfx950: keep them classic
            os.environ.setdefault("ROCBLAS_USE_HIPBLASLT", "0")
        self.model = LlamaStub(model_cfg, self.n_all, max_ctx, device=self.device, impl=impl, seed=seed,
                               residual_in_gemm=residual_in_gemm, split_qkv=split_qkv, fused_mlp=fused_mlp,
                               fused_qkv=fused_qkv, row_scale_norm=row_scale_norm, fused_head=fused_head,
                               fused_resid=fused_resid, fused_rms=fused_rms, prune_last=prune_last,
                               library_gemm=library_gemm, small_weights=micro_weights)
        self.impl = impl
        self.weight_bytes = self.model.weight_bytes()
        self.active: Dict[int, Request] = {}            # slot -> request
        self.free: List[int] = list(range(slots - 1, -1, -1))
        # the realtime micro pool: slots [slots, n_all), never in ``free`` /
        # ``conv_lru``, so no serving step ever reads or writes their KV rows
        # (the two streams never share a slot)
        self.free_micro: List[int] = list(range(slots + self.micro_slots - 1, slots - 1, -1))
        n_all = self.n_all
        # Conversation KV residency (BASELINE config 4): when a request of a
        # conversation completes, its slot keeps the KV of the dialog so far
        # (prompt + generated tokens except the last) and parks in an LRU;
        # the conversation's next turn is admitted into that slot and only
        # prefills its new tokens.  Parked slots count as free: they are
        # evicted (LRU) when no truly free slot is left.
        self.conv_lru: "collections.OrderedDict[int, int]" = collections.OrderedDict()
        self.s_conv = np.full(n_all, -1, dtype=np.int64)
        self.s_cached = np.zeros(n_all, dtype=np.int64)
        self.kv_reused_tokens = 0
        self.kv_evictions = 0
        self.kv_imported = 0
        self.kv_stale = 0                                   # parked copies found outdated at admission
        self.replay_tokens = 0                              # dialog tokens prefilled by non-resident replays
        self.replay_nonzero = 0                             # ... of which not the id 0 (placeholders were 0)
        self._importing: Dict[int, int] = {}                # slot -> conv: KV arriving (migration in flight)
        # per-slot host state (the batch builder is vectorised over these)
        self.s_prompt = np.zeros((n_all, max_ctx), dtype=np.int32)
        self.s_plen = np.zeros(n_all, dtype=np.int64)
        self.s_pref = np.zeros(n_all, dtype=np.int64)       # prompt tokens prefilled
        self.s_gen = np.zeros(n_all, dtype=np.int64)        # tokens generated
        self.s_gmax = np.zeros(n_all, dtype=np.int64)       # tokens to generate
        self.s_seq = np.zeros(n_all, dtype=np.int64)        # admission order
        self.s_out_idx = np.zeros(n_all, dtype=np.int64)    # row of my last token in the step output
        self.s_out_step = np.full(n_all, -2, dtype=np.int64)
        self.s_active = np.zeros(n_all, dtype=bool)
        self.s_tier = np.zeros(n_all, dtype=np.int64)
        self.s_micro = np.zeros(n_all, dtype=bool)
        self.s_micro[slots:] = True
        self.s_temp = np.zeros(n_all, dtype=np.float32)     # sampling temperature (0: greedy)
        self.s_seed = np.zeros(n_all, dtype=np.uint64)      # sampling seed
        self.s_topk = np.zeros(n_all, dtype=np.int32)       # top-k of a sampling slot (0: off)
        self.s_topp = np.ones(n_all, dtype=np.float32)      # top-p of a sampling slot (1: off)
        self.sampled_steps = 0                              # forwards that ended in the sampling head
        self.truncated_steps = 0                            # ... and drew a top-k / top-p row again (``truncated_head``)
        self.s_logp = np.zeros(n_all, dtype=bool)           # the slot's request asks for log-probabilities
        self.logprob_steps = 0                              # forwards that scored a row (``logprob_head``)
        # penalties: the slot's (presence, frequency, repetition) and the
        # position its window starts at (``s_plen - n_own``: the message's own
        # capped prompt, not a resident or replayed context before it)
        self.s_pen = np.zeros(n_all, dtype=bool)
        self.s_penp = np.zeros((n_all, 3), dtype=np.float32)
        self.s_pfrom = np.zeros(n_all, dtype=np.int64)
        self.penalised_steps = 0                            # forwards that drew a penalised row (``penalised_head``)
        self.d_hist = None                                  # the device-side token history (first penalised request)
        # allow-lists and logit biases (``logit_edit_kernels.h``): the slot's
        # lists, host side (allocated with the first request that has one):
        # ``h_eids[s]`` = allow ids then bias ids, ``h_evals[s]`` the bias
        # values at the bias ids' places, ``s_ecnt[s]`` = (n_allow, n_bias).
        # ``s_minp``: float32 log(min_p) of a sampling slot (-inf: off)
        self.s_edit = np.zeros(n_all, dtype=bool)
        self.s_ecnt = np.zeros((n_all, 2), dtype=np.int32)
        self.h_eids = self.h_evals = None
        self.s_minp = np.full(n_all, -np.inf, dtype=np.float32)
        self._eligibility_seen = False                      # a request has named min_p, an allow-list or a bias
        self.edited_steps = 0                               # forwards that edited a row by such a list (``logit_edit``)
        # stop tokens and sequences (``stop_kernels.h``): the slot's entry
        # table ``h_stop[s]`` (int32 [STOP_ENTRIES][1 + STOP_LEN], allocated
        # with the first request that has one), how many entries, ``min_tokens``
        # and whether an entry is longer than one token (its slot's tokens are
        # then recorded in ``d_hist``)
        self.s_stop = np.zeros(n_all, dtype=bool)
        self.s_shist = np.zeros(n_all, dtype=bool)
        self.s_nstop = np.zeros(n_all, dtype=np.int32)
        self.s_mintok = np.zeros(n_all, dtype=np.int32)
        self.s_stopkey = np.full(n_all, -1 << 62, dtype=np.int64)   # admission key of the request last stopped in the slot
        self.h_stop = None
        self._stop_pins = self._stop_pins_m = None          # the steps' stop results, copied back behind the ids
        self.stopped_total = 0                              # requests ended by a stop
        self.stop_steps = 0                                 # forwards that ran ``stop_match``
        self.stop_dropped_rows = 0                          # decode rows computed after their request's stop
        # host copy of every scored token's log-probability and alternatives,
        # per slot, next to ``h_tokens`` (allocated with the first request that asks)
        self.h_lp = self.h_top_ids = self.h_top_lp = None
        # host copy of every generated token id, per slot (written when the
        # step that sampled it is reaped; steps of one pool are reaped in
        # launch order, so a slot's next request never overwrites a row
        # before the previous one's completion copied it out)
        self.h_tokens = np.zeros((n_all, max_ctx), dtype=np.int32)
        # processing deadline per slot (monotonic ns, 0 = none): a request
        # still running past it is aborted by ``expire`` (the reference runs
        # every message under context.WithTimeout(msg.Timeout),
        # `internal/priorityqueue/worker.go:162-188`)
        self.s_deadline = np.zeros(n_all, dtype=np.int64)
        self.expired_total = 0
        self.cancelled_total = 0
        self._admit_seq = 0
        self._mean_plen = 16.0                              # EMA of admitted prompt lengths
        # realtime lane: requests of tiers < fast_tiers are prefilled ahead of
        # every other admitted prompt (their admission order key is shifted
        # below all others), and the dispatcher may admit them past the
        # step's prefill headroom (``lane_capacity``)
        self.fast_tiers = 1
        self.warmed_shapes = 0
        self.page = page
        self.gpu_index = gpu_index
        self.max_inflight = max(1, max_inflight)
        self.step_id = 0
        self.total_tokens = 0
        self.completed_total = 0
        self.completed_tokens = 0
        self.matmul_flops = 0                            # GEMM FLOPs of every launched forward (``_step_flops``)
        self._q: Deque[_Inflight] = collections.deque()
        self._reaped: List[_Inflight] = []               # reaped by launch(), not yet returned
        self._fence: List[object] = []                   # events of steps dropped by abort_all
        self.host_ns = np.zeros(3, dtype=np.int64)       # [batch build, wait for GPU, enqueue forward] host time
        self._prev_out = None                            # device int32 [n_samples] of the last launched step
        # pinned staging rings (a buffer is reused only after the step that
        # read it has finished: launch keeps <= max_inflight steps queued, so
        # step k reuses step k - ring's buffer only once that one was reaped)
        ring = max(2, self.max_inflight)
        # (+ a sampling step's 1 / T and two key words per sampled row, padded to whole 256-row tiles,
        #  row index, top_k and top_p of its truncating rows, and the row index of a step's
        #  log-probability rows, and a penalised step's block: 10 words per penalised row and the token
        #  rows to record, and an edited step's block: 6 words per row and its two lists, ids and values,
        #  and a stop step's block: 7 words per row and its entries)
        stop_words = 1 + STOP_ROW_WORDS + STOP_ENTRIES * STOP_ENT_WORDS
        self._pins = [self._alloc_pin(4 * (8 * self.token_budget + (22 + 4 * LE_MAX + stop_words) * slots + 64
                                           + 3 * row_scale_len(slots) + 4))
                      for _ in range(ring)]
        # sampled token ids copied back behind each forward (read at reap)
        self._out_pins = [self._alloc_pin(4 * self.n_all).view(torch.int32) for _ in range(ring)]
        # log-probability rows copied back likewise
        self._lp_pins = [self._alloc_lp_pin(self.n_all) for _ in range(ring)]
        # realtime micro-forwards: their own queue, staging, token gather source
        self._qm: Deque[_Inflight] = collections.deque()
        self._reaped_m: List[_Inflight] = []
        self._prev_out_m = None
        self.micro_id = 0
        self.micro_steps = 0
        self.micro_gpu_ms = 0.0                          # device time of timed micro-forwards (``time_steps``)
        self.micro_timed = 0
        self._mg: Dict[int, tuple] = {}                  # bucket -> (graph, static inputs, token ids, output)
        self.micro_graph_steps = 0
        if self.micro:
            mr = self.micro_inflight + 1
            # a micro step's staging: tokens, pos, slot (3T), samples + decode
            # gather rows (<= 3T) and ~one 1-token tile per row (4T) -- sized
            # so it never grows (a grown pinned buffer frees the old one
            # behind the copies still queued from it)
            self._pins_m = [self._alloc_pin(4 * (12 * self.micro_budget + 2 * self.micro_slots + 64
                                                 + 3 * row_scale_len(self.micro_slots)
                                                 + (20 + 4 * LE_MAX + stop_words) * self.micro_slots + 4))
                            for _ in range(mr)]
            self._out_pins_m = [self._alloc_pin(4 * self.micro_slots).view(torch.int32) for _ in range(mr)]
            self._lp_pins_m = [self._alloc_lp_pin(self.micro_slots) for _ in range(mr)]
        # segment-tiled MFMA attention on the HIP path (per-token otherwise)
        self.use_tiles = impl == "hip"
        self._state_pins = [self._alloc_pin(4 * slots) for _ in range(2)]
        self._slot_state_d = torch.zeros(slots, dtype=torch.int32, device=self.device)
        # fault injection: {"fail_launch": n} raises on the next
        # n launches (a HIP error / OOM), {"slow_ms": x} stalls every launch,
        # {"drop_heartbeat": True} stops the load-page census
        self.fault: Dict[str, float] = {}
        self.tracer = None          # utils.tracing.RequestTracer (backend step spans)
        # GPU execution time of every forward step (timing events around it;
        # the start event's timestamp is when the GPU reached the step, so the
        # difference is device time, not queueing): bench.py's lock-step
        # attribution (slowest vs mean GPU of a multi-rank job)
        self.time_steps = False
        self.gpu_step_ms = 0.0
        self.gpu_steps = 0
        self.gpu_step_max_ms = 0.0
        if self.cuda and page is not None and page.dev_ptr is None:
            page.register_device()
        if page is not None:
            page.set_health(True)
            page.write_host(0, slots, 0, 0)

    def _alloc_pin(self, nbytes: int) -> torch.Tensor:
        t = torch.empty(nbytes, dtype=torch.uint8)
        return t.pin_memory() if self.cuda else t

    def _alloc_lp_pin(self, rows: int) -> tuple:
        return (self._alloc_pin(4 * (1 + LP_TOP) * rows).view(torch.float32).view(rows, 1 + LP_TOP),
                self._alloc_pin(4 * LP_TOP * rows).view(torch.int32).view(rows, LP_TOP))

    # ------------------------------------------------------------------ admission
    def free_slots(self) -> int:
        return len(self.free) + len(self.conv_lru)

    def inflight(self) -> int:
        """Requests holding a slot (serving pool + realtime micro pool)."""
        return self.slots - self.free_slots() + self.micro_slots - len(self.free_micro)

    def _big_active(self) -> np.ndarray:
        return self.s_active & ~self.s_micro if self.micro else self.s_active

    def _take_slot(self) -> int:
        if self.free:
            return self.free.pop()
        conv, s = self.conv_lru.popitem(last=False)          # evict the least recently used context
        self.s_conv[s] = -1
        self.kv_evictions += 1
        return s

    def resident_context(self, conv: int) -> int:
        """Tokens of conversation ``conv`` resident in this engine's KV (0 if none)."""
        s = self.conv_lru.get(conv)
        return int(self.s_cached[s]) if s is not None else 0

    def admit_capacity(self) -> int:
        """How many new requests the NEXT step can take: free slots, bounded
        by the step's prefill headroom (token budget - decode tokens - prompt
        tokens already admitted but not yet prefilled) over the running mean
        prompt length.  The dispatcher admits at most this many, so requests
        that could not start prefilling next step wait in the priority queue
        (where tier order and aging apply), not in a FIFO inside the engine."""
        free = len(self.free) + len(self.conv_lru)
        if free == 0:
            return 0
        act = self._big_active()
        pending = int((self.s_plen[act] - self.s_pref[act]).sum())
        head = self.step_budget() - int(act.sum()) - pending
        if head <= 0:
            return 0
        # round UP: the last admitted prompt may spill into the following step
        # (chunked prefill), so a saturated step fills its token budget -- GEMM
        # cost is quantised in 256-row tiles, the tail rows are nearly free
        return min(free, max(1, -(-head // max(1, int(round(self._mean_plen))))))

    # ------------------------------------------------------------------ KV migration (N11)
    def export_kv(self, conv: int):
        """(slot, tokens) of conversation ``conv``'s parked KV, or (-1, 0)
        when it is not resident here (evicted, or a turn is in flight)."""
        s = self.conv_lru.get(conv)
        if s is None:
            return -1, 0
        return s, int(self.s_cached[s])

    def drop_parked(self, conv: int) -> None:
        """Forget a parked conversation (its KV moved to another GPU); the
        slot is free for the next admission (stream order keeps the pending
        pack copy ahead of any later write to it)."""
        s = self.conv_lru.pop(conv, None)
        if s is not None:
            self.s_conv[s] = -1
            self.s_cached[s] = 0
            self.free.insert(0, s)          # reused last (``free`` pops from the end)

    def import_kv(self, conv: int, tokens: int) -> int:
        """Park an incoming conversation's KV (``tokens`` positions) in a
        slot; returns the slot the caller unpacks into.  The conversation's
        turn is then admitted like any resident turn (prefills only its new
        tokens)."""
        self.drop_parked(conv)
        s = self._take_slot()
        self.s_conv[s] = conv
        self.s_cached[s] = int(tokens)
        self.conv_lru[conv] = s
        self.kv_imported += 1
        return s

    def reserve_import(self, conv: int, tokens: int = 0) -> int:
        """A slot for an incoming conversation's KV while the transfer is in
        flight on the migration stream: out of the free list and the LRU
        (so no admission can take it) until ``finish_import`` parks it."""
        self.drop_parked(conv)
        s = self._take_slot()
        self.s_conv[s] = -1
        self.s_cached[s] = int(tokens)
        self._importing[s] = conv
        return s

    def finish_import(self, conv: int, slot: int, tokens: int) -> None:
        """The KV landed in ``slot``: park it like a resident dialog (the
        conversation's held turn is admitted next and reuses it)."""
        if self._importing.pop(slot, None) is None:
            return                                          # aborted meanwhile (evacuation)
        old = self.conv_lru.pop(conv, None)
        if old is not None and old != slot:
            self.s_conv[old] = -1
            self.free.append(old)
        self.s_conv[slot] = conv
        self.s_cached[slot] = int(tokens)
        self.conv_lru[conv] = slot
        self.kv_imported += 1

    def resident_kv_tokens(self) -> int:
        """KV positions held in this GPU's cache right now: the context of
        every active request (prompt + generated so far) plus every parked
        dialog -- the live HBM occupancy of the KV pool (the pool itself is
        preallocated, so allocator figures never move)."""
        act = self.s_active
        n = int((self.s_plen[act] + self.s_gen[act]).sum())
        if self.conv_lru:
            n += int(self.s_cached[np.fromiter(self.conv_lru.values(), dtype=np.int64)].sum())
        return n + int(self.s_cached[list(self._importing)].sum()) if self._importing else n

    def kv_token_capacity(self) -> int:
        return self.slots * self.max_ctx

    def kv_bytes_per_token(self) -> int:
        c = self.cfg
        return c.layers * 2 * c.kv_heads * c.head_dim * 2          # K and V, bf16 (128 KiB for Llama-3-8B)

    def ready_tokens(self) -> int:
        """Tokens the next launch would run right now: one per decoding slot
        plus the pending prefill, capped at the token budget."""
        act = self._big_active()
        if not act.any():
            return 0
        plen, pref = self.s_plen[act], self.s_pref[act]
        return min(self.step_budget(), int((pref >= plen).sum()) + int((plen - pref).clip(min=0).sum()))

    def step_budget(self) -> int:
        """Tokens the next step may carry: ``token_budget``, or the realtime
        cap while a realtime-lane request is active (at least one more than
        the decode rows, which every step must carry)."""
        cap = self.rt_step_tokens
        if cap <= 0 or cap >= self.token_budget or not self.active:
            return self.token_budget
        act = self.s_active
        if not (act & (self.s_tier < self.fast_tiers)).any():
            return self.token_budget
        dec = int((self.s_pref[act] >= self.s_plen[act]).sum())
        return max(cap, dec + 1)

    def lane_capacity(self) -> int:
        """Slots a realtime request may take beyond ``admit_capacity``: every
        free (or parked) slot, plus the free micro-pool slots.  Its prefill
        goes first in the next step (or into the next micro-forward), so it
        starts computing there instead of waiting for headroom."""
        return len(self.free) + len(self.conv_lru) + len(self.free_micro)

    def _to_micro(self, r: Request) -> bool:
        """Serve ``r`` on the micro pool: a realtime request, a free micro
        slot, and no resident KV of its dialog in the serving pool (a
        resident turn stays where its context is)."""
        return (self.micro and 0 <= r.tier < self.fast_tiers and bool(self.free_micro)
                and not (r.conv >= 0 and r.conv in self.conv_lru))

    def admit(self, reqs: Sequence[Request]) -> List[Request]:
        now = time.monotonic_ns()
        out = []
        cap = self.max_ctx - 1
        for r in reqs:
            micro = self._to_micro(r)
            if not micro and not self.free and not self.conv_lru:
                if self.micro:
                    continue                                  # (a later realtime request may still fit)
                break
            if r.max_tokens > 0:
                r.gen_tokens = min(int(r.gen_tokens), int(r.max_tokens))   # (the request's own count from here on)
            if r.gen_tokens < 1:
                r.gen_tokens = 1
            plen = max(1, min(len(r.prompt), cap - r.gen_tokens + 1))
            r.prompt = np.asarray(r.prompt[:plen], dtype=np.int64) % self.cfg.vocab
            if len(r.prompt) == 0:
                r.prompt = np.zeros(1, dtype=np.int64)
            n_own = len(r.prompt)                             # (before any replay is prepended)
            r.micro = micro
            r.aborted = False
            r.out_tokens = None
            r.out_logprobs = r.out_top_ids = r.out_top_logprobs = None
            r.finish_reason = ""
            r.stop_entry = -1
            base = 0
            s = self.conv_lru.pop(r.conv, None) if (r.conv >= 0 and not micro) else None
            if micro:
                # a micro-pool slot keeps no dialog KV: the turn replays its
                # history (``r.history``) and nothing is parked afterwards
                s = self.free_micro.pop()
            elif s is not None:
                base = int(self.s_cached[s])
                if r.history is not None and base < len(r.history):
                    # a stale copy: this GPU served an earlier turn, later turns
                    # ran elsewhere -- attending over it would drop them
                    base = 0
                    self.kv_stale += 1
                if base + len(r.prompt) + r.gen_tokens > cap + 1:
                    base = 0                                  # context window full: restart the dialog KV
            else:
                s = self._take_slot()
            if base == 0 and ((r.history is not None and len(r.history)) or (r.prefix is not None and len(r.prefix))):
                # not resident here: replay the dialog -- its compressed
                # context (if a window was evicted), then the most recent
                # history tokens that fit
                room = cap + 1 - r.gen_tokens - len(r.prompt)
                if room > 0:
                    pre = np.asarray(r.prefix if r.prefix is not None else (), dtype=np.int64)[:room // 4]
                    hist = np.asarray(r.history if r.history is not None else (), dtype=np.int64)
                    keep = room - len(pre)
                    h = hist[len(hist) - keep:] if 0 < keep < len(hist) else (hist if keep > 0 else hist[:0])
                    r.prompt = np.concatenate([pre % self.cfg.vocab, h % self.cfg.vocab, r.prompt])
                    self.replay_tokens += len(pre) + len(h)
                    self.replay_nonzero += int(np.count_nonzero(pre)) + int(np.count_nonzero(h))
            r.slot = s
            r.reused = base
            r.prefilled = 0
            r.generated = 0
            r.out_idx = r.out_step = -1
            r.admitted_ns = now
            r.deadline_ns = now + int(r.timeout_ns) if r.timeout_ns > 0 else 0
            self.s_deadline[s] = r.deadline_ns
            self.active[s] = r
            n = len(r.prompt)
            self.s_prompt[s, base:base + n] = r.prompt
            self.s_plen[s] = base + n
            self.s_pref[s] = base
            self.s_gen[s] = 0
            self.s_gmax[s] = r.gen_tokens
            if r.temperature:
                t = float(r.temperature)
                self.s_temp[s] = t if (t > 0 and math.isfinite(t)) else 0.0
                self.s_seed[s] = int(r.seed) & 0xFFFFFFFFFFFFFFFF
            else:
                self.s_temp[s] = 0.0
            # truncation is active only on a slot that samples
            on = self.s_temp[s] > 0
            self.s_topk[s] = max(0, int(r.top_k)) if on else 0
            tp = float(r.top_p)
            self.s_topp[s] = tp if (on and 0.0 < tp < 1.0) else 1.0
            # log-probabilities: greedy slots too
            self.s_logp[s] = self.scores_logprobs and int(r.logprobs) >= 0
            if self.s_logp[s] and self.h_lp is None:
                self.h_lp = np.zeros((self.n_all, self.max_ctx), dtype=np.float32)
                self.h_top_ids = np.zeros((self.n_all, self.max_ctx, LP_TOP), dtype=np.int32)
                self.h_top_lp = np.zeros((self.n_all, self.max_ctx, LP_TOP), dtype=np.float32)
            # penalties, greedy slots too; a value off its range is off
            self.s_pen[s] = False
            if (r.presence_penalty or r.frequency_penalty or r.repetition_penalty != 1.0) and self.runs_model:
                pv = np.array([r.presence_penalty, r.frequency_penalty, r.repetition_penalty], dtype=np.float32)
                if np.isfinite(pv).all() and pv[2] > 0:
                    self.s_penp[s] = pv
                    self.s_pen[s] = bool(pv[0] != 0 or pv[1] != 0 or pv[2] != 1)
                    self.s_pfrom[s] = base + n - n_own
            # min_p: a sampling slot only; a value that rounds to 0 permille is off
            # (nothing to reset before the first request that names one of the three)
            named = bool(r.min_p) or r.allowed is not None or r.logit_bias is not None
            if named:
                self._eligibility_seen = True
            if self._eligibility_seen:
                self.s_minp[s] = -np.inf
                self.s_edit[s] = False
            if on and r.min_p:
                mp = float(r.min_p)
                if math.isfinite(mp) and 0.0 < mp <= 1.0:
                    self.s_minp[s] = min_p_log(mp)
            # allow-list and logit bias, greedy slots too: at most LE_MAX
            # entries each, ids that fit an int32 (any other id is outside
            # every vocabulary), finite non-zero bias values
            if named and (r.allowed is not None or r.logit_bias is not None) and self.runs_model:
                al = np.asarray(r.allowed if r.allowed is not None else (), dtype=np.int64).reshape(-1)[:LE_MAX]
                bi, bv = r.logit_bias if r.logit_bias is not None else ((), ())
                bi = np.asarray(bi, dtype=np.int64).reshape(-1)
                bv = np.asarray(bv, dtype=np.float32).reshape(-1)[:len(bi)]
                ok = np.isfinite(bv) & (bv != 0)
                bi, bv = bi[:len(bv)][ok][:LE_MAX], bv[ok][:LE_MAX]
                na, nb = len(al), len(bi)
                if na or nb:
                    if self.h_eids is None:
                        self.h_eids = np.zeros((self.n_all, 2 * LE_MAX), dtype=np.int32)
                        self.h_evals = np.zeros((self.n_all, 2 * LE_MAX), dtype=np.float32)
                    i32 = lambda v: np.where((v >= 0) & (v < 1 << 31), v, -1).astype(np.int32)   # noqa: E731
                    self.h_eids[s, :na] = i32(al)
                    self.h_eids[s, na:na + nb] = i32(bi)
                    self.h_evals[s, :na] = 0
                    self.h_evals[s, na:na + nb] = bv
                    self.s_ecnt[s] = (na, nb)
                    self.s_edit[s] = True
            # stop entries, greedy slots too: at most STOP_ENTRIES of 1..STOP_LEN
            # tokens (any other is dropped); an id that fits no int32 is outside
            # every vocabulary and never matches
            if self.h_stop is not None:
                self.s_stop[s] = self.s_shist[s] = False
            if r.stop and self.runs_model:
                ent = [np.asarray(e, dtype=np.int64).reshape(-1) for e in r.stop]
                ent = [e for e in ent if 1 <= len(e) <= STOP_LEN][:STOP_ENTRIES]
                if ent:
                    if self.h_stop is None:
                        self.h_stop = np.zeros((self.n_all, STOP_ENTRIES, STOP_ENT_WORDS), dtype=np.int32)
                        ring = max(2, self.max_inflight)
                        self._stop_pins = [self._alloc_pin(4 * self.n_all).view(torch.int32) for _ in range(ring)]
                        if self.micro:
                            self._stop_pins_m = [self._alloc_pin(4 * self.micro_slots).view(torch.int32)
                                                 for _ in range(self.micro_inflight + 1)]
                    tab = self.h_stop[s]
                    tab[:] = 0
                    for i, e in enumerate(ent):
                        tab[i, 0] = len(e)
                        tab[i, 1:1 + len(e)] = np.where((e >= 0) & (e < 1 << 31), e, -1)
                    self.s_nstop[s] = len(ent)
                    self.s_mintok[s] = min(max(int(r.min_tokens), 0), int(r.gen_tokens))
                    self.s_stop[s] = True
                    self.s_shist[s] = bool((tab[:len(ent), 0] > 1).any())
            if (self.s_pen[s] or (self.h_stop is not None and self.s_shist[s])) and self.d_hist is None:
                # the device-side token history, indexed [slot][absolute
                # position] (``penalty_kernels.h``).  Not filled: a fill would
                # be queued on this call's stream and nothing orders it with
                # the records on the pools' streams.  None is needed, and no
                # synchronisation beyond stream order: a slot's new occupant
                # records every position of its window, in forwards of the
                # slot's own pool and stream, before the first head that reads
                # it; nothing outside a window is ever read, and the micro
                # pool has slots and a stream of its own
                self.d_hist = torch.empty((self.n_all, self.max_ctx), dtype=torch.int32, device=self.device)
            # prefill order key: realtime-lane tiers sort before everything else
            self.s_seq[s] = self._admit_seq - (1 << 48 if 0 <= r.tier < self.fast_tiers else 0)
            r.seq_key = int(self.s_seq[s])
            self._admit_seq += 1
            self.s_active[s] = True
            self.s_tier[s] = r.tier
            self.s_conv[s] = -1 if micro else r.conv
            self.kv_reused_tokens += base
            if not micro:                                     # (the serving steps' headroom estimate)
                self._mean_plen += 0.01 * (n - self._mean_plen)
            out.append(r)
        return out

    # ------------------------------------------------------------------ abort (timeout / cancel)
    def _abort_slots(self, slots) -> List[Request]:
        """Take the active requests of ``slots`` out of the batch: their slots
        return to the free list for the NEXT launch.  Steps already queued on
        the GPU still compute their rows; a request admitted into the slot
        afterwards is prefilled by a later step on the same stream, so stream
        order keeps it from reading anything the aborted request wrote.  The
        aborted turn's KV is partial, so it is never parked for reuse."""
        out = []
        for s in slots:
            s = int(s)
            r = self.active.pop(s, None)
            if r is None:
                continue
            self.s_active[s] = False
            self.s_deadline[s] = 0
            self.s_conv[s] = -1
            self.s_cached[s] = 0
            # reused first (``_take_slot`` pops from the end)
            (self.free_micro if self.s_micro[s] else self.free).append(s)
            # steps still queued on the GPU list it among their first tokens:
            # their reap must not stamp an attempt that no longer exists
            r.aborted = True
            out.append(r)
        return out

    def expire(self, now_ns: Optional[int] = None) -> List[Request]:
        """Abort every active request whose processing deadline
        (``Request.timeout_ns`` after admission) has passed; returns them so
        the caller can retry or dead-letter them.  Requests whose last token
        is already launched completed at that launch and are not touched."""
        if not self.active:
            return []
        now = time.monotonic_ns() if now_ns is None else int(now_ns)
        d = self.s_deadline
        hit = np.flatnonzero(self.s_active & (d > 0) & (d < now))
        if not len(hit):
            return []
        out = self._abort_slots(hit)
        self.expired_total += len(out)
        return out

    def cancel(self, req_ids: Sequence[int]) -> List[Request]:
        """Abort the active requests with these ids (``DELETE
        /api/v1/messages/{id}`` on a request in flight); returns the ones
        found (a request that completed or was never admitted is not)."""
        want = {int(x) for x in req_ids}
        if not want or not self.active:
            return []
        out = self._abort_slots([s for s, r in self.active.items() if r.req_id in want])
        self.cancelled_total += len(out)
        return out

    # ------------------------------------------------------------------ step
    def _build(self, micro: bool = False):
        """Vectorised batch construction over the per-slot state arrays of
        one pool (the serving slots, or with ``micro`` the realtime micro
        pool): decode rows first (one token per generating slot, ids gathered
        on the device from the pool's previous step output), then chunked
        prefill in admission order up to the step's token budget.  Returns
        int32 arrays."""
        if self.micro:
            act = np.flatnonzero(self.s_active & (self.s_micro if micro else ~self.s_micro))
        else:
            act = np.flatnonzero(self.s_active)
        plen, pref = self.s_plen[act], self.s_pref[act]
        is_dec = pref >= plen
        dec = act[is_dec]
        D = len(dec)
        prev = (self.micro_id if micro else self.step_id) - 1
        if D and (self.s_out_step[dec] != prev).any():
            raise RuntimeError("decode token source is not the previous step")
        pre = act[~is_dec]
        if len(pre):
            pre = pre[np.argsort(self.s_seq[pre], kind="stable")]
        rem = self.s_plen[pre] - self.s_pref[pre]
        budget = (self.micro_budget if micro else self.step_budget()) - D
        before = np.cumsum(rem) - rem
        take = np.clip(budget - before, 0, rem)
        keep = take > 0
        pre, take = pre[keep], take[keep]
        n_pre = int(take.sum())
        T = D + n_pre
        a0 = self.s_pref[pre]
        # prefill token rows: slot pre[i] contributes prompt[a0:a0+take]
        start = D + np.cumsum(take) - take                   # first row of each chunk
        rep = np.repeat(np.arange(len(pre)), take)
        off = np.arange(n_pre) - (start[rep] - D) if n_pre else np.zeros(0, np.int64)
        p_slot = pre[rep]
        p_pos = a0[rep] + off
        toks = np.zeros(T, dtype=np.int32)
        pos = np.empty(T, dtype=np.int32)
        slot = np.empty(T, dtype=np.int32)
        d_pos = self.s_plen[dec] + self.s_gen[dec] - 1
        pos[:D] = d_pos
        slot[:D] = dec
        if n_pre:
            toks[D:] = self.s_prompt[p_slot, p_pos]
            pos[D:] = p_pos
            slot[D:] = p_slot
        fin = a0 + take >= self.s_plen[pre]                   # chunk completes the prompt
        samp = np.concatenate([np.arange(D), (start + take - 1)[fin]]).astype(np.int32)
        samp_slots = np.concatenate([dec, pre[fin]])
        dec_rows = np.arange(D, dtype=np.int32)
        dec_src = self.s_out_idx[dec].astype(np.int32)
        # attention tiles: decode rows are 1-token tiles; chunks cut at 16
        nt = (take + 15) // 16
        trep = np.repeat(np.arange(len(pre)), nt)
        toff = (np.arange(int(nt.sum())) - np.repeat(np.cumsum(nt) - nt, nt)) * 16
        tiles = np.empty((D + len(trep), 4), dtype=np.int32)
        tiles[:D, 0] = dec_rows
        tiles[:D, 1] = 1
        tiles[:D, 2] = dec
        tiles[:D, 3] = d_pos
        if len(trep):
            tiles[D:, 0] = start[trep] + toff
            tiles[D:, 1] = np.minimum(16, take[trep] - toff)
            tiles[D:, 2] = pre[trep]
            tiles[D:, 3] = a0[trep] + toff
        self.s_pref[pre] += take
        return toks, pos, slot, samp, samp_slots, dec_rows, dec_src, tiles, n_pre, D

    def warm_shapes(self, sizes: Optional[Sequence[int]] = None) -> int:
        """Run one throw-away forward at every token count a cold start can
        produce, before serving.

        A saturated warm-up only ever runs ~token_budget-token steps; the
        first SMALL step afterwards (a gateway going idle -> busy, or the first
        requests after start) used to pay the one-time GEMM kernel selection /
        code-object load of small-M shapes -- measured at ~135 ms for the
        first T = 1 forward of the 8B stub (``bench/cold_shapes.py``,
        ``profiles/r2_cold_shapes.md``) -- on live requests.  Every T in
        1..32 is run (lm_head rows = T), then a geometric ladder up to the
        token budget.  Must be called on an idle engine (uses scratch rows of
        free slots; nothing it writes is ever read by a request)."""
        if not self.cuda:
            return 0
        if self.active or self.conv_lru or self._q or self._qm:
            raise RuntimeError("warm_shapes needs an idle engine")
        if sizes is None:
            ladder, t = [], 48
            while t < self.token_budget:
                ladder.append(t)
                t = t * 3 // 2
            sizes = list(range(1, 33)) + ladder + [self.token_budget]
        dev = self.device
        n = 0
        with self.stream_ctx():
            for T in sizes:
                T = int(min(max(1, T), self.token_budget))
                r = torch.arange(T, device=dev, dtype=torch.int32)
                seg = min(16, self.max_ctx)
                slot = (r // seg) % self.slots
                pos = r % seg
                t0 = torch.arange(0, T, seg, device=dev, dtype=torch.int32)
                tiles = torch.stack([t0, torch.clamp(T - t0, max=seg), (t0 // seg) % self.slots,
                                     torch.zeros_like(t0)], 1).contiguous() if self.use_tiles else None
                samp = torch.arange(min(T, self.slots), device=dev, dtype=torch.long)
                self.model.forward(torch.zeros(T, dtype=torch.long, device=dev), pos.contiguous(),
                                   slot.contiguous(), samp, tiles=tiles, n_dec=0)
                n += 1
            if getattr(self.model, "prune_last", False) and hasattr(self.model, "warm_tail"):
                # the pruned last layer runs at the sampled-row count: a finer ladder
                tail, t = list(range(1, 33)), 32
                while t < self.token_budget:
                    t = max(t + 1, t * 9 // 8)
                    tail.append(min(t, self.token_budget))
                n += self.model.warm_tail(tail)
        if self.rt_stream is not None:
            # the micro-forwards' stream: its per-stream GEMM workspaces and
            # first launches there, on the micro pool's own slots
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(self.rt_stream):
                T = 1
                while T <= self.micro_budget:
                    r = torch.arange(T, device=dev, dtype=torch.int32)
                    slot = (self.slots + r % self.micro_slots).to(torch.int32)
                    pos = (r // self.micro_slots).to(torch.int32)
                    tiles = torch.stack([r, torch.ones_like(r), slot, pos], 1).contiguous() \
                        if self.use_tiles else None
                    samp = torch.arange(min(T, self.micro_slots), device=dev, dtype=torch.long)
                    self._micro_forward(torch.zeros(T, dtype=torch.long, device=dev), pos.contiguous(),
                                        slot.contiguous(), samp, tiles, 0)
                    n += 1
                    T *= 2
        if self.micro_graph:
            n += self._capture_micro_graphs()
        torch.cuda.synchronize(dev)
        self.warmed_shapes = n
        return n

    def _launch_micro_graph(self, Tb: int, t0: float, t_mono: int, pos, slot, samp_slots, dec_src) -> bool:
        """A decode-only micro-forward of D <= Tb rows as a replay of bucket
        Tb's graph: one staging copy, the decode-id gather from the previous
        micro-forward's output, the replay, the id copy back.  Rows D.. Tb
        stay on the scratch slot."""
        graph, g_in, g_tok, out = self._mg[Tb]
        D = len(pos)
        buf = np.empty(7 * Tb, dtype=np.int32)
        buf[:Tb] = 0
        buf[:D] = pos
        buf[Tb:2 * Tb] = self.scratch_slot
        buf[Tb:Tb + D] = slot
        til = buf[2 * Tb:6 * Tb].reshape(Tb, 4)
        til[:, 0] = np.arange(Tb)
        til[:, 1] = 1
        til[:, 2] = buf[Tb:2 * Tb]
        til[:, 3] = buf[:Tb]
        buf[6 * Tb:6 * Tb + D] = dec_src
        buf[6 * Tb + D:] = 0
        sid = self.micro_id
        k = sid % len(self._pins_m)
        pin = self._pins_m[k]
        pin.numpy()[:buf.nbytes] = buf.view(np.uint8)
        host_out = self._out_pins_m[k]
        prev = self._prev_out_m
        with torch.cuda.stream(self.rt_stream):
            g_in.copy_(pin[:buf.nbytes].view(torch.int32), non_blocking=True)
            g_tok[:D] = prev.index_select(0, g_in[6 * Tb:6 * Tb + D].long()).long()
            if D < Tb:
                g_tok[D:] = 0
            ev0 = self._start_event()
            te = time.perf_counter_ns()
            graph.replay()
            self.host_ns[2] += time.perf_counter_ns() - te
            host_out[:D].copy_(out[:D], non_blocking=True)
            ev = self._end_event(D, ev0 is not None)
        return self._retire(sid, D, 0, D, D, samp_slots, out, host_out, ev, ev0, t0, t_mono, True, graph=True)

    def _micro_forward(self, tok, pos, slot, samp, tiles, n_dec: int, graph: bool = False, **skw):
        """Issue one micro-forward on the current stream: the model's small
        GEMMs sized for ``micro_cus`` CUs, or, with ``micro_gemm = "rocblas"``,
        rocBLAS.  ``rocblas`` applies to eager micro-forwards only: the
        captured graphs (``graph``: the capture and its two warm-ups) always
        hold the hand-written kernels, so graph-replayed decode steps run
        those whatever ``micro_gemm`` says.  ``micro_weights = "fp8"``: every
        micro-forward, eager or captured, reads the quantised layer weights."""
        if self.micro_weights == "fp8":
            skw["quant"] = True
        if self.micro_cus and self.micro_gemm == "rocblas" and not graph:
            with _blas("cublas"):
                return self.model.forward(tok, pos, slot, samp, tiles=tiles, n_dec=n_dec, **skw)
        if self.micro_cus:
            skw["small_cus"] = self.micro_cus
        return self.model.forward(tok, pos, slot, samp, tiles=tiles, n_dec=n_dec, **skw)

    def _capture_micro_graphs(self) -> int:
        """Capture the decode-only micro-forward once per row bucket on the
        micro stream (after ``warm_shapes`` ran it eagerly: workspaces and
        first launches exist).  Static inputs per bucket: int32 [pos | slot |
        tiles (4 per row) | gather rows] and the int64 token ids; every row
        starts on the scratch slot at position 0, so a replay's padding rows
        write and read only that slot."""
        dev, rt = self.device, self.rt_stream
        pool = torch.cuda.graph_pool_handle()
        n = 0
        for Tb in self.MICRO_GRAPH_BUCKETS:
            if Tb > max(self.MICRO_GRAPH_BUCKETS[0], self.micro_slots):
                break
            g_in = torch.zeros(6 * Tb + Tb, dtype=torch.int32, device=dev)
            g_tok = torch.zeros(Tb, dtype=torch.long, device=dev)
            pos, slot = g_in[:Tb], g_in[Tb:2 * Tb]
            til = g_in[2 * Tb:6 * Tb].view(Tb, 4)
            slot.fill_(self.scratch_slot)
            til[:, 0] = torch.arange(Tb, device=dev, dtype=torch.int32)
            til[:, 1] = 1
            til[:, 2] = self.scratch_slot
            samp = torch.arange(Tb, device=dev, dtype=torch.long)
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(rt):
                for _ in range(2):
                    self._micro_forward(g_tok, pos, slot, samp, til, Tb, graph=True)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, pool=pool, stream=rt, capture_error_mode="thread_local"):
                out = self._micro_forward(g_tok, pos, slot, samp, til, Tb, graph=True)
            torch.cuda.synchronize(dev)
            self._mg[Tb] = (graph, g_in, g_tok, out)
            n += 1
        return n

    def inject(self, **fault) -> None:
        """Fault injection: ``fail_launch=n``, ``slow_ms=x``, ``drop_heartbeat=True``
        (0/False clears one)."""
        for k, v in fault.items():
            if k not in ("fail_launch", "slow_ms", "drop_heartbeat"):
                raise ValueError(f"unknown fault {k!r}")
            if v:
                self.fault[k] = v
            else:
                self.fault.pop(k, None)

    def fence(self, events) -> None:
        """Device events the next launch waits for (work that may still write
        slots this engine is about to reuse: evacuated steps, abandoned KV
        imports)."""
        self._fence.extend(e for e in events if e is not None)

    def abort_all(self) -> List[Request]:
        """Evacuate: drop every queued step and active request (slots are
        freed) and return the unfinished requests so the caller can re-route
        them.  Steps not yet reaped by ``finish`` count as unfinished (their
        completions were never reported): at-least-once.  Makes no GPU call,
        so it is safe after a device error; reap first if the GPU is fine."""
        steps = list(self._q) + self._reaped + list(self._qm) + self._reaped_m
        out = [r for f in steps for r in f.completed]
        out += list(self.active.values())
        for r in out:
            r.aborted = True
        # steps still queued on the GPU keep reading their pinned staging
        # buffers (the async H2D copy may not have run yet): the next launch
        # must not refill a buffer before they finish, so their events stay
        # as a fence (waited in launch; a dead device raises there instead)
        self._fence.extend(f.event for f in list(self._q) + list(self._qm) if f.event is not None)
        self._q.clear()
        self._reaped = []
        self._prev_out = None
        self._qm.clear()
        self._reaped_m = []
        self._prev_out_m = None
        self.active.clear()
        self.s_active[:] = False
        self.s_deadline[:] = 0
        self.conv_lru.clear()
        self._importing.clear()
        self.s_conv[:] = -1
        self.free = list(range(self.slots - 1, -1, -1))
        self.free_micro = list(range(self.slots + self.micro_slots - 1, self.slots - 1, -1))
        return out

    def launch(self, wait_cb=None) -> None:
        """Build the next token batch and enqueue its forward (async).

        If ``max_inflight`` steps are already queued, wait for the oldest;
        with ``wait_cb`` the wait polls the step's event and calls
        ``wait_cb()`` in between (the gateway keeps ingesting/dispatching
        while the GPU computes) instead of blocking."""
        if self.fault:
            if self.fault.get("fail_launch", 0) > 0:
                self.fault["fail_launch"] -= 1
                if self.fault["fail_launch"] <= 0:
                    del self.fault["fail_launch"]
                raise RuntimeError("HIP error: out of memory (injected fault)")
            if self.fault.get("slow_ms"):
                time.sleep(self.fault["slow_ms"] / 1e3)
        ts = time.perf_counter_ns()
        if self._fence:                                # steps dropped by abort_all still in flight
            for ev in self._fence:
                ev.synchronize()
            self._fence = []
        while len(self._q) >= self.max_inflight:       # bound the run-ahead (and staging reuse)
            if wait_cb is None:
                self._reaped.append(self._reap(block=True))  # handed to the next finish()
                continue
            f = self._reap(block=False)
            if f is not None:
                self._reaped.append(f)
                continue
            if self.micro:
                self.pump_micro()                      # realtime micro-forwards keep flowing meanwhile
            if not wait_cb():
                time.sleep(0.0002)
        self.host_ns[1] += time.perf_counter_ns() - ts
        self._launch_pool(False)

    def close(self) -> None:
        """Drain the GPU work of this engine.  The CU-partition streams
        (``micro_stream=partition``) are process-wide and stay alive
        (``cu_partition.partition_streams``): tensors this engine allocated
        on them may outlive it, and freeing one returns its block to the
        stream it was allocated on."""
        if self.cuda:
            torch.cuda.synchronize(self.device)

    def stream_ctx(self):
        """Context that makes the serving steps' stream current (a no-op
        unless the chip is CU-partitioned): anything else ordered with the
        serving steps -- KV imports, the slot census -- runs inside it."""
        return torch.cuda.stream(self.main_stream) if self.main_stream is not None else _NullCtx()

    def _launch_pool(self, micro: bool) -> bool:
        """Build one pool's next token batch and enqueue its forward: the
        serving step, or (``micro``) a realtime micro-forward on the micro
        stream.  False if the pool had no token to run."""
        t0 = time.perf_counter()
        tb = time.perf_counter_ns()
        t_mono = time.monotonic_ns()
        toks, pos, slot, samp, samp_slots, dec_rows, dec_src, tiles, n_pre, n_dec = self._build(micro)
        self.host_ns[0] += time.perf_counter_ns() - tb
        T = len(toks)
        if T == 0:
            return False
        dev = self.device
        S, D, NT = len(samp), len(dec_rows), len(tiles)
        # a step with a sampling row (temperature > 0) ends in the sampling
        # head; an all-greedy step is the call (and the staging buffer) it
        # always was.  The captured micro graphs hold the greedy head: a
        # decode micro-forward with a sampling row takes the eager path.
        temp = self.s_temp[samp_slots]
        sampling = bool(S) and bool((temp > 0).any())
        # rows that ask for log-probabilities, greedy or sampling: scored again
        # on their own path (``logprob_head``).  The captured graphs hold no
        # such path either
        lrows = np.flatnonzero(self.s_logp[samp_slots]) if S else np.zeros(0, dtype=np.int64)
        L = len(lrows)
        # penalised slots: every token row of theirs in this forward is recorded
        # in the device history, and their sampled rows are drawn again on
        # their own path (``penalised_head``), greedy rows first.  Eager in the
        # micro pool as well.  A row that also truncates leaves ``trunc``
        # (and so are the token rows of slots that hold a stop entry longer
        # than one token: ``stop_match`` reads their generated tokens there)
        if self.d_hist is None:
            qrows = np.zeros(0, dtype=np.int64)
        elif self.h_stop is not None:
            qrows = np.flatnonzero(self.s_pen[slot] | self.s_shist[slot])
        else:
            qrows = np.flatnonzero(self.s_pen[slot])
        Q = len(qrows)
        # sampled rows with stop entries: compared after the head's last
        # overwrite (``stop_match``), the result read when the step is reaped.
        # Eager in the micro pool as well.  ``max_tokens`` alone needs none of it
        srows = np.flatnonzero(self.s_stop[samp_slots]) if (self.h_stop is not None and S) \
            else np.zeros(0, dtype=np.int64)
        RS = len(srows)
        # Slots with an allow-list or a logit bias take the same path, their
        # penalty off (a span whose slot is -1: no history is read, and none
        # is recorded for them)
        if self.h_eids is not None and S:
            edit = self.s_edit[samp_slots]
            prows = np.flatnonzero(edit | self.s_pen[samp_slots] if Q else edit)
        else:
            edit = None
            prows = np.flatnonzero(self.s_pen[samp_slots]) if (Q and S) else np.zeros(0, dtype=np.int64)
        P = len(prows)
        n_greedy = 0
        if P:
            hot = temp[prows] > 0
            n_greedy = int(P - hot.sum())
            prows = np.concatenate([prows[~hot], prows[hot]])
        if micro and self._mg and n_pre == 0 and D == T and self._prev_out_m is not None and not sampling and not L \
                and not Q and not P and not RS:
            Tb = next((b for b in self.MICRO_GRAPH_BUCKETS if b >= T and b in self._mg), 0)
            if Tb:
                return self._launch_micro_graph(Tb, t0, t_mono, pos, slot, samp_slots, dec_src)
        Sp = row_scale_len(S) if sampling else 0
        # rows that also ask for top-k / top-p / min_p (RM: one of them asks for min_p)
        if sampling:
            minp = self.s_minp[samp_slots]
            by_m = minp > -np.inf
            keep = ~self.s_pen[samp_slots] if edit is None else ~(self.s_pen[samp_slots] | edit)
            trows = np.flatnonzero((temp > 0) & ((self.s_topk[samp_slots] > 0) | (self.s_topp[samp_slots] < 1) | by_m)
                                   & keep)
        else:
            trows = ()
        R = len(trows)
        RM = R if (R and by_m[trows].any()) else 0
        # edited rows (E: one of the P rows has an allow-list, a bias or,
        # penalised, a min_p; N: the words of their lists)
        E = N = 0
        if P:
            ps = samp_slots[prows]
            pm = self.s_minp[ps]
            if edit is not None and edit[prows].any():
                ec = np.where(self.s_edit[ps][:, None], self.s_ecnt[ps], 0)
                en = ec.sum(axis=1)
                N = int(en.sum())
            E = P if (N or (pm > -np.inf).any()) else 0
        NS = 0
        if RS:
            st_slots = samp_slots[srows]
            st_cnt = self.s_nstop[st_slots].astype(np.int64)
            NS = int(st_cnt.sum())
        # the step's staging buffer, one copy to the device.  A block a step
        # does not use is empty: the buffer is then what it is without the feature
        lay = _Staging(
            ("tok", T), ("pos", T), ("slot", T), ("samp", S), ("dec_rows", D), ("dec_src", D), ("tiles", 4 * NT),
            # sampling rows: 1 / T and the row keys of the S sampled rows, both
            # whole 256-row tiles long and 16-byte aligned on the device (the
            # epilogue's vector loads)
            ("inv_temp", Sp, 4), ("keys", 2 * Sp),
            ("trunc_rows", R), ("trunc_k", R), ("trunc_p", R), ("trunc_minp", RM),
            ("logp", L),
            # per penalised row its index, span (slot, from, split, end),
            # parameters, top_k and top_p, then the token rows to record
            ("pen_rows", P), ("pen_spans", 4 * P), ("pen_params", 3 * P), ("pen_k", P), ("pen_p", P), ("record", Q),
            # per edited row log(min_p) and the span (allow_off, n_allow,
            # bias_off, n_bias), then the N ids and the N values of the rows' lists
            ("edit_minp", E), ("edit_spans", 4 * E), ("edit_ids", N), ("edit_vals", N),
            # per stop row its index and record (slot, gen_from, end,
            # min_tokens, ent_off, n_ent), then the rows' entries, packed
            ("stop_rows", RS), ("stop_records", STOP_ROW_WORDS * RS), ("stop_entries", STOP_ENT_WORDS * NS))
        h = lay.host
        h("tok")[:] = toks
        h("pos")[:] = pos
        h("slot")[:] = slot
        h("samp")[:] = samp
        h("dec_rows")[:] = dec_rows
        h("dec_src")[:] = dec_src
        h("tiles")[:] = tiles.reshape(-1)
        if sampling:
            it = h("inv_temp", f32=True)
            it[:S] = inv_temperature(temp)
            it[S:] = 0
            kk = h("keys", (Sp, 2))
            kk[:S] = row_keys(self.s_seed[samp_slots], self.s_gen[samp_slots]).view(np.int32)
            kk[S:] = 0
        if R:
            h("trunc_rows")[:] = trows
            h("trunc_k")[:] = self.s_topk[samp_slots[trows]]
            h("trunc_p", f32=True)[:] = self.s_topp[samp_slots[trows]]
            if RM:
                h("trunc_minp", f32=True)[:] = minp[trows]
        if L:
            h("logp")[:] = lrows
        if P:
            h("pen_rows")[:] = prows
            sp = h("pen_spans", (P, 4))
            sp[:, 0] = np.where(self.s_pen[ps], ps, -1)
            sp[:, 1] = self.s_pfrom[ps]
            sp[:, 2] = self.s_plen[ps]
            sp[:, 3] = self.s_plen[ps] + self.s_gen[ps]
            h("pen_params", (P, 3), f32=True)[:] = self.s_penp[ps]
            h("pen_k")[:] = self.s_topk[ps]
            h("pen_p", f32=True)[:] = self.s_topp[ps]
        if Q:
            h("record")[:] = qrows
        if E:
            h("edit_minp", f32=True)[:] = pm
            es = h("edit_spans", (E, 4))
            es[:] = 0
            if N:
                off = np.cumsum(en) - en
                es[:, 0] = off
                es[:, 1] = ec[:, 0]
                es[:, 2] = off + ec[:, 0]
                es[:, 3] = ec[:, 1]
                e_ids, e_vals = h("edit_ids"), h("edit_vals", f32=True)
                for i in np.flatnonzero(en):
                    a, n = int(off[i]), int(en[i])
                    e_ids[a:a + n] = self.h_eids[ps[i], :n]
                    e_vals[a:a + n] = self.h_evals[ps[i], :n]
        if RS:
            h("stop_rows")[:] = srows
            rec = h("stop_records", (RS, STOP_ROW_WORDS))
            rec[:, 0] = np.where(self.s_shist[st_slots], st_slots, -1)
            rec[:, 1] = self.s_plen[st_slots]
            rec[:, 2] = self.s_plen[st_slots] + self.s_gen[st_slots]
            rec[:, 3] = self.s_mintok[st_slots]
            rec[:, 4] = np.cumsum(st_cnt) - st_cnt
            rec[:, 5] = st_cnt
            # (the rows' first ``st_cnt`` entries, row by row: the order the offsets count)
            h("stop_entries", (NS, STOP_ENT_WORDS))[:] = \
                self.h_stop[st_slots][np.arange(STOP_ENTRIES)[None, :] < st_cnt[:, None]]
        nbytes = lay.buf.nbytes
        sid = self.micro_id if micro else self.step_id
        pins, outs = (self._pins_m, self._out_pins_m) if micro else (self._pins, self._out_pins)
        host_lp = (self._lp_pins_m if micro else self._lp_pins)[sid % len(pins)] if L else None
        host_stop = (self._stop_pins_m if micro else self._stop_pins)[sid % len(pins)] if RS else None
        # (the requests of those rows and their slots' admission keys, as this launch sees them)
        stop_reqs = ([self.active[x] for x in st_slots.tolist()], self.s_seq[st_slots]) if RS else None
        k = sid % len(pins)
        pin = pins[k]
        if pin.numel() < nbytes:
            pin = pins[k] = self._alloc_pin(2 * nbytes)
        pin.numpy()[:nbytes] = lay.buf.view(np.uint8)
        host_out = outs[k]
        prev = self._prev_out_m if micro else self._prev_out
        stream = self.rt_stream if micro else self.main_stream
        ctx = torch.cuda.stream(stream) if stream is not None else _NullCtx()
        with ctx:
            lay.dbuf = pin[:nbytes].to(dev, non_blocking=True).view(torch.int32)
            d = lay.dev
            tok_d = d("tok").long()
            if D:
                if prev is None:
                    raise RuntimeError("decode token without a previous step output")
                tok_d.index_copy_(0, d("dec_rows").long(), prev.index_select(0, d("dec_src").long()).long())
            til = d("tiles", (NT, 4)) if self.use_tiles else None
            skw = {}
            if sampling:
                skw = {"inv_temp": d("inv_temp", f32=True), "keys": d("keys", (Sp, 2))}
                self.sampled_steps += 1
                if R:
                    skw["trunc"] = Truncate(d("trunc_rows").long(), d("trunc_k"), d("trunc_p", f32=True),
                                            d("trunc_minp", f32=True) if RM else None)
                    self.truncated_steps += 1
            if L:
                skw["logp"] = d("logp").long()
                self.logprob_steps += 1
            if Q or P:
                ed = LogitEdit(d("edit_ids"), d("edit_vals", f32=True), d("edit_spans", (E, 4))) if N else None
                skw["pen"] = Penalise(self.d_hist, d("record"), d("pen_rows").long(), d("pen_spans", (P, 4)),
                                      d("pen_params", (P, 3), f32=True), d("pen_k"), d("pen_p", f32=True), n_greedy,
                                      ed, d("edit_minp", f32=True) if E else None)
                self.edited_steps += int(N > 0)
                self.penalised_steps += int(P > 0)
            if RS:
                skw["stop"] = Stops(self.d_hist, None, d("stop_rows").long(), d("stop_records", (RS, STOP_ROW_WORDS)),
                                    d("stop_entries", (NS, STOP_ENT_WORDS)))
                self.stop_steps += 1
            ev0 = self._start_event()
            te = time.perf_counter_ns()
            fwd = self._micro_forward if micro else self.model.forward
            out = fwd(tok_d, d("pos"), d("slot"), d("samp").long(), tiles=til, n_dec=D, **skw)
            if L or RS:                                # (a ``HeadOut``: the tokens alone otherwise)
                out, lp, ids, flags = out.tokens, out.lp, out.ids, out.stop_flags
            self.host_ns[2] += time.perf_counter_ns() - te
            if not micro:
                self._census(T)
            # the sampled ids come back behind the forward (read at reap)
            host_out[:S].copy_(out, non_blocking=True)
            if L:
                host_lp[0][:L].copy_(lp, non_blocking=True)
                host_lp[1][:L].copy_(ids, non_blocking=True)
            if RS:
                host_stop[:RS].copy_(flags, non_blocking=True)
            ev = self._end_event(T, ev0 is not None)
        return self._retire(sid, T, n_pre, n_dec, S, samp_slots, out, host_out, ev, ev0, t0, t_mono, micro,
                            lp_rows=lrows if L else None, host_lp=host_lp, stop_rows=srows if RS else None,
                            host_stop=host_stop, stop_reqs=stop_reqs)

    def _retire(self, sid: int, T: int, n_pre: int, n_dec: int, S: int, ss, out, host_out, ev, ev0,
                t0: float, t_mono: int, micro: bool, graph: bool = False, lp_rows=None, host_lp=None,
                stop_rows=None, host_stop=None, stop_reqs=None) -> bool:
        """The deterministic bookkeeping behind every enqueued forward (a
        serving step, an eager micro-forward or a graph replay): every sampled
        slot gets one token, finished requests leave their slots, and the
        step joins its pool's in-flight queue."""
        gidx = self.s_gen[ss].copy()
        self.s_gen[ss] += 1
        self.s_out_idx[ss] = np.arange(len(ss))
        self.s_out_step[ss] = sid
        g = self.s_gen[ss]
        firsts = [self.active[int(x)] for x in ss[g == 1]]
        done = ss[g >= self.s_gmax[ss]]
        completed = []
        for x in done.tolist():
            r = self.active.pop(x)
            completed.append(r)
            self._leave_slot(x, r, int(self.s_gen[x]))
        self.s_active[done] = False
        f = _Inflight(sid, ev, T, n_pre, n_dec, completed, firsts, t0, out, t_mono, ev0, micro=micro,
                      samp_slots=ss, gidx=gidx, host_out=host_out, lp_rows=lp_rows, host_lp=host_lp,
                      stop_rows=stop_rows, host_stop=host_stop, stop_reqs=stop_reqs)
        if micro:
            self._prev_out_m = out
            self._qm.append(f)
            self.micro_id += 1
            self.micro_steps += 1
            self.micro_graph_steps += int(graph)
        else:
            self._prev_out = out
            self._q.append(f)
            self.step_id += 1
        self.total_tokens += T
        self.matmul_flops += self._step_flops(T, S)
        self.completed_total += len(completed)
        self.completed_tokens += sum(len(r.prompt) + r.gen_tokens - 1 for r in completed)
        return True

    def _leave_slot(self, x: int, r: Request, generated: int) -> None:
        """Request ``r`` (already out of ``active``) completes in slot ``x``
        after ``generated`` tokens: the slot is freed, or parked with the
        dialog's KV."""
        r.prefilled = int(self.s_plen[x]) - r.reused
        r.generated = generated
        if self.s_micro[x]:
            # a micro slot never parks dialog KV (conv_lru holds serving slots only): always freed
            self.s_conv[x] = -1
            self.free_micro.append(x)
        elif r.conv >= 0:
            # park the dialog KV: every position but the last sampled token
            self.s_cached[x] = self.s_plen[x] + generated - 1
            old = self.conv_lru.pop(r.conv, None)
            if old is not None and old != x:           # a stale copy elsewhere: free it
                self.s_conv[old] = -1
                self.free.append(old)
            self.conv_lru[r.conv] = x
        else:
            self.s_conv[x] = -1
            self.free.append(x)

    def _reap_stops(self, f: _Inflight) -> None:
        """Act on a reaped step's stop results.  The bookkeeping of a step is
        decided at launch and a stop is known only now, up to ``max_inflight``
        steps later, so for each row that matched an entry and whose request
        has no stop recorded yet (steps of a pool are reaped in launch order:
        the first match wins):
          * the request still holds its slot: it completes here, into this
            step's ``completed``, cut after the matched token.  The slot is
            free (or parked) for the NEXT launch; steps already queued still
            compute its rows -- their tokens are dropped here
            (``stop_dropped_rows``) -- and stream order keeps a new occupant,
            prefilled by a later step on the same stream, from reading
            anything they write, exactly as ``_abort_slots`` argues.  Their
            ids land in ``h_tokens`` rows of the slot before any id of the
            new occupant does (reaps are FIFO), which rewrites every row it
            reads;
          * a later launch already completed it at its full length: that
            step's reap delivers it, and its outputs are cut there to the
            length recorded here (``r.generated``); the tokens counted at
            that launch are corrected, and so is the parked context if the
            slot is still parked as that request left it.  The gateway
            admits a conversation's next turn only once the previous turn's
            completion has been delivered -- it is reported by the later
            step's reap, after this one -- so no next turn can have been
            admitted in between; an engine-level caller that admits one
            sooner is detected by the slot's admission key and keeps the
            uncut context (every position of it was computed)."""
        reqs, keys = f.stop_reqs
        slots = f.samp_slots[f.stop_rows]
        # rows of a request whose stop an earlier step recorded (admission keys
        # are unique, so the slot's last stop is that of the row's own request)
        late = self.s_stopkey[slots] == keys
        self.stop_dropped_rows += int(late.sum())
        flags = f.host_stop.numpy()[:len(reqs)]
        for i in np.flatnonzero((flags >= 0) & ~late).tolist():
            r = reqs[i]
            if r.seq_key != int(keys[i]) or r.aborted:     # (an attempt that was aborted, or admitted again since)
                continue
            k, x = int(flags[i]), int(slots[i])
            gi = int(f.gidx[f.stop_rows[i]])
            r.finish_reason = "stop"
            r.stop_entry = k
            self.s_stopkey[x] = r.seq_key
            self.stopped_total += 1
            if self.active.get(x) is r:
                del self.active[x]
                self.s_active[x] = False
                self._leave_slot(x, r, gi + 1)
                f.completed.append(r)
                self.completed_total += 1
                self.completed_tokens += len(r.prompt) + gi
            else:
                self.completed_tokens -= r.generated - (gi + 1)
                r.generated = gi + 1
                if r.conv >= 0 and not self.s_micro[x] and self.conv_lru.get(r.conv) == x \
                        and int(self.s_seq[x]) == r.seq_key and not self.s_active[x]:
                    self.s_cached[x] = self.s_plen[x] + gi

    def _step_flops(self, T: int, S: int) -> int:
        """Matrix-multiply FLOPs of one forward of ``T`` tokens sampling ``S``
        rows: every layer's qkv / o / gate-up / down over every row (the last
        layer's o + MLP over the sampled rows only, with ``prune_last``) and
        the LM head over the sampled rows.  Attention (<= max_ctx keys per
        row, ~0.2 % at the serving shape) is not counted."""
        c = self.cfg
        d, hd = c.dim, c.head_dim
        qkv = d * (c.heads + 2 * c.kv_heads) * hd
        rest = c.heads * hd * d + 3 * d * c.ffn                 # o + gate/up + down
        last = S if getattr(self.model, "prune_last", False) else T
        return 2 * (T * (c.layers * qkv + (c.layers - 1) * rest) + last * rest + S * c.vocab * d)

    # ------------------------------------------------------------------ realtime micro-forwards
    def micro_pending(self) -> bool:
        """A micro-pool request still has tokens no launched micro-forward
        computes (prefill left, or generation not yet launched to the end)."""
        if not self.micro or len(self.free_micro) == self.micro_slots:
            return False
        act = self.s_active & self.s_micro
        return bool(act.any())

    def pump_micro(self) -> int:
        """Reap finished micro-forwards (their results go to the next
        ``finish`` / ``finish_micro``) and launch the next ones while the
        micro pool has work and fewer than ``micro_inflight`` are queued.
        Bookkeeping is deterministic (greedy decode always yields a token),
        so a realtime request's whole prefill + decode chain can be queued
        at once: each micro-forward gathers its decode ids on the device from
        the previous one.  Returns the number launched."""
        if not self.micro:
            return 0
        while self._qm:
            f = self._reap(block=False, micro=True)
            if f is None:
                break
            self._reaped_m.append(f)
        n = 0
        while len(self._qm) < self.micro_inflight and self.micro_pending():
            if not self._launch_pool(True):
                break
            n += 1
        return n

    def finish_micro(self) -> StepResult:
        """Results of the micro-forwards reaped so far (non-blocking)."""
        done, self._reaped_m = self._reaped_m, []
        return self._result(done)

    def _start_event(self):
        """Timing event before a forward (``time_steps``), or None."""
        if self.cuda and self.time_steps:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record()
            return ev0
        return None

    def _end_event(self, T: int, timing: bool):
        """Completion event of the forward just enqueued (None: the step ran
        synchronously on the host)."""
        if not self.cuda:
            return None
        ev = torch.cuda.Event(enable_timing=timing)
        ev.record()
        return ev

    def _check_hung(self, f: _Inflight) -> None:
        if self.step_timeout_s > 0 and f.t0_ns and \
                time.monotonic_ns() - f.t0_ns > self.step_timeout_s * 1e9:
            raise BackendHung(f"forward step {f.step} ({f.T} tokens) incomplete "
                              f"{(time.monotonic_ns() - f.t0_ns) / 1e9:.1f} s after launch")

    def _reap(self, block: bool, micro: bool = False) -> Optional[_Inflight]:
        q = self._qm if micro else self._q
        if not q:
            return None
        f = q[0]
        if f.event is not None:
            if block:
                if self.step_timeout_s > 0:
                    while not f.event.query():         # bounded: a hung GPU surfaces as BackendHung
                        self._check_hung(f)
                        time.sleep(0.0001)
                else:
                    f.event.synchronize()
            elif not f.event.query():
                self._check_hung(f)
                return None
        q.popleft()
        now = time.monotonic_ns()
        if f.ev_start is not None:
            ms = f.ev_start.elapsed_time(f.event)
            if micro:
                self.micro_gpu_ms += ms
                self.micro_timed += 1
            else:
                self.gpu_step_ms += ms
                self.gpu_steps += 1
                self.gpu_step_max_ms = max(self.gpu_step_max_ms, ms)
        if self.tracer is not None:
            self.tracer.step(f.step, f.t0_ns, now, f.T)
        if f.host_out is not None and f.samp_slots is not None and len(f.samp_slots):
            # the step's sampled ids (valid now: the copy ran before its event)
            ss = f.samp_slots
            ok = f.gidx < self.max_ctx
            self.h_tokens[ss[ok], f.gidx[ok]] = f.host_out.numpy()[:len(ss)][ok]
            if f.lp_rows is not None:
                # ... and the scored rows' log-probabilities, under the same guard
                keep = ok[f.lp_rows]
                rows = f.lp_rows[keep]
                lp = f.host_lp[0].numpy()[:len(keep)][keep]
                self.h_lp[ss[rows], f.gidx[rows]] = lp[:, 0]
                self.h_top_lp[ss[rows], f.gidx[rows]] = lp[:, 1:]
                self.h_top_ids[ss[rows], f.gidx[rows]] = f.host_lp[1].numpy()[:len(keep)][keep]
        if f.stop_reqs is not None:
            self._reap_stops(f)
        for r in f.firsts:
            if not r.aborted:
                r.first_token_ns = now
        for r in f.completed:
            r.done_ns = now
            if not r.finish_reason:
                r.finish_reason = "length"
            r.out_tokens = self.h_tokens[r.slot, :min(r.generated, self.max_ctx)].copy()
            if r.logprobs >= 0 and self.h_lp is not None:
                n = len(r.out_tokens)
                r.out_logprobs = self.h_lp[r.slot, :n].copy()
                r.out_top_ids = self.h_top_ids[r.slot, :n].copy()
                r.out_top_logprobs = self.h_top_lp[r.slot, :n].copy()
        if self.page is not None and not self.cuda and not self.fault.get("drop_heartbeat") and not micro:
            self.page.write_host(self.inflight(), self.free_slots(), f.T, f.step)
        return f

    def queued_steps(self) -> int:
        """Forward steps launched and not yet reaped (serving steps and
        realtime micro-forwards)."""
        return len(self._q) + len(self._qm)

    def poll_one(self) -> bool:
        """Reap the oldest queued step if the GPU finished it (non-blocking);
        its results are returned by the next ``finish``."""
        f = self._reap(block=False)
        if f is None:
            if self._qm:
                return self.pump_micro() > 0 or bool(self._reaped_m)
            return False
        self._reaped.append(f)
        return True

    @staticmethod
    def _result(done: List[_Inflight]) -> StepResult:
        comp = [r for f in done for r in f.completed]
        firsts = [r for f in done for r in f.firsts]
        return StepResult(sum(f.T for f in done), sum(f.n_pre for f in done), sum(f.n_dec for f in done),
                          comp, firsts, (time.perf_counter() - done[0].t0) * 1e3 if done else 0.0)

    def finish(self, block: bool = False) -> StepResult:
        """Reap finished steps (and micro-forwards).  Non-blocking unless
        ``block`` (then waits for every queued one)."""
        done: List[_Inflight] = self._reaped
        self._reaped = []
        while self._q:
            f = self._reap(block=block)
            if f is None:
                break
            done.append(f)
        if self.micro:
            while True:
                self.pump_micro()
                done.extend(self._reaped_m)
                self._reaped_m = []
                if not block or not (self._qm or self.micro_pending()):
                    break
                f = self._reap(block=True, micro=True)
                if f is not None:
                    done.append(f)
        return self._result(done)

    def step(self) -> StepResult:
        """Synchronous step: launch + wait."""
        self.launch()
        return self.finish(block=True)

    def sync(self) -> None:
        self.finish(block=True)

    # ------------------------------------------------------------------ N9 page
    def _census(self, tokens: int) -> None:
        if self.page is None or not self.cuda or self.page.dev_ptr is None or self.fault.get("drop_heartbeat"):
            return
        pin = self._state_pins[self.step_id % 2]
        st = pin.numpy().view(np.int32)
        st[:] = 0
        if self.active:
            a = np.fromiter(self.active.keys(), dtype=np.int64)
            st[a[a < self.slots]] = 1                      # (the serving pool's census)
        self._slot_state_d.copy_(pin.view(torch.int32), non_blocking=True)
        from .. import _native
        _native.require_hipops().slot_census(self._slot_state_d.data_ptr(), self.slots, int(tokens),
                                             int(self.step_id) & 0xFFFFFFFF, self.page.dev_ptr,
                                             torch.cuda.current_stream(self.device).cuda_stream)

    def drain(self, max_steps: int = 10000) -> List[Request]:
        out = []
        for _ in range(max_steps):
            if not self.active:
                break
            out.extend(self.step().completed)
        out.extend(self.finish(block=True).completed)
        return out
