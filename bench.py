#!/usr/bin/env python3
"""Headline benchmark: gateway requests/s at a fixed p99 enqueue->dispatch
latency, 4-tier mix (10/30/40/20), Poisson arrivals, 1 MI355X backend per
process (Llama-3-8B-shaped stub, random bf16 weights) -- BASELINE.json's
metric/config.

    python bench.py                       # 1 GPU, defaults
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one gateway tick on every rank: ingest the requests that
arrived (Poisson clock), GPU-preprocess them (text_analyze + MFMA
classifier), push into the native 4-tier queue, dispatch into free backend
batch slots (multi-GPU: all_gather of load vectors + all_to_all of request
descriptors through the node-local shared-memory control plane, KV
migration on the RCCL data group; a GPU that is ahead of its peers may run
one extra local forward instead of idling at the exchange), and run one full
32-layer continuous-batching forward (chunked prefill + decode) on the
backend.

Calibration (untimed, inside the warmup phase): the backend is driven in
saturation to measure its service capacity C (req/s); the timed phase then
offers Poisson load at ``--util`` x C per GPU (weak scaling) and reports the
dispatched requests/s over exactly K timed steps, bracketed by barrier +
torch.cuda.synchronize(), max wall time over ranks.  p99 latency is measured
from each request's Poisson ARRIVAL time (so ingest wait + preprocess + queue
time all count) to the moment a backend slot admits it; the pure
enqueue->dispatch p99 is reported too.

A plain run serves one timed window at ``--util`` and reports it.  ``--full``
adds what the headline figure does not need: the SLO search (further windows
at the ``--slo-climb`` / ``--slo-backoff`` utilisations; the headline is then
the best window that held the operating point) and the secondary null-backend
gateway measurement.  ``--dump-outputs DIR`` writes the outputs of one fixed,
seeded batch served after the timed steps (``dump_outputs``).
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

import numpy as np

from llm_message_queue_amd.utils.harness import comm_evidence, lockstep_report, self_launch

BASELINE_RPS = 10000.0          # "sustain > 10,000 req/s" (reference docs target)
P99_TARGET_MS = 500.0           # BASELINE.md operating point (all tiers)
REALTIME_P99_TARGET_MS = 100.0  # BASELINE.md operating point (realtime tier)
METRIC = "requests/sec + p99 enqueue->dispatch latency, 4-tier mix at 1/2/4/8 backends"


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--slots", type=int, default=1536)
    ap.add_argument("--max-ctx", type=int, default=512)
    ap.add_argument("--token-budget", type=int, default=4096)
    ap.add_argument("--token-budget-by-rank", default="",
                    help="lock-step experiments: per-rank token budget overrides, e.g. '1:2048' (rank 1 takes "
                         "half-size steps)")
    ap.add_argument("--realtime-step-tokens", type=int, default=0,
                    help="cap a step at this many tokens while a realtime request is in the batch (A/B of "
                         "backend.realtime_step_tokens; 0 = off)")
    ap.add_argument("--realtime-mode", default="", choices=["", "off", "cap", "micro"],
                    help="how realtime requests are served (backend.realtime_mode): off = in the serving steps, "
                         "cap = --realtime-step-tokens, micro = realtime micro-forwards over their own slot pool on "
                         "their own stream; '' = cap if --realtime-step-tokens > 0 else off")
    ap.add_argument("--micro-slots", type=int, default=96, help="micro mode: KV slots of the realtime pool")
    ap.add_argument("--micro-inflight", type=int, default=1, help="micro mode: micro-forwards queued ahead")
    ap.add_argument("--micro-budget", type=int, default=512, help="micro mode: tokens per micro-forward")
    ap.add_argument("--micro-stream", default="partition", choices=["high", "same", "partition"],
                    help="micro mode: a high-priority HIP stream of their own, the serving stream, or a CU "
                         "partition of the chip of their own (--micro-cus; the serving steps get the rest)")
    ap.add_argument("--micro-cus", type=int, default=64, help="micro partition: CUs of the realtime partition")
    ap.add_argument("--no-micro-graph", action="store_true",
                    help="micro mode: launch decode micro-forwards kernel by kernel instead of replaying HIP graphs")
    ap.add_argument("--gen-tokens", type=int, default=4)
    ap.add_argument("--inflight", type=int, default=2, help="forward steps queued ahead on the GPU")
    ap.add_argument("--aging-ms", default="50,100,150,200",
                    help="per-tier aging deadlines (realtime,high,normal,low), ms")
    ap.add_argument("--prompt-cap", type=int, default=32)
    ap.add_argument("--util", type=float, default=0.98,
                    help="offered load as a fraction of the calibrated capacity.  0.98 keeps every tier's p99 "
                         "arrival->dispatch well inside the targets on one GPU and on the 8-rank simulated node "
                         "(profiles/r4_sim_breakdown.jsonl).  1.0 also holds the operating point on one GPU "
                         "(profiles/r4_util_ab_1gpu.jsonl: 5,512 vs 5,424-5,431 req/s, realtime p99 10-15 ms, all "
                         "tiers <= 86 ms) but lifts the 8-rank sim's all-tier p99 to 165-242 ms; the SLO search "
                         "below re-serves at lower utilisations if a window misses the operating point")
    ap.add_argument("--slo-backoff", default="0.98,0.95,0.9,0.85,0.75",
                    help="--full: utilisations re-served (in order, same process) when the window at --util misses the "
                         "operating point; value = req/s at the highest one that held it (0 if none did)")
    ap.add_argument("--slo-climb", default="1.0,1.02,1.04",
                    help="--full: utilisations tried next (in order, same process) while the window at --util and every "
                         "later one HOLD the operating point; the headline is the best window that held it.  '' = "
                         "no climb (VERDICT r4 weak #4: a search that only backs off caps the headline below what "
                         "the SLO allows)")
    ap.add_argument("--slo-budget-s", type=float, default=150.0,
                    help="wall-time bound of the SLO search: no further window starts once the search has used "
                         "this long minus one window's duration")
    ap.add_argument("--test-miss-above-util", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--steady-ticks", type=int, default=-1,
                    help="untimed serving ticks at the offered rate before the timed window, so it starts in "
                         "steady state (-1 = max(60, 4 x --warmup))")
    ap.add_argument("--tick-ms", type=float, default=0.0, help="minimum serving tick period (0 = dynamic)")
    ap.add_argument("--rate", type=float, default=0.0, help="per-GPU offered req/s (0 = calibrate)")
    ap.add_argument("--no-classifier", action="store_true")
    ap.add_argument("--no-residual-gemm", action="store_true",
                    help="o/down as F.linear + fused residual-add RMSNorm (default: residual in the GEMM epilogue)")
    ap.add_argument("--no-row-scale", action="store_true",
                    help="fused GEMMs read rmsnorm'd rows instead of raw rows + a per-row scale (A/B)")
    ap.add_argument("--no-fused-head", action="store_true",
                    help="LM head on hipBLASLt + torch.argmax instead of the GEMM with the argmax epilogue")
    ap.add_argument("--fused-resid", action="store_true",
                    help="o / down projections on the hand-written residual-add GEMM epilogue (the default; "
                         "kept for the A/B scripts)")
    ap.add_argument("--no-fused-resid", action="store_true",
                    help="A/B: o / down projections on hipBLASLt beta = 1")
    ap.add_argument("--fused-rms", action="store_true",
                    help="A/B: the RMSNorm row scales from the residual GEMM's epilogue instead of a separate "
                         "row_rms pass (default off: profiles/r5_resid_rms_bench.jsonl)")
    ap.add_argument("--resid-epi", default="lds", choices=["regs", "lds", "pre"],
                    help="the fused residual tile through registers (GM_EPI_RESID), staged into LDS by DMA "
                         "(GM_EPI_RESID_LDS, default) or with its first quarter prefetched (GM_EPI_RESID_PRE)")
    ap.add_argument("--no-fused-qkv", action="store_true",
                    help="qkv on hipBLASLt + rope_kv instead of the GEMM with the RoPE/KV epilogue (A/B)")
    ap.add_argument("--no-fused-mlp", action="store_true",
                    help="gate/up on hipBLASLt + silu_mul instead of the hand-written SwiGLU GEMM (A/B)")
    ap.add_argument("--library-gemm", action="store_true",
                    help="hipBLASLt for the sub-wave o / down projections and small LM heads (round-5 routing); "
                         "default: every GEMM on the hand-written kernels (skinny below 65 rows, split-K where "
                         "whole tiles leave CUs idle)")
    ap.add_argument("--no-library-gemm", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-prune-last", action="store_true",
                    help="run the last layer's o projection and MLP on every row (A/B; default: sampled rows only)")
    ap.add_argument("--split-qkv", action="store_true",
                    help="q and kv as two GEMMs into one buffer (bench/qkv_split.py; default: one fused QKV GEMM)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json-out", default="")
    ap.add_argument("--trace-out", default="", help="Chrome trace of sampled requests + backend steps (timed phase)")
    ap.add_argument("--trace-sample", type=int, default=20, help="trace every Nth completed request")
    ap.add_argument("--cpu-dry-run", action="store_true",
                    help="rehearse the multi-rank control flow on CPU (gloo, tiny model); not a measurement")
    ap.add_argument("--sim-gpu", default="",
                    help="with --cpu-dry-run: per-rank relative GPU speeds, e.g. '1,0.97,1.02' (cycled over "
                         "ranks); each rank's backend is a SimEngine (the engine's host side for real, the 8B "
                         "forward as a simulated device clock) at the serving config's slots / token budget -- "
                         "for studying multi-GPU dynamics (lock-step vs GPU speed spread) without the GPUs")
    ap.add_argument("--pin-cpu", action="store_true",
                    help="with --cpu-dry-run: pin rank r to CPU core r (mod the core count) -- CPU-rehearsal "
                         "hygiene for --sim-gpu runs; on GPUs: the same as --cpu-bind gpu")
    ap.add_argument("--cpu-bind", default="auto", choices=["auto", "gpu", "core", "off"],
                    help="host placement of each rank (parallel/placement.py): gpu = the physical cores of its "
                         "GPU's socket (sysfs local_cpulist), split evenly among the ranks on that socket, for "
                         "every thread of the rank and its front-door feeder; auto = gpu when the job has more "
                         "than one rank (a one-GPU run stays as launched); core = rank r -> core r; off")
    ap.add_argument("--no-extra-steps", action="store_true",
                    help="multi-rank A/B: never launch an extra local forward while the peers are still "
                         "behind at the per-tick exchange (pure lock-step)")
    ap.add_argument("--ingress", default="per-rank", choices=["per-rank", "rank0", "rank0-funnel"],
                    help="per-rank: every GPU process fronts its own Poisson stream (weak scaling, one ingress "
                         "per GPU); rank0: one front door for the job (the `cli serve` topology): a feeder "
                         "process writes N x the per-GPU rate as RAW records into ONE shared ring that every "
                         "rank drains, decodes and GPU-preprocesses; rank0-funnel: the r2 form, rank 0 "
                         "preprocesses the whole job's traffic on GPU 0 and the planner spreads it (A/B)")
    ap.add_argument("--door-share", default="fair", choices=["greedy", "fair"],
                    help="--ingress rank0: each pump takes everything the shared ring holds (greedy) or only up "
                         "to an even 1/world share of the ring's traffic (fair: ShmRing balanced pop, what "
                         "`cli serve`'s ring threads do)")
    ap.add_argument("--lb", default="least_connections",
                    choices=["round_robin", "least_connections", "weighted_random", "adaptive_load", "local_first"],
                    help="multi-GPU placement strategy (loadbalancer.algorithm)")
    ap.add_argument("--control-plane", default="shm", choices=["shm", "gloo", "nccl"],
                    help="per-tick load/descriptor exchange: host gloo group or RCCL on a side stream")
    ap.add_argument("--data-backend", default="", choices=["", "nccl", "gloo"],
                    help="data plane (KV migration): nccl = RCCL after a preflight (gloo fallback, flagged in "
                         "comm.data_backend), gloo; '' = nccl on GPUs, gloo in --cpu-dry-run")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the SLO search's further windows "
                         "(--slo-climb / --slo-backoff) and the secondary null-backend gateway measurement "
                         "(--gateway-only-s).  A plain run serves ONE window at --util")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, serve one fixed, seeded batch of requests through the same "
                         "preprocessor and backend and write what their caller receives (priorities, prompt token "
                         "ids, generated token ids) as DIR/<name>.npy -- the same arrays for the same arguments, "
                         "so two builds can be compared output for output")
    ap.add_argument("--dump-requests", type=int, default=256, help="--dump-outputs: requests of the fixed batch")
    ap.add_argument("--gateway-only-s", type=float, default=3.0,
                    help="with --full: seconds of the secondary null-backend gateway measurement (0 = skip)")
    ap.add_argument("--gateway-only-rate", type=float, default=50000.0)
    return ap.parse_args(argv)


class FrontDoorFeed:
    """``--ingress rank0``: the job's one front door.  A feeder process
    (``gateway/door_feed.py``, started by rank 0 before anything touches
    the GPU) writes every Poisson arrival, at its arrival time, as the RAW
    record the native HTTP ingress writes (arrival ns, id, JSON body --
    `csrc/ingress/http_ingress.cpp`) into ONE shared ring, and every rank
    drains it, decodes and GPU-preprocesses what it pops -- the topology of
    `cli serve` (its C++ front door feeds one MPMC ring all ranks drain).
    Until round 4 rank 0's own Python shipped the records round-robin into
    per-rank rings, so every rank-0 host stall delayed the whole job's
    arrivals (realtime p99 110 ms in that mode)."""

    RING_BYTES = 256 << 20

    def __init__(self, world: int, rank: int, job: str, seed: int, share: int = 1):
        import subprocess
        from llm_message_queue_amd import _native
        self.rank = rank
        self.share = share
        self.name = f"llmq-benchdoor-{job}-{os.environ.get('MASTER_PORT', '0')}"
        self._R = _native.shmring().ShmRing
        self.ring = None
        self.proc = None
        if rank == 0:
            self.ring = self._R(self.name, self.RING_BYTES, "create")
            self.proc = subprocess.Popen(
                [sys.executable, "-m", "llm_message_queue_amd.gateway.door_feed", "--ring", self.name,
                 "--ring-bytes", str(self.RING_BYTES), "--seed", str(seed)],
                cwd=os.path.dirname(os.path.abspath(__file__)), stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                text=True)
            self._cmd(None)                      # the pool is built: "ok 0"

    def _cmd(self, line):
        if self.proc is None:
            return
        if line is not None:
            self.proc.stdin.write(line + "\n")
            self.proc.stdin.flush()
        ack = self.proc.stdout.readline()
        if not ack.startswith("ok"):
            raise RuntimeError(f"front-door feeder: {ack!r}")

    def attach(self) -> None:
        if self.ring is None:
            self.ring = self._R(self.name, 0, "attach")

    def start(self, rate: float, t0: float) -> None:
        self._cmd(f"rate {rate!r} {t0!r}")

    def stop(self) -> None:
        self._cmd("stop")

    def receive(self):
        from llm_message_queue_amd.gateway.shm_bridge import decode_raw
        return [decode_raw(b) for _, b in self.ring.pop(4096, 0, self.share, self.rank if self.share > 1 else -1)]

    def backlog(self) -> int:
        return int(self.ring.size())

    def close(self) -> None:
        if self.proc is not None:
            self._cmd("exit")
            self.proc.wait(timeout=30)
            self.ring.unlink()
        self.ring.close()


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(a, engine, pre, use_gpu: bool) -> dict:
    """``--dump-outputs DIR``.  The timed steps serve Poisson arrivals on the
    wall clock, so no two runs form the same batches; what is written is
    therefore one more pass of the same path over a FIXED batch, after the
    timed steps and their drain (the engine is idle, its slots are free):
    ``--dump-requests`` messages of a seeded ``Workload`` go through the
    preprocessor the gateway ingests with (text_analyze + classifier + prompt
    token ids) and, admitted together, through the backend engine's forward
    steps until each has its ``--gen-tokens`` greedy tokens.  Written, one
    row per request in the order the workload made them: ``priority`` and
    ``prompt_len`` [n], ``prompt_ids`` [n, prompt_cap] (0-padded), and
    ``tokens`` [n, gen_tokens], the ids a caller reads from
    ``Request.out_tokens`` -- all float64, which holds every id exactly."""
    from llm_message_queue_amd.backend.engine import Request
    from llm_message_queue_amd.gateway.workload import Workload

    row_bytes = 8 * (2 + a.prompt_cap + a.gen_tokens)
    n = max(1, min(a.dump_requests, DUMP_MAX_BYTES // row_bytes, engine.free_slots()))
    msgs = Workload(seed=a.seed * 1000 + 424243).make(n)
    pre.process_batch(msgs, use_gpu=use_gpu, prompt_cap=a.prompt_cap)
    arrays = {"priority": np.array([int(m.priority) for m in msgs], dtype=np.float64),
              "prompt_len": np.zeros(n, dtype=np.float64),
              "prompt_ids": np.zeros((n, a.prompt_cap), dtype=np.float64)}
    reqs = []
    for i, m in enumerate(msgs):
        ids = np.asarray(m.prompt_ids if m.prompt_ids is not None else (), dtype=np.uint32)[:a.prompt_cap]
        arrays["prompt_len"][i] = len(ids)
        arrays["prompt_ids"][i, :len(ids)] = ids
        p = ids.astype(np.int64).astype(np.int32) if len(ids) else np.zeros(1, dtype=np.int32)
        reqs.append(Request(req_id=i, prompt=p, gen_tokens=a.gen_tokens, tier=2))
    if hasattr(engine, "model"):                 # (a SimEngine computes no tokens)
        admitted = engine.admit(reqs)
        if len(admitted) != n:
            raise RuntimeError(f"--dump-outputs: the idle engine admitted {len(admitted)} of {n} requests")
        done = engine.drain()
        if len(done) != n:
            raise RuntimeError(f"--dump-outputs: {len(done)} of {n} requests completed")
        tokens = np.zeros((n, a.gen_tokens), dtype=np.float64)
        for r in done:
            tokens[r.req_id, :len(r.out_tokens)] = r.out_tokens
        arrays["tokens"] = tokens
    os.makedirs(a.dump_outputs, exist_ok=True)
    for name, arr in arrays.items():
        np.save(os.path.join(a.dump_outputs, f"{name}.npy"), arr)
    return {"dir": a.dump_outputs, "requests": n, "arrays": {k: list(v.shape) for k, v in arrays.items()}}


def main(argv=None) -> int:
    a = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and a.gpus > 1:
        return self_launch(a, argv, __file__)
    if env_world is not None and int(env_world) != a.gpus:
        print(f"bench: --gpus {a.gpus} but the launcher started WORLD_SIZE={env_world} ranks; refusing to "
              "report a number for a different GPU count", file=sys.stderr, flush=True)
        return 3
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if a.pin_cpu and a.cpu_dry_run and hasattr(os, "sched_setaffinity"):
        cores = sorted(os.sched_getaffinity(0))
        os.sched_setaffinity(0, {cores[int(os.environ.get("LOCAL_RANK", rank)) % len(cores)]})
    # rank 0 starts the front-door feeder process before anything here
    # touches the GPU (a child process, never an exec)
    job = os.environ.get("TORCHELASTIC_RUN_ID", str(os.getpid() if world == 1 else "bench"))
    door = (FrontDoorFeed(world, rank, job, a.seed, share=world if a.door_share == "fair" else 1)
            if a.ingress == "rank0" and world > 1 else None)
    import torch

    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.backend.slot_page import SlotPage
    from llm_message_queue_amd.balancer.load_balancer import Endpoint, LoadBalancer
    from llm_message_queue_amd.gateway.router import STAGES, Gateway, LatencyRecorder, StageRecorder
    from llm_message_queue_amd.gateway.workload import PoissonArrivals, Workload
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    from llm_message_queue_amd.parallel.comm import init_from_env, local_device_index
    from llm_message_queue_amd.preprocess.preprocessor import Preprocessor
    from llm_message_queue_amd.utils.config import default_config

    local = int(os.environ.get("LOCAL_RANK", "0"))
    dry = a.cpu_dry_run
    from llm_message_queue_amd.ops import gemm as _G
    _G.RESID_EPI = {"regs": _G.EPI_RESID, "lds": _G.EPI_RESID_LDS, "pre": _G.EPI_RESID_PRE}[a.resid_epi]
    if dry:
        # CPU rehearsal of the exact control flow (collectives, tick counts,
        # reductions) with a tiny model and gloo -- never a measurement
        dev = torch.device("cpu")
        comm = init_from_env(backend=a.data_backend or "gloo",
                             control="gloo" if a.control_plane == "nccl" else a.control_plane)
        if not a.sim_gpu:
            a.model, a.slots, a.max_ctx, a.token_budget, a.prompt_cap = "tiny", 16, 64, 128, 16
    else:
        if not torch.cuda.is_available():
            print("bench.py needs a GPU (MI355X)", file=sys.stderr)
            return 2
        local = local_device_index()
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        # every thread of this rank (and rank 0's feeder process) on its GPU's
        # socket, before the serving threads start (they inherit it)
        from llm_message_queue_amd.parallel.placement import bind_rank
        binding = bind_rank("gpu" if a.pin_cpu else a.cpu_bind,
                            extra_pids=[door.proc.pid] if door is not None and door.proc is not None else ())
        comm = init_from_env(backend=a.data_backend or None, control=a.control_plane)
    comm_kind = "solo" if world == 1 else str(getattr(comm, "backend", a.control_plane))
    evidence = comm_evidence(comm, dev, world, dry, binding=None if dry else binding)

    def dsync():
        if not dry:
            torch.cuda.synchronize(dev)

    cfg = default_config()
    cfg.preprocessor.classifier = not a.no_classifier
    cfg.queue.enable_metrics = False
    # The reference's per-tier max_concurrent (100/200/500/1000, sized for its
    # 50-goroutine workers) would cap in-flight work far below the batch slots
    # of one GPU; in the bench each tier may use every slot of the job.
    # Aging deadlines (queue.levels[*].max_wait_time, the anti-starvation
    # knob) derived from the 500 ms p99 target instead of the reference's
    # defaults (1 s / 5 s / 30 s / 5 min): a tier whose oldest request waited
    # longer is served first, so strict priority cannot push the low tier's
    # tail past the SLO under Poisson bursts at high utilisation.
    aging_ms = [float(x) for x in a.aging_ms.split(",")]
    for lv, ms in zip(sorted(cfg.queue.levels, key=lambda lv: lv.priority), aging_ms):
        lv.max_concurrent = a.slots * world
        lv.max_wait_time = int(ms * 1e6)
    page = SlotPage(f"bench{job}", rank)
    budget = a.token_budget
    for item in filter(None, a.token_budget_by_rank.split(",")):
        r_, b_ = item.split(":")
        if int(r_) == rank:
            budget = int(b_)
    sim_speed = None
    if dry and a.sim_gpu:
        from llm_message_queue_amd.backend.sim_engine import SimEngine
        speeds = [float(x) for x in a.sim_gpu.split(",")]
        sim_speed = speeds[rank % len(speeds)]
        engine = SimEngine(speed=sim_speed, slots=a.slots, max_ctx=a.max_ctx, token_budget=budget,
                           max_inflight=a.inflight, page=page, gpu_index=rank, seed=1000 + rank)
    else:
        engine = BackendEngine(LlamaConfig.by_name(a.model), slots=a.slots, max_ctx=a.max_ctx,
                               token_budget=budget, device=dev, impl="ref" if dry else "hip", seed=1000 + rank,
                               page=page, gpu_index=rank, max_inflight=a.inflight,
                               residual_in_gemm=not a.no_residual_gemm, split_qkv=a.split_qkv,
                               fused_mlp=False if a.no_fused_mlp else None,
                               fused_qkv=False if a.no_fused_qkv else None, row_scale_norm=not a.no_row_scale,
                               fused_head=False if a.no_fused_head else None,
                               fused_resid=False if a.no_fused_resid else None,
                               fused_rms=True if a.fused_rms else None,
                               prune_last=not a.no_prune_last, realtime_step_tokens=a.realtime_step_tokens,
                               realtime_mode=a.realtime_mode, micro_slots=a.micro_slots,
                               micro_inflight=a.micro_inflight, micro_budget=a.micro_budget,
                               micro_stream=a.micro_stream, micro_cus=a.micro_cus,
                               library_gemm=a.library_gemm, micro_graph=not a.no_micro_graph)
    pre = Preprocessor(cfg.preprocessor, use_gpu=not dry, device=str(dev))
    lbcfg = cfg.loadbalancer
    lbcfg.algorithm = a.lb
    lbcfg.health_check_interval = 0
    lb = LoadBalancer(lbcfg)
    for j in range(world):          # every rank's balancer lists every GPU (cli serve does the same)
        lb.add_endpoint(Endpoint(id=f"gpu{j}", type="llm", gpu_index=j, page=page if j == rank else None,
                                 max_connections=a.slots))
    cfg.gpu.extra_steps = not a.no_extra_steps
    gw = Gateway(cfg, preprocessor=pre, engine=engine, comm=comm, load_balancer=lb,
                 use_gpu_preprocess=not dry, prompt_cap=a.prompt_cap, gen_tokens=a.gen_tokens)
    wl = Workload(seed=a.seed * 1000 + rank)
    # one throw-away forward per cold-start shape (small T / small lm_head
    # M): their one-time GEMM kernel selection must not land on live
    # requests when the gateway goes idle -> busy (engine.warm_shapes)
    warmed = engine.warm_shapes()

    def sync_all():
        dsync()
        comm.barrier()

    # ---------------------------------------------------------------- warmup + calibration
    # Saturation phase: keep 2x slots of work queued; measure the backend's
    # token throughput over the second half and convert it to requests/s with
    # the measured tokens per completed request (robust to the prefill/decode
    # waves a saturated start produces).
    # W untimed warm-up ticks (>= 20), then 60 measured saturated ticks; the
    # tick counts are fixed so every rank issues the same collectives
    w0 = max(a.warmup, 20)
    warm = w0 + 60
    t_c0 = None
    tok0 = rt0 = done0 = 0
    for i in range(warm):
        backlog = gw.pending() + engine.inflight()
        need = max(0, 2 * a.slots - backlog)
        if need:
            gw.submit(wl.make(need))
        gw.tick()
        if i == w0 - 1:
            dsync()
            t_c0 = time.perf_counter()
            tok0, rt0, done0 = engine.total_tokens, engine.completed_tokens, engine.completed_total
            gw.host_profile(reset=True)
            sat_eng0 = engine.host_ns.copy()
    dsync()
    t_c1 = time.perf_counter()
    n_sat = warm - w0
    host_sat = dict(gw.host_profile(), engine_build=round(float(engine.host_ns[0] - sat_eng0[0]) / n_sat / 1e6, 3),
                    engine_sync=round(float(engine.host_ns[1] - sat_eng0[1]) / n_sat / 1e6, 3),
                    engine_enqueue=round(float(engine.host_ns[2] - sat_eng0[2]) / n_sat / 1e6, 3),
                    tick_ms=round((t_c1 - t_c0) * 1e3 / n_sat, 3),
                    tokens_per_tick=round((engine.total_tokens - tok0) / n_sat, 1))
    tok_rate = (engine.total_tokens - tok0) / max(1e-9, t_c1 - t_c0)
    done = max(1, engine.completed_total - done0)
    tok_per_req = max(1.0, (engine.completed_tokens - rt0) / done)
    cap_local = tok_rate / tok_per_req
    caps = comm.all_gather_i64(np.array([int(cap_local * 1000)], dtype=np.int64))[:, 0] / 1000.0
    # job capacity per GPU = mean over ranks: the dispatch planner moves a
    # slower rank's excess to GPUs with free slots, so the job (not its
    # slowest member) is what the offered load is sized against
    capacity = float(np.mean(caps))
    # rank0 ingress: one front door takes the whole job's traffic
    front_door = a.ingress in ("rank0", "rank0-funnel")
    if door is not None:
        comm.barrier()                   # the ring exists (rank 0 made it) before the others attach
        door.attach()
    # drain the calibration backlog (untimed)
    gw.drop_pending()

    def busy_local():
        # the stop decision must be GLOBAL: every tick is a collective, so all
        # ranks have to run the same number of them
        return (engine.inflight() + engine.queued_steps() + len(gw.remote_out)
                + sum(len(v) for v in gw._done_owed.values()) + gw.pending() + gw.inbox_size()
                + gw.preprocessing()
                + gw.awaiting_kv()
                + (door.backlog() if door is not None else 0))

    def drain(pump_fn=None, cap_ticks=2000):
        busy = comm.all_gather_i64(np.array([busy_local()], dtype=np.int64))
        n = 0
        while busy.max() > 0 and n < cap_ticks:
            if pump_fn is not None:
                pump_fn()        # no new arrivals (rate 0); takes what the front door's rings still hold
            gw.tick()
            n += 1
            busy = comm.all_gather_i64(np.array([busy_local()], dtype=np.int64))
        return n

    drain()
    tick_s = a.tick_ms / 1e3
    clock = {"next_tick": 0.0}
    feed = {"arrivals": None}

    def pump():
        if door is not None:
            msgs = door.receive()
            if msgs:
                gw.submit(msgs)
            return
        arrivals = feed["arrivals"]
        due = arrivals.due(time.monotonic())
        if due:
            msgs = wl.make(len(due))
            for m, ts in zip(msgs, due):
                m.arrival_ns = int(ts * 1e9)
            gw.submit(msgs)

    def serve_tick():
        # Dynamic batching: ticks run back-to-back while there is work (a
        # busy forward is the batching window); while a launch waits for the
        # GPU the gateway keeps pulling arrivals through ``pump`` (ingest +
        # dispatch into free slots).  An idle gateway sleeps until the next
        # arrival.  --tick-ms > 0 adds a minimum tick period.
        arrivals = feed["arrivals"]
        now = time.monotonic()
        if tick_s > 0 and now < clock["next_tick"]:
            time.sleep(clock["next_tick"] - now)
        elif world == 1 and engine.inflight() == 0 and gw.pending() == 0 and arrivals.t_next is not None \
                and arrivals.t_next > now:
            time.sleep(min(arrivals.t_next - now, 0.05))
        clock["next_tick"] = max(clock["next_tick"] + tick_s, time.monotonic())
        pump()
        gw.tick(pump=pump)

    # A serving process keeps long-lived state (queues, slots, stores); a
    # full cyclic-GC pass over it is a multi-ms stall that lands on whatever
    # requests are waiting.  Freeze the warm heap and collect between runs.
    gc.collect()
    gc.freeze()
    gc.disable()
    steady = a.steady_ticks if a.steady_ticks >= 0 else max(60, 4 * a.warmup)

    def window(util: float, attempt: int) -> dict:
        """Serve Poisson load at ``util`` x the calibrated capacity: an
        untimed steady phase, then exactly ``a.steps`` timed ticks, then an
        untimed drain that accounts for every request.  The same number of
        collectives on every rank (each tick is one)."""
        rate = a.rate if a.rate > 0 else util * capacity
        # rank0: the feeder process offers world x rate into the shared ring;
        # rank0-funnel: rank 0's own clock does
        my_rate = 0.0 if door is not None else ((rate * world if rank == 0 else 0.0) if front_door else rate)
        arrivals = feed["arrivals"] = PoissonArrivals(my_rate, seed=a.seed * 1000 + rank + 7919 * attempt)
        gw.reset_latency()
        # ------------------------------------------------------------ steady state (untimed)
        # Serve the offered Poisson load for a fixed number of ticks so the
        # timed window starts with the queues, batch slots and prefill/decode
        # mix of a running system, not from the empty one a drain leaves.
        # The arrival clock keeps running into the timed window.
        c0 = {k: gw.counters[k] for k in ("submitted", "completed", "rejected", "expired")}
        sync_all()
        mono0 = time.monotonic()
        arrivals.reset(mono0)
        if door is not None:
            door.start(rate * world, mono0)
        clock["next_tick"] = mono0
        for _ in range(steady):
            serve_tick()
        gw.reset_latency()
        # ------------------------------------------------------------ timed
        gw.host_profile(reset=True)
        eng_host0 = engine.host_ns.copy()
        tracer = None
        if a.trace_out and attempt == 0:
            from llm_message_queue_amd.utils.tracing import RequestTracer
            tracer = RequestTracer(sample_every=a.trace_sample)
            gw.tracer = engine.tracer = tracer
        # the window edge's device synchronise must not stall live arrivals:
        # let the queued forwards finish while still ingesting/admitting, so
        # the synchronise itself finds an idle GPU
        gw.quiesce(pump)
        d0 = gw.counters["dispatched"]
        r0 = gw.counters["remote_sent"]
        x0 = gw.counters["extra_steps"]
        tok0 = engine.total_tokens
        fl0, ct0, cn0 = engine.matmul_flops, engine.completed_tokens, engine.completed_total
        ms0, mg0, mt0 = engine.micro_steps, engine.micro_gpu_ms, engine.micro_timed
        gw.lockstep_stats(reset=True)
        engine.gpu_step_ms, engine.gpu_steps, engine.gpu_step_max_ms = 0.0, 0, 0.0
        engine.time_steps = True
        sync_all()
        sub0 = gw.counters["submitted"]
        t0 = time.perf_counter()
        for _ in range(a.steps):
            serve_tick()
        # same at the closing edge: arrivals during the final device drain are
        # ingested and admitted, not left waiting behind the synchronise
        gw.quiesce(pump)
        sync_all()
        t1 = time.perf_counter()
        eng_host1 = engine.host_ns.copy()          # (the untimed drain below must not count)
        host_timed = gw.host_profile()
        engine.time_steps = False
        arrived_local = gw.counters["submitted"] - sub0
        # dispatches and backend tokens of the WINDOW (the untimed drain below
        # dispatches the requests still queued at t1; those must not count)
        dispatched_local = gw.counters["dispatched"] - d0
        tokens_local = engine.total_tokens - tok0
        work_local = [engine.matmul_flops - fl0, engine.completed_tokens - ct0, engine.completed_total - cn0,
                      engine.micro_steps - ms0, int((engine.micro_gpu_ms - mg0) * 1000), engine.micro_timed - mt0]
        remote_local = gw.counters["remote_sent"] - r0
        extra_local = gw.counters["extra_steps"] - x0
        if tracer is not None:
            gw.tracer = engine.tracer = None
            tracer.dump(a.trace_out if world == 1 else f"{a.trace_out}.rank{rank}")
        elapsed_local = t1 - t0
        # untimed: finish every request offered since the steady phase began
        # and account for all of them (served, rejected or shed -- none lost)
        arrivals.rate = 0.0
        if door is not None:
            door.stop()
        drain(pump)
        acct = comm.all_gather_i64(np.array([gw.counters[k] - c0[k] for k in ("submitted", "completed", "rejected",
                                                                              "expired")],
                                            dtype=np.int64)).sum(axis=0)
        agg = comm.all_gather_i64(np.array([int(elapsed_local * 1e9), dispatched_local, tokens_local,
                                            arrived_local], dtype=np.int64))
        elapsed = agg[:, 0].max() / 1e9
        work = comm.all_gather_i64(np.array(work_local, dtype=np.int64)).sum(axis=0)
        lockstep = lockstep_report(gw, engine, comm, elapsed)
        lockstep["ingested_by_rank"] = [int(v) for v in agg[:, 3].tolist()]   # requests each rank preprocessed
        # ... over the whole attempt (steady phase + timed window + drain): the
        # front door's balanced ring share evens THIS out (rank0 ingress)
        lockstep["ingested_total_by_rank"] = [int(v) for v in comm.all_gather_i64(
            np.array([gw.counters["submitted"] - c0["submitted"]], dtype=np.int64))[:, 0].tolist()]
        # extra forwards a rank launched while its peers were behind (Gateway._extra_local_step)
        lockstep["extra_steps_by_rank"] = [int(v) for v in
                                           comm.all_gather_i64(np.array([extra_local], dtype=np.int64))[:, 0].tolist()]
        remote_in_window = int(comm.all_gather_i64(np.array([remote_local], dtype=np.int64)).sum())
        dispatched = int(agg[:, 1].sum())
        tokens = int(agg[:, 2].sum())
        arrived = int(agg[:, 3].sum())
        arr = comm.all_gather_i64(gw.rec.arr.reshape(-1)).sum(axis=0).reshape(gw.rec.arr.shape)
        enq = comm.all_gather_i64(gw.rec.enq.reshape(-1)).sum(axis=0).reshape(gw.rec.enq.shape)
        lat = LatencyRecorder(len(gw.tiers)).summary(arr, enq)
        gw.flush_latency()
        arr_d = comm.all_gather_i64(gw.rec_done.arr.reshape(-1)).sum(axis=0).reshape(gw.rec_done.arr.shape)
        lat_done = LatencyRecorder(len(gw.tiers)).summary(arr_d, arr_d)
        # per-stage, per-tier attribution of arrival -> admission, job-wide
        # and per rank (where multi-rank latency goes: VERDICT r3 next #1)
        sh = gw.rec_stage.h
        st_h = comm.all_gather_i64(sh.reshape(-1)).reshape((world,) + sh.shape)
        sp = gw.rec_stage.paths
        st_p = comm.all_gather_i64(sp.reshape(-1)).reshape((world,) + sp.shape)
        breakdown = StageRecorder.summary(st_h.sum(axis=0), st_p.sum(axis=0))
        if world > 1:
            per = [StageRecorder.summary(st_h[r], st_p[r]) for r in range(world)]
            breakdown["p99_ms_by_rank"] = {s: [p[s]["p99_ms"] for p in per] for s in STAGES}
            breakdown["admitted_by_path_by_rank"] = [p["admitted_by_path"] for p in per]
        # Sustained throughput: requests dispatched inside the window (counted
        # at t1, before the untimed drain), capped by the requests that
        # arrived in it -- a window that starts with a queue must not read
        # above the offered rate, and under overload (dispatches < arrivals)
        # the dispatch rate is what counts.  Latency histograms cover every
        # dispatch from t0 through the drain: requests that arrived in the
        # window and were dispatched after t1 count.
        value = min(dispatched, arrived) / elapsed if elapsed > 0 else 0.0
        met = bool(lat["p99_ms"] <= P99_TARGET_MS and lat["p99_by_tier_ms"][0] <= REALTIME_P99_TARGET_MS)
        if a.test_miss_above_util > 0 and util > a.test_miss_above_util:
            met = False                   # test hook: pretend this operating point missed the SLO
        return {"util": util, "rate": rate, "value": value, "elapsed": elapsed, "lat": lat, "lat_done": lat_done,
                "met": met, "dispatched": dispatched, "tokens": tokens, "arrived": arrived, "work": work,
                "remote_in_window": remote_in_window, "lockstep": lockstep, "acct": acct,
                "host_timed": host_timed, "eng_host": eng_host1 - eng_host0, "breakdown": breakdown}

    # ---------------------------------------------------------------- SLO search
    # The headline is requests/s AT the operating point (BASELINE.json: p99
    # <= 500 ms over all tiers, realtime p99 <= 100 ms): if the window at
    # --util misses it, the same process re-serves at lower utilisations and
    # reports the highest one that held the SLO.  Every rank takes the same
    # decision (the latency summary is all-gathered), so the collective
    # counts stay aligned.
    # Both directions: a first window that holds the SLO climbs through
    # --slo-climb while every window keeps holding it; one that misses backs
    # off through --slo-backoff.  The headline is the best window that held
    # it (its value is still capped by what was dispatched AND what arrived
    # in the window).  The decision inputs are all-gathered, so every rank
    # runs the same windows.
    # A plain run serves the one window at --util (value = its rate if it held
    # the operating point, else 0); the search's further windows need --full.
    backoff = [u for u in (float(x) for x in a.slo_backoff.split(",") if x) if u < a.util] if a.full else []
    climb = [u for u in (float(x) for x in a.slo_climb.split(",") if x) if u > a.util] if a.full else []
    tried = []
    best = res = None
    t_search = time.monotonic()
    utils = [a.util]
    k = 0
    while utils:
        u = utils.pop(0)
        t_w = time.monotonic()
        res = window(u, k)
        k += 1
        tried.append({"util": round(u, 4), "value": round(res["value"], 2), "met": res["met"],
                      "p99_ms": round(res["lat"]["p99_ms"], 3),
                      "p99_by_tier_ms": [round(x, 3) for x in res["lat"]["p99_by_tier_ms"]],
                      "p99_e2e_by_tier_ms": [round(x, 3) for x in res["lat_done"]["p99_by_tier_ms"]],
                      "window_s": round(time.monotonic() - t_w, 2)})
        if res["met"] and (best is None or res["value"] > best["value"]):
            best = res
        if k == 1:
            up = bool(res["met"])
            utils = list(climb) if up else list(backoff)
        elif res["met"] != up:
            break                         # climbed past the knee / backed off into the SLO
        # bounded wall time: another window must fit (the slowest one so far)
        over = time.monotonic() - t_search + max(t["window_s"] for t in tried) > a.slo_budget_s
        if int(comm.all_gather_i64(np.array([int(over)], dtype=np.int64)).max()):
            break
    if best is not None:
        res = best
    gc.enable()
    if door is not None:
        comm.barrier()
        door.close()
    lat, lat_done, elapsed = res["lat"], res["lat_done"], res["elapsed"]
    dispatched, tokens, arrived = res["dispatched"], res["tokens"], res["arrived"]
    acct = res["acct"]
    value = res["value"] if res["met"] else 0.0
    slo = {"util_tried": [t["util"] for t in tried], "attempts": tried,
           "value_util": round(res["util"], 4) if res["met"] else None,
           # the first window (at --util) next to the headline, so a climbed
           # value can be compared with single-window rounds
           "first_window": {"util": tried[0]["util"], "value": tried[0]["value"] if tried[0]["met"] else 0.0,
                            "met": tried[0]["met"]},
           "search_s": round(time.monotonic() - t_search, 1),
           "directions": "climb + backoff" if a.full else "none (one window at --util; --full searches)"}
    if not res["met"]:
        slo["reason"] = (f"no utilisation in {slo['util_tried']} held p99 <= {P99_TARGET_MS} ms (all tiers) and "
                         f"realtime p99 <= {REALTIME_P99_TARGET_MS} ms; value is 0 by construction")
    eh = res["eng_host"]
    work = res["work"]
    # what one request is: the tokens a completed request
    # ran through the backend (prompt + replayed history + generated - 1), and
    # the window's GEMM FLOP rate against the MI355X dense bf16 peak
    tok_per_req = float(work[1]) / max(1, int(work[2]))
    flops_per_s = float(work[0]) / elapsed if elapsed > 0 else 0.0
    out = {
        "metric": METRIC,
        "value": round(value, 2),
        "unit": "requests/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(elapsed * 1e3 / max(1, a.steps), 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": round(value / BASELINE_RPS, 4),
        "dtype": "bf16",
        "data": "CPU DRY RUN of the control flow -- not a measurement" if dry else
                "synthetic (Poisson arrivals, 10/30/40/20 tier mix, random-init weights)",
        "config": {"model": f"{a.model}-stub (32L, random bf16)" if a.model == "llama3-8b" else a.model,
                   "global_batch": a.slots * world, "seq_len": a.max_ctx,
                   # seq_len above is the KV window per slot (max_ctx), not the
                   # served request: prompts are <= prompt_cap tokens, see
                   # "request_shape" at the top level
                   "seq_len_is": "max_ctx", "max_ctx": a.max_ctx,
                   "realtime_mode": engine.realtime_mode,
                   "micro": ({"slots": engine.micro_slots, "inflight": engine.micro_inflight,
                              "budget": engine.micro_budget, "stream": engine.micro_stream,
                              "cus": engine.micro_cus or None}
                             if engine.micro else None),
                   "parallelism": f"dp{world}", "ingress": a.ingress, "door_share": a.door_share, "placement": a.lb,
                   "token_budget_by_rank": a.token_budget_by_rank or None,
                   "sim_gpu": a.sim_gpu or None, "extra_steps": not a.no_extra_steps,
                   "control_plane": comm_kind, "token_budget": a.token_budget,
                   "realtime_step_tokens": a.realtime_step_tokens,
                   "gen_tokens": a.gen_tokens, "prompt_cap": a.prompt_cap, "inflight": a.inflight,
                   "aging_ms": a.aging_ms, "util": round(res["util"], 4),
                   "classifier": not a.no_classifier, "residual_in_gemm": not a.no_residual_gemm,
                   "split_qkv": a.split_qkv, "fused_mlp": bool(engine.model.fused_mlp),
                   "fused_qkv": bool(engine.model.fused_qkv),
                   "row_scale_norm": bool(engine.model.row_scale_norm),
                   "fused_head": bool(engine.model.fused_head),
                   "fused_resid": bool(engine.model.fused_resid), "resid_epi": a.resid_epi,
                   "fused_rms": bool(getattr(engine.model, "fused_rms", False)),
                   "prune_last": bool(getattr(engine.model, "prune_last", False)),
                   "library_gemm": bool(getattr(engine.model, "library_gemm", True))},
        # realtime tier, arrival -> LAST generated token (the 8B backend's 4
        # forwards included); the headline's clock is arrival -> dispatch
        "realtime_p99_e2e_ms": round(lat_done["p99_by_tier_ms"][0], 3),
        "realtime_mode": engine.realtime_mode,
        "request_shape": {"mean_prompt_tokens": round(tok_per_req - (a.gen_tokens - 1), 2),
                          "gen_tokens": a.gen_tokens, "tokens_per_request": round(tok_per_req, 2),
                          "prompt_cap": a.prompt_cap, "max_ctx": a.max_ctx},
        "backend_matmul_tflops": round(flops_per_s / 1e12, 1),
        # GEMM FLOP/s over the MI355X dense bf16 peak (2.5 PFLOP/s, no sparsity)
        "mfma_peak_fraction": round(flops_per_s / 2.5e15, 4),
        "micro_forwards": ({"count": int(work[3]), "per_s": round(int(work[3]) / elapsed, 1) if elapsed > 0 else 0.0,
                            "mean_gpu_ms": round(work[4] / 1000.0 / max(1, int(work[5])), 3),
                            "graph_replays": int(getattr(engine, "micro_graph_steps", 0)),
                            "micro_graph": bool(getattr(engine, "micro_graph", False))}
                           if engine.micro else None),
        "p99_ms": round(lat["p99_ms"], 3),                       # arrival -> dispatch
        "p50_ms": round(lat["p50_ms"], 3),
        "p99_enqueue_to_dispatch_ms": round(lat["p99_enq_ms"], 3),
        "p99_e2e_ms": round(lat_done["p99_ms"], 3),
        "p50_e2e_ms": round(lat_done["p50_ms"], 3),
        "p99_e2e_by_tier_ms": [round(x, 3) for x in lat_done["p99_by_tier_ms"]],
        "p99_by_tier_ms": [round(x, 3) for x in lat["p99_by_tier_ms"]],
        "requests_by_tier": lat["count_by_tier"],
        "p99_target_ms": P99_TARGET_MS,
        # BASELINE.md operating point: p99 enqueue->dispatch <= 500 ms over
        # all tiers and <= 100 ms for the realtime tier (judged on the
        # stricter arrival->dispatch clock, which adds ingest + preprocess)
        "p99_target_met": bool(res["met"]),
        # stricter still: arrival -> last generated token of the 8B backend
        "p99_e2e_target_met": bool(lat_done["p99_ms"] <= P99_TARGET_MS),
        "slo_search": slo,
        "offered_rate_per_gpu": round(res["rate"], 2),
        "dispatch_rate_in_window": round(dispatched / elapsed, 2) if elapsed > 0 else 0.0,
        "arrival_rate_in_window": round(arrived / elapsed, 2) if elapsed > 0 else 0.0,
        "remote_dispatched": int(comm.all_gather_i64(np.array([gw.counters["remote_sent"]], dtype=np.int64)).sum()),
        "remote_dispatched_in_window": res["remote_in_window"],
        "comm": evidence,
        # the data plane the job ran on: "nccl" (RCCL passed its preflight on
        # every rank), "gloo-fallback" (it did not: flagged), "gloo", "none"
        "data_plane": evidence.get("data_backend", "none"),
        "lockstep": res["lockstep"],
        "latency_breakdown": res["breakdown"],
        "steady_ticks": steady,
        "requests_accounted": {"offered": int(acct[0]), "completed": int(acct[1]), "rejected": int(acct[2]),
                               "shed": int(acct[3]), "lost": int(acct[0] - acct[1] - acct[2] - acct[3])},
        "warm_shapes": warmed,
        "calibrated_capacity_per_gpu": round(capacity, 2),
        "backend_tokens_per_s": round(tokens / elapsed, 1) if elapsed > 0 else 0.0,
        "dispatched": dispatched,
        "host_ms_per_tick_saturated": host_sat,
        "host_ms_per_tick": dict(res["host_timed"], engine_build=round(
            float(eh[0]) / max(1, a.steps) / 1e6, 3), engine_sync=round(
            float(eh[1]) / max(1, a.steps) / 1e6, 3), engine_enqueue=round(
            float(eh[2]) / max(1, a.steps) / 1e6, 3)),
    }
    if a.full and a.gateway_only_s > 0:
        # Secondary, untimed-by-contract measurement: the gateway path alone
        # (GPU preprocess + native queue + dispatcher) against a null backend,
        # Poisson load at --gateway-only-rate per GPU.
        from llm_message_queue_amd.backend.null_engine import NullEngine
        gw2 = Gateway(cfg, preprocessor=pre, engine=NullEngine(), use_gpu_preprocess=not dry,
                      prompt_cap=a.prompt_cap, gen_tokens=1)
        arr2 = PoissonArrivals(a.gateway_only_rate, seed=99 + rank)
        sync_all()
        g0 = time.monotonic()
        arr2.reset(g0)
        while time.monotonic() - g0 < a.gateway_only_s:
            # the load generator shares this thread: generating a whole
            # backlog between two ticks would starve the gateway of ticks
            # once the offered rate passes its capacity (served rate falling
            # as the offered one rises); a bounded slice per tick keeps the
            # measurement at the gateway's own ceiling
            due = arr2.due(time.monotonic(), limit=8192)
            if due:
                msgs = wl.make(len(due))
                for m, ts in zip(msgs, due):
                    m.arrival_ns = int(ts * 1e9)
                gw2.submit(msgs)
            gw2.tick()
        g1 = time.monotonic()
        s2 = comm.all_gather_i64(np.array([gw2.counters["dispatched"], int((g1 - g0) * 1e9)], dtype=np.int64))
        arr_h = comm.all_gather_i64(gw2.rec.arr.reshape(-1)).sum(axis=0).reshape(gw2.rec.arr.shape)
        enq_h = comm.all_gather_i64(gw2.rec.enq.reshape(-1)).sum(axis=0).reshape(gw2.rec.enq.shape)
        l2 = LatencyRecorder(len(gw2.tiers)).summary(arr_h, enq_h)
        out["gateway_only"] = {"requests_per_s": round(float(s2[:, 0].sum() / (s2[:, 1].max() / 1e9)), 1),
                               "offered_per_gpu": a.gateway_only_rate, "p99_ms": round(l2["p99_ms"], 3),
                               "p99_enqueue_to_dispatch_ms": round(l2["p99_enq_ms"], 3),
                               "note": "null backend: gateway path only (what the reference's 10k msg/s "
                                       "target measures); not the headline value"}
    if a.dump_outputs and rank == 0:
        out["dumped_outputs"] = dump_outputs(a, engine, pre, use_gpu=not dry)
    if rank == 0:
        line = json.dumps(out)
        print(line, flush=True)
        if a.json_out:
            with open(a.json_out, "w") as fh:
                fh.write(line + "\n")
    page.close(unlink=True)
    engine.close()
    if world > 1:
        import torch.distributed as dist
        if getattr(comm, "data_backend", "") == "gloo-fallback":
            # an RCCL group that failed its preflight may still hold a helper
            # thread inside the communicator: tearing it down could block, so
            # this rank ends here (its result line is already out)
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
