"""What the log-probability path costs at the serving shape (V = 128256, K =
4096; R = 1, 64 and 900 rows that ask): the kernel alone (``token_logprobs``
over given logits), the store-epilogue GEMM that makes those logits
(``gemm``), the two together (``HipOps.logprob_head``) and, as the yardstick,
the fused greedy head on the same rows (``lm_head_argmax``).  They alternate
inside every round; each figure is the median over ``--rounds`` of the median
of ``--iters`` event-timed calls.  Every R also reports the worst ``|device -
twin|`` of the kernel's values over (at most 16 of) its rows against
``ops.sampling.logprob_bound``.  One JSON line per R.

The logits are the GEMM's own (x, w ~ N(0, 1), N(0, 0.02^2): a spread of a
few units, as a model's)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S
from llm_message_queue_amd.ops.llama_ops import HipOps

STEP_MS = 41.0          # the serving step the shares are quoted against (docs/performance.md)


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(3):
        fn()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,64,900")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprob_head: needs a GPU")
    dev = torch.device("cuda")
    V, K = a.vocab, a.dim
    torch.manual_seed(0)
    w = (torch.randn(V, K, device=dev) * 0.02).to(torch.bfloat16)
    ops = HipOps()
    for R in [int(t) for t in a.rows.split(",")]:
        x = torch.randn(R, K, device=dev).to(torch.bfloat16)
        out = torch.empty(R, dtype=torch.int32, device=dev)
        lg = torch.empty((R, V), dtype=torch.bfloat16, device=dev)
        G.gemm(x, w, out=lg)
        tok = G.lm_head_argmax(x, w).clone()
        lp = torch.empty((R, 1 + G.LP_TOP), dtype=torch.float32, device=dev)
        ids = torch.empty((R, G.LP_TOP), dtype=torch.int32, device=dev)
        runs = {"gemm_ms": lambda: G.gemm(x, w, out=lg),
                "kernel_ms": lambda: G.token_logprobs(lg, tok, out_lp=lp, out_id=ids),
                "head_ms": lambda: ops.logprob_head(x, w, tok),
                "fused_argmax_ms": lambda: G.lm_head_argmax(x, w, out=out)}
        r = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                r[k].append(timed(fn, a.iters))
        res = {"R": R, "V": V, "K": K}
        for k, v in r.items():
            res[k] = round(sorted(v)[len(v) // 2], 4)
            res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        res["head_pct_of_step"] = round(100 * res["head_ms"] / STEP_MS, 2)
        res["head_over_fused"] = round(res["head_ms"] / res["fused_argmax_ms"], 2)
        # the kernel against the twin on the same logits
        n = min(R, 16)
        G.token_logprobs(lg, tok, out_lp=lp, out_id=ids)
        want_lp, want_ids = S.logprob_reference(lg[:n].double().cpu().numpy(), tok[:n].cpu().numpy())
        res["ids_equal_twin"] = bool(np.array_equal(ids[:n].cpu().numpy(), want_ids))
        res["worst_abs_err"] = float(np.abs(lp[:n].cpu().numpy().astype(np.float64) - want_lp).max())
        res["bound"] = S.logprob_bound(V)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
