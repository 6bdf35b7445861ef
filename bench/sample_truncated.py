"""What the top-k / top-p path costs at the serving shape (V = 128256, K =
4096; R = 1, 64 and 900 truncating rows): the selection-and-draw kernel
(``sample_truncated`` over given logits), the store-epilogue GEMM that makes
those logits (``gemm``), the two together (``HipOps.truncated_head``) and, as
the yardstick, the fused sampling head on the same rows (``lm_head_sample``).
The four alternate inside every round; each figure is the median over
``--rounds`` of the median of ``--iters`` event-timed calls.  The kernel is
timed per truncation mix: ``k`` (top_k = 50), ``p`` (top_p = 0.9), ``kp``
(both), ``off`` (neither: the draw alone).  One JSON line per R.
``--sweep-vocab``: instead, the kernel alone at one row over V = 1,024 ..
``--vocab`` (its fixed cost against its cost per column).

The logits are the GEMM's own (x, w ~ N(0, 1), N(0, 0.02^2): a spread of a
few units, as a model's), so the histogram sees a realistic number of groups."""
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

MIXES = {"k": (50, 1.0), "p": (0, 0.9), "kp": (50, 0.9), "off": (0, 1.0)}
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
    ap.add_argument("--sweep-vocab", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_truncated: needs a GPU")
    dev = torch.device("cuda")
    V, K = a.vocab, a.dim
    torch.manual_seed(0)
    if a.sweep_vocab:
        # the kernel alone at one row over V (logits ~ 1.3 N(0, 1)): fixed cost against per-column cost
        it = torch.full((1,), 1.25, dtype=torch.float32, device=dev)
        keys = torch.from_numpy(S.row_keys(np.zeros(1, dtype=np.uint64), 0).view(np.int32)).to(dev)
        out = torch.empty(1, dtype=torch.int32, device=dev)
        for Vs in (1024, 16384, 65536, V):
            lg = (1.3 * torch.randn(1, Vs, device=dev)).to(torch.bfloat16)
            res = {"sweep": "vocab", "R": 1, "V": Vs}
            for m, (k, p) in MIXES.items():
                tk = torch.full((1,), k, dtype=torch.int32, device=dev)
                tp = torch.full((1,), p, dtype=torch.float32, device=dev)
                ms = [timed(lambda: G.sample_truncated(lg, it, keys, tk, tp, out=out), a.iters)
                      for _ in range(a.rounds)]
                res[f"kernel_{m}_ms"] = round(sorted(ms)[len(ms) // 2], 4)
            print(json.dumps(res), flush=True)
        return
    w = (torch.randn(V, K, device=dev) * 0.02).to(torch.bfloat16)
    ops = HipOps()
    for R in [int(t) for t in a.rows.split(",")]:
        x = torch.randn(R, K, device=dev).to(torch.bfloat16)
        Rp = G.row_scale_len(R)
        it = torch.zeros(Rp, dtype=torch.float32, device=dev)
        it[:R] = 1.0 / 0.8
        keys = torch.zeros((Rp, 2), dtype=torch.int32, device=dev)
        keys[:R] = torch.from_numpy(S.row_keys(np.arange(R, dtype=np.uint64), 0).view(np.int32)).to(dev)
        out = torch.empty(R, dtype=torch.int32, device=dev)
        lg = torch.empty((R, V), dtype=torch.bfloat16, device=dev)
        G.gemm(x, w, out=lg)
        par = {m: (torch.full((R,), k, dtype=torch.int32, device=dev),
                   torch.full((R,), p, dtype=torch.float32, device=dev)) for m, (k, p) in MIXES.items()}
        runs = {"gemm_ms": lambda: G.gemm(x, w, out=lg),
                "head_kp_ms": lambda: ops.truncated_head(x, w, it, keys, *par["kp"]),
                "fused_sample_ms": lambda: G.lm_head_sample(x, w, it, keys, out=out)}
        for m in MIXES:
            runs[f"kernel_{m}_ms"] = (lambda tk, tp: lambda: G.sample_truncated(lg, it, keys, tk, tp, out=out))(*par[m])
        r = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                r[k].append(timed(fn, a.iters))
        res = {"R": R, "V": V, "K": K}
        for k, v in r.items():
            res[k] = round(sorted(v)[len(v) // 2], 4)
            res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        res["head_kp_pct_of_step"] = round(100 * res["head_kp_ms"] / STEP_MS, 2)
        res["head_kp_over_fused"] = round(res["head_kp_ms"] / res["fused_sample_ms"], 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
