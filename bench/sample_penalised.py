"""What the penalised path costs at the serving shape (V = 128256, K = 4096;
R = 1 and 900 penalised rows; history lengths 19 -- the benchmark's request
shape -- and 512): ``HipOps.penalised_head`` with every row greedy
(``greedy``: GEMM, edit, greedy pick) and with every row sampling under top_k
= 50 / top_p = 0.9 (``sample``: GEMM, edit, truncated draw), the edit alone
(``penalise``), the greedy pick alone (``argmax``), the record kernel for
2,048 token rows (``record``) and, as the yardstick, ``HipOps.truncated_head``
on the same rows (the same logits GEMM, no edit).  They alternate inside every
round; each figure is the median over ``--rounds`` of the median of
``--iters`` event-timed calls.  One JSON line per (R, history length)."""
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
MAX_CTX = 1024


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
    ap.add_argument("--rows", default="1,900")
    ap.add_argument("--hist", default="19,512")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_penalised: needs a GPU")
    dev = torch.device("cuda")
    V, K = a.vocab, a.dim
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    w = (torch.randn(V, K, device=dev) * 0.02).to(torch.bfloat16)
    ops = HipOps()
    for R in [int(t) for t in a.rows.split(",")]:
        x = torch.randn(R, K, device=dev).to(torch.bfloat16)
        hot = torch.full((R,), 1.0 / 0.8, dtype=torch.float32, device=dev)
        cold = torch.zeros(R, dtype=torch.float32, device=dev)
        keys = torch.from_numpy(S.row_keys(np.arange(R, dtype=np.uint64), 0).view(np.int32)).to(dev)
        tk = torch.full((R,), 50, dtype=torch.int32, device=dev)
        tp = torch.full((R,), 0.9, dtype=torch.float32, device=dev)
        tk0, tp1 = torch.zeros_like(tk), torch.ones_like(tp)
        out = torch.empty(R, dtype=torch.int32, device=dev)
        lg = torch.empty((R, V), dtype=torch.bfloat16, device=dev)
        G.gemm(x, w, out=lg)
        # a history as a generation leaves it: a third of the entries repeat earlier ones
        h = rng.integers(0, V, (R, MAX_CTX)).astype(np.int32)
        h[:, 2::3] = h[:, 1::3][:, :h[:, 2::3].shape[1]]
        hist = torch.from_numpy(h).to(dev)
        params = torch.tensor([[0.5, 0.3, 1.2]], dtype=torch.float32, device=dev).repeat(R, 1)
        T = 2048
        tok = torch.randint(0, V, (T,), device=dev)
        pos = torch.randint(0, MAX_CTX, (T,), dtype=torch.int32, device=dev)
        slot = torch.randint(0, R, (T,), dtype=torch.int32, device=dev)
        rec = torch.arange(T, dtype=torch.int32, device=dev)
        for n in [int(t) for t in a.hist.split(",")]:
            sp = np.zeros((R, 4), dtype=np.int32)
            sp[:, 0] = np.arange(R)
            sp[:, 2] = n // 2
            sp[:, 3] = n
            spans = torch.from_numpy(sp).to(dev)
            runs = {"truncated_head_ms": lambda: ops.truncated_head(x, w, hot, keys, tk, tp),
                    "greedy_ms": lambda: ops.penalised_head(x, w, cold, keys, tk0, tp1, hist, spans, params,
                                                            n_greedy=R),
                    "sample_ms": lambda: ops.penalised_head(x, w, hot, keys, tk, tp, hist, spans, params,
                                                            n_greedy=0),
                    "gemm_ms": lambda: G.gemm(x, w, out=lg),
                    "penalise_ms": lambda: G.penalise(lg, hist, spans, params),
                    "argmax_ms": lambda: G.penalised_argmax(lg, out=out),
                    "record_ms": lambda: G.history_record(hist, tok, pos, slot, rec)}
            r = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    r[k].append(timed(fn, a.iters))
            res = {"R": R, "V": V, "K": K, "hist": n}
            for k, v in r.items():
                res[k] = round(sorted(v)[len(v) // 2], 4)
                res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
            for m in ("greedy", "sample"):
                res[f"{m}_pct_of_step"] = round(100 * res[f"{m}_ms"] / STEP_MS, 2)
                res[f"{m}_over_truncated"] = round(res[f"{m}_ms"] / res["truncated_head_ms"], 2)
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
