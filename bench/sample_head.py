"""The LM head's three ways to a next token at the serving shape (V = 128256,
K = 4096; M = 256 and 1024 sampled rows): the greedy head (``lm_head_argmax``),
the sampling head with every row sampling (``lm_head_sample``: the same GEMM
with the Gumbel-max epilogue) and the unfused baseline (``F.linear``, scale,
torch Gumbel noise, argmax over the [M][V] logits).  The three alternate
inside every round; each figure is the median over ``--rounds`` of the median
of ``--iters`` event-timed calls.  One JSON line per M.

``--argmax-lib PATH``: time only ``gemm_argmax`` of the kernel module at
PATH (this tree's build or another commit's) -- for an A/B of the greedy head
between two builds, run alternately, one process per side and round."""
import argparse
import importlib.util
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S


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


def med(v):
    return round(sorted(v)[len(v) // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,1024")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--argmax-lib", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_head: needs a GPU")
    dev = torch.device("cuda")
    V, K = a.vocab, a.dim
    torch.manual_seed(0)
    w = (torch.randn(V, K, device=dev) * 0.02).to(torch.bfloat16)
    if a.argmax_lib:
        spec = importlib.util.spec_from_file_location("_hipops", a.argmax_lib)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        st = torch.cuda.current_stream().cuda_stream
        for M in [int(t) for t in a.rows.split(",")]:
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            pv = torch.empty(M * (V // 256), dtype=torch.float32, device=dev)
            pi = torch.empty(M * (V // 256), dtype=torch.int32, device=dev)
            out = torch.empty(M, dtype=torch.int32, device=dev)
            ms = [timed(lambda: mod.gemm_argmax(x.data_ptr(), w.data_ptr(), M, V, K, pv.data_ptr(), pi.data_ptr(),
                                                out.data_ptr(), st), a.iters) for _ in range(a.rounds)]
            print(json.dumps({"lib": a.argmax_lib, "M": M, "V": V, "K": K, "argmax_ms": med(ms),
                              "argmax_ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                              "tokens_sum": int(out.long().sum())}), flush=True)
        return
    for M in [int(t) for t in a.rows.split(",")]:
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        Mp = G.row_scale_len(M)
        it = torch.zeros(Mp, dtype=torch.float32, device=dev)
        it[:M] = 1.0 / 0.8
        keys = torch.zeros((Mp, 2), dtype=torch.int32, device=dev)
        keys[:M] = torch.from_numpy(S.row_keys(np.arange(M, dtype=np.uint64), 0).view(np.int32)).to(dev)
        out = torch.empty(M, dtype=torch.int32, device=dev)

        def unfused():
            lg = torch.nn.functional.linear(x, w).float()
            u = torch.rand(M, V, device=dev)
            g = -torch.log(-torch.log(u.clamp_min(1e-20)))
            return torch.argmax(lg * it[:M, None] + g, dim=-1)

        r = {"M": M, "V": V, "K": K, "argmax_ms": [], "sample_ms": [], "unfused_ms": []}
        for _ in range(a.rounds):
            r["argmax_ms"].append(timed(lambda: G.lm_head_argmax(x, w, out=out), a.iters))
            r["sample_ms"].append(timed(lambda: G.lm_head_sample(x, w, it, keys, out=out), a.iters))
            r["unfused_ms"].append(timed(unfused, a.iters))
        for k in ("argmax_ms", "sample_ms", "unfused_ms"):
            r[k + "_min_max"] = [round(min(r[k]), 4), round(max(r[k]), 4)]
            r[k] = med(r[k])
        r["sample_over_argmax_us"] = round((r["sample_ms"] - r["argmax_ms"]) * 1e3, 1)
        r["sample_over_argmax_pct"] = round(100 * (r["sample_ms"] / r["argmax_ms"] - 1), 2)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
