#!/usr/bin/env python3
"""bf16 ``skinny`` against ``skinny_fp8`` (W8A16: e4m3 weight codes decoded in
registers) on the four layer GEMMs of Llama-3-8B at micro-forward row counts,
on the whole chip and on a CU partition (``backend.cu_partition``).

Each (place, shape, M) is timed with HIP events in alternating order
(bf16 / fp8 / bf16 / fp8 ..., ``--rounds`` rounds of ``--iters`` launches);
every round rotates through ``--copies`` copies of the weights (together
larger than the 256 MiB MALL) so a launch streams its weights from HBM as a
micro-forward's does.  One JSON line each: median ms of both, the bf16
rounds' spread (max - min over the median), weight bytes per second of both,
the speed-up.

    python bench/skinny_fp8.py --cus 0 64 --out profiles/skinny_fp8.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (("qkv", 6144, 4096, "store"), ("o", 4096, 4096, "resid"), ("gate_up", 28672, 4096, "swiglu"),
          ("down", 4096, 14336, "resid"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, nargs="*", default=[0, 64], help="0 = the whole chip, else a CU partition")
    ap.add_argument("--m", type=int, nargs="*", default=[8, 64, 128])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from llm_message_queue_amd.backend.cu_partition import partition_streams, release_streams
    from llm_message_queue_amd.ops import gemm as G
    dev = torch.device("cuda", 0)
    epis = {"store": G.SK_STORE, "resid": G.SK_RESID, "swiglu": G.SK_SWIGLU}
    chip = torch.cuda.get_device_properties(dev).multi_processor_count
    fh = open(a.out, "a") if a.out else None
    g = torch.Generator(device=dev).manual_seed(0)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for cus in a.cus:
        stream = partition_streams(dev, cus)[1] if cus else torch.cuda.current_stream(dev)
        plan_cus = cus or chip
        for name, N, K, epi in SHAPES:
            ws = [(torch.randn(N, K, generator=g, device=dev) * 0.02).to(torch.bfloat16) for _ in range(a.copies)]
            qs = [G.quantize_rows(w) for w in ws]
            for M in a.m:
                x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
                out = torch.zeros(M, N // 2 if epi == "swiglu" else N, dtype=torch.bfloat16, device=dev)
                runs = {"bf16": lambda i: G.skinny(x, ws[i % a.copies], out, epis[epi], cus=plan_cus)}
                runs["fp8"] = lambda i: G.skinny_fp8(x, *qs[i % a.copies], out, epis[epi], cus=plan_cus)
                with torch.cuda.stream(stream):
                    for fn in runs.values():
                        timed(fn, a.copies)                       # warm-up: scratch, code objects
                    ms = {k: [] for k in runs}
                    for _ in range(a.rounds):
                        for k, fn in runs.items():                # A / B / A / B
                            ms[k].append(timed(fn, a.iters))
                med = {k: statistics.median(v) for k, v in ms.items()}
                row = {"cus": plan_cus, "partition": bool(cus), "gemm": name, "N": N, "K": K, "epi": epi, "M": M,
                       "splits": G.skinny_splits(N, K, plan_cus, M),
                       "bf16_ms": round(med["bf16"], 4),
                       "bf16_spread": round((max(ms["bf16"]) - min(ms["bf16"])) / med["bf16"], 4),
                       "bf16_tbs": round(N * K * 2 / med["bf16"] / 1e9, 3)}
                row["fp8_ms"] = round(med["fp8"], 4)
                row["fp8_tbs"] = round(N * K / med["fp8"] / 1e9, 3)
                row["fp8_speedup"] = round(med["bf16"] / med["fp8"], 3)
                line = json.dumps(row)
                print(line, flush=True)
                if fh:
                    fh.write(line + "\n")
                    fh.flush()
            del ws, qs
        torch.cuda.synchronize(dev)
    if fh:
        fh.close()
    if any(a.cus):
        release_streams()
    return 0


if __name__ == "__main__":
    sys.exit(main())
