#!/usr/bin/env python3
"""The FP8-weight 256x256-tile GEMM (``gemm_fp8`` / ``gemm_swiglu_fp8`` /
``gemm_residual_fp8``) against the kernels a forward runs today, on the four
layer GEMMs of Llama-3-8B at the row counts of prefill-carrying micro-forwards,
on a CU partition and on the whole chip.  Three candidates a (place, shape, M):

    skinny   ``skinny_fp8`` in 128-row chunks: what a quant forward runs while
             ``fp8_plan`` says "skinny"
    tile     the FP8-weight tile kernel, split-K as the model plans it
    bf16     the bf16 kernel the model picks at that M, over the decoded weights

The method of ``bench/skinny_fp8.py``: HIP events, ``--rounds`` rounds of
``--iters`` launches with the candidates alternating within a round, every
launch on the next of ``--copies`` copies of the weights (together larger than
the 256 MiB MALL).  One JSON line each: median microseconds, the spread (max -
min over the median) of skinny and bf16, weight TB/s, and the two ratios.  The
``fp8_plan`` thresholds in ``ops/gemm.py`` are read off these rows.

    python bench/gemm_fp8_tile.py --cus 64 0 --out profiles/fp8_tile_gemm_ab.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (("qkv", 6144, 4096, "store"), ("o", 4096, 4096, "resid"), ("gu", 28672, 4096, "swiglu"),
          ("down", 4096, 14336, "resid"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cus", type=int, nargs="*", default=[64, 0], help="0 = the whole chip, else a CU partition")
    ap.add_argument("--m", type=int, nargs="*", default=[65, 96, 128, 192, 256, 384, 512, 1024])
    ap.add_argument("--gemms", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from llm_message_queue_amd.backend.cu_partition import partition_streams, release_streams
    from llm_message_queue_amd.ops import gemm as G
    from llm_message_queue_amd.ops import quant as Q
    dev = torch.device("cuda", 0)
    sk_epi = {"store": G.SK_STORE, "resid": G.SK_RESID, "swiglu": G.SK_SWIGLU}
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
            if name not in a.gemms:
                continue
            qs = [G.quantize_rows((torch.randn(N, K, generator=g, device=dev) * 0.02).to(torch.bfloat16))
                  for _ in range(a.copies)]
            ws = [Q.dequantize(*q) for q in qs]                   # the decoded weights, bf16
            for M in a.m:
                x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
                out = torch.zeros(M, N // 2 if epi == "swiglu" else N, dtype=torch.bfloat16, device=dev)
                rs = torch.ones(G.row_scale_len(M), dtype=torch.float32, device=dev) if epi != "resid" else None
                tile_fn = {"store": G.gemm_fp8, "swiglu": G.gemm_swiglu_fp8}.get(epi)
                bf16_fn = {"store": G.gemm, "swiglu": G.gemm_swiglu}.get(epi)
                # the model's bf16 choice (models/llama_stub.py): on a partition the skinny kernel
                # up to 64 rows only; on the chip qkv up to 256 and o / down up to 512 rows
                sk_max = G.SKINNY_MAX_M if cus else {"store": G.SKINNY_PROJ_MAX_M, "resid": G.SKINNY_RESID_MAX_M,
                                                     "swiglu": G.SKINNY_MAX_M}[epi]
                runs = {"skinny": lambda i: G.skinny_fp8(x, *qs[i % a.copies], out, sk_epi[epi], row_scale=rs,
                                                         cus=plan_cus)}
                if epi == "resid":
                    runs["tile"] = lambda i: G.gemm_residual_fp8(x, *qs[i % a.copies], out, split_cus=plan_cus)
                else:
                    runs["tile"] = lambda i: tile_fn(x, *qs[i % a.copies], out=out, row_scale=rs, split_cus=plan_cus)
                if M <= sk_max:
                    bf16_kind = "skinny"
                    runs["bf16"] = lambda i: G.skinny(x, ws[i % a.copies], out, sk_epi[epi], row_scale=rs,
                                                      cus=plan_cus)
                elif epi == "resid":
                    bf16_kind = "tile"
                    runs["bf16"] = lambda i: G.gemm_residual(x, ws[i % a.copies], out, split_cus=plan_cus)
                else:
                    bf16_kind = "tile"
                    runs["bf16"] = lambda i: bf16_fn(x, ws[i % a.copies], out=out, row_scale=rs, split_cus=plan_cus)
                with torch.cuda.stream(stream):
                    for fn in runs.values():
                        timed(fn, a.copies)                       # warm-up: scratch, code objects
                    ms = {k: [] for k in runs}
                    for _ in range(a.rounds):
                        for k, fn in runs.items():                # a / b / c / a / b / c
                            ms[k].append(timed(fn, a.iters))
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
                split = G.split_all(M, N, K, plan_cus)
                split = G.split_plan(M, N, K, plan_cus) if split is None else split
                row = {"cus": plan_cus, "partition": bool(cus), "gemm": name, "N": N, "K": K, "epi": epi, "M": M,
                       "tiles": G._tiles(M, N), "split_full": split, "bf16_kernel": bf16_kind,
                       "skinny_us": round(1e3 * med["skinny"], 2), "skinny_spread": round(spread["skinny"], 4),
                       "tile_us": round(1e3 * med["tile"], 2), "tile_spread": round(spread["tile"], 4),
                       "bf16_us": round(1e3 * med["bf16"], 2), "bf16_spread": round(spread["bf16"], 4),
                       "skinny_tbs": round(N * K / med["skinny"] / 1e9, 3),
                       "tile_tbs": round(N * K / med["tile"] / 1e9, 3),
                       "bf16_tbs": round(N * K * 2 / med["bf16"] / 1e9, 3),
                       "tile_vs_skinny": round(med["skinny"] / med["tile"], 3),
                       "tile_vs_bf16": round(med["bf16"] / med["tile"], 3)}
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
