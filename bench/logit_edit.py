"""What an allow-list, a logit bias and ``min_p`` cost at the serving shape (V
= 128256, K = 4096; R = 1 and 900 sampling rows under top_k = 50 / top_p =
0.9, 19-token histories): ``HipOps.penalised_head`` without the new inputs
(``parent``), with a 64-id allow-list and 16 bias entries a row
(``allow_bias``) and with the 16 bias entries only (``bias``);
``HipOps.truncated_head`` without (``truncated``) and with ``min_p`` = 0.05
(``min_p``); the edit kernel alone over ready logits (``edit_allow_bias`` /
``edit_bias``) and the sampler alone without / with ``min_p`` (``draw`` /
``draw_min_p``, and ``draw_masked``: the same draw over rows the allow-list
has masked; ``draw_k5`` / ``draw_masked_k5``: both again under top_k = 5, whose
fifth largest value lies in the sampler's first key window on either kind of
row).  They alternate inside every round; each figure is the median
over ``--rounds`` of the median of ``--iters`` event-timed calls.  One JSON
line per R."""
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
N_ALLOW, N_BIAS, HIST = 64, 16, 19


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
    ap.add_argument("--rows", default="900,1")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--dim", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logit_edit: needs a GPU")
    dev = torch.device("cuda")
    V, K = a.vocab, a.dim
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    w = (torch.randn(V, K, device=dev) * 0.02).to(torch.bfloat16)
    ops = HipOps()
    for R in [int(t) for t in a.rows.split(",")]:
        x = torch.randn(R, K, device=dev).to(torch.bfloat16)
        hot = torch.full((R,), 1.0 / 0.8, dtype=torch.float32, device=dev)
        keys = torch.from_numpy(S.row_keys(np.arange(R, dtype=np.uint64), 0).view(np.int32)).to(dev)
        tk = torch.full((R,), 50, dtype=torch.int32, device=dev)
        tp = torch.full((R,), 0.9, dtype=torch.float32, device=dev)
        tk5 = torch.full((R,), 5, dtype=torch.int32, device=dev)
        out = torch.empty(R, dtype=torch.int32, device=dev)
        lg = torch.empty((R, V), dtype=torch.bfloat16, device=dev)
        G.gemm(x, w, out=lg)
        h = rng.integers(0, V, (R, MAX_CTX)).astype(np.int32)
        hist = torch.from_numpy(h).to(dev)
        params = torch.tensor([[0.5, 0.3, 1.2]], dtype=torch.float32, device=dev).repeat(R, 1)
        sp = np.zeros((R, 4), dtype=np.int32)
        sp[:, 0], sp[:, 2], sp[:, 3] = np.arange(R), HIST // 2, HIST
        spans = torch.from_numpy(sp).to(dev)
        # per row 64 allowed ids, then 16 bias entries, half of them on allowed ids
        per = N_ALLOW + N_BIAS
        ids = np.empty((R, per), dtype=np.int32)
        for r in range(R):
            ids[r, :N_ALLOW] = rng.permutation(V)[:N_ALLOW]
            ids[r, N_ALLOW:N_ALLOW + N_BIAS // 2] = ids[r, :N_BIAS // 2]
            ids[r, N_ALLOW + N_BIAS // 2:] = rng.integers(0, V, N_BIAS - N_BIAS // 2)
        vals = rng.uniform(-5, 5, (R, per)).astype(np.float32)
        off = np.arange(R, dtype=np.int32) * per
        both = np.stack([off, np.full(R, N_ALLOW), off + N_ALLOW, np.full(R, N_BIAS)], axis=1).astype(np.int32)
        only = both.copy()
        only[:, 1] = 0
        ids_d, vals_d = torch.from_numpy(ids.reshape(-1)).to(dev), torch.from_numpy(vals.reshape(-1)).to(dev)
        both_d, only_d = torch.from_numpy(both).to(dev), torch.from_numpy(only).to(dev)
        lmp = torch.from_numpy(np.broadcast_to(S.min_p_log(0.05), (R,)).copy()).to(dev)

        def head(**kw):
            return lambda: ops.penalised_head(x, w, hot, keys, tk, tp, hist, spans, params, n_greedy=0, **kw)
        runs = {"parent_ms": head(),
                "allow_bias_ms": head(edit=(ids_d, vals_d, both_d)),
                "bias_ms": head(edit=(ids_d, vals_d, only_d)),
                "truncated_ms": lambda: ops.truncated_head(x, w, hot, keys, tk, tp),
                "min_p_ms": lambda: ops.truncated_head(x, w, hot, keys, tk, tp, log_min_p=lmp),
                "edit_allow_bias_ms": lambda: G.logit_edit(lg, ids_d, vals_d, both_d),
                "edit_bias_ms": lambda: G.logit_edit(lg, ids_d, vals_d, only_d),
                "draw_ms": lambda: G.sample_truncated(lg, hot, keys, tk, tp, out=out),
                "draw_min_p_ms": lambda: G.sample_truncated(lg, hot, keys, tk, tp, out=out, log_min_p=lmp)}
        r = {k: [] for k in runs}
        for _ in range(a.rounds):
            G.gemm(x, w, out=lg)                      # (the draws run over unmasked logits)
            for k in ("draw_ms", "draw_min_p_ms"):
                r[k].append(timed(runs[k], a.iters))
            k5 = lambda: G.sample_truncated(lg, hot, keys, tk5, tp, out=out)      # noqa: E731
            r.setdefault("draw_k5_ms", []).append(timed(k5, a.iters))
            for k, fn in runs.items():
                if not k.startswith("draw"):
                    r[k].append(timed(fn, a.iters))
            G.gemm(x, w, out=lg)
            G.logit_edit(lg, ids_d, vals_d, both_d)
            r.setdefault("draw_masked_ms", []).append(timed(runs["draw_ms"], a.iters))
            r.setdefault("draw_masked_k5_ms", []).append(timed(k5, a.iters))
        res = {"R": R, "V": V, "K": K, "hist": HIST, "n_allow": N_ALLOW, "n_bias": N_BIAS}
        for k, v in r.items():
            res[k] = round(sorted(v)[len(v) // 2], 4)
            res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        for m, base in (("allow_bias", "parent"), ("bias", "parent"), ("min_p", "truncated")):
            res[f"{m}_added_ms"] = round(res[f"{m}_ms"] - res[f"{base}_ms"], 4)
            res[f"{m}_over_{base}"] = round(res[f"{m}_ms"] / res[f"{base}_ms"], 3)
            res[f"{m}_added_pct_of_step"] = round(100 * res[f"{m}_added_ms"] / STEP_MS, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
