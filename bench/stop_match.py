"""What the stop decision costs, and what a stop gives back.

``--mode kernel`` (default): ``stop_match_kernel`` (``ops.gemm.stop_match``)
over R = 900 and R = 1 flagged rows, each with 8 entries of 8 tokens over a
19-token window of generated tokens (``entries8x8_ms``), and with 8 one-token
entries that read no history (``tokens8_ms``).  The variants alternate inside
every round; each figure is the median over ``--rounds`` of the median of
``--iters`` event-timed calls.  One JSON line per R.

``--mode engine``: the tiny model through the HIP engine with ``gen_tokens =
16``, ``--requests`` greedy requests in waves that fill the slots, once where
every request stops at its fourth token (its stop token is its own fourth
baseline token) and once where every request carries a stop token that never
matches, next to the same requests without any stop key.  The three cases
alternate inside every round; completed requests per second (the median over
``--rounds``, with the minimum and maximum), the forward steps and the tokens
those steps computed, and the engine's counters, one JSON line per case.  The
tiny model's step is a fraction of a millisecond, so the host's per-request
work bounds the rate here; the steps and tokens show what a stop gives back."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from llm_message_queue_amd.ops import gemm as G
from llm_message_queue_amd.ops import sampling as S

STEP_MS = 41.0          # the serving step the shares are quoted against (docs/performance.md)
MAX_CTX = 1024
WINDOW = 19


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


def kernel(a):
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    V = a.vocab
    for R in [int(t) for t in a.rows.split(",")]:
        hist = rng.integers(0, V, (R, MAX_CTX)).astype(np.int32)
        tok = rng.integers(0, V, R).astype(np.int32)
        rows = np.zeros((R, S.STOP_ROW_WORDS), dtype=np.int32)
        rows[:, 0] = np.arange(R)
        rows[:, 1] = 40
        rows[:, 2] = 40 + WINDOW - 1                         # 18 generated before this step's token
        rows[:, 4] = np.arange(R) * S.STOP_ENTRIES
        rows[:, 5] = S.STOP_ENTRIES
        ent = np.zeros((R * S.STOP_ENTRIES, S.STOP_ENT_WORDS), dtype=np.int32)
        ent[:, 0] = S.STOP_LEN
        ent[:, 1:] = rng.integers(0, V, (len(ent), S.STOP_LEN))
        for r in range(0, R, 2):                             # every other row matches, at its last entry
            ent[r * S.STOP_ENTRIES + 7, 1:] = list(hist[r, 40 + WINDOW - 8:40 + WINDOW - 1]) + [tok[r]]
        one = ent.copy()
        one[:, 0] = 1
        none = rows.copy()
        none[:, 0] = -1
        d = lambda x: torch.from_numpy(x).to(dev)            # noqa: E731
        tok_d, hist_d, rows_d, none_d, ent_d, one_d = d(tok), d(hist), d(rows), d(none), d(ent), d(one)
        out = torch.empty(R, dtype=torch.int32, device=dev)
        got = G.stop_match(tok_d, hist_d, rows_d, ent_d).cpu().numpy()
        assert np.array_equal(got, S.stop_match_reference(tok, hist, rows, ent)) and (got[::2] == 7).all()
        runs = {"entries8x8_ms": lambda: G.stop_match(tok_d, hist_d, rows_d, ent_d, out=out),
                "tokens8_ms": lambda: G.stop_match(tok_d, None, none_d, one_d, out=out)}
        r = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                r[k].append(timed(fn, a.iters))
        res = {"mode": "kernel", "R": R, "window": WINDOW, "entries": S.STOP_ENTRIES, "entry_len": S.STOP_LEN}
        for k, v in r.items():
            res[k] = round(sorted(v)[len(v) // 2], 4)
            res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
            res[k.replace("_ms", "_pct_of_step")] = round(100 * res[k] / STEP_MS, 4)
        print(json.dumps(res), flush=True)


def engine(a):
    from llm_message_queue_amd.backend.engine import BackendEngine, Request
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    gen, n = 16, a.requests
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, 1024, 8 + i % 9).astype(np.int32) for i in range(n)]

    def serve(stops):
        eng = BackendEngine(LlamaConfig.tiny(), slots=a.slots, max_ctx=64, token_budget=2048, device="cuda", impl="hip")
        pend = [Request(req_id=i, prompt=prompts[i].copy(), gen_tokens=gen, stop=stops[i] if stops else None)
                for i in range(n)]
        done = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while len(done) < n:
            if pend and eng.free:
                adm = eng.admit(pend[:len(eng.free)])
                pend = pend[len(adm):]
            eng.launch()
            for r in eng.finish().completed:
                done[r.req_id] = r
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.close()
        return eng, done, dt

    _, base, _ = serve(None)                                 # (also the warm-up)
    cases = (("baseline", None),
             ("none_stops", [[[1 << 20]]] * n),
             ("all_stop_at_4", [[[int(base[i].out_tokens[3])]] for i in range(n)]))
    rates, last = {name: [] for name, _ in cases}, {}
    for _ in range(a.rounds):
        for name, stops in cases:
            eng, done, dt = serve(stops)
            rates[name].append(n / dt)
            last[name] = (eng, done)
    for name, _ in cases:
        eng, done = last[name]
        toks = [len(done[i].out_tokens) for i in range(n)]
        v = sorted(rates[name])
        print(json.dumps({"mode": "engine", "case": name, "requests": n, "slots": a.slots, "gen_tokens": gen,
                          "rounds": a.rounds, "req_per_s": round(v[len(v) // 2], 1),
                          "req_per_s_min_max": [round(v[0], 1), round(v[-1], 1)], "steps": eng.step_id,
                          "step_tokens": eng.total_tokens, "mean_generated": round(float(np.mean(toks)), 2),
                          "stopped_total": eng.stopped_total, "stop_steps": eng.stop_steps,
                          "stop_dropped_rows": eng.stop_dropped_rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "engine"), default="kernel")
    ap.add_argument("--rows", default="900,1")
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--requests", type=int, default=16384)
    ap.add_argument("--slots", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stop_match: needs a GPU")
    (kernel if a.mode == "kernel" else engine)(a)


if __name__ == "__main__":
    main()
