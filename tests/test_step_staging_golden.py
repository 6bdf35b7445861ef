"""What a step stages and which head ops it calls, against a recorded run.

A scenario of requests that between them use every per-row option is served
by the engine on the reference ops, and per launch two things are compared
with ``tests/golden/step_staging.json``: the sha256 of the pinned staging
buffer the step filled, and the sequence of ``ops`` head methods the forward
called, each with a sha256 over its arguments that do not depend on the
model's arithmetic (row indices, temperatures, keys, truncation and penalty
parameters, edit lists, stop records; for activations and tokens only the row
count; for the history only whether there is one).

The file uses only what a refactor of the route from a request's options to
the head's kernels leaves alone -- ``BackendEngine`` on the CPU, ``Request``,
``admit`` / ``launch`` / ``pump_micro`` / ``finish``, the staging pins and
their allocator, the ``ops`` method names and signatures, and the fact that
every launch of either pool goes through ``_launch_pool(micro)`` (wrapped
here to cut the records per launch: ``launch`` and ``finish`` pump the micro
pool themselves) -- so it passes unchanged before and after one, and the
fixture is what the tree before it records:

    python tests/test_step_staging_golden.py --write

The records must not depend on the model: the scenario runs with two model
seeds and the two runs must agree before either is compared with the file.
Stop entries name ids outside the vocabulary, so no request stops early and
the schedule is a function of the requests alone.
"""
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_staging.json")

# min_p values whose staged float32(log(.)) does not hang on the last bit of
# the host's float64 log: ``test_min_p_values_are_safe`` moves the float64
# log one ulp either way with np.nextafter and gets the same float32
MIN_P = (0.25, 0.05)

HEADS = ("history_record", "sample_head", "greedy_head", "truncated_head", "penalised_head", "stop_match",
         "logprob_head")
# arguments hashed by row count only (activations, tokens), by presence only
# (the device history), and not at all (the weight)
ROWS_ONLY = {"x", "tok"}
PRESENCE_ONLY = {"hist"}
SKIP = {"w"}


def _feed(h, v):
    """One argument into the hash: tensors and arrays as dtype, shape and
    bytes; tuples element by element; scalars and None by their repr."""
    if v is None or isinstance(v, (bool, int, float, str)):
        h.update(repr(v).encode())
    elif isinstance(v, (tuple, list)):
        h.update(b"(")
        for e in v:
            _feed(h, e)
        h.update(b")")
    else:
        a = v.detach().cpu().contiguous().numpy() if torch.is_tensor(v) else np.ascontiguousarray(v)
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    h.update(b";")


def _call_hash(sig, a, kw):
    """sha256 over a head call's model-independent arguments, bound to the
    op's signature with its defaults, so that passing a default by name, by
    position or not at all is one call."""
    b = sig.bind(*a, **kw)
    b.apply_defaults()
    h = hashlib.sha256()
    for name, v in b.arguments.items():
        if name in SKIP:
            continue
        h.update(name.encode() + b"=")
        if name in ROWS_ONLY:
            _feed(h, int(v.shape[0]))
        elif name in PRESENCE_ONLY:
            _feed(h, v is None)
        else:
            _feed(h, v)
    return h.hexdigest()


def _spy(eng, calls, steps):
    """Record the forward's head calls in ``calls`` (not the calls one
    reference head makes to another) and, around every launch of either
    pool, one entry of ``steps``: the pool, the sha256 of the pin the launch
    filled (every pin of the pool is zeroed first) and the calls it made."""
    ops = eng.model.ops
    depth = [0]
    for name in HEADS:
        inner = getattr(ops, name)
        sig = inspect.signature(inner)

        def wrapped(*a, _inner=inner, _sig=sig, _name=name, **kw):
            if depth[0] == 0:
                calls.append([_name, _call_hash(_sig, a, kw)])
            depth[0] += 1
            try:
                return _inner(*a, **kw)
            finally:
                depth[0] -= 1
        setattr(ops, name, wrapped)
    launch = eng._launch_pool

    def launch_pool(micro):
        pins = eng._pins_m if micro else eng._pins
        for p in pins:
            p.zero_()
        sid, n0 = (eng.micro_id if micro else eng.step_id), len(calls)
        ran = launch(micro)
        if ran:
            steps.append({"pool": "micro" if micro else "serving", "pin": _pin_hash(pins[sid % len(pins)]),
                          "ops": calls[n0:]})
        return ran
    eng._launch_pool = launch_pool


def _pin_hash(pin):
    return hashlib.sha256(pin.numpy().tobytes()).hexdigest()


def _zeroed_pins(eng):
    """Pins that start too small for any step and grow zero-filled, so that a
    grown pin's bytes behind the step's are defined and its length (the
    engine's growth rule) is part of the hash."""
    eng._alloc_pin = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8)
    eng._pins = [torch.zeros(64, dtype=torch.uint8) for _ in eng._pins]


def _prompt(i, n):
    return np.random.default_rng(500 + i).integers(0, 1024, n).astype(np.int32)


I32 = lambda v: np.asarray(v, dtype=np.int32)      # noqa: E731
F32 = lambda v: np.asarray(v, dtype=np.float32)    # noqa: E731


def _requests():
    """(admit-from step, Request): eight at once fill the slots, the rest
    follow as rows leave, the last ones plain, so every block of the staging
    buffer is used in some step, unused in another, and several together."""
    from llm_message_queue_amd.backend.engine import Request
    spec = [
        (0, 4, 3, {}),                                                                    # plain greedy
        (0, 9, 8, dict(logprobs=2)),                                                      # logprobs, greedy
        (0, 5, 5, dict(temperature=0.8, seed=11)),                                        # temperature only
        (0, 7, 6, dict(temperature=0.9, seed=12, top_k=5, top_p=0.9, logprobs=0)),        # truncated + logprobs
        (0, 3, 4, dict(temperature=0.7, seed=13, min_p=MIN_P[0])),                        # min_p, not penalised
        (0, 6, 7, dict(presence_penalty=0.5)),                                            # presence, greedy
        (0, 8, 6, dict(temperature=1.1, seed=14, frequency_penalty=0.3, top_k=8, min_p=MIN_P[1])),
        (0, 5, 5, dict(repetition_penalty=1.3)),                                          # repetition, greedy
        (1, 4, 4, dict(allowed=I32([3, 5, 7, 9]))),                                       # allow-list, no penalty
        (1, 6, 5, dict(logit_bias=(I32([10, 2000000]), F32([2.0, -3.0])), presence_penalty=0.2,
                       temperature=0.6, seed=15)),                                        # bias + penalty
        (1, 5, 6, dict(stop=[[5000]], max_tokens=4)),                                     # one-token stop, max_tokens
        (1, 7, 6, dict(stop=[[5000, 5001, 5002], [7000]], min_tokens=2, temperature=0.5, seed=16)),
        (1, 3, 3, dict(allowed=I32([1, 2]), logit_bias=(I32([2]), F32([1.5])), temperature=0.8, seed=17,
                       top_p=0.8)),                                                       # allow + bias, sampling
        (1, 4, 2, dict(frequency_penalty=0.4, stop=[[6000, 6001]], logprobs=1)),          # penalty + stop + logprobs
        (8, 5, 7, {}),                                                                    # plain again, late
        (8, 2, 6, {}),
    ]
    return [(at, Request(req_id=i, prompt=_prompt(i, n), gen_tokens=g, **kw)) for i, (at, n, g, kw) in enumerate(spec)]


def run_pool(seed):
    """The serving pool's records, one per launch."""
    from llm_message_queue_amd.backend.engine import BackendEngine
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=8, max_ctx=64, token_budget=24, device="cpu", impl="ref",
                        max_inflight=2, seed=seed)
    _zeroed_pins(eng)
    calls, steps = [], []
    _spy(eng, calls, steps)
    pend = _requests()
    done = 0
    for step in range(60):
        if not pend and not eng.active:
            break
        ready = [r for at, r in pend if at <= step]
        got = {id(r) for r in eng.admit(ready)} if ready else set()
        pend = [(at, r) for at, r in pend if id(r) not in got]
        eng.launch()
        done += len(eng.finish(block=True).completed)
    done += len(eng.finish(block=True).completed)
    assert done == len(_requests()) and not eng.active
    counters = {k: int(getattr(eng, k)) for k in ("sampled_steps", "truncated_steps", "logprob_steps",
                                                  "penalised_steps", "edited_steps", "stop_steps", "stopped_total")}
    return {"steps": steps, "counters": counters}


def run_micro(seed):
    """A realtime request with options on the micro pool beside a plain one
    on the serving pool: one record per launch of either pool."""
    from llm_message_queue_amd.backend.engine import BackendEngine, Request
    from llm_message_queue_amd.models.llama_stub import LlamaConfig
    eng = BackendEngine(LlamaConfig.tiny(), slots=8, max_ctx=64, token_budget=32, device="cpu", impl="ref", seed=seed,
                        realtime_mode="micro", micro_slots=4)
    reqs = [Request(req_id=0, prompt=_prompt(40, 6), gen_tokens=4, tier=0, temperature=0.9, seed=21, top_k=6,
                    logprobs=1, presence_penalty=0.4, stop=[[5000, 5001]], logit_bias=(I32([4]), F32([0.5]))),
            Request(req_id=1, prompt=_prompt(41, 5), gen_tokens=3, tier=2),
            Request(req_id=2, prompt=_prompt(42, 4), gen_tokens=3, tier=0, temperature=0.7, seed=22,
                    min_p=MIN_P[0])]
    calls, steps = [], []
    _spy(eng, calls, steps)
    assert len(eng.admit(reqs)) == 3 and reqs[0].micro and reqs[2].micro and not reqs[1].micro
    done = 0
    for _ in range(40):
        if not eng.active and not eng.queued_steps():
            break
        eng.launch()
        eng.pump_micro()
        done += len(eng.finish(block=True).completed)
    assert done == 3 and eng.micro_steps > 0
    return {"steps": steps}


def record(seed):
    return {"pool": run_pool(seed), "micro": run_micro(seed)}


def test_min_p_values_are_safe():
    from llm_message_queue_amd.ops.sampling import min_p_log
    for mp in MIN_P:
        lg = np.log(np.float64(round(mp * 1000) / 1000.0))
        want = np.float32(lg)
        assert np.float32(np.nextafter(lg, -np.inf)) == want == np.float32(np.nextafter(lg, np.inf))
        assert min_p_log(mp) == want


def test_staged_bytes_and_head_calls_match_the_recorded_run():
    a, b = record(0), record(1)
    assert a == b                                   # nothing recorded depends on the model's weights
    with open(GOLDEN) as f:
        want = json.load(f)
    # the scenario does what it is for: every head is called in some step and
    # not in another, every counter moves, nothing stops early
    steps = a["pool"]["steps"]
    for name in HEADS:
        n = sum(any(c[0] == name for c in s["ops"]) for s in steps)
        assert 0 < n < len(steps), name
    c = a["pool"]["counters"]
    assert c["stopped_total"] == 0 and all(v > 0 for k, v in c.items() if k != "stopped_total"), c
    micro = [s for s in a["micro"]["steps"] if s["pool"] == "micro"]
    assert len(micro) >= 4 and any(len(s["ops"]) >= 6 for s in micro) and len(micro) < len(a["micro"]["steps"])
    for part in ("pool", "micro"):
        assert len(a[part]["steps"]) == len(want[part]["steps"]), part
        for i, (got, exp) in enumerate(zip(a[part]["steps"], want[part]["steps"])):
            assert got == exp, (part, i)
    assert a == want


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_step_staging_golden.py --write")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec = record(0)
    assert rec == record(1), "the records depend on the model seed"
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN, len(rec["pool"]["steps"]), "+", len(rec["micro"]["steps"]), "launches")
