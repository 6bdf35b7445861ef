"""Engine isolation on the HIP path: one deterministic schedule served twice
by ``BackendEngine(impl="hip")``, the second time with everything its
bookkeeping says no live row may read overwritten before every launch
(``engine_isolation_cases``: KV tails, history outside the windows, the
kernels' ``torch.empty`` scratch, the result pins).  The runs must agree bit
for bit.  A mismatch means a kernel or the engine reads state it does not own;
the message names the request, generated index, launch, slot and windows.

The windows, and the engine code they encode (a change to that bookkeeping
changes ``engine_isolation_cases.Poisoner._windows`` with it):

  KV positions of slot s valid before a launch
    active   ``s_pref[s] + max(s_gen[s] - 1, 0)``.  ``BackendEngine._build``
             advances ``s_pref`` by the chunk it stages and places a decode
             row at ``s_plen + s_gen - 1``; ``_retire`` adds one to ``s_gen``
             per sampled row, so the last sampled token has no KV yet.
    parked   ``s_cached[s]`` where ``conv_lru[s_conv[s]] == s``:
             ``_leave_slot`` parks ``s_plen + generated - 1`` positions, every
             one but the last sampled token's (``_reap_stops`` cuts it back
             for a stop found late).
    else     none (``_abort_slots`` and ``_leave_slot`` free the slot; its
             next occupant starts at ``s_pref = 0`` in ``admit``).
  device history of slot s
    active with ``s_pen[s]`` or ``s_shist[s]``: ``[lo, valid)`` with ``lo =
    s_pfrom[s]`` (``admit``: ``base + n - n_own``, the message's own prompt)
    if penalised, else ``s_plen[s]`` (``_launch_pool``'s stop records start
    at ``s_plen``); the launch itself records positions from ``valid`` on
    before any head reads them.  Every other row: none.

The precondition (two clean runs agree) is a test of its own: the HIP
forwards of these shapes are deterministic.  The KV control (poison one
position early must change tokens) runs on the CPU engine only; the two
history controls also run here, as they write nothing but ids inside the
vocabulary.
"""
import pytest
import torch

import engine_isolation_cases as C

pytestmark = pytest.mark.gpu

HIP = ("hip", "cuda:0")
# ``ops.gemm._scratch``'s users, and those the scenarios' small steps reach
# (every trunk GEMM of a step this small is the skinny kernel: no split-K
# tile, and the RMS epilogue is off by default)
SCRATCH_USERS = ("split", "rms", "skinny", "head", "trunc", "pen")
REACHED = {"skinny", "head", "trunc", "pen", "logp"}
PENALISED = {sp.rid for sp in C.SERVING if any(k.endswith("_penalty") for k in sp.kw)}


def _precondition(scenario, stream="partition"):
    a, b = C.clean(scenario, *HIP, stream), C.clean(scenario, *HIP, stream, which="B")
    assert a is not b
    msg = C.describe(a, b)
    if msg:
        msg += "\n" + C.first_hidden_difference(scenario, *HIP, stream)
    assert msg == ""
    return a


def test_two_clean_runs_agree():
    _precondition("serving")


def test_serving_scenario_covers_its_cases():
    C.check_serving_coverage(C.clean("serving", *HIP))


@pytest.mark.parametrize("classes", [("kv",), ("hist",), ("scratch",), ("pins",), C.CLASSES],
                         ids=["kv", "hist", "scratch", "pins", "all"])
def test_poisoned_serving_run_is_bit_identical(classes):
    p = C.poisoned("serving", *HIP, classes=classes)
    C.check_poison_counts(p, classes)
    if "scratch" in classes:
        print("scratch users poisoned:", sorted(p.scratch_hit), "; not reached:",
              sorted(set(SCRATCH_USERS) - p.scratch_hit))
        assert REACHED <= p.scratch_hit, (sorted(p.scratch_used), sorted(p.scratch_hit))
    assert C.describe(C.clean("serving", *HIP), p) == ""


def test_control_history_front_poison_one_position_late_changes_a_penalised_request():
    p = C.poisoned("serving", *HIP, classes=("hist",), hist_lo_shift=1)
    assert set(C.changed(C.clean("serving", *HIP), p)) & PENALISED


def test_control_history_tail_poison_one_position_early_changes_a_penalised_request():
    p = C.poisoned("serving", *HIP, classes=("hist",), hist_hi_shift=-1)
    assert set(C.changed(C.clean("serving", *HIP), p)) & PENALISED


@pytest.mark.parametrize("stream", ["partition", "high"])
def test_two_clean_micro_runs_agree(stream):
    C.check_micro_coverage(_precondition("micro", stream), graphs=True)


@pytest.mark.parametrize("stream", ["partition", "high"])
def test_poisoned_micro_run_is_bit_identical(stream):
    a = C.clean("micro", *HIP, stream)
    p = C.poisoned("micro", *HIP, stream, classes=C.CLASSES)
    C.check_poison_counts(p, C.CLASSES)
    assert any(L["micro"] and L["hist"] for L in p.launches)
    print("scratch users poisoned:", sorted(p.scratch_hit), "; not reached:",
          sorted(set(SCRATCH_USERS) - p.scratch_hit))
    assert {"skinny", "head", "pen", "logp"} <= p.scratch_hit, (sorted(p.scratch_used), sorted(p.scratch_hit))
    assert C.describe(a, p) == ""
    torch.cuda.synchronize()
