"""Engine isolation on the CPU reference engine (``impl="ref"``): the state
``BackendEngine`` carries from step to step, checked by poisoning everything
its bookkeeping says no live row may read (``engine_isolation_cases``) and
requiring bit-identical results.

The controls show that the poison is effective here: moving a window edge by
one position into live data changes what requests generate.  The reference
engine has no scratch workspaces, so the ``scratch`` class exists only in
``test_gpu_engine_isolation.py``.
"""
import pytest

import engine_isolation_cases as C

PENALISED = {sp.rid for sp in C.SERVING if any(k.endswith("_penalty") for k in sp.kw)}


def test_two_clean_runs_agree():
    a, b = C.clean("serving"), C.clean("serving", which="B")
    assert a is not b
    assert C.describe(a, b) == ""


def test_serving_scenario_covers_its_cases():
    C.check_serving_coverage(C.clean("serving"))


@pytest.mark.parametrize("classes", [("kv",), ("hist",), ("pins",), ("kv", "hist", "pins")],
                         ids=["kv", "hist", "pins", "all"])
def test_poisoned_serving_run_is_bit_identical(classes):
    p = C.poisoned("serving", classes=classes)
    C.check_poison_counts(p, classes)
    assert C.describe(C.clean("serving"), p) == ""


def test_micro_scenario_clean_and_poisoned():
    a, b = C.clean("micro"), C.clean("micro", which="B")
    assert C.describe(a, b) == ""
    C.check_micro_coverage(a, graphs=False)          # (graphs are captured on the GPU only)
    classes = ("kv", "hist", "pins")
    p = C.poisoned("micro", classes=classes)
    C.check_poison_counts(p, classes)
    assert any(L["micro"] and L["hist"] for L in p.launches)
    assert C.describe(a, p) == ""


# ----------------------------------------------------------------------------- controls
def test_control_kv_poison_one_position_early_changes_tokens():
    p = C.poisoned("serving", classes=("kv",), kv_shift=-1)
    assert C.changed(C.clean("serving"), p)


def test_control_history_front_poison_one_position_late_changes_a_penalised_request():
    p = C.poisoned("serving", classes=("hist",), hist_lo_shift=1)
    assert set(C.changed(C.clean("serving"), p)) & PENALISED


def test_control_history_tail_poison_one_position_early_changes_a_penalised_request():
    p = C.poisoned("serving", classes=("hist",), hist_hi_shift=-1)
    assert set(C.changed(C.clean("serving"), p)) & PENALISED
