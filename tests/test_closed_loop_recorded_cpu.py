"""The seven closed-loop entries on the host backend (device = -1) against their recorded outputs: the host section
of tests/golden/closed_loop_entries.npz, written by tools/record_closed_loop_entries.py (which also documents the
case set).  An absolute pin: the anchor tests compare one entry with the next and the entries share their loop, so
this file says what each call returned when it was recorded.  Every array but the wall-clock ones, bit for bit
(sweep_cases.same: NaN positions included), dtype and shape too."""
import os
import sys

import pytest

import sweep_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_closed_loop_entries as REC  # noqa: E402

CALLS = {f"{e}_{form}" for e in ("sweep", "traffic", "convoy", "noisy", "traced", "warm")
         for form in ("per_ego", "shared", "b1")} | {"loop_both", "loop_none", "loop_b1"}


@pytest.fixture(scope="module")
def recorded():
    return REC.load_section("host")


def test_the_fixture_holds_the_case_set(recorded):
    """Every call of the case set is there, and the set does what it is for: an ego leaves before the first sync,
    the others run to the cap, the histories of egos 4 and 1 are kept, the noise reaches the applied control,
    carrying the plans changes the controls and every ego that ran was reset at least once (its first step)."""
    assert {k.split("__")[0] for k in recorded} == CALLS and len(recorded) >= 250
    nz = {k.split("__")[1]: v for k, v in recorded.items() if k.startswith("noisy_per_ego__")}
    assert nz["n_steps"][5] < 8 and nz["n_steps"].max() == REC.STEPS
    assert nz["hist_egos"].tolist() == REC.HIST_EGOS and nz["hist_x"].shape == (2, REC.STEPS + 1, 5)
    assert not SC.same(nz["hist_ua"], nz["hist_u"]) and nz["quant"].shape == (6, 11)
    assert not SC.same(recorded["warm_per_ego__hist_u"], recorded["traced_per_ego__hist_u"])
    n_reset, ran = recorded["warm_per_ego__warmq"][:, 0], recorded["warm_per_ego__n_steps"]
    assert ((n_reset >= 1) & (n_reset <= ran))[ran > 0].all() and (ran > 0).any()


def test_entries_equal_the_recorded_outputs(recorded):
    assert REC.differences(REC.record(-1), recorded) == []
