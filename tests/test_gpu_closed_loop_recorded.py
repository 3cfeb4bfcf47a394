"""The seven closed-loop entries on the device against their recorded outputs: the device section of
tests/golden/closed_loop_entries.npz (tools/record_closed_loop_entries.py documents the case set; the section was
recorded twice, bit-identically, before it was committed).  Every array but the wall-clock ones, bit for bit
(sweep_cases.same: NaN positions included), dtype and shape too.  The host twin is
tests/test_closed_loop_recorded_cpu.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_closed_loop_entries as REC  # noqa: E402

pytestmark = pytest.mark.gpu


def test_entries_equal_the_recorded_outputs():
    recorded = REC.load_section("device")
    assert len(recorded) >= 250
    assert REC.differences(REC.record(0), recorded) == []
