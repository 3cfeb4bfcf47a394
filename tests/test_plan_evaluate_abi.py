"""The evaluator's C boundary: libmpcplan.so exports exactly the entry points the companion header
include/mpcplan_evaluate.h declares (tests/test_plan_abi.py does the same for include/mpcplan.h, which stays the
solver's boundary with its 12 entries), the Python binding lists them, its column names mirror the header's enums, and
MPCPLAN_VERSION is not stepped (callers detect the evaluator by the presence of the symbols)."""
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "mpcplan_evaluate.h")
LIB = os.path.join(PKG, "libmpcplan.so")


def header_text():
    with open(HEADER) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return LIB


def test_library_exports_the_declared_evaluator_entries(built):
    names = sorted(set(re.findall(r"^\s*int\s+(plan_[a-z_]+)\s*\(", header_text(), flags=re.M)))
    assert names == ["plan_check_verdicts", "plan_evaluate_chunks", "plan_evaluate_chunks_device"]
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(plan_[a-z_]+)$", out, flags=re.M))
    assert not [n for n in names if n not in exported]
    import mpcplan
    assert sorted(mpcplan.EVALUATE_EXPORTS) == names
    assert exported == set(mpcplan.EXPORTS) | set(mpcplan.EVALUATE_EXPORTS)
    assert mpcplan.lib().plan_version() == 3


def test_python_names_mirror_the_headers_enums(built):
    import mpcplan
    src = header_text()
    enums = [re.findall(r"[A-Z][A-Z0-9_]+", body) for body in re.findall(r"enum\s*\{(.*?)\}", src, flags=re.S)]
    rows, cols, bits = enums
    assert [n[len("PLAN_EVR_"):].lower() for n in rows] == [
        {"slack": "s"}.get(n, n) for n in mpcplan.EV_ROW_NAMES]
    assert cols[-1] == "PLAN_EV_NQ" and [n[len("PLAN_EVQ_"):].lower() for n in cols[:-1]] == list(mpcplan.EV_SUMMARY_NAMES)
    assert [n[len("PLAN_CHKB_"):].lower() for n in bits] == list(mpcplan.CHECK_NAMES)
    assert int(re.search(r"#define\s+PLAN_EV_NR\s+(\d+)", src).group(1)) == mpcplan.PLAN_EV_NR == len(rows)
    for name in ("DISTANCE", "VELOCITY", "CONTROLS", "LATERAL_DEV", "SLACK"):
        v = float(re.search(rf"#define\s+PLAN_CHK_{name}_TOL\s+([0-9.]+)", src).group(1))
        assert v == getattr(mpcplan, f"PLAN_CHK_{name}_TOL"), name
    import sanity_checks as SC
    assert (mpcplan.PLAN_CHK_DISTANCE_TOL, mpcplan.PLAN_CHK_VELOCITY_TOL, mpcplan.PLAN_CHK_CONTROLS_TOL,
            mpcplan.PLAN_CHK_LATERAL_DEV_TOL, mpcplan.PLAN_CHK_SLACK_TOL) == (
        SC.PLAN_DISTANCE_TOL, SC.PLAN_VELOCITY_TOL, SC.PLAN_CONTROLS_TOL, SC.PLAN_LATERAL_DEV_TOL, SC.PLAN_SLACK_TOL)
