"""The refusals of the C entries that take host arrays, and of their *_device twins, replayed on host contexts
(device = -1): every single-fault call of tests/entry_refusal_cases.py gets the return code and the exact
*_last_error() text that was recorded for it before the entry layer was restated, and the calls that have nothing to
do (B == 0, n == 0, no output asked for) return success without touching an argument."""
import numpy as np
import pytest

import entry_refusal_cases as E


@pytest.fixture(scope="module")
def cx():
    import __graft_entry__ as g
    g.build()
    return E.Contexts()


def test_table_is_complete():
    """Every case has a recorded row and every row a case; the ten entries and their six twins are all there."""
    keys = [(entry, label) for entry, label, _, _ in E.CASES]
    assert len(set(keys)) == len(keys)
    assert set(keys) == set(E.EXPECTED)
    assert {e for e, _ in keys} == set(E.SIGNATURES) and len(E.SIGNATURES) == 16


@pytest.mark.parametrize("entry,label,kind,over", E.CASES, ids=[f"{c[0]}-{c[1]}" for c in E.CASES])
def test_refusal(cx, entry, label, kind, over):
    rc, text, args = cx.call(entry, kind, over)
    print(entry, "|", label, "|", rc, "|", text)
    assert (rc, text) == E.EXPECTED[(entry, label)]
    fresh = E.good_args(entry)
    for name, a in args.items():
        if isinstance(a, np.ndarray) and name not in over:
            assert np.array_equal(a, fresh[name], equal_nan=True), (name, "written by a refused call")


@pytest.mark.parametrize("entry,label,over", E.NOOPS, ids=[f"{c[0]}-{c[1]}" for c in E.NOOPS])
def test_nothing_to_do_is_success(cx, entry, label, over):
    kind = "plan" if entry.startswith("plan_") else "mo2"
    rc, _, args = cx.call(entry, kind, over)
    assert rc == 0
    fresh = E.good_args(entry)
    for name, a in args.items():
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, fresh[name], equal_nan=True), (name, "written by a call with nothing to do")
