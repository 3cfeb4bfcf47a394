"""Static resources of the plan-trace kernels (CPU test: reads the gfx950 code object's metadata from libmpcqp.so
with the ROCm LLVM tools, tools/kernel_resources.py).  tg_gap_kernel and tg_hist_kernel (csrc/trace_kernels.h) are
plain load / compare / store kernels whose lookahead table travels as a kernel argument: they use no scratch and no
LDS.  A lookahead lookup that turned into a dynamically indexed private copy of the argument would show up here as
scratch."""
import os
import re

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "safe-autonomous-driving-mpc_amd", "libmpcqp.so")
KERNELS = ("tg_gap_kernel", "tg_hist_kernel", "tg_init_kernel")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("ROCm LLVM tools not available")
    import __graft_entry__ as g
    g.build()
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    out = {}
    for k in kernel_resources(LIB):
        m = re.match(r"_Z\d+(tg_\w+?_kernel)", k["name"])
        if m:
            out[m.group(1)] = k
    return out


def test_trace_kernels_present(kernels):
    assert set(KERNELS) <= set(kernels), sorted(kernels)


@pytest.mark.parametrize("name", KERNELS)
def test_trace_kernels_use_no_scratch_and_no_lds(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["lds"] == 0, k
    assert k["vgpr"] > 0 and k["sgpr"] > 0, k                # the record was parsed
