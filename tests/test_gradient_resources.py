"""Static resources of the gradient kernels (CPU test: reads the gfx950 code object's metadata from libmpcqp.so with
the ROCm LLVM tools, tools/kernel_resources.py).  mpc_gradient_kernel<GL, OBS> (csrc/gradient_kernel.h) exists for
GL = 16, 32, 64 with and without obstacles, uses no scratch (the per-lane row loop, the stage gradients and the
sweep's five-vectors stay in registers), and its static LDS is the header's gr_lds_doubles (26 N + 6) at the longest horizon of
the lane group (N = GL - 1) times the 64 / GL instances of a wavefront."""
import os

import pytest

from conftest import PKG, ROOT

LIB = os.path.join(PKG, "libmpcqp.so")
KEYS = [(gl, obs) for gl in (16, 32, 64) for obs in (0, 1)]


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("ROCm LLVM tools not available")
    import __graft_entry__ as g
    g.build()
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import gradient_kernel_key, kernel_resources
    return {gradient_kernel_key(k["name"]): k for k in kernel_resources(LIB) if gradient_kernel_key(k["name"])}


def test_the_six_kernels_are_present(kernels):
    assert sorted(kernels) == KEYS


@pytest.mark.parametrize("gl,obs", KEYS)
def test_no_scratch_and_the_layouts_lds(kernels, gl, obs):
    k = kernels[(gl, obs)]
    assert k["scratch"] == 0, k
    n = gl - 1
    per_instance = (5 * (n + 1) + (n + 1) + 4 * 5 * n + 1) & ~1      # Xr, kap, and ct, A, q, c [N][5] each
    assert k["lds"] == 8 * per_instance * (64 // gl), k
    assert k["vgpr"] > 0 and k["sgpr"] > 0, k                # the record was parsed
