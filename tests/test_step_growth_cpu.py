"""CPU: step_growth of csrc/pk_step.hpp -- the clamped step-size MULTIPLIER hnew = hs * step_growth(err^(-1/Q)) that the distributive
throughput kernel takes in place of hnew = hs / step_fac(err^(1/Q)) -- compiled for the host with g++ as tests/test_step_control_cpu.py does,
and held to the reciprocal of step_fac: the same rule, clamps [1/5, 6] for [1/6, 5], safety 0.9 for 1 / 0.9."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"

SHIM = r"""
#include "pk_step.hpp"
extern "C" {
double shim_fac(double root) { return pk::step_fac(root); }
double shim_growth(double root_inv) { return pk::step_growth(root_inv); }
double shim_growth_all(double root_inv, double hi, double safety) { return pk::step_growth(root_inv, hi, safety); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_growth")
    (d / "shim.cpp").write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(d / "shim.cpp"),
                    "-o", str(d / "libshim.so")], check=True)
    lib = C.CDLL(str(d / "libshim.so"))
    for f, n in ((lib.shim_fac, 1), (lib.shim_growth, 1), (lib.shim_growth_all, 3)):
        f.argtypes, f.restype = [C.c_double] * n, C.c_double
    return lib


def bits(x):
    return int(np.float64(x).view(np.int64))


def test_step_growth_is_the_reciprocal_of_step_fac(shim):
    """A log sweep of r = err^(1/Q) over 1e-3 .. 1e3, both clamps and the free range between them (r in 0.15 .. 4.5).  Four ulps: 1 / r,
    the product with 0.9 and the literal 0.9 itself round once each on one side; 1 / 0.9, the product and the division on the other."""
    worst, free = 0.0, 0
    for r in 10.0 ** np.linspace(-3.0, 3.0, 6001):
        want = 1.0 / shim.shim_fac(r)
        got = shim.shim_growth(1.0 / r)
        worst = max(worst, abs(got - want) / np.spacing(want))
        free += 0.2 < got < 6.0
        assert abs(got - want) <= 4.0 * np.spacing(want), (r, got, want)
    print("largest |step_growth(1 / r) - 1 / step_fac(r)|: %.2f ulps; %d of 6001 samples between the clamps" % (worst, free))
    assert free > 1000


def test_step_growth_sits_on_its_clamps(shim):
    for x in (0.0, 1e-30, 1e-3, 0.2, 0.2 / 0.9 * (1.0 - 1e-15)):
        assert bits(shim.shim_growth(x)) == bits(0.2), x
    for x in (6.0 / 0.9 * (1.0 + 1e-15), 7.0, 1e3, 1e30, np.inf):
        assert bits(shim.shim_growth(x)) == bits(6.0), x
    for x in (0.25, 0.5, 1.0, 1.0 / 0.9, 3.0, 6.0):
        assert bits(shim.shim_growth(x)) == bits(x * 0.9) and 0.2 < shim.shim_growth(x) < 6.0, x
    # the other two arguments: the cap and the safety factor
    assert shim.shim_growth_all(10.0, 4.0, 0.8) == 4.0 and shim.shim_growth_all(0.1, 4.0, 0.8) == 0.2
    assert bits(shim.shim_growth_all(2.0, 4.0, 0.8)) == bits(2.0 * 0.8)


def test_a_nan_takes_the_shrinking_clamp_as_in_step_fac(shim):
    """C's fmin / fmax drop a NaN: step_fac(NaN) is its upper edge 5 (the step shrinks fivefold), step_growth(NaN) the matching lower edge
    1 / 5.  The kernels test err before they call either."""
    assert shim.shim_fac(np.nan) == 5.0
    assert bits(shim.shim_growth(np.nan)) == bits(0.2)
    assert bits(shim.shim_growth(np.nan)) == bits(1.0 / shim.shim_fac(np.nan))
