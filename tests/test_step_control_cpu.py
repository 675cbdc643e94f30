"""CPU: step_h0 and step_fac of csrc/pk_step.hpp -- the first step and the clamped step-size divisor that the kernels call -- compiled
for the host with g++ (-ffp-contract=off: neither function holds a product that feeds an addition) and checked on value tables."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"

SHIM = r"""
#include "pk_step.hpp"
extern "C" {
double shim_h0(double d0, double d1, double h0) { return pk::step_h0(d0, d1, h0); }
double shim_fac(double root) { return pk::step_fac(root); }
double shim_fac_lo(double root, double lo) { return pk::step_fac(root, lo); }
double shim_fac_all(double root, double lo, double safety_inv) { return pk::step_fac(root, lo, safety_inv); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_step")
    (d / "shim.cpp").write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(d / "shim.cpp"),
                    "-o", str(d / "libshim.so")], check=True)
    lib = C.CDLL(str(d / "libshim.so"))
    for f, n in ((lib.shim_h0, 3), (lib.shim_fac, 1), (lib.shim_fac_lo, 2), (lib.shim_fac_all, 3)):
        f.argtypes, f.restype = [C.c_double] * n, C.c_double
    return lib


def bits(x):
    return int(np.float64(x).view(np.int64))


def test_step_h0_table(shim):
    nan, inf = np.nan, np.inf
    for d0, d1, h0, want in [(2.0, 4.0, 0.0, 0.01 * 2.0 / 4.0), (3.0, 7.0, -1.0, 0.01 * 3.0 / 7.0), (0.0, 4.0, 0.0, 1e-6), (2.0, 0.0, 0.0, 1e-6),
                             (1e-5, 4.0, 0.0, 1e-6), (nan, 4.0, 0.0, 1e-6), (2.0, nan, 0.0, 1e-6), (nan, nan, 0.0, 1e-6), (2.0, inf, 0.0, 1e-6),
                             (inf, inf, 0.0, 1e-6), (2.0, 4.0, 0.25, 0.25), (nan, 0.0, 1.0, 1.0), (2.0, 4.0, nan, 0.01 * 2.0 / 4.0),
                             (2.0, 4.0, inf, inf)]:
        assert bits(shim.shim_h0(d0, d1, h0)) == bits(want), (d0, d1, h0)


def test_step_fac_table(shim):
    s = 1.0 / 0.9
    for root in (0.0, 1e-3, 0.9 / 6.0, 0.15, 0.2, 0.45, 0.5, 1.0, 4.4, 4.5, 4.6, 1e30):
        assert bits(shim.shim_fac(root)) == bits(max(1.0 / 6.0, min(5.0, root * s)))
        assert bits(shim.shim_fac_lo(root, 0.5)) == bits(max(0.5, min(5.0, root * s)))
        assert bits(shim.shim_fac_lo(root, 1.0 / 3.0)) == bits(max(1.0 / 3.0, min(5.0, root * s)))
        assert bits(shim.shim_fac_all(root, 0.25, 1.0 / 0.8)) == bits(max(0.25, min(5.0, root * (1.0 / 0.8))))
    assert shim.shim_fac(0.0) == 1.0 / 6.0 and shim.shim_fac_lo(0.0, 0.5) == 0.5 and shim.shim_fac_lo(0.0, 0.3) == 0.3
    assert shim.shim_fac(1e30) == 5.0 and shim.shim_fac_all(4.1, 0.25, 1.0 / 0.8) == 5.0 and shim.shim_fac_all(3.9, 0.25, 1.0 / 0.8) < 5.0
    assert shim.shim_fac(np.nan) == 5.0                                  # C's fmin drops the NaN: the clamp's upper edge (the kernels test err before they call it)
