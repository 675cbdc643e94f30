"""CPU: the point-loss and fold-change derivatives of csrc/pk_network_loss_grad.hpp, compiled for the host with g++ (-ffp-contract=off) and
called through a shim, against the numpy restatement of tests/net_objgrad_reference.py; and that restatement against
Richardson-extrapolated central differences of ``oracle.network_models.pointwise_loss``.

Formula against formula.  Both sides evaluate diff = obs - pred with one rounding and then at most 8 further operations (mode 5:
|pred| + 1e-6, two quotients, a square, a product, a sum; the others fewer), each with relative error 2^-53 of a term no larger than
``mag`` (the sum of the absolute values of the terms, returned by the restatement), plus libm: log 1 ulp (twice, mode 2), tanh 2 ulp
(mode 3), sqrt correctly rounded -- glibc's documented bounds.  Two evaluations, so

    |shim - restatement| <= 2 (8 + 4) 2^-53 mag = OPS_POINT 2^-53 mag,        OPS_POINT = 24.

Mode 2 subtracts two logarithms: ``mag`` carries the first-order effect of their rounding on the result (see the reference module), so
the same bound holds where they nearly cancel.  The fold-change tangent is p (one division), p dc, the difference and a division on one
side, da / c_m, p dc / c_m and the difference on the other: 4 operations each, OPS_FOLD = 8, mag = |da| / c_m + |p dc| / c_m.

Against the oracle: D(h) = (rho(pred + h) - rho(pred - h)) / 2h at h = 1e-3 and 5e-4, R = (4 D(h / 2) - D(h)) / 3.  As in
test_net_sens_reference_cpu.py the consistency |D(h) - D(h / 2)| is the tolerance (MARGIN = 2: R's truncation remainder is O(h^4), its
rounding noise at most 5/3 of the larger D's), plus the rounding of the difference quotient itself, which the consistency of an exactly
quadratic loss does not show: two values of rho, each within 16 2^-53 of itself, divided by 2 (h / 2)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import net_objgrad_reference as og
from oracle import network_models as nm

CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"
U = 2.0 ** -53
OPS_POINT, OPS_FOLD = 24, 8
MARGIN = 2.0

SHIM = r"""
#include "pk_network_loss_grad.hpp"
extern "C" {
void shim_dpred(int mode, int n, const double* obs, const double* pred, double* out) {
  for (int k = 0; k < n; ++k) out[k] = pk::point_loss_dpred(mode, obs[k], pred[k]);
}
void shim_fold(int n, const double* a, const double* c, const double* da, const double* dc, double* out) {
  for (int k = 0; k < n; ++k) out[k] = pk::fold_change_tangent(a[k], c[k], da[k], dc[k]);
}
}
"""
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_loss_grad")
    (d / "shim.cpp").write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(d / "shim.cpp"),
                    "-o", str(d / "libshim.so")], check=True)
    lib = C.CDLL(str(d / "libshim.so"))
    lib.shim_dpred.argtypes, lib.shim_dpred.restype = [C.c_int, C.c_int, DP, DP, DP], None
    lib.shim_fold.argtypes, lib.shim_fold.restype = [C.c_int, DP, DP, DP, DP, DP], None
    return lib


def _p(a):
    return a.ctypes.data_as(DP)


def _grid():
    """(obs, pred) pairs: a spread of residuals of both signs, the branch points exactly (|diff| = 0.5 and 20 with binary-exact operands),
    pred < 0 and pred = 0 (mode 5), diff < 0 (mode 2: NaN), diff -> 0+."""
    obs, pred = [], []
    for o in (0.25, 1.0, 3.5, 30.0):
        for d in (-25.0, -20.0, -3.0, -0.5, -0.25, -1e-3, 0.0, 1e-12, 1e-3, 0.25, 0.5, 0.75, 3.0, 20.0, 25.0):
            obs.append(o); pred.append(o - d)
    rng = np.random.default_rng(11)
    o = rng.uniform(0.1, 4.0, 200); p = o * np.exp(0.5 * rng.standard_normal(200))
    return np.concatenate([obs, o]), np.concatenate([pred, p])


@pytest.mark.parametrize("mode", range(8))
def test_point_loss_dpred_against_the_restatement(shim, mode):
    obs, pred = _grid()
    assert ((obs - pred) == 0.5).any() and ((obs - pred) == -20.0).any() and (pred < 0).any() and (pred == 0).any()
    out = np.full(obs.size, 7.0)
    shim.shim_dpred(mode, obs.size, _p(obs), _p(pred), _p(out))
    want, mag = np.array([og.np_point_loss_dpred(mode, float(o), float(p)) for o, p in zip(obs, pred)]).T
    if mode == 2:
        # NaN exactly where the value is NaN: a negative residual under the logarithm
        val = np.array([nm.pointwise_loss(2, float(o - p), float(o), float(p)) for o, p in zip(obs, pred)])
        assert np.array_equal(np.isnan(out), np.isnan(val)) and np.array_equal(np.isnan(out), np.isnan(want))
        assert np.isnan(out).any() and (obs - pred < 0).sum() == np.isnan(out).sum()
    else:
        assert np.isfinite(out).all()
    ok = ~np.isnan(want)
    worst = np.max(np.abs(out[ok] - want[ok]) / (U * mag[ok] + 1e-300))
    print(f"mode {mode}: worst |shim - restatement| / (2^-53 mag) = {worst:.2f} (bound {OPS_POINT})")
    assert worst <= OPS_POINT
    # the branch the value takes at a kink: mode 1 the quadratic at |diff| = 0.5, mode 3 log cosh at |diff| = 20
    if mode == 1:
        k = np.where(obs - pred == 0.5)[0][0]
        assert out[k] == -0.5 and og.np_point_loss_dpred(1, 1.0, 1.0 - 0.75)[0] == -0.5 and og.np_point_loss_dpred(1, 1.0, 1.75)[0] == 0.5
    if mode == 3:
        k = np.where(obs - pred == 20.0)[0][0]
        assert out[k] == -np.tanh(20.0) or abs(out[k] + np.tanh(20.0)) <= 4 * U
        k = np.where(obs - pred == 25.0)[0][0]
        assert out[k] == -1.0


def test_fold_change_tangent_with_each_floor_active(shim):
    eps = og.EPS
    rng = np.random.default_rng(12)
    a = np.concatenate([[0.5, eps, 0.5 * eps, 0.0, 2.0, 3.0, eps, 0.0, 2 * eps], rng.uniform(0.01, 5.0, 100)])
    c = np.concatenate([[2.0, 2.0, 2.0, 2.0, eps, 0.0, eps, 0.5 * eps, 2 * eps], rng.uniform(0.01, 5.0, 100)])
    da = rng.standard_normal(a.size); dc = rng.standard_normal(a.size)
    out = np.empty(a.size)
    shim.shim_fold(a.size, _p(a), _p(c), _p(da), _p(dc), _p(out))
    want, mag = np.array([og.np_fold_tangent(float(x), float(y), float(u), float(v)) for x, y, u, v in zip(a, c, da, dc)]).T
    assert (np.abs(out - want) <= OPS_FOLD * U * mag).all()
    # numerator floor active (a <= eps, equality included): only the baseline term; baseline floor active: only da / eps; both: 0
    for k in (1, 2, 3):
        assert abs(out[k] - (-(eps / c[k]) * dc[k] / c[k])) <= OPS_FOLD * U * abs(out[k])
    for k in (4, 5):
        assert abs(out[k] - da[k] / eps) <= OPS_FOLD * U * abs(out[k])
    assert out[6] == 0.0 and out[7] == 0.0
    # against a central difference of the floored fold change itself, away from the floors
    fc = lambda x, y: max(x, eps) / max(y, eps)
    for k in range(9, a.size):
        h = 1e-6
        fd = (fc(a[k] + h * da[k], c[k] + h * dc[k]) - fc(a[k] - h * da[k], c[k] - h * dc[k])) / (2 * h)
        assert abs(fd - out[k]) <= 1e-7 * (1.0 + mag[k])          # O(h^2) truncation + 2^-53 / h rounding, both ~1e-10 of the terms here


@pytest.mark.parametrize("mode", range(8))
def test_restatement_against_extrapolated_differences_of_the_oracle(mode):
    rng = np.random.default_rng(13 + mode)
    obs = rng.uniform(0.3, 4.0, 300)
    diff = rng.uniform(-3.0, 3.0, 300)
    diff[:40] = rng.choice([-1.0, 1.0], 40) * rng.uniform(19.0, 24.0, 40)                 # both branches of mode 3
    if mode == 2:
        diff = np.abs(diff) + 0.05                                                         # the logarithm needs a positive residual
    pred = obs - diff
    h = 1e-3
    away = np.ones(diff.size, bool)
    for kink in (0.5, 20.0):
        away &= np.abs(np.abs(diff) - kink) > 4 * h
    away &= np.abs(pred) > 4 * h
    assert away.sum() >= 250 and (np.abs(diff[away]) > 20).any() and (pred[away] < 0).any()
    rho = lambda o, p: nm.pointwise_loss(mode, o - p, o, p)
    worst = 0.0
    for o, p in zip(obs[away], pred[away]):
        o, p = float(o), float(p)
        D = [(rho(o, p + e) - rho(o, p - e)) / (2 * e) for e in (h, h / 2)]
        R = (4.0 * D[1] - D[0]) / 3.0
        cons = abs(D[0] - D[1])
        floor = 16 * U * (abs(rho(o, p + h / 2)) + abs(rho(o, p - h / 2)) + 2e-3) / h
        got = og.np_point_loss_dpred(mode, o, p)[0]
        tol = MARGIN * cons + floor
        worst = max(worst, abs(got - R) / tol)
        assert abs(got - R) <= tol, (mode, o, p, got, R, cons)
    print(f"mode {mode}: worst |restatement - R| / (MARGIN |D(h) - D(h/2)| + rounding) = {worst:.3f}")
