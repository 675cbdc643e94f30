"""CPU: the per-row rules of the native Levenberg-Marquardt driver (csrc/pk_lm.hpp) -- free set, Marquardt scaling, damped masked solve,
projection, predicted reduction, accept rule and damping update -- compiled for the host with g++ (-ffp-contract=off) and held to a numpy
restatement of the rules of paramest/multistart.py::fit_rows_batch; the pure-host behaviour of the entry point; and once a stand-alone
sanitizer build of the largest solve."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"

SHIM = r"""
#include <vector>
#include "pk_lm.hpp"
using namespace pk;
extern "C" {
void shim_step(int P, const double* A, const unsigned char* fr, const double* DD, const double* g, double mu, int lv, double* step) {
  std::vector<double> L(lm_tri_len(P));
  lm_damped_step(P, A, P, fr, DD, g, mu, lv, L.data(), step, LmSerial());
}
double shim_project_pred(int P, const double* A, const double* g, const double* p, const double* lb, const double* ub, const double* step,
                         double* trial, double* dp) {
  std::vector<double> work(P);
  lm_project(P, p, lb, ub, step, trial, dp, LmSerial());
  return lm_predicted(P, A, P, g, dp, work.data(), LmSerial());
}
// one trial round of one row, as the accept kernel runs it: first acceptable level (-1: none) and the damping value after it
int shim_round(double mu, double cost, int K, const double* cn, const double* pred, double* mu_out, double* rho_out) {
  for (int lv = 0; lv < K; ++lv) {
    const double rho = lm_rho(cost, cn[lv], pred[lv]);
    if (lm_acceptable(cost, cn[lv], rho)) { *mu_out = lm_mu_accept(mu, lv, rho); *rho_out = rho; return lv; }
  }
  *mu_out = lm_mu_reject(mu, K);
  return -1;
}
double shim_pow4(int lv) { return lm_pow4(lv); }
double shim_scale(double aii) { return lm_scale(aii); }
int shim_fixed(double p, double lb, double ub, double g) { return lm_fixed(p, lb, ub, g); }
int shim_done(int n_free, double gnorm, double cost) { return lm_row_done(n_free, gnorm, cost); }
int shim_converged(double dc, double cn, double dx, double xn, double ftol, double xtol) { return lm_converged(dc, cn, dx, xn, ftol, xtol); }
int shim_levels(int trial_levels, long long pending, int tries) { return lm_round_levels(trial_levels, pending, tries); }
}
"""

# The sanitizer run: the P = 138 solve (every index of the packed triangle is touched) and the failed pivot, in a program of its own.
MAIN = r"""
#include <cstdio>
#include <vector>
#include "pk_lm.hpp"
using namespace pk;
int main() {
  const int P = 138;
  std::vector<double> A((size_t)P * P), DD(P), g(P), step(P), L(lm_tri_len(P)), p(P, 0.5), lb(P, 0.0), ub(P, 1.0), trial(P), dp(P), work(P);
  std::vector<unsigned char> fr(P, 1);
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) A[(size_t)i * P + j] = (i == j ? P + 1.0 : 0.0) + 1.0 / (1.0 + i + j);
  for (int i = 0; i < P; ++i) { DD[i] = lm_scale(A[(size_t)i * P + i]); g[i] = (i % 7) - 3.0; fr[i] = i % 5 != 0; }
  lm_damped_step(P, A.data(), P, fr.data(), DD.data(), g.data(), 1e-3, 2, L.data(), step.data(), LmSerial());
  double worst = 0.0;                                   // residual of the damped system on the free set
  for (int i = 0; i < P; ++i) {
    if (!fr[i]) { if (step[i] != 0.0) return 2; continue; }
    double s = g[i] + 1e-3 * 16.0 * DD[i] * DD[i] * step[i];
    for (int j = 0; j < P; ++j) if (fr[j]) s += A[(size_t)i * P + j] * step[j];
    worst = fmax(worst, fabs(s));
  }
  if (!(worst < 1e-9)) return 3;
  lm_project(P, p.data(), lb.data(), ub.data(), step.data(), trial.data(), dp.data(), LmSerial());
  const double pred = lm_predicted(P, A.data(), P, g.data(), dp.data(), work.data(), LmSerial());
  if (!(pred > 0.0)) return 4;
  A[(size_t)17 * P + 17] = -1.0;                         // a negative pivot in the free block: zero step
  lm_damped_step(P, A.data(), P, fr.data(), DD.data(), g.data(), 1e-3, 0, L.data(), step.data(), LmSerial());
  for (int i = 0; i < P; ++i) if (step[i] != 0.0) return 5;
  std::printf("ok %.3e %.6e\n", worst, pred);
  return 0;
}
"""

DBL, U8P = C.c_double, C.POINTER(C.c_ubyte)
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_lm")
    (d / "shim.cpp").write_text(SHIM)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{CSRC}", str(d / "shim.cpp"),
                    "-o", str(d / "libshim.so")], check=True)
    lib = C.CDLL(str(d / "libshim.so"))
    lib.shim_step.argtypes, lib.shim_step.restype = [C.c_int, DP, U8P, DP, DP, DBL, C.c_int, DP], None
    lib.shim_project_pred.argtypes, lib.shim_project_pred.restype = [C.c_int] + [DP] * 8, DBL
    lib.shim_round.argtypes, lib.shim_round.restype = [DBL, DBL, C.c_int, DP, DP, DP, DP], C.c_int
    lib.shim_pow4.argtypes, lib.shim_pow4.restype = [C.c_int], DBL
    lib.shim_scale.argtypes, lib.shim_scale.restype = [DBL], DBL
    lib.shim_fixed.argtypes, lib.shim_fixed.restype = [DBL] * 4, C.c_int
    lib.shim_done.argtypes, lib.shim_done.restype = [C.c_int, DBL, DBL], C.c_int
    lib.shim_converged.argtypes, lib.shim_converged.restype = [DBL] * 6, C.c_int
    lib.shim_levels.argtypes, lib.shim_levels.restype = [C.c_int, C.c_longlong, C.c_int], C.c_int
    return lib


def dp(a):
    return a.ctypes.data_as(DP)


def bits(x):
    return int(np.float64(x).view(np.int64))


def spd(rng, P):
    """A = M^T M with M [3 P + 2, P] standard normal, made exactly symmetric.  Its condition number is about ((sqrt 3 + 1) / (sqrt 3 - 1))^2
    = 14 at large P (Marchenko-Pastur edges) and the damping only lowers it, so two backward-stable solves of the damped system differ by a
    few P * cond * 2^-53 < 1e-12 relative: the 1e-10 (1 + |step|) bound below leaves two orders of room and none for a wrong entry."""
    M = rng.standard_normal((3 * P + 2, P))
    A = M.T @ M
    return 0.5 * (A + A.T)


def step_ref(A, free, DD, g, mu, lv):
    """The damped system of fit_rows_batch (multistart.py, host algebra) for one row."""
    Af = A * (free[:, None] & free[None, :])
    Af[np.arange(A.shape[0]), np.arange(A.shape[0])] += np.where(free, (mu * 4.0 ** lv) * DD ** 2, 1.0)
    return np.linalg.solve(Af, np.where(free, -g, 0.0))


def run_step(shim, A, free, DD, g, mu, lv):
    P = A.shape[0]
    out = np.full(P, np.nan)
    fr = np.ascontiguousarray(free.astype(np.uint8))
    shim.shim_step(P, dp(np.ascontiguousarray(A)), fr.ctypes.data_as(U8P), dp(DD), dp(g), mu, lv, dp(out))
    return out


@pytest.mark.parametrize("P", [1, 2, 7, 64, 138])
def test_damped_masked_solve_matches_numpy(shim, P):
    rng = np.random.default_rng(1000 + P)
    A = spd(rng, P)
    DD = np.maximum(np.sqrt(np.diag(A)), 1e-12)
    assert all(bits(shim.shim_scale(a)) == bits(d) for a, d in zip(np.diag(A), DD))
    one_free = np.zeros(P, bool); one_free[P // 2] = True
    masks = [np.ones(P, bool), one_free, np.zeros(P, bool)] + [rng.random(P) < q for q in (0.3, 0.8)]
    for k, free in enumerate(masks):
        g = rng.standard_normal(P) * 10.0
        for lv, mu in ((0, 1e-3), (2, 1e-3), (5, 7.0), (0, 1e-12)):
            got = run_step(shim, A, free, DD, g, mu, lv)
            want = step_ref(A, free, DD, g, mu, lv)
            assert np.all(np.abs(got - want) <= 1e-10 * (1.0 + np.abs(want))), (P, k, lv, np.abs(got - want).max())
            assert np.all(got[~free] == 0.0) and not np.signbit(got[~free]).any()
    assert np.all(run_step(shim, A, np.zeros(P, bool), DD, rng.standard_normal(P), 1e-3, 0) == 0.0)


def test_failed_factorisation_gives_a_zero_step(shim):
    rng = np.random.default_rng(5)
    P = 7
    A = spd(rng, P)
    DD = np.maximum(np.sqrt(np.diag(A)), 1e-12)
    g = rng.standard_normal(P)
    free = np.ones(P, bool)
    bad = A.copy(); bad[3, 3] = -1.0                                   # negative pivot
    assert np.all(run_step(shim, bad, free, DD, g, 1e-3, 0) == 0.0)
    assert np.all(run_step(shim, np.zeros((P, P)), free, np.zeros(P), g, 1e-3, 0) == 0.0)       # zero pivot: nothing on the diagonal
    sing = np.ones((P, P))                                              # rank one, no damping: the second pivot is 0
    assert np.all(run_step(shim, sing, free, np.zeros(P), g, 1e-3, 0) == 0.0)
    nan = A.copy(); nan[0, 0] = np.nan
    assert np.all(run_step(shim, nan, free, DD, g, 1e-3, 0) == 0.0)
    inf = A.copy(); inf[2, 2] = np.inf
    assert np.all(run_step(shim, inf, free, DD, g, 1e-3, 0) == 0.0)
    # masked away, the bad entry does no harm: the fixed variable gets 0 and the rest is the numpy solve
    fr = free.copy(); fr[3] = False
    got = run_step(shim, bad, fr, DD, g, 1e-3, 1)
    want = step_ref(bad, fr, DD, g, 1e-3, 1)
    assert got[3] == 0.0 and np.all(np.abs(got - want) <= 1e-10 * (1.0 + np.abs(want)))


@pytest.mark.parametrize("P", [1, 2, 7, 64, 138])
def test_projection_and_predicted_reduction(shim, P):
    rng = np.random.default_rng(2000 + P)
    A = spd(rng, P)
    g = rng.standard_normal(P) * 5.0
    lb, ub = -np.ones(P), np.ones(P)
    p = np.clip(rng.uniform(-1.2, 1.2, P), lb, ub) if P > 2 else np.zeros(P)        # some variables start on the box
    if P > 2:                                                           # two steps certainly leave the box, one cannot
        p[0], g[0], p[1], g[1], p[2] = lb[0], 3.0, ub[1], -2.0, 0.0
    # a descent step, short enough that the quadratic term is about a tenth of the linear one: every term of g . dp has one sign, so the
    # result carries no cancellation and "1e-13 relative" is a bound on rounding alone (two nested sums of P terms: < 2 P 2^-53 = 3e-14)
    step = -g * (0.1 / (1.5 * P))
    trial, d = np.empty(P), np.empty(P)
    pred = shim.shim_project_pred(P, dp(A), dp(g), dp(p), dp(lb), dp(ub), dp(step), dp(trial), dp(d))
    want_trial = np.clip(p + step, lb, ub)
    want_dp = want_trial - p
    np.testing.assert_array_equal(trial, want_trial)
    np.testing.assert_array_equal(d, want_dp)
    if P > 2:
        assert ((want_dp == 0.0) & (step != 0.0)).any() and (want_dp != 0.0).any()      # some steps were cut at the box
    want = -(g @ want_dp + 0.5 * want_dp @ (A @ want_dp))
    assert want > 0.0 and abs(pred - want) <= 1e-13 * abs(want)


def round_ref(mu, cost, cn, pred):
    """The accept rule and damping update of fit_rows_batch, with its own expressions."""
    cn, pred = np.asarray(cn, float), np.asarray(pred, float)
    K = cn.size
    rho = np.where(pred > 0, (cost - cn) / np.where(pred > 0, pred, 1.0), -1.0)
    okl = (cn < cost) & (rho > 1e-4)
    if not okl.any():
        return -1, mu * 4.0 ** K
    lvl = int(np.argmax(okl))
    return lvl, float(np.maximum(mu * 4.0 ** lvl * np.where(rho[lvl] > 0.75, 1.0 / 3.0, 1.0), 1e-12))


@pytest.mark.parametrize("name,mu,cost,cn,pred,lvl", [
    ("first level taken, good gain", 1e-3, 10.0, [5.0, 4.0, 3.0], [6.0, 5.0, 4.0], 0),
    ("first level taken, poor gain", 1e-3, 10.0, [9.0, 4.0, 3.0], [6.0, 5.0, 4.0], 0),
    ("second level taken with rho > 0.75", 0.37, 10.0, [11.0, 2.0, 1.0], [6.0, 9.0, 4.0], 1),
    ("third level taken, rho just above 1e-4", 0.37, 10.0, [11.0, 10.5, 9.9995], [6.0, 9.0, 4.0], 2),
    ("none taken", 0.123, 10.0, [11.0, 12.0, 10.0000001], [6.0, 9.0, 4.0], -1),
    ("none taken, one level", 0.123, 10.0, [11.0], [6.0], -1),
    ("floor at 1e-12", 2e-12, 10.0, [1.0], [9.5], 0),
    ("pred <= 0", 1e-3, 10.0, [5.0, 5.0], [0.0, -3.0], -1),
    ("cn == cost", 1e-3, 10.0, [10.0, 10.0, 10.0], [1e-30, 5.0, -1.0], -1),
    ("rho at most 1e-4", 1e-3, 10.0, [9.9999], [2.0], -1),
    ("twelve levels rejected", 1e-3, 1.0, [2.0] * 12, [1.0] * 12, -1),
])
def test_accept_rule_and_damping_update_are_the_python_expressions(shim, name, mu, cost, cn, pred, lvl):
    cn_a, pred_a = np.asarray(cn, float), np.asarray(pred, float)
    mu_out, rho_out = C.c_double(np.nan), C.c_double(np.nan)
    got = shim.shim_round(mu, cost, cn_a.size, dp(cn_a), dp(pred_a), C.byref(mu_out), C.byref(rho_out))
    want_lvl, want_mu = round_ref(mu, cost, cn, pred)
    assert want_lvl == lvl, name                                        # the table says what it claims
    assert got == lvl, name
    assert bits(mu_out.value) == bits(want_mu), name
    if lvl >= 0:
        assert bits(rho_out.value) == bits((cost - cn[lvl]) / pred[lvl])
    if name == "floor at 1e-12":
        assert mu_out.value == 1e-12


def test_small_rules(shim):
    for lv in range(13):
        assert bits(shim.shim_pow4(lv)) == bits(4.0 ** lv)
    # free set: fixed iff on a bound with the gradient pointing out of the box
    for p, lb, ub, g, fixed in [(0.0, 0.0, 1.0, 2.0, 1), (0.0, 0.0, 1.0, -2.0, 0), (0.0, 0.0, 1.0, 0.0, 0), (1.0, 0.0, 1.0, -1e-300, 1), (1.0, 0.0, 1.0, 3.0, 0),
                                (0.5, 0.0, 1.0, 9.0, 0), (0.5, 0.5, 0.5, 1.0, 1), (0.5, 0.5, 0.5, -1.0, 1), (0.5, 0.5, 0.5, 0.0, 0), (0.0, 0.0, 1.0, np.nan, 0)]:
        assert shim.shim_fixed(p, lb, ub, g) == fixed, (p, lb, ub, g)
    assert shim.shim_scale(0.0) == 1e-12 and shim.shim_scale(4.0) == 2.0 and shim.shim_scale(1e-30) == 1e-12
    # done: nothing free, or |g_free| < 1e-14 max(1, cost)
    assert shim.shim_done(0, 5.0, 1.0) == 1 and shim.shim_done(3, 0.0, 0.0) == 1 and shim.shim_done(3, 0.9e-14, 0.5) == 1
    assert shim.shim_done(3, 1e-14, 0.5) == 0 and shim.shim_done(3, 0.9e-8, 1e6) == 1 and shim.shim_done(3, 1.1e-8, 1e6) == 0
    # convergence of an accepted step: dc <= ftol max(cn, 1e-300) or dx <= xtol (xtol + |trial|)
    f = x = 1e-10
    assert shim.shim_converged(1e-11, 1.0, 1.0, 1.0, f, x) == 1 and shim.shim_converged(1e-9, 1.0, 1.0, 1.0, f, x) == 0
    assert shim.shim_converged(1.0, 1.0, 1e-10, 1.0, f, x) == 1 and shim.shim_converged(1.0, 1.0, 1.1e-10, 1.0, f, x) == 0
    assert shim.shim_converged(0.0, 0.0, 1.0, 1.0, f, x) == 1 and shim.shim_converged(1e-200, 0.0, 1.0, 1.0, f, x) == 0
    # levels of a round: three while at most 256 rows pend, one beyond; the caller's number otherwise; never past the 12 tries
    assert [shim.shim_levels(0, m, 0) for m in (1, 256, 257, 480)] == [3, 3, 1, 1]
    assert shim.shim_levels(0, 5, 9) == 3 and shim.shim_levels(0, 5, 10) == 2 and shim.shim_levels(5, 5, 10) == 2 and shim.shim_levels(12, 999, 0) == 12
    assert shim.shim_levels(1, 5, 11) == 1 and shim.shim_levels(7, 5, 0) == 7


def test_entry_point_host_behaviour(built_lib):
    from phoskintime_amd import _capi
    cnt = (C.c_int64 * 6)()
    assert built_lib.pk_fit_protein_rows_batch(None, 0, 4, 1, None, None, 0, None, 14, None, 0, None, 0, None, None, None, 0, None, None,
                                               None, None, None, None, None, C.byref(cnt)) < 0
    o = _capi.FitOpts(max_iter=-5, trial_levels=9, log_space=7, use_reg=7, ftol=0.5, xtol=0.25)
    built_lib.pk_default_fit_opts(C.byref(o))
    assert (o.max_iter, o.trial_levels, o.log_space, o.use_reg, o.ftol, o.xtol) == (100, 0, 0, 0, 1e-10, 1e-10)
    built_lib.pk_default_fit_opts(None)
    d = _capi.default_fit_opts(max_iter=3, use_reg=1)
    assert (d.max_iter, d.trial_levels, d.use_reg, d.ftol) == (3, 0, 1, 1e-10)
    with pytest.raises(TypeError):
        _capi.default_fit_opts(nonsense=1)


def test_fit_opts_struct_size(tmp_path):
    from phoskintime_amd import _capi
    root = Path(__file__).resolve().parents[1]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "phoskin.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(pk_fit_opts), '
                   'offsetof(pk_fit_opts, use_reg), offsetof(pk_fit_opts, xtol)); return 0;}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(_capi.FitOpts), _capi.FitOpts.use_reg.offset, _capi.FitOpts.xtol.offset] == [32, 12, 24]


def test_largest_solve_and_failed_pivot_run_clean_under_sanitizers(tmp_path):
    """A stand-alone host program over pk_lm.hpp (its own main, nothing loaded into Python) with the address and undefined-behaviour
    sanitizers: the P = 138 damped solve with a mixed free set, its projection and predicted reduction, then the failed-pivot path."""
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = tmp_path / "lm_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{CSRC}", str(tmp_path / "main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
