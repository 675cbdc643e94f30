"""CPU: the long-double restatement of one Levenberg-Marquardt iteration (tests/lm_reference.py) against the host build of csrc/pk_lm.hpp
that tests/test_lm_rows_cpu.py compiles with g++ -- so that the reference is known to state the rules of the kernels before
tests/test_gpu_fit_native_exact.py holds the kernels to it.  Synthetic J, r and boxes at P in {1, 6, 23, 64, 138} (23: the first packed
triangle longer than a workgroup; 138: the largest size with a sensitivity kernel); some variables sit on bounds, one case has an empty
free set.  Both sides get the same float64 A and g.

Steps: two backward-stable solves of one system differ by at most P cond 2^-52 |step| (norm-wise; cond: the 2-norm condition number of the
damped matrix).  The free set, the done flag and the accept choices are decisions and must agree exactly."""
import ctypes as C

import numpy as np
import pytest

import lm_reference as ref
from test_lm_rows_cpu import SHIM, U8P, dp, shim  # noqa: F401  (shim: the module-scoped fixture that compiles SHIM)

U = 2.0 ** -53
SIZES = [1, 6, 23, 64, 138]


def _case(P, kind):
    """J [3 P + 2, P], r, a box and a point with variables on both bounds.  kind "mixed": gradient signs as they fall; "empty": every
    variable on its lower bound with a positive gradient component, so nothing is free."""
    rng = np.random.default_rng([91, P, kind == "empty"])
    F = 3 * P + 2
    J = rng.standard_normal((F, P))
    r = rng.standard_normal(F) * 3.0
    lb, ub = -rng.uniform(0.5, 1.5, P), rng.uniform(0.5, 1.5, P)
    p = rng.uniform(-0.4, 0.4, P)
    if kind == "empty":
        p = lb.copy()
        J = np.abs(J); r = np.abs(r)                                     # g = J^T r > 0 in every component
    else:
        on_lb, on_ub = np.arange(P) % 4 == 1, np.arange(P) % 4 == 3
        p[on_lb], p[on_ub] = lb[on_lb], ub[on_ub]
    lam = 0.7
    isig = rng.uniform(0.5, 2.0, F + P)
    A, g, _, _ = ref.normal_equations(ref.weighted_jacobian(J, None, isig, False), np.concatenate([r, (lam / P) * p * p * isig[F:]]), p, lam,
                                      isig[F:], True)
    A64 = np.asarray(A, dtype=np.float64)
    A64 = np.ascontiguousarray(np.tril(A64) + np.tril(A64, -1).T)       # exactly symmetric, as lm_normal_kernel writes it
    return A64, np.asarray(g, dtype=np.float64), p, lb, ub


@pytest.mark.parametrize("kind", ["mixed", "empty"])
@pytest.mark.parametrize("P", SIZES)
def test_one_iteration_matches_the_host_build(shim, P, kind):
    A, g, p, lb, ub = _case(P, kind)
    cost = 17.0
    it = ref.one_iteration(A, g, p, lb, ub, mu=1e-3, levels=12, cost=cost)
    free = np.array([not shim.shim_fixed(p[i], lb[i], ub[i], g[i]) for i in range(P)])
    assert np.array_equal(free, it["free"])
    if kind == "empty":
        assert not free.any() and it["done"]
    elif P > 1:
        assert free.any() and not free.all()
    DD = np.array([shim.shim_scale(A[i, i]) for i in range(P)])
    assert np.all(np.abs(DD - np.asarray(it["DD"], float)) <= 2 * U * DD)
    gnorm = float(np.sqrt(np.sum(np.where(free, g, 0.0) ** 2)))
    assert bool(shim.shim_done(int(free.sum()), gnorm, cost)) == it["done"]
    fr = np.ascontiguousarray(free.astype(np.uint8))
    worst = 0.0
    for lv in range(12):
        step = np.full(P, np.nan)
        shim.shim_step(P, dp(A), fr.ctypes.data_as(U8P), dp(DD), dp(g), 1e-3, lv, dp(step))
        want = np.asarray(it["step"][lv], float)
        tol = P * it["cond"][lv] * 2.0 * U * np.linalg.norm(want)
        err = np.linalg.norm(step - want)
        worst = max(worst, err / tol) if tol > 0 else worst
        assert err <= tol, (P, lv, err, tol)
        assert np.all(step[~free] == 0.0) and np.all(want[~free] == 0.0)
        trial, d = np.empty(P), np.empty(P)
        pred = shim.shim_project_pred(P, dp(A), dp(g), dp(p), dp(lb), dp(ub), dp(step), dp(trial), dp(d))
        assert np.all(trial >= lb) and np.all(trial <= ub)
        assert np.linalg.norm(trial - np.asarray(it["trial"][lv], float)) <= tol + 2 * U * np.linalg.norm(trial)
        # pred = -(g . dp + 1/2 dp^T A dp): the move's error tol through the model's slope g + A dp, and two nested sums of P terms
        wdp = np.asarray(it["dp"][lv], float)
        slope = np.linalg.norm(g + A @ wdp)
        mags = np.abs(g) @ np.abs(wdp) + 0.5 * np.abs(wdp) @ (np.abs(A) @ np.abs(wdp))
        assert abs(pred - float(it["pred"][lv])) <= slope * (tol + 2 * U * np.linalg.norm(p)) + (2 * P + 6) * U * mags, (P, lv)
        if kind == "empty":
            assert np.array_equal(trial, p) and pred == 0.0 and float(it["pred"][lv]) == 0.0
    print(f"[P {P} {kind}] worst |step - ref| / (P cond 2^-52 |step|) {worst:.3e}  cond {it['cond'][0]:.3e} .. {it['cond'][11]:.3e}", flush=True)


@pytest.mark.parametrize("P", SIZES)
def test_accept_choices_match_the_host_build(shim, P):
    """Trial costs placed at chosen gain ratios around the reference's predicted reductions: rejected levels first (cost not lower, gain at
    most 1e-4, no predicted reduction), then an acceptable one; every ordering of K = 1, 3 and 12 levels gives the level `pick` gives."""
    A, g, p, lb, ub = _case(P, "mixed")
    cost = 17.0
    pred = np.asarray(ref.one_iteration(A, g, p, lb, ub, levels=12, cost=cost)["pred"], float)
    assert np.all(pred > 0.0)
    tables = [[0.5], [-0.2], [5e-5], [-0.2, 5e-5, 0.9], [5e-5, 0.3, 0.9], [0.0, -1.0, 2e-4], [-0.3, 0.0, 5e-5],
              [-0.1] * 11 + [0.8], [-0.1] * 12, [5e-5] * 5 + [0.76] + [0.9] * 6]
    for rhos in tables:
        K = len(rhos)
        cn = cost - np.asarray(rhos) * pred[:K]
        pd = pred[:K].copy()
        want, margins = ref.pick(cost, cn, pd)
        assert all(abs(m[0]) > 4e-5 for m in margins)                   # no decision of the table sits on its threshold
        mu_out, rho_out = C.c_double(np.nan), C.c_double(np.nan)
        got = shim.shim_round(1e-3, cost, K, dp(cn), dp(pd), C.byref(mu_out), C.byref(rho_out))
        assert got == want, (P, rhos)
        assert want == next((k for k, x in enumerate(rhos) if x > 1e-4), -1)
    # a level the model does not believe in (pred <= 0) is never taken, whatever its cost
    cn = np.array([1.0, 1.0]); pd = np.array([0.0, -2.0])
    mu_out, rho_out = C.c_double(np.nan), C.c_double(np.nan)
    assert shim.shim_round(1e-3, cost, 2, dp(cn), dp(pd), C.byref(mu_out), C.byref(rho_out)) == ref.pick(cost, cn, pd)[0] == -1


def test_residual_and_normal_equations_against_float64_numpy():
    """The helper's own arithmetic: residual, cost, A and g against the same expressions in float64 (the sums' float64 rounding bounds
    them: (n + 2) u sum |terms|), the 1e6 rule, the zero rule, the ridge diagonal in its own slot and the chain rule's column weights."""
    rng = np.random.default_rng(5)
    F, P, lam = 65, 10, 0.3
    flat, target = rng.uniform(0.1, 2.0, F), rng.uniform(0.1, 2.0, F)
    p = rng.uniform(-1.0, 1.0, P)
    isig = 1.0 / rng.uniform(0.5, 2.0, F + P)
    flat[7] = np.nan
    r, cost = ref.residual(flat, target, p, lam, isig, True)
    want = np.concatenate([(flat - target) * isig[:F], lam / P * p * p * isig[F:]])
    want[7] = 1e6
    assert r.dtype == np.longdouble and float(r[7]) == 1e6
    assert np.all(np.abs(np.asarray(r, float) - want) <= 4 * U * np.abs(want))
    assert abs(float(cost) - 0.5 * np.sum(want * want)) <= (F + P + 2) * U * 0.5 * np.sum(want * want)
    assert ref.residual(flat, target, p, lam, isig, False)[0].shape == (F,)
    d = rng.standard_normal((F, P))
    d[3, 4] = np.inf
    th = np.exp(p)
    Jw = ref.weighted_jacobian(d, th, isig, True)
    assert float(Jw[3, 4]) == 0.0
    d[3, 4] = 0.0
    J64 = d * th[None, :] * isig[:F, None]
    assert np.all(np.abs(np.asarray(Jw, float) - J64) <= 3 * U * np.abs(J64))
    assert np.array_equal(np.asarray(ref.weighted_jacobian(d, th, isig, False), float), np.asarray(ref._ld(d) * ref._ld(isig)[:F, None], float))
    A, g, absA, absg = ref.normal_equations(Jw, r, p, lam, isig[F:], True)
    dd = 2.0 * lam / P * p * isig[F:]
    A64 = J64.T @ J64 + np.diag(dd * dd)
    g64 = J64.T @ want[:F] + dd * want[F:]
    assert np.all(np.abs(np.asarray(A, float) - A64) <= (F + 8) * 2 * U * np.asarray(absA, float))
    assert np.all(np.abs(np.asarray(g, float) - g64) <= (F + 8) * 2 * U * np.asarray(absg, float))
    A0, g0, _, _ = ref.normal_equations(Jw, r[:F], p, lam, None, False)
    assert np.array_equal(np.asarray(A - A0, float)[~np.eye(P, dtype=bool)], np.zeros(P * P - P))
    assert np.all(np.abs(np.asarray(np.diag(A - A0), float) - dd * dd) <= 4 * U * np.diag(A64))
