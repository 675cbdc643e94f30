"""CPU: the exact parameter derivative of the oracle (oracle.protein_models.sens_exact_lti: Frechet derivative of the augmented matrix
exponential) against an independent construction, against the oracle's own solution, and against the central difference it replaces as
the reference of the sensitivity kernels -- in the regimes where the fits run (tests/test_gpu_sens_regimes.py builds on it)."""
import functools

import numpy as np
import pytest
from scipy.linalg import expm

from oracle import protein_models as pm

SHAPES = [(pm.DIST, 4), (pm.DIST, 12), (pm.SUCC, 6), (pm.RAND, 3), (pm.RAND, 5)]
T = pm.TIME_POINTS


@functools.lru_cache(maxsize=None)
def _case(model, n, regime):
    rng = np.random.default_rng(1000 * model + 10 * n + pm.SENS_REGIMES.index(regime))
    th, y0 = pm.sens_regime(regime, model, n, rng, 1)
    y0 = y0[0] if y0.ndim == 2 else y0
    sol, dsol = pm.sens_exact_lti(model, th[0], y0, n, T)
    for a in (th, y0, sol, dsol):
        a.setflags(write=False)
    return th[0], y0, sol, dsol


def _van_loan(model, th, y0, n, t):
    """d y(t_k) / d theta_c from the block exponential expm([[A, E_c], [0, A]] dt) = [[X, L], [0, X]] (Van Loan 1978): no call shared with
    sens_exact_lti except expm itself.  w = [z'; z] is stepped as one vector."""
    M, b = pm.lti_matrix(model, th, n)
    S = M.shape[0]
    A = np.zeros((S + 1, S + 1)); A[:S, :S] = M; A[:S, S] = b
    M0, b0 = pm.lti_matrix(model, np.zeros(th.size), n)
    out = np.zeros((t.size, S, th.size))
    for c in range(th.size):
        e = np.zeros(th.size); e[c] = 1.0
        M1, b1 = pm.lti_matrix(model, e, n)
        E = np.zeros_like(A); E[:S, :S] = M1 - M0; E[:S, S] = b1 - b0
        blk = np.block([[A, E], [np.zeros_like(A), A]])
        w = np.concatenate((np.zeros(S + 1), y0, [1.0]))
        for k in range(1, t.size):
            w = expm(blk * (t[k] - t[k - 1])) @ w
            out[k, :, c] = w[:S]
    return out


def _central_difference(model, th, y0, n, t):
    """tests/test_gpu_sens.py, _oracle_jac, on the unflattened solution."""
    cols = []
    for c in range(th.size):
        h = 1e-5 * max(1.0, abs(th[c]))
        tp, tm = th.copy(), th.copy()
        tp[c] += h; tm[c] -= h
        cols.append((pm.solve_exact_lti(model, tp, y0, n, t) - pm.solve_exact_lti(model, tm, y0, n, t)) / (2 * h))
    return np.stack(cols, axis=2)


def _err(d, ref):
    return float(np.max(np.abs(d - ref) / (1.0 + np.abs(ref))))


def test_the_models_are_affine_in_theta():
    """E_c = Aug(e_c) - Aug(0) is the exact direction only if Aug is affine in theta: Aug(theta) = Aug(0) + sum_c theta_c E_c."""
    for model, n in SHAPES:
        th = np.random.default_rng(n).uniform(0.0, 20.0, pm.n_params(model, n))
        A0 = pm._augmented(model, np.zeros(th.size), n)
        acc = A0.copy()
        for c in range(th.size):
            e = np.zeros(th.size); e[c] = 1.0
            E = pm._augmented(model, e, n) - A0
            assert np.array_equal(E, pm._augmented(model, e, n, analytic=True) - pm._augmented(model, np.zeros(th.size), n, analytic=True))
            acc += th[c] * E
        assert np.max(np.abs(acc - pm._augmented(model, th, n))) <= 1e-12 * 20.0 * n


@pytest.mark.parametrize("regime", pm.SENS_REGIMES)
@pytest.mark.parametrize("model,n", SHAPES)
def test_exact_derivative_agrees_with_the_van_loan_block_exponential(model, n, regime):
    th, y0, sol, dsol = _case(model, n, regime)
    assert np.isfinite(dsol).all() and np.all(dsol[0] == 0.0)
    assert _err(dsol, _van_loan(model, th, y0, n, T)) <= 1e-9
    assert pm.band_error(sol, pm.solve_exact_lti(model, th, y0, n, T)) <= 1e-3


@pytest.mark.parametrize("model,n", SHAPES)
def test_exact_derivative_agrees_with_central_differences_at_moderate_rates(model, n):
    """theta ~ U(0.2, 2), random y0: the inputs of tests/test_gpu_sens.py, where the difference quotient is good to 1e-8."""
    rng = np.random.default_rng(100 * model + n)
    th = rng.uniform(0.2, 2.0, pm.n_params(model, n)); y0 = rng.uniform(0.3, 1.5, pm.n_states(model, n))
    _, dsol = pm.sens_exact_lti(model, th, y0, n, T)
    assert _err(dsol, _central_difference(model, th, y0, n, T)) <= 1e-8


def test_central_differences_cannot_serve_where_the_fits_run():
    """Rates log-uniform on 1e-8 .. 20 (randmod's box): the difference quotient with h = 1e-5 max(1, |theta|) is further from the exact
    derivative than the limit the kernels are held to (1e-7) -- a rate of 1e-8 is stepped to -1e-5, and the solution's curvature in a
    slow rate over t = 960 is not small against h.  Hence the exact reference."""
    worst = 0.0
    for model, n in ((pm.DIST, 4), (pm.SUCC, 6), (pm.RAND, 3)):
        th, y0, _, dsol = _case(model, n, "loguniform")
        worst = max(worst, _err(_central_difference(model, th, y0, n, T), dsol))
    assert worst > 1e-7


@pytest.mark.parametrize("model,n", SHAPES)
def test_steady_start_moves_the_tangents_and_not_the_states(model, n):
    th, y0, sol, dsol = _case(model, n, "steady")
    assert np.max(np.abs(sol - y0[None, :])) <= 1e-9
    assert np.max(np.abs(dsol)) >= 1e-2
    assert np.max(np.abs(dsol[1])) >= 1e-2                      # already at t = 0.5: a transient, not a drift


def test_column_subset_equals_the_full_derivative():
    th, y0, sol, dsol = _case(pm.DIST, 12, "uniform")
    cols = [0, 5, 27]
    s2, d2 = pm.sens_exact_lti(pm.DIST, th, y0, 12, T, cols=cols)
    assert np.array_equal(s2, sol) and np.array_equal(d2, dsol[:, :, cols])


def test_flat_and_jacobian_follows_the_library_layout():
    """flatten_observables layout, zero rows where clipped and at t0, 1 / y0 under normalize."""
    model, n = pm.RAND, 3
    S = pm.n_states(model, n)
    rng = np.random.default_rng(2)
    sol = rng.standard_normal((T.size, S)); dsol = rng.standard_normal((T.size, S, 4))
    y0 = rng.uniform(0.5, 2.0, S)
    flat, d = pm.flat_and_jacobian(model, sol, dsol, y0, n)
    assert flat.shape == (T.size - 5 + T.size + n * T.size,) and d.shape == (flat.size, 4)
    np.testing.assert_array_equal(flat, pm.flatten_observables(model, np.clip(sol, 0, None), n))
    assert (flat == 0.0).any() and np.all(d[flat == 0.0] == 0.0)
    k = 7
    assert np.array_equal(d[k - 5], np.where(sol[k, 0] < 0, 0.0, dsol[k, 0]))                  # R(t_k), k >= 5
    assert np.array_equal(d[T.size - 5 + k], np.where(sol[k, 1] < 0, 0.0, dsol[k, 1]))         # P(t_k)
    assert np.array_equal(d[T.size - 5 + T.size + 2 * T.size + k], np.where(sol[k, 4] < 0, 0.0, dsol[k, 4]))      # site 3 at t_k
    assert np.all(d[T.size - 5] == 0.0) and np.all(d[T.size - 5 + T.size] == 0.0)              # P(t0), site 1 at t0: data
    raw_f, raw_d = pm.flat_and_jacobian(model, sol, dsol, y0, n, clip_nonneg=False)
    assert (raw_f < 0.0).any() and np.abs(raw_d[raw_f < 0.0]).max() > 0.0
    nf, nd = pm.flat_and_jacobian(model, sol, dsol, y0, n, clip_nonneg=False, normalize=True)
    scale = pm.flatten_observables(model, np.repeat(y0[None, :], T.size, axis=0), n)
    np.testing.assert_allclose(nf * scale, raw_f, rtol=1e-15)
    np.testing.assert_allclose(nd * scale[:, None], raw_d, rtol=1e-15)
