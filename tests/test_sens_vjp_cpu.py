"""CPU: the VJP entry point exists and refuses a null context, the binding lists it, the two modes the GPU test uses as its reference
(tests/sens_vjp_reference.py) agree with central differences of the oracle's flat, and `cost_and_grad_rows` adds the ridge rows, the
log-space chain rule and batched sigma correctly around a numpy stand-in for the launch (checked against central differences of the
fit's own cost formula).

Measured here: worst |g - central difference| / (1 + |g|) 2.6e-9 for the two modes and 1.0e-9 for cost_and_grad_rows; the limit is 1e-8,
the one tests/test_sens_metric_cpu.py holds the same difference quotient (relative step 1e-5) to."""
import numpy as np
import pytest
import torch

from oracle import protein_models as pm
import sens_vjp_reference as ref

SYMBOL = "pk_solve_protein_sens_vjp_batch"
CD_LIMIT = 1e-8


def test_symbol_is_exported_and_listed(built_lib):
    from phoskintime_amd import _capi
    assert SYMBOL in _capi.SYMBOLS
    assert hasattr(built_lib, SYMBOL)
    assert built_lib.pk_version() == 200


def test_null_context_is_an_error_not_a_crash(built_lib):
    assert getattr(built_lib, SYMBOL)(None, 0, 4, 1, None, None, 0, None, 14, None, None, 0, None, 0, None, None, None, None, None) < 0


def test_python_entry_points_exist():
    from phoskintime_amd import autograd, batch
    from phoskintime_amd.paramest import multistart
    assert callable(batch.solve_ode_vjp_batch) and callable(autograd.solve_flat) and callable(multistart.cost_and_grad_rows)


# ------------------------------------------------------------------------------------------------ the two modes
def _flat_of(mid, theta, y0, n, t, normalize):
    sol = pm.solve_exact_lti(mid, theta, y0, n, t)
    return pm.flat_and_jacobian(mid, sol, np.zeros(sol.shape + (0,)), y0, n, normalize=normalize)[0]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("T", [14, 6, 5])
@pytest.mark.parametrize("model,n", [("distmod", 2), ("succmod", 3), ("randmod", 2)])
def test_both_modes_against_central_differences(model, n, T, normalize):
    """value and grad of both modes on flat_and_jacobian(sens_exact_lti) against central differences of the same value formed from
    solve_exact_lti, relative step 1e-5 max(1, |theta|); T = 6 / 5: one mRNA slot / none."""
    mid = pm.MODEL_IDS[model]
    P, S = pm.n_params(mid, n), pm.n_states(mid, n)
    rng = np.random.default_rng([13, mid, n, T])
    th = rng.uniform(0.3, 2.0, size=P)
    y0 = rng.uniform(0.3, 1.5, size=S)
    t = pm.TIME_POINTS[:T]
    sol, dsol = pm.sens_exact_lti(mid, th, y0, n, t)
    v, d = ref.flat_reference(model, sol, dsol, y0, n, normalize=normalize)
    F = v.size
    assert F == max(T - 5, 0) + T + n * T and d.shape == (F, P)
    assert np.all(d[ref.t0_entries(n, T)] == 0.0)
    w = rng.uniform(0.5, 2.0, size=F); w[rng.random(F) < 0.2] = 0.0
    target = v * (1.0 + 0.1 * rng.normal(size=F)) + 0.05 * rng.normal(size=F)
    for mode, tg in (("linear", None), ("least_squares", target)):
        value, g, _, _ = ref.vjp(v, d, w, tg)
        direct = float(w @ v) if tg is None else 0.5 * float(np.sum((w * (v - tg)) ** 2))
        assert value == pytest.approx(direct, rel=1e-13)
        worst = 0.0
        for p in range(P):
            h = 1e-5 * max(1.0, abs(th[p]))
            hp = th.copy(); hm = th.copy(); hp[p] += h; hm[p] -= h
            cd = (ref.vjp(_flat_of(mid, hp, y0, n, t, normalize), d, w, tg)[0] - ref.vjp(_flat_of(mid, hm, y0, n, t, normalize), d, w, tg)[0]) / (2 * h)
            worst = max(worst, abs(g[p] - cd) / (1.0 + abs(g[p])))
        print(f"FIG modes {model} {n} T={T} normalize={normalize} {mode}: worst={worst:.2e}")
        assert worst <= CD_LIMIT, mode


def test_bounds_are_linear_in_the_limits_and_skip_t0():
    rng = np.random.default_rng(5)
    n, T = 2, 6
    F = 1 + T + n * T
    v = rng.uniform(0.1, 2.0, size=F); d = rng.normal(size=(F, 3)); w = rng.uniform(0.5, 2.0, size=F); tg = v + 0.1
    ev = 1e-6 * np.abs(v); ed = 1e-7 * (1 + np.abs(d))
    for target in (None, tg):
        bv, bg = ref.bounds(v, d, w, target, ev, ed, n, T)
        bv2, bg2 = ref.bounds(v, d, w, target, 2 * ev, 2 * ed, n, T)
        assert bv > 0 and (bg > 0).all() and bv2 == pytest.approx(2 * bv) and np.allclose(bg2, 2 * bg)
        only_t0 = np.zeros(F); only_t0[ref.t0_entries(n, T)] = 1.0
        assert ref.bounds(v, d, w, target, only_t0, only_t0[:, None] * np.ones((1, 3)), n, T)[0] == 0.0
    assert (ref.bounds(v, d, w, None, ev, 0 * ed, n, T)[1] == 0).all() and (ref.bounds(v, d, w, tg, ev, 0 * ed, n, T)[1] > 0).all()


# ------------------------------------------------------------------------------------------------ cost_and_grad_rows on a stub
class _Stub:
    """What batch.solve_ode_vjp_batch returns, from the exact derivative and the reference's two modes."""

    def __init__(self, model, theta, init_cond, num_psites, t, w, target=None, want_flat=False, **kw):
        mid = pm.MODEL_IDS[model]
        th = np.atleast_2d(np.asarray(theta, float))
        w = np.asarray(w, float); tg = None if target is None else np.asarray(target, float)
        val, grad = [], []
        for k, row in enumerate(th):
            sol, dsol = pm.sens_exact_lti(mid, row, init_cond, num_psites, t)
            v, d = ref.flat_reference(model, sol, dsol, init_cond, num_psites)
            a, g, _, _ = ref.vjp(v, d, w[k] if w.ndim == 2 else w, None if tg is None else (tg[k] if tg.ndim == 2 else tg))
            val.append(a); grad.append(g)
        self.value = torch.tensor(np.array(val)); self.grad = torch.tensor(np.array(grad)); self.flat = None
        self.status = torch.zeros(len(th), dtype=torch.int32)


@pytest.fixture
def stubbed(monkeypatch):
    from phoskintime_amd import batch
    calls = []

    def fake(model, theta, init_cond, num_psites, t, w, target=None, **kw):
        calls.append(kw)
        return _Stub(model, theta, init_cond, num_psites, t, w, target, **kw)

    monkeypatch.setattr(batch, "solve_ode_vjp_batch", fake)
    return calls


def _fit_cost(model, n, t, p, y0, target, sig, lam, log_space):
    """The cost of fit_rows_batch for one row, from the closed-form solution: 0.5 |([flat ; lam / P p^2] - [target ; 0]) / sigma|^2."""
    mid = pm.MODEL_IDS[model]
    theta = np.exp(p) if log_space else p
    f = _flat_of(mid, theta, y0, n, t, False)
    if lam > 0.0 or sig.size > f.size:
        f = np.concatenate([f, (lam / p.size) * p ** 2]); target = np.concatenate([target, np.zeros(p.size)])
    return 0.5 * float(np.sum(((f - target) / sig) ** 2))


@pytest.mark.parametrize("sigma_kind", ["none", "shared", "batched"])
@pytest.mark.parametrize("model,n,lam", [("distmod", 2, 0.0), ("distmod", 2, 0.7), ("randmod", 2, 0.3), ("succmod", 2, 0.5)])
def test_cost_and_grad_rows_against_central_differences(stubbed, model, n, lam, sigma_kind):
    from phoskintime_amd.paramest import multistart
    mid = pm.MODEL_IDS[model]
    P, S = pm.n_params(mid, n), pm.n_states(mid, n)
    log_space = model == "randmod"
    rng = np.random.default_rng([17, mid, n, int(10 * lam)])
    R = 3
    t = pm.TIME_POINTS[:7]
    theta = rng.uniform(0.3, 2.0, size=(R, P))
    p = np.log(theta) if log_space else theta
    y0 = rng.uniform(0.3, 1.5, size=S)
    Nd = 2 + 7 + n * 7
    target = rng.uniform(0.1, 1.0, size=(R, Nd))
    lams = np.array([lam, 0.0, 2 * lam])                                     # per-row lambda; a row at 0 beside regularised ones
    Nr = Nd + (P if lam > 0 else 0)
    sigma = {"none": None, "shared": rng.uniform(0.5, 2.0, size=Nr), "batched": rng.uniform(0.5, 2.0, size=(R, Nr))}[sigma_kind]
    cost, grad = multistart.cost_and_grad_rows(model, n, t, p, y0, target, sigma=sigma, lam=lams)
    assert len(stubbed) == 1                                                 # one launch for all rows
    assert cost.shape == (R,) and grad.shape == (R, P)
    worst = 0.0
    for k in range(R):
        sig = np.ones(Nr) if sigma is None else (sigma[k] if sigma.ndim == 2 else sigma)
        c0 = _fit_cost(model, n, t, p[k], y0, target[k], sig, lams[k], log_space)
        assert float(cost[k]) == pytest.approx(c0, rel=1e-11)
        for j in range(P):
            h = 1e-5 * max(1.0, abs(p[k, j]))
            hp = p[k].copy(); hm = p[k].copy(); hp[j] += h; hm[j] -= h
            cd = (_fit_cost(model, n, t, hp, y0, target[k], sig, lams[k], log_space) - _fit_cost(model, n, t, hm, y0, target[k], sig, lams[k], log_space)) / (2 * h)
            worst = max(worst, abs(float(grad[k, j]) - cd) / (1.0 + abs(cd)))
    print(f"FIG cost_and_grad_rows {model} {n} lam={lam} sigma={sigma_kind}: worst={worst:.2e}")
    assert worst <= CD_LIMIT


def test_cost_and_grad_rows_log_space_default_and_sigma_length(stubbed):
    from phoskintime_amd.paramest import multistart
    n, t = 2, pm.TIME_POINTS[:6]
    P, S = pm.n_params(2, n), pm.n_states(2, n)
    p = np.log(np.full((1, P), 0.8))
    target = np.full(1 + 6 + 2 * 6, 0.5)
    c_def, g_def = multistart.cost_and_grad_rows("randmod", n, t, p, np.ones(S), target)
    c_log, g_log = multistart.cost_and_grad_rows("randmod", n, t, p, np.ones(S), target, log_space=True)
    c_lin, g_lin = multistart.cost_and_grad_rows("randmod", n, t, np.exp(p), np.ones(S), target, log_space=False)
    assert torch.equal(c_def, c_log) and torch.equal(g_def, g_log)            # randmod is fitted in log space, as build_free_bounds has it
    assert float(c_lin[0]) == pytest.approx(float(c_log[0]), rel=1e-13)
    np.testing.assert_allclose(g_log.numpy(), g_lin.numpy() * 0.8, rtol=1e-13)
    with pytest.raises(ValueError):
        multistart.cost_and_grad_rows("randmod", n, t, p, np.ones(S), target, sigma=np.ones(target.size), lam=1.0)     # Nr = Nd + P with ridge rows
