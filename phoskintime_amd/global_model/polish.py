"""Polish of network candidates: a bounded Levenberg-Marquardt fit of a handful of entries of each candidate vector, every other entry held.

``polish_batch(driver="native")`` hands the whole fit to the library (``NetworkEngine.fit_batch`` -> ``pk_network_fit_batch``: state in
HBM, four small kernels between the integrator launches).  ``driver="python"`` is its twin: it issues the same two launches per iteration
through the public engine methods -- ``simulate_objective_grad_batch`` on the active rows for ``pred`` / ``dpred``, one plain
``simulate_objective_batch(method="rosw")`` launch per trial round on (levels x pending rows) candidates -- and does the algebra between them
in numpy by the rules of csrc/pk_lm.hpp and csrc/pk_net_fit.hpp (``paramest/multistart.py`` keeps the protein fit's twin the same way).  The
twin pays a host round trip of ``dpred`` per iteration; it exists to be read and to hold the native driver to.

Cost consistency: a launch with tangents controls its steps on state and tangents together, so its objectives lie within rtol / atol of the
plain launch's, not on them.  Both drivers compare costs of plain launches only; the tangent launch gives ``J^T J`` and ``J^T r``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np

MU0 = 1e-3              # csrc/pk_lm.hpp: kLmMu0
MAX_TRIES = 12          # kLmMaxTries
REASONS = {0: "ftol / xtol", 1: "gradient / empty free set", 2: "damping budget", 3: "max_iter", 4: "Jacobian launch flagged"}


@dataclass
class PolishResult:
    x: np.ndarray                       # [B, n_var]
    cost: np.ndarray                    # [B] 1/2 obj_w . F
    F: np.ndarray                       # [B, 3]
    JTJ: Optional[np.ndarray]           # [B, K, K] at each row's last Jacobian phase
    reason: np.ndarray                  # [B] see REASONS
    status: np.ndarray                  # [B]
    counters: dict
    g: Optional[np.ndarray] = None      # driver="python", want_g: [B, K] J^T r of each row's last Jacobian phase


def softplus(x):
    x = np.asarray(x, float)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def softplus_prime(x):
    x = np.asarray(x, float)
    return np.where(x > 20.0, 1.0, 1.0 / (1.0 + np.exp(-x)))


def cost_of(F, obj_w):
    """1/2 ((w0 F0 + w1 F1) + w2 F2), each operation rounded once: the bits of the library's nf_cost."""
    F = np.asarray(F, float)
    return 0.5 * ((obj_w[0] * F[..., 0] + obj_w[1] * F[..., 1]) + obj_w[2] * F[..., 2])


def _seq_sum(w):
    s = 0.0
    for v in np.asarray(w, float).ravel():
        s += float(v)
    return s


def residual_rows(loss_data, obj_w, lambdas):
    """(scale [n_obs], obs [n_obs]) of the observation rows sqrt(obj_w[m] norm_m lambda_m w_i) (pred_i - obs_i), in (protein | rna | phospho)
    list order; norm_m = 1 / max(1e-6, sum w) as the loss handle forms it."""
    scl, obs = [], []
    for m, k in enumerate(("prot", "rna", "pho")):
        w = np.asarray(loss_data["w_" + k], float)
        s = _seq_sum(w)
        norm = 1.0 / (s if s > 1e-6 else 1e-6)
        scl.append(np.sqrt(((float(obj_w[m]) * norm) * float(lambdas[m])) * w))
        obs.append(np.asarray(loss_data["obs_" + k], float))
    return np.concatenate(scl), np.concatenate(obs)


def prior_columns(cols, n_K, N, sites):
    cols = np.asarray(cols)
    return ((cols >= n_K) & (cols < n_K + 4 * N)) | ((cols >= n_K + 4 * N + sites) & (cols < n_K + 5 * N + sites))


def prior_rows(xc, cols, defaults, obj_w, lam_prior, shape, raw):
    """(r [K], d [K]): prior residual and its derivative for the fitted entries ``xc`` (0 where a column carries no prior)."""
    K = len(cols)
    r, d = np.zeros(K), np.zeros(K)
    if defaults is None:
        return r, d
    n_K, N, sites = shape
    has = prior_columns(cols, n_K, N, sites)
    sp = np.sqrt((((obj_w[0] + obj_w[1]) + obj_w[2]) * lam_prior) / (5 * N))
    dd = np.asarray(defaults, float)[np.asarray(cols)]
    p = softplus(xc) if raw else np.asarray(xc, float)
    with np.errstate(all="ignore"):
        r = np.where(has, sp * ((p - dd) / (dd + 1e-6)), 0.0)
        d = np.where(has, (sp / (dd + 1e-6)) * (softplus_prime(xc) if raw else 1.0), 0.0)
    return np.where(np.isfinite(r), r, 0.0), np.where(np.isfinite(d), d, 0.0)


def normal_equations(pred, dpred, scl, obs, pr, pd):
    """A = J^T J, g = J^T r of one row: observation rows first, prior rows (residual ``pr``, derivative ``pd``) last; non-finite entries
    count 0."""
    with np.errstate(all="ignore"):
        J = scl[:, None] * dpred
        r = scl * (pred - obs)
    J = np.where(np.isfinite(J), J, 0.0)
    r = np.where(np.isfinite(r), r, 0.0)
    A = J.T @ J + np.diag(pd * pd)
    g = J.T @ r + pr * pd
    return A, g


def damped_step(A, g, free, DD, mu, lv):
    """lm_damped_step: the step of damping level ``lv``; 0 where the factorisation fails and in fixed entries."""
    K = g.size
    mask = free[:, None] & free[None, :]
    M = np.where(mask, A, 0.0)
    M[np.arange(K), np.arange(K)] = np.where(free, np.diag(A) + (mu * 4.0 ** lv) * (DD * DD), 1.0)
    rhs = np.where(free, -g, 0.0)
    step = np.zeros(K)
    if np.all(np.isfinite(M)):
        try:
            Lc = np.linalg.cholesky(M)
            step = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
            step = np.where(np.isfinite(step), step, 0.0)
        except np.linalg.LinAlgError:
            step = np.zeros(K)
    return np.where(free, step, 0.0)


def round_levels(trial_levels, pending, tries):
    L = trial_levels if trial_levels > 0 else (3 if pending <= 256 else 1)
    return min(L, MAX_TRIES - tries)


def _python_driver(x0, cols, lb, ub, bounds_batched, obj_w, rows_of, jac, plain, max_iter, trial_levels, ftol, xtol, want_g):
    """The lockstep loop of pk_network_fit_batch on the host.  ``jac(X [k, n_var]) -> (pred [k, n_obs], dpred [k, n_obs, K], status [k])``;
    ``plain(X [m, n_var]) -> (F [m, 3], status [m])``; ``rows_of(x_row) -> (scl, obs, prior r, prior d)``."""
    x = np.array(x0, float, copy=True)
    B, K = x.shape[0], len(cols)
    box = lambda row: ((lb[row], ub[row]) if bounds_batched else (lb, ub))
    for row in range(B):
        lo, hi = box(row)
        x[row, cols] = np.minimum(np.maximum(x[row, cols], lo), hi)
    mu = np.full(B, MU0)
    F, st = plain(x)
    F = np.array(F, float, copy=True)
    status = np.array(st, np.int32, copy=True)
    cost = cost_of(F, obj_w)
    cnt = [0, B, 3, 0, 0, 0]
    active = np.ones(B, bool)
    why = np.full(B, 3, np.int32)
    JTJ = np.zeros((B, K, K))
    G = np.zeros((B, K))
    for it in range(1, max_iter + 1):
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        cnt[0] = it
        pred, dpred, stj = jac(x[idx])
        cnt[1] += idx.size; cnt[2] += 3; cnt[3] += 1; cnt[4] += 1
        pend, free_of, DD_of = [], {}, {}
        for j, row in enumerate(idx):
            if int(stj[j]) != 0:
                active[row] = False; why[row] = 4; status[row] = int(stj[j])
                continue
            status[row] = 0
            scl, obs, pr, pd = rows_of(x[row])
            A, g = normal_equations(np.asarray(pred[j], float), np.asarray(dpred[j], float), scl, obs, pr, pd)
            JTJ[row], G[row] = A, g
            lo, hi = box(row)
            p = x[row, cols]
            fixed = ((p <= lo) & (g > 0.0)) | ((p >= hi) & (g < 0.0))
            free = ~fixed
            DD = np.maximum(np.sqrt(np.maximum(np.diag(A), 0.0)), 1e-12)
            gn = float(np.sqrt(np.sum(np.where(free, g, 0.0) ** 2)))
            if not free.any() or gn < 1e-14 * max(1.0, cost[row]):
                active[row] = False; why[row] = 1
            else:
                pend.append(row); free_of[row] = free; DD_of[row] = DD
        tries = 0
        while tries < MAX_TRIES and pend:
            m = len(pend)
            L = round_levels(trial_levels, m, tries)
            tries += L
            Xt = np.empty((L * m, x.shape[1]))
            predred = np.empty(L * m)
            for lv in range(L):
                for q, row in enumerate(pend):
                    lo, hi = box(row)
                    p = x[row, cols]
                    step = damped_step(JTJ[row], G[row], free_of[row], DD_of[row], mu[row], lv)
                    trial = np.minimum(np.maximum(p + step, lo), hi)
                    dp = trial - p
                    Xt[lv * m + q] = x[row]
                    Xt[lv * m + q, cols] = trial
                    predred[lv * m + q] = -(float(G[row] @ dp) + 0.5 * float(dp @ (JTJ[row] @ dp)))
            Ft, stt = plain(Xt)
            cnt[1] += L * m; cnt[2] += 3; cnt[3] += 1; cnt[5] += 1
            nxt = []
            for q, row in enumerate(pend):
                sel, rho, cn = -1, -1.0, 0.0
                for lv in range(L):
                    slot = lv * m + q
                    status[row] |= int(stt[slot])
                    cn = float(cost_of(np.asarray(Ft[slot], float), obj_w))
                    rho = (cost[row] - cn) / predred[slot] if predred[slot] > 0.0 else -1.0
                    if int(stt[slot]) == 0 and cn < cost[row] and rho > 1e-4:
                        sel = lv
                        break
                if sel < 0:
                    mu[row] *= 4.0 ** L
                    nxt.append(row)
                    continue
                slot = sel * m + q
                trial = Xt[slot, cols]
                dx, xn = float(np.sqrt(np.sum((trial - x[row, cols]) ** 2))), float(np.sqrt(np.sum(trial ** 2)))
                conv = (cost[row] - cn) <= ftol * max(cn, 1e-300) or dx <= xtol * (xtol + xn)
                mu[row] = max(mu[row] * 4.0 ** sel * (1.0 / 3.0 if rho > 0.75 else 1.0), 1e-12)
                x[row, cols] = trial
                cost[row] = cn
                F[row] = Ft[slot]
                if conv:
                    active[row] = False; why[row] = 0
            pend = nxt
        for row in pend:
            active[row] = False; why[row] = 2
    names = ("iterations", "simulated", "launches", "host_waits", "jacobian_phases", "trial_rounds")
    return PolishResult(x, cost, F, JTJ, why, status, dict(zip(names, cnt)), G if want_g else None)


def polish_batch(eng, loss, loss_data, x0, t_eval, cols, lb=None, ub=None, obj_w=(1.0, 1.0, 1.0), defaults=None, lambdas=(1.0, 1.0, 1.0, 0.0),
                 y0=None, raw: bool = False, max_iter: int = 50, trial_levels: int = 0, ftol: float = 1e-10, xtol: float = 1e-10,
                 driver: str = "native", launches: Optional[Tuple[Callable, Callable]] = None, net_shape=None, want_g: bool = False,
                 kernel: str = "auto", fail_value: float = 1e12, **solver_kw) -> PolishResult:
    """Drive each candidate ``x0[b]`` to the nearest local minimum of ``1/2 sum_m obj_w[m] F_m`` over its entries ``cols`` inside the box
    ``[lb, ub]`` ([K] or [B, K]; None = no box), by bounded Levenberg-Marquardt.  ``driver="native"``: ``eng.fit_batch``.
    ``driver="python"``: the host twin described in the module docstring; it needs ``loss_data`` (the dict ``loss`` was made from) for the
    residual scales.  ``launches = (jac, plain)`` replaces the twin's two engine launches (``jac(X) -> pred, dpred, status``;
    ``plain(X) -> F, status``) -- then ``eng`` may be None and ``net_shape = (n_K, N, total_sites)`` names the layout of the candidate
    vector for the prior rows.  ``solver_kw``: rtol, atol, max_steps, err_norm of both launches."""
    if driver not in ("native", "python"):
        raise ValueError("driver must be 'native' or 'python'")
    obj_w = tuple(float(v) for v in obj_w)
    if len(obj_w) != 3 or not all(v >= 0.0 for v in obj_w):
        raise ValueError("obj_w must be three weights >= 0")
    cols = np.asarray(np.atleast_1d(cols), dtype=np.int64).reshape(-1)
    if driver == "native":
        if launches is not None:
            raise ValueError("launches belongs to driver='python'")
        x, cost, F, JTJ, reason, status, counters = eng.fit_batch(
            loss, x0, t_eval, cols, lb=lb, ub=ub, obj_w=obj_w, defaults=defaults, lambdas=lambdas, y0=y0, raw=raw, max_iter=max_iter,
            trial_levels=trial_levels, ftol=ftol, xtol=xtol, kernel=kernel, fail_value=fail_value, **solver_kw)
        host = lambda t: t.cpu().numpy()
        return PolishResult(host(x), host(cost), host(F), host(JTJ), host(reason), host(status), counters)
    x0 = np.atleast_2d(np.asarray(x0.cpu().numpy() if hasattr(x0, "cpu") else x0, dtype=np.float64))
    B, K = x0.shape[0], cols.size
    if K < 1 or np.unique(cols).size != K or cols.min() < 0 or cols.max() >= x0.shape[1]:
        raise ValueError("cols must name >= 1 distinct entries of the candidate vector")
    if (lb is None) != (ub is None):
        raise ValueError("lb and ub: give both or neither")
    lb = np.full(K, -np.inf) if lb is None else np.asarray(lb, float)
    ub = np.full(K, np.inf) if ub is None else np.asarray(ub, float)
    if lb.shape != ub.shape or lb.shape not in ((K,), (B, K)):
        raise ValueError(f"lb and ub must both be [{K}] or [{B}, {K}]")
    shape = net_shape if net_shape is not None else (eng.n_K, eng.N, eng.total_sites)
    scl, obs = residual_rows(loss_data, obj_w, lambdas)
    dflt = None if defaults is None else np.asarray(defaults.cpu().numpy() if hasattr(defaults, "cpu") else defaults, float)

    def rows_of(xrow):
        pr, pd = prior_rows(xrow[cols], cols, dflt, obj_w, float(lambdas[3]), shape, raw)
        return scl, obs, pr, pd

    if launches is None:
        kw = dict(y0=y0, raw=raw, defaults=defaults, lambdas=lambdas, fail_value=fail_value, **solver_kw)
        kw.setdefault("rtol", 1e-7); kw.setdefault("atol", 1e-9)
        if y0 is not None and np.ndim(y0) == 2:
            raise ValueError("driver='python' takes one y0 for every candidate")

        def jac(X):
            out = eng.simulate_objective_grad_batch(loss, X, t_eval, cols, want_F=False, want_sums=False, want_pred=True, kernel=kernel, **kw)
            if out is None:
                raise RuntimeError("the tangent launch was refused: " + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode())
            return out["pred"].cpu().numpy(), out["dpred"].cpu().numpy(), out["status"].cpu().numpy()

        def plain(X):
            out = eng.simulate_objective_batch(loss, X, t_eval, method="rosw", kernel="workspace" if kernel == "hbm" else "lds", **kw)
            if out is None:
                raise RuntimeError("the plain launch was refused: " + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode())
            return out[1].cpu().numpy(), out[2].cpu().numpy()
    else:
        jac, plain = launches
    return _python_driver(x0, cols, lb, ub, lb.ndim == 2, obj_w, rows_of, jac, plain, int(max_iter), int(trial_levels), float(ftol), float(xtol), want_g)


def covariance(JTJ, cost, n_obs: int, K: int, absolute_sigma: bool = False):
    """Covariance of the K fitted entries of one candidate from its ``JTJ`` and final ``cost``, as ``scipy.optimize.curve_fit`` reports it:
    ``(J^T J)^-1`` times the residual variance ``2 cost / (n_obs - K)`` unless ``absolute_sigma``.  None where J^T J is singular.  Feed it
    to ``paramest.identifiability.ci.confidence_intervals`` for Wald intervals.  (``cost`` includes the constant prior of the held entries,
    which makes the variance conservative when lambda_prior > 0.)"""
    A = np.asarray(JTJ, float)
    try:
        pcov = np.linalg.inv(A)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(pcov)):
        return None
    if not absolute_sigma and n_obs > K:
        pcov = pcov * (2.0 * float(cost) / (n_obs - K))
    return pcov
