"""Reference for d(metric)/d(theta) shared by tests/test_sens_metric_cpu.py and tests/test_gpu_sens_metric.py (not a test module).

With v[k, i] the post-processed value of observed row i < 2 + n at output time k (clipped at 0, scaled by 1 / y0[i] under `normalize`, as
flat is), d[k, i, p] its post-processed derivative (scaled alike, zero where the clip is active, zero at k = 0: the initial values are
data), L = T (2 + n), vbar the mean of v and m the metric of oracle.protein_models.compute_Y:

    total_signal    g[p] = sum d
    mean_activity   g[p] = sum d / L
    variance        g[p] = (2 / L) sum (v - vbar) d
    dynamics        g[p] = 2 sum_i sum_{k >= 1} (v[k, i] - v[k-1, i]) (d[k, i, p] - d[k-1, i, p])
    l2_norm         g[p] = sum v d / m, and 0 where m = 0

`gradient` states them in torch (float64) so that the tests can propagate the limits the kernels are already held to through G_p(v, d) to
first order by autograd: bound_p = sum |dG_p/dd| eps_d + sum |dG_p/dv| eps_v over k >= 1, bound_m = sum |dm/dv| eps_v.
"""
import numpy as np
import torch

from oracle import protein_models as pm

METRICS = pm.METRICS


def post_process(sol, dsol, y0, n, clip_nonneg=True, normalize=False):
    """(v [T, 2 + n], d [T, 2 + n, C]) from (sol [T, S], dsol [T, S, C]) as pm.flat_and_jacobian post-processes them, on ALL observed rows
    and ALL times (flat drops the mRNA row at the first five)."""
    sol = np.array(sol, dtype=float)
    dsol = np.array(dsol, dtype=float)
    dsol[0] = 0.0
    if clip_nonneg:
        neg = sol < 0.0
        sol[neg] = 0.0
        dsol[neg] = 0.0
    if normalize:
        inv = 1.0 / np.asarray(y0, float)
        sol = sol * inv[None, :]
        dsol = dsol * inv[None, :, None]
    return sol[:, :2 + n].copy(), dsol[:, :2 + n, :].copy()


def metric_value(v, name):
    """m(v) in torch, the closed forms of compute_Y."""
    L = v.numel()
    if name == "total_signal":
        return v.sum()
    if name == "mean_activity":
        return v.sum() / L
    if name == "variance":
        return ((v - v.mean()) ** 2).sum() / L
    if name == "dynamics":
        return ((v[1:] - v[:-1]) ** 2).sum()
    if name == "l2_norm":
        return torch.sqrt((v ** 2).sum())
    raise ValueError(name)


def gradient(v, d, name):
    """g [C] = G(v [T, R], d [T, R, C]): the five formulas, in torch."""
    L = v.numel()
    if name == "total_signal":
        return d.sum(dim=(0, 1))
    if name == "mean_activity":
        return d.sum(dim=(0, 1)) / L
    if name == "variance":
        return (2.0 / L) * ((v - v.mean())[:, :, None] * d).sum(dim=(0, 1))
    if name == "dynamics":
        return 2.0 * ((v[1:] - v[:-1])[:, :, None] * (d[1:] - d[:-1])).sum(dim=(0, 1))
    if name == "l2_norm":
        m = torch.sqrt((v ** 2).sum())
        g = (v[:, :, None] * d).sum(dim=(0, 1))
        return g / m if float(m.detach()) != 0.0 else torch.zeros_like(g)
    raise ValueError(name)


def reference(v, d, name, n):
    """(m_ref, g_ref [C]) in numpy: m_ref = compute_Y(v_ref), g_ref by the formulas."""
    g = gradient(torch.as_tensor(v), torch.as_tensor(d), name).numpy()
    return pm.compute_Y(v, n, name), g


def bounds(v, d, name, eps_v, eps_d):
    """(bound_m, bound_g [C]): the limits eps_v [T, R] / eps_d [T, R, C] of the values / derivatives propagated to first order through
    m(v) and G_p(v, d); k = 0 carries no error (the initial values are data)."""
    ev = torch.as_tensor(np.array(eps_v, dtype=float)); ed = torch.as_tensor(np.array(eps_d, dtype=float))
    ev[0] = 0.0; ed[0] = 0.0
    tv = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    td = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    (dm_dv,) = torch.autograd.grad(metric_value(tv, name), tv)
    bound_m = float((dm_dv.abs() * ev).sum())
    g = gradient(tv, td, name)
    # G_p depends on d[..., p] alone: one backward pass of sum_p G_p gives every dG_p / dd[k, i, p]
    (dg_dd,) = torch.autograd.grad(g.sum(), td, retain_graph=True, allow_unused=True)
    bg = (dg_dd.abs() * ed).sum(dim=(0, 1)) if dg_dd is not None else torch.zeros(d.shape[2], dtype=torch.float64)
    if name in ("variance", "dynamics", "l2_norm"):                  # the others do not depend on v
        for p in range(d.shape[2]):
            (dg_dv,) = torch.autograd.grad(g[p], tv, retain_graph=True)
            bg[p] = bg[p] + (dg_dv.abs() * ev).sum()
    return bound_m, bg.detach().numpy()
