"""An exact reference for the network's forward sensitivities, independent of the kernel (helper, no tests).

``tangent_reference`` integrates the oracle's tangent ODE  s' = f_y(y) s + f_theta(y),  s(t0) = 0,  jointly with the state by
``scipy.integrate.odeint`` (LSODA) at rtol = atol = 1e-12.  Both terms come from central differences of ``oracle.network_models.rhs``
itself, with the sixth-order central stencil (45 (g(e) - g(-e)) - 9 (g(2e) - g(-2e)) + g(3e) - g(-3e)) / (60 e):  f_y column by
column (step e = 1e-2 max(1, |y_j|)), shared by all tangent columns as the product J s_c, and f_theta for each column's own entry (step
1e-2 theta_c).  The right-hand side is smooth between its branch points (|v| at 0, u >= 0) and bilinear in (theta, y) apart from the
squashes x / (1 + |x|) and the saturating factors x / (1 + x), for which the truncation error e^6 g^(7) / 140 is ~1e-13 of the term; the
rounding error is ~2 ulp(g) / e ~ 2e-14 of a row's terms, and a structural zero of J comes out as an exact 0.  Where a TF input changes
sign the right-hand side is only C^1; a stencil is shrunk until all its points lie on the branch the value takes (``stencil`` below).  Differencing along the
direction s_c itself would be cheaper but scales the step by 1 / max|s_c|: its rounding noise in the rows of small tangents then sits
above the 1e-12 tolerance and LSODA grinds through ~1e4 steps per piece.  The kinase forcing is piecewise constant, so the interval is cut at the kinase-bucket
edges: each piece is one odeint call with the edge as ``tcrit`` and the bucket of its START time frozen (what a step of the integrators
sees), so no piece ever evaluates the right-hand side across a discontinuity.

LSODA's Newton iteration is given the block-diagonal approximation blockdiag(J, .., J) of the augmented Jacobian, J = the oracle's
``fd_jacobian``; that only affects the convergence of the corrector, not what is solved.

The references of candidates 0..2 of the four ``network_m*_small`` fixtures are stored in ``tests/golden/net_sens_m*_small.npz``
(``tools/make_golden_net_sens.py`` runs this module; 1-3 minutes per candidate on a CPU) with their own tolerance-halving self-consistency
(the same integration at 1e-10).  ``np_dpred`` / ``np_metric_grads`` restate the chain from dY to the fold-change observables and the
scalar metrics in plain loops."""
from pathlib import Path

import numpy as np
from scipy.integrate import odeint

from oracle import network_models as nm

GOLDEN = Path(__file__).resolve().parent / "golden"
NAMES = ["network_m0_small", "network_m1_small", "network_m2_small", "network_m4_small"]
KINDS = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
N_CAND = 3
RTOL_GPU, ATOL_GPU = 1e-8, 1e-10


def slices(net):
    """{group: (start, stop)} of the candidate vector [c_k | A | B | C | D | Dp | E | tf_scale]."""
    nK, N, s = net.n_K, net.N, net.total_sites
    b = [0, nK, nK + N, nK + 2 * N, nK + 3 * N, nK + 4 * N, nK + 4 * N + s, nK + 5 * N + s, nK + 5 * N + s + 1]
    return {k: (b[i], b[i + 1]) for i, k in enumerate(KINDS)}


def row_to_params(net, row):
    sl = slices(net)
    return nm.Params(*(np.array(row[sl[k][0]:sl[k][1]], dtype=float) for k in nm.PARAM_KEYS), float(row[sl["tf_scale"][0]]))


def columns_one_per_kind(net, which=1):
    """One column per parameter kind: entry ``which`` of each group (clamped to the group), and tf_scale -> (cols, names)."""
    sl = slices(net)
    cols, names = [], []
    for k in KINDS:
        a, b = sl[k]
        j = min(which, b - a - 1)
        cols.append(a + j); names.append(k if k == "tf_scale" else f"{k}_{j}")
    return np.asarray(cols, dtype=np.int32), names


def _pieces(net, t_eval):
    """[(t_a, t_b, output indices in (t_a, t_b])] between consecutive kinase-bucket edges inside (t[0], t[-1])."""
    t0, t1 = float(t_eval[0]), float(t_eval[-1])
    edges = [t0] + [float(g) for g in net.kin_grid if t0 < g < t1] + [t1]
    return [(a, b, [k for k in range(1, len(t_eval)) if a < t_eval[k] <= b]) for a, b in zip(edges[:-1], edges[1:])]


def tangent_reference(net, row, cols, t_eval, y0=None, rtol=1e-12, atol=1e-12, mxstep=500000, delta=1e-2):
    """(Y [T, S], dY [T, S, K]) for the physical candidate ``row`` and the columns ``cols``."""
    row = np.asarray(row, dtype=float); t_eval = np.asarray(t_eval, dtype=float)
    S, K = net.S, len(cols)
    y = (nm.default_y0(net) if y0 is None else np.asarray(y0, float)).copy()
    z = np.concatenate([y, np.zeros(S * K)])
    Y = np.empty((t_eval.size, S)); dY = np.zeros((t_eval.size, S, K))
    Y[0] = y
    p0 = row_to_params(net, row)

    def stencil(fun, e, sig):
        """d fun / d eps at 0 by the sixth-order central difference with step e.  The right-hand side is only C^1 where a TF input
        changes sign (|v| and the u >= 0 branch of the synthesis rate), and a stencil that straddles such a point is wrong by O(e) times
        the jump of the second derivative -- so e is quartered until all its points lie on the branch the value takes (``sig``: the
        signs of the TF inputs, which are linear along every line the stencils walk, so the two end points decide)."""
        s0 = sig(0.0)
        while e > 1e-9 and (sig(3 * e) != s0 or sig(-3 * e) != s0):
            e *= 0.25
        return (45.0 * (fun(e) - fun(-e)) - 9.0 * (fun(2 * e) - fun(-2 * e)) + (fun(3 * e) - fun(-3 * e))) / (60.0 * e)

    def branch(p, yy, tb):
        return tuple(nm.tf_inputs(net, p, yy, nm.site_rates(net, p, tb)[1]) >= 0.0)

    def bump(v, j, h):
        w = v.copy(); w[j] += h
        return w

    for (ta, tb_, outs) in _pieces(net, t_eval):
        tmid = ta if ta == tb_ else 0.5 * (ta + tb_)           # any time inside the piece gives its bucket; the start time's bucket rules

        def f(zz, _t):
            yy = zz[:S]
            out = np.empty_like(zz)
            out[:S] = nm.rhs(net, p0, yy, tmid)
            J = np.empty((S, S))
            for j in range(S):
                J[:, j] = stencil(lambda h: nm.rhs(net, p0, bump(yy, j, h), tmid), delta * max(1.0, abs(yy[j])),
                                  lambda h: branch(p0, bump(yy, j, h), tmid))
            for c in range(K):
                ft = stencil(lambda h: nm.rhs(net, row_to_params(net, bump(row, cols[c], h)), yy, tmid), delta * abs(row[cols[c]]),
                             lambda h: branch(row_to_params(net, bump(row, cols[c], h)), yy, tmid))
                out[S * (1 + c): S * (2 + c)] = J @ zz[S * (1 + c): S * (2 + c)] + ft
            return out

        def jac(zz, _t):
            J = nm.fd_jacobian(net, p0, zz[:S], tmid)
            out = np.zeros((zz.size, zz.size))
            for c in range(K + 1):
                out[S * c: S * (c + 1), S * c: S * (c + 1)] = J
            return out

        ts = np.array([ta] + [t_eval[k] for k in outs] + ([tb_] if not outs or t_eval[outs[-1]] != tb_ else []))
        sol = odeint(f, z, ts, Dfun=jac, col_deriv=False, rtol=rtol, atol=atol, mxstep=mxstep, tcrit=[tb_])
        for q, k in enumerate(outs):
            Y[k] = sol[1 + q, :S]
            dY[k] = sol[1 + q, S:].reshape(K, S).T
        z = sol[-1].copy()
    return Y, dY


def load_golden(name):
    """The stored references of fixture ``name``: dict(cols [K], names, X [N_CAND, n_var] physical, t, Y [N_CAND, T, S],
    dY [N_CAND, T, S, K], self_err [N_CAND, K]: max |dY(1e-12) - dY(1e-10)| per column)."""
    g = np.load(GOLDEN / (name.replace("network_", "net_sens_") + ".npz"))
    return {k: g[k] for k in g.files}


def fixture(name):
    g = np.load(GOLDEN / f"{name}.npz")
    net = nm.Network.from_npz(g)
    X = np.stack([nm.params_to_row(nm.Params.from_npz(g, k)) for k in range(N_CAND)])
    return g, net, X


# ---------------------------------------------------------------------------------------------- numpy restatement of the output chain
def np_dpred(net, ld, Y, dY, eps=1e-12):
    """(pred [n_obs], dpred [n_obs, K]) by plain loops: total protein (P + sites / all 2^ns states), mRNA row, site row (combinatorial:
    all masks with the site's bit); fold change max(a, eps) / max(c, eps) differentiated through numerator and baseline, derivative 0
    through an active floor."""
    oy, ns, comb = net.offset_y, net.n_sites, net.model == 2
    K = dY.shape[2]
    pred, dpred = [], []

    def one(idx, t, tb):
        a = sum(Y[t, s] for s in idx); c = sum(Y[tb, s] for s in idx)
        da = sum((dY[t, s] for s in idx), np.zeros(K)); dc = sum((dY[tb, s] for s in idx), np.zeros(K))
        if not a > eps:
            a, da = eps, np.zeros(K)
        if not c > eps:
            c, dc = eps, np.zeros(K)
        pred.append(a / c); dpred.append(da / c - a * dc / (c * c))

    for i, t in zip(ld["p_prot"], ld["t_prot"]):
        cnt = (1 << int(ns[i])) if comb else 1 + int(ns[i])
        one([oy[i] + 1 + m for m in range(cnt)], int(t), int(ld["prot_base_idx"]))
    for i, t in zip(ld["p_rna"], ld["t_rna"]):
        one([oy[i]], int(t), int(ld["rna_base_idx"]))
    for i, j, t in zip(ld["p_pho"], ld["s_pho"], ld["t_pho"]):
        idx = [oy[i] + 1 + m for m in range(1 << int(ns[i])) if (m >> int(j)) & 1] if comb else [oy[i] + 2 + int(j)]
        one(idx, int(t), int(ld["pho_base_idx"]))
    return np.asarray(pred), np.asarray(dpred).reshape(len(pred), K)


def np_metric_grads(pred, dpred):
    """{metric: (value, d value / d x [K])} for total_signal, mean, variance, l2_norm over pred."""
    n = pred.size
    mu = pred.mean()
    nrm = np.sqrt(np.sum(pred * pred))
    return {"total_signal": (pred.sum(), dpred.sum(axis=0)), "mean": (mu, dpred.sum(axis=0) / n),
            "variance": (np.mean((pred - mu) ** 2), 2.0 / n * np.sum((pred - mu)[:, None] * dpred, axis=0)),
            "l2_norm": (nrm, np.sum(pred[:, None] * dpred, axis=0) / nrm)}
