"""Reference for one iteration of the native bounded Levenberg-Marquardt fit (pk_fit_protein_rows_batch: csrc/pk_lm.hip, csrc/pk_lm.hpp),
shared by tests/test_lm_reference_cpu.py and tests/test_gpu_fit_native_exact.py (not a test module).  Plain numpy in np.longdouble (64-bit
mantissa on x86: 2^-11 of a double's unit roundoff), for ONE row; no torch, no library.

With flat [F] and dflat [F, P] as a solve wrote them, p [P] the point in the fitted space, theta_eff = exp(p) under log_space, isig [Nr] =
1 / sigma (ones without sigma), Nr = F + (P if use_reg else 0):

    residual            r_f = (flat_f - target_f) isig_f  (f < F);   r_{F+i} = (lam / P) p_i^2 isig_{F+i};   non-finite -> 1e6
    cost                1/2 sum_f r_f^2
    weighted Jacobian   Jw_fi = dflat_fi (theta_eff_i if log_space else 1) isig_f;   non-finite -> 0
    normal equations    A = Jw^T Jw + diag(d^2),  g = Jw^T r_data + d r_ridge,  d_i = 2 (lam / P) p_i isig_{F+i}
    one iteration       free set, Marquardt scaling DD_i = max(sqrt A_ii, 1e-12), done rule; for every damping level lv the step of
                        (A masked to the free set + mu 4^lv DD^2 on the free diagonal, identity rows for fixed variables) x = -g_free,
                        the trial point clip(p + step), dp = trial - p and the predicted reduction -(g . dp + 1/2 dp^T A dp) (A unmasked)
    pick                the first level with rho = (cost - cn) / pred > 1e-4 (rho = -1 where pred <= 0) and cn < cost

The sums of magnitudes that come back with A and g are what a rounding bound scales with."""
import numpy as np

LD = np.longdouble


def _ld(x):
    return np.asarray(x, dtype=LD)


def weighted_jacobian(dflat, theta_eff, isig, log_space):
    """Jw [F, P] in long double; isig may carry the ridge entries behind the F data entries (they are not used here)."""
    J = _ld(dflat)
    if log_space:
        J = J * _ld(theta_eff)[None, :]
    J = J * _ld(isig)[:J.shape[0], None]
    return np.where(np.isfinite(J), J, LD(0))


def normal_equations(Jw, r, p, lam, isig_ridge, use_reg):
    """(A [P, P], g [P], sum |terms of A| [P, P], sum |terms of g| [P]).  r [Nr]: data entries, then the ridge entries when use_reg;
    isig_ridge [P] = isig[F:] (ignored without use_reg)."""
    Jw = _ld(Jw)
    F, P = Jw.shape
    r = _ld(r)
    A = Jw.T @ Jw
    absA = np.abs(Jw).T @ np.abs(Jw)
    g = Jw.T @ r[:F]
    absg = np.abs(Jw).T @ np.abs(r[:F])
    if use_reg:
        d = LD(2) * (LD(lam) / LD(P)) * _ld(p) * _ld(isig_ridge)
        d = np.where(np.isfinite(d), d, LD(0))
        A = A + np.diag(d * d)
        absA = absA + np.diag(d * d)
        g = g + d * r[F:]
        absg = absg + np.abs(d * r[F:])
    return A, g, absA, absg


def residual(flat, target, p, lam, isig, use_reg):
    """(r [Nr], cost) in long double."""
    flat, p, isig = _ld(flat), _ld(p), _ld(isig)
    F, P = flat.shape[0], p.shape[0]
    r = (flat - _ld(target)) * isig[:F]
    if use_reg:
        r = np.concatenate([r, (LD(lam) / LD(P)) * p * p * isig[F:F + P]])
    r = np.where(np.isfinite(r), r, LD(1e6))
    return r, LD(0.5) * np.sum(r * r)


def _solve_refined(M, b):
    """M x = b for a symmetric positive definite M given in long double: float64 LAPACK, then refinement with the residual in long double
    (each step gains a factor cond 2^-53; two steps leave the float64 solve's error below cond^2 2^-106 relative).  None when M is not
    positive definite in float64 (the fit takes a zero step there)."""
    M64, b64 = np.asarray(M, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not (np.all(np.isfinite(M64)) and np.all(np.isfinite(b64))):
        return None
    try:
        np.linalg.cholesky(M64)
    except np.linalg.LinAlgError:
        return None
    x = _ld(np.linalg.solve(M64, b64))
    for _ in range(2):
        res = _ld(b) - _ld(M) @ x
        x = x + _ld(np.linalg.solve(M64, np.asarray(res, dtype=np.float64)))
    return x


def one_iteration(A, g, p, lb, ub, mu=1e-3, levels=12, cost=0.0):
    """The algebra between a Jacobian phase and the trial solves for one row.  Returns a dict:
      free [P] bool    not (on a bound with the gradient pointing out of the box)                (lm_fixed)
      DD [P]           max(sqrt A_ii, 1e-12)                                                     (lm_scale)
      done bool        nothing free, or |g_free| < 1e-14 max(1, cost)                            (lm_row_done; `cost`: the row's cost)
      gfree_norm       |g_free|
      step, trial, dp [levels, P], pred [levels], cond [levels] (2-norm condition number of each damped matrix, float64)."""
    A, g, p, lb, ub = _ld(A), _ld(g), _ld(p), _ld(lb), _ld(ub)
    P = p.shape[0]
    fixed = ((p <= lb) & (g > 0)) | ((p >= ub) & (g < 0))
    free = ~fixed
    DD = np.maximum(np.sqrt(np.maximum(np.diag(A), LD(0))), LD(1e-12))
    gfree = np.where(free, g, LD(0))
    gnorm = np.sqrt(np.sum(gfree * gfree))
    done = bool(not free.any() or gnorm < LD(1e-14) * max(LD(1), LD(cost)))
    step, trial, dp = (np.zeros((levels, P), dtype=LD) for _ in range(3))
    pred, cond = np.zeros(levels, dtype=LD), np.zeros(levels)
    mask = free[:, None] & free[None, :]
    for lv in range(levels):
        M = np.where(mask, A, LD(0))
        M[np.arange(P), np.arange(P)] += np.where(free, LD(mu) * LD(4.0 ** lv) * DD * DD, LD(1))
        x = _solve_refined(M, -gfree)
        if x is not None:
            x = np.where(np.isfinite(x), x, LD(0))
            step[lv] = np.where(free, x, LD(0))
        with np.errstate(all="ignore"):
            M64 = np.asarray(M, dtype=np.float64)
            cond[lv] = np.linalg.cond(M64) if np.all(np.isfinite(M64)) else np.inf
        trial[lv] = np.minimum(np.maximum(p + step[lv], lb), ub)
        dp[lv] = trial[lv] - p
        pred[lv] = -(np.sum(g * dp[lv]) + LD(0.5) * np.sum(dp[lv] * (A @ dp[lv])))
    return dict(free=free, DD=DD, done=done, gfree_norm=gnorm, step=step, trial=trial, dp=dp, pred=pred, cond=cond)


def pick(cost, cn, pred):
    """(level, margins): the first level lv with cn[lv] < cost and rho > 1e-4 (-1: none), and for every level looked at (up to and
    including the accepted one) the pair (rho - 1e-4, cn / cost - 1) its decision rests on."""
    cost = LD(cost)
    margins = []
    for lv, (c, pd) in enumerate(zip(_ld(cn).ravel(), _ld(pred).ravel())):
        rho = (cost - c) / pd if pd > 0 else LD(-1)
        margins.append((float(rho - LD(1e-4)), float(c / cost - LD(1)) if cost != 0 else float("inf")))
        if c < cost and rho > LD(1e-4):
            return lv, margins
    return -1, margins
