"""GPU: the native Levenberg-Marquardt fit (pk_fit_protein_rows_batch, csrc/pk_lm.hip) against the long-double restatement of ONE
iteration (tests/lm_reference.py, held to the host build of csrc/pk_lm.hpp by tests/test_lm_reference_cpu.py), and the per-row argument
layouts of the header against one-row calls.  tests/test_gpu_fit_native.py compares the native driver with the Python driver, which
restates the same rules, at rtol 1e-5; here every bound is derived from the summation lengths and the number formats.  Every case pins
kernel="group", so a row's solves do not depend on the batch around it.

What each test would catch (csrc/pk_lm.hip unless batch.py is named):
  (a) start state          lm_gather_kernel: the clip `fmin(fmax(x, lb), ub)` and its `bounds_batched` index; `pr.mu[row] = kLmMu0`.
                           lm_accept_kernel, init path: `flat + slot * pr.F` with slot = q, lm_residual's `target_batched` / `sigma_batched`
                           index and its ridge entry `(lam[row] / P) x^2 isig(F + i)`; the 256 partial sums and `cn[lv] = 0.5 t`; shared
                           sigma [Nr] catches `sigma_batched` ignored in lm_isig (row 1 would read past the one row there is).
                           The driver: `why` initialised to 3, counters {0, R, 1, 0, 0, 0}.
  (b) normal equations     lm_normal_kernel: F = 24 a tile loop that assumes a full tile (`nf` ignored); F = 32 a loop that runs one tile too
                           many or too few at `f0 < F`; F = 65 a loop that stops at `f0 + kLmTile <= F` (the last tile's single row is the
                           last site at the last output time); P = 26 the packed-triangle walk `o -= P - j; ++j` past the first
                           256 entries (entries 256..350 would stay 0 or land in the wrong slot); the ridge diagonal `acc[lm_tri(P, tid, tid)]
                           += d d` in the wrong slot or before the data rows; `v *= w[i]` under log_space (w = exp(p), column not row);
                           `lm_isig(pr, row, f0 + ff)` indexed by ff alone; the mirrored write `A[j P + i] = v`.
  (c) iterate              lm_normal_kernel's g_acc (`Jt[ff P + tid] * rt[ff]`, the ridge `d * rrow[F + tid]`), lm_fixed / lm_scale inputs;
                           lm_trials_kernel: `pr.mu[row]`, the level `lv = blockIdx.y`, `slot = lv * m + q`; lm_accept_kernel: `pred[lv * m +
                           q]`, the first acceptable level, `trials + (sel * m + q) * P`.  Belonging together catches a wrong slot in
                           `flat + slot * pr.F` or in the copy of x into p: r and cost would be those of another trial.
  (d) per-row layouts      (i) `row * pr.S` written as `q * pr.S` in lm_gather_kernel / lm_trials_kernel (y0_out of a pending list shorter than
                           the batch), `row * pr.F` as `q * pr.F` in lm_residual, `row * P` in the bounds of lm_normal_kernel and
                           lm_trials_kernel, `c < pr.S` of lm_gather_kernel's P-wide element loop (S = 5, 8, 5 against P = 10, 16, 9; none
                           of these sizes has S > P); (iii) batch.py `if lbb != ubb` expanding the wrong one;
                           (iv) keeps (i) from passing on rows that are copies of each other.
  (e) optional outputs     the arena carve `pr.r = r ? r : cv.take(...)`, `pr.A = JTJ ? JTJ : ...` (a NULL written through, or a carve that
                           overlaps theta_w), `if (reason)`.
  (f) stationarity         the whole loop: a fit that stops early (lm_converged fed the wrong norms, lm_row_done fed another row's cost)
                           leaves a projected gradient far above the Python driver's."""
import ctypes as C

import numpy as np
import pytest

import lm_reference as ref
from oracle import protein_models as pm
from test_gpu_fit_native import _report, _same_steps, eng, ms  # noqa: F401  (eng, ms: the module-scoped fixtures)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
FIELDS = ("p", "cost", "r", "JTJ", "reason")


# ------------------------------------------------------------------------------------------------------------------ problems and calls

def _shared(eng, model, n, R, seed, t=pm.TIME_POINTS, ridge=False, sigma=None, lam_zeros=0, box=None):
    """The construction of test_gpu_fit_native._problem on a grid of the caller's: shared y0 = 1, one noisy target, one box.  randmod is
    fitted in log space.  sigma: None | "shared" [Nr] | "rows" [R, Nr]; `lam_zeros` rows get lam = 0 among per-row lam > 0."""
    mid = pm.MODEL_IDS[model]
    S, P = pm.n_states(mid, n), pm.n_params(mid, n)
    log_space = model == "randmod"
    box = box or ((1e-3, 10.0) if log_space else (0.0, 2.0))
    rng = np.random.default_rng([seed, mid, n, R, len(t)])
    truth = rng.uniform(0.3, 1.5, size=P)
    y0 = np.ones(S)
    t = np.asarray(t, float)
    target = eng.solve_ode_batch(model, truth[None], y0, n, t, want_sol=False, kernel="group").flat.cpu().numpy()[0]
    target = np.abs(target * (1.0 + 0.02 * rng.standard_normal(target.size)))
    F = target.size
    lb, ub = np.full(P, box[0]), np.full(P, box[1])
    P0 = truth * rng.uniform(0.2, 4.0, size=(R, P))                      # not clipped: the fit's own clip is under test
    if log_space:
        P0, lb, ub = np.log(P0), np.log(lb), np.log(ub)
    lam = None
    if ridge:
        lam = rng.uniform(0.01, 0.2, size=R)
        lam[:lam_zeros] = 0.0
    Nr = F + (P if ridge else 0)
    sg = {None: None, "shared": rng.uniform(0.5, 2.0, size=Nr), "rows": rng.uniform(0.5, 2.0, size=(R, Nr))}[sigma]
    return dict(model=model, n=n, t=t, P0=P0, y0=y0, target=target, lb=lb, ub=ub, lam=lam, sigma=sg, ridge=ridge, log_space=log_space,
                P=P, S=S, F=F, Nr=Nr, R=R)


def _per_row(eng, model, n, R, seed, ridge, sigma):
    """Every row its own y0 in U(0.3, 1.5), its own truth and target, its own box -- lb = truth U(0.4, 1.05), ub = lb + truth U(0.1, 1):
    where lb > truth or ub < truth the row ends on that bound -- and its own lam."""
    mid = pm.MODEL_IDS[model]
    S, P = pm.n_states(mid, n), pm.n_params(mid, n)
    log_space = model == "randmod"
    rng = np.random.default_rng([seed, mid, n, R])
    t = pm.TIME_POINTS
    truth = rng.uniform(0.3, 1.5, size=(R, P))
    y0 = rng.uniform(0.3, 1.5, size=(R, S))
    target = eng.solve_ode_batch(model, truth, y0, n, t, want_sol=False, kernel="group").flat.cpu().numpy()
    target = np.abs(target * (1.0 + 0.02 * rng.standard_normal(target.shape)))
    F = target.shape[1]
    lb = truth * rng.uniform(0.4, 1.05, size=(R, P))
    ub = lb + truth * rng.uniform(0.1, 1.0, size=(R, P))
    P0 = truth * rng.uniform(0.2, 4.0, size=(R, P))
    if log_space:
        P0, lb, ub = np.log(P0), np.log(lb), np.log(ub)
    lam = rng.uniform(0.01, 0.2, size=R) if ridge else None
    Nr = F + (P if ridge else 0)
    sg = {None: None, "shared": rng.uniform(0.5, 2.0, size=Nr), "rows": rng.uniform(0.5, 2.0, size=(R, Nr))}[sigma]
    return dict(model=model, n=n, t=t, P0=P0, y0=y0, target=target, lb=lb, ub=ub, lam=lam, sigma=sg, ridge=ridge, log_space=log_space,
                P=P, S=S, F=F, Nr=Nr, R=R)


def _take(x, rows, ndim_rows):
    """Rows of a per-row argument; a shared one (fewer dimensions) passes as it is."""
    return x if x is None or np.ndim(x) < ndim_rows else x[rows]


def _args(pb, rows=None, shared_form=False):
    """Arguments of fit_rows_batch for `rows` of the problem.  shared_form (one row k): that row's arguments as [S] / [F] / [Nr] / [P]."""
    rows = slice(None) if rows is None else rows
    a = dict(P0=pb["P0"][rows], y0=_take(pb["y0"], rows, 2), target=_take(pb["target"], rows, 2), sigma=_take(pb["sigma"], rows, 2),
             lam=_take(pb["lam"], rows, 1), lb=_take(pb["lb"], rows, 2), ub=_take(pb["ub"], rows, 2))
    if shared_form:
        a = {k: (v if v is None or k in ("P0", "lam") or np.ndim(v) == 1 else v[0]) for k, v in a.items()}
    return a


def _fit(ms, pb, rows=None, shared_form=False, driver="native", **kw):
    a = _args(pb, rows, shared_form)
    extra = dict(driver="native") if driver == "native" else dict(lm_algebra="host", device_algebra=True)
    return ms.fit_rows_batch(pb["model"], pb["n"], pb["t"], a["P0"], a["y0"], a["target"], sigma=a["sigma"], lam=0.0 if a["lam"] is None else a["lam"],
                             bounds=(a["lb"], a["ub"]), force_reg=pb["ridge"], jacobian="sens", kernel="group", **extra, **kw)


def _same_bits(a, b, rows=slice(None)):
    return [f for f in FIELDS if not np.array_equal(getattr(a, f), getattr(b, f)[rows])]


def _row(x, k, ndim_rows):
    return x if np.ndim(x) < ndim_rows else x[k]


def _isig(pb, k):
    return np.ones(pb["Nr"], dtype=LD) if pb["sigma"] is None else LD(1) / np.asarray(_row(pb["sigma"], k, 2), dtype=LD)


def _lam(pb, k):
    return 0.0 if pb["lam"] is None else float(pb["lam"][k])


# ------------------------------------------------------------------------------------------------------------------ the reference side

def _thetas(pb, p):
    """The parameter vectors a reference solve may be handed for the fitted points p [m, P].  The fit forms theta = exp(p) on the device and
    nobody outside sees those bits: under log space the reference is evaluated at torch's exp on the same device and at its two
    neighbours (every component one ulp up / down), and the spread over the three is added to every bound that rests on theta."""
    if not pb["log_space"]:
        return [np.asarray(p, float)]
    import torch
    th = torch.exp(torch.as_tensor(np.asarray(p, float), device="cuda")).cpu().numpy()
    return [th, np.nextafter(th, np.inf), np.nextafter(th, -np.inf)]


def _flat_at(eng, pb, p, rows):
    """flat [variants][m, F] of ONE solve launch per variant for the problems `rows` at the points p [m, P], options as the fit's."""
    y0 = pb["y0"] if pb["y0"].ndim == 1 else pb["y0"][rows]
    return [eng.solve_ode_batch(pb["model"], th, y0, pb["n"], pb["t"], want_sol=False, kernel="group").flat.cpu().numpy() for th in _thetas(pb, p)]


def _residuals_at(eng, pb, p, rows):
    """[variants][m] of (r, cost) in long double."""
    return [[ref.residual(fl[j], _row(pb["target"], k, 2), p[j], _lam(pb, k), _isig(pb, k), pb["ridge"]) for j, k in enumerate(rows)]
            for fl in _flat_at(eng, pb, p, rows)]


def _check_r_and_cost(tag, eng, pb, fit, rows=None):
    """r within 4 ulp per entry (a difference, the reciprocal of sigma and a product: 1.5 ulp; the ridge entry's four operations and the
    reciprocal: 2.5 ulp) and cost within (Nr + 260) 2^-53 sum r^2 (Nr products, strided sums of at most Nr / 256 + 1 terms, the sum of the
    256 partials, the factor 1/2 exact) of residual() at flat(p returned), plus the spread over exp's neighbours under log space."""
    rows = np.arange(pb["R"]) if rows is None else np.asarray(rows)
    var = _residuals_at(eng, pb, fit.p, rows)
    worst_r = worst_c = spread_r = spread_c = 0.0
    for j in range(rows.size):
        r0, c0 = var[0][j]
        sr = np.max([np.abs(v[j][0] - r0) for v in var], axis=0).astype(float)
        sc = float(max(abs(v[j][1] - c0) for v in var))
        r64 = np.asarray(r0, float)
        worst_r = max(worst_r, float(np.max(np.abs(fit.r[j] - r0).astype(float) / (4.0 * np.spacing(np.abs(r64)) + sr))))
        worst_c = max(worst_c, float(abs(fit.cost[j] - c0)) / ((pb["Nr"] + 260) * U * float(np.sum(r0 * r0)) + sc))
        spread_r = max(spread_r, float(np.max(sr / np.maximum(np.abs(r64), 1e-300)))); spread_c = max(spread_c, sc / float(c0))
    print(f"[{tag}] r: max |r - ref| / (4 ulp + spread) {worst_r:.3e}  cost: max |cost - ref| / ((Nr + 260) u sum r^2 + spread) {worst_c:.3e}  "
          f"exp spread: r {spread_r:.3e} relative, cost {spread_c:.3e} relative", flush=True)
    assert worst_r <= 1.0 and worst_c <= 1.0
    return worst_r, worst_c


def _normal_at(eng, pb, p0, rcs):
    """[variants][R] of (A, g, absA, d2) from ONE solve_ode_sens_batch call per variant on every row, in order, with the fit's options."""
    out = []
    for v, th in enumerate(_thetas(pb, p0)):
        dflat = eng.solve_ode_sens_batch(pb["model"], th, pb["y0"], pb["n"], pb["t"]).dflat.cpu().numpy()
        rows = []
        for k in range(pb["R"]):
            isig = _isig(pb, k)
            Jw = ref.weighted_jacobian(dflat[k], th[k], isig, pb["log_space"])
            A, g, absA, _ = ref.normal_equations(Jw, rcs[v][k][0], p0[k], _lam(pb, k), isig[pb["F"]:], pb["ridge"])
            d = LD(2) * (LD(_lam(pb, k)) / pb["P"]) * np.asarray(p0[k], dtype=LD) * isig[pb["F"]:] if pb["ridge"] else np.zeros(pb["P"], dtype=LD)
            rows.append((A, g, absA, d * d))
        out.append(rows)
    return out


# ------------------------------------------------------------------------------------------------------------------ (a) start state

@pytest.mark.parametrize("case", ["distmod3", "randmod2"])
def test_start_state(eng, ms, case):
    """max_iter = 0: p = clip(P0) bit for bit, reason 3, one solve launch and nothing else, r and cost of the start point.
    Measured on MI355X (ratios to the bounds of _check_r_and_cost):
      distmod n = 3, 7 rows                                                   r 0.125 (half an ulp)   cost 7.9e-3
      randmod n = 2, 6 rows, log space, ridge, lam = 0 twice, shared sigma    r 0.41                  cost 6.5e-3
    (spread of the reference over exp's neighbours: 1.1e-8 relative in r, 5.9e-12 in cost)."""
    pb = _shared(eng, "distmod", 3, 7, 21) if case == "distmod3" else _shared(eng, "randmod", 2, 6, 22, ridge=True, sigma="shared", lam_zeros=2,
                                                                                     box=(1e-3, 2.0))
    fit = _fit(ms, pb, max_iter=0)
    p0 = np.clip(pb["P0"], pb["lb"], pb["ub"])
    assert (p0 != pb["P0"]).any()                                        # the clip has work to do
    assert np.array_equal(fit.p, p0)
    assert np.array_equal(fit.reason, np.full(pb["R"], 3, np.int32))
    assert fit.counters == dict(iterations=0, solves=pb["R"], launches=1, host_waits=0, jacobian_phases=0, trial_rounds=0)
    assert fit.r.shape == (pb["R"], pb["Nr"])
    assert np.all(fit.JTJ == 0.0)                                        # never written: the caller's buffer as it was handed in
    _check_r_and_cost(f"a {case}", eng, pb, fit)


# ------------------------------------------------------------------------------------------------------------------ (b), (c)

SHORT3, SHORT4 = np.array([0.0, 1.0, 4.0]), np.array([0.0, 1.0, 4.0, 16.0])
NORMAL_CASES = {                    # model, n, t, F, P, keyword arguments of _shared
    "F24": ("distmod", 7, SHORT3, 24, 18, {}),
    "F32": ("distmod", 7, SHORT4, 32, 18, {}),
    "F65": ("distmod", 3, pm.TIME_POINTS, 65, 10, {}),
    "P26": ("distmod", 11, pm.TIME_POINTS, 177, 26, {}),
    "succ6": ("succmod", 6, pm.TIME_POINTS, 107, 16, {}),
    "rand2": ("randmod", 2, pm.TIME_POINTS, None, None, dict(ridge=True, sigma="rows")),
    "n62": ("distmod", 62, pm.TIME_POINTS, 891, 128, {}),
}
NORMAL_PARAMS = [(c, R) for c in NORMAL_CASES if c != "n62" for R in (1, 5)] + [("n62", 2)]
SEED_BC = 31


def _one_iteration_case(eng, ms, case, R):
    model, n, t, F, P, kw = NORMAL_CASES[case]
    pb = _shared(eng, model, n, R, SEED_BC, t=t, **kw)
    if F is not None:
        assert (pb["F"], pb["P"]) == (F, P)
    return pb, _fit(ms, pb, max_iter=1)


def _reference_iteration(eng, pb):
    """The reference's first iteration of every row: (clip(P0), residuals [variants][R], normal equations [variants][R], one_iteration
    [variants][R], picks [R] of (level, margins) or None for a row that is done at once).  Three launches per variant of exp: the start
    residuals, the Jacobian, and -- for the first variant alone -- the trial costs of all 12 levels of every row."""
    R = pb["R"]
    rows = np.arange(R)
    p0 = np.clip(pb["P0"], pb["lb"], pb["ub"])
    rcs = _residuals_at(eng, pb, p0, rows)
    nrm = _normal_at(eng, pb, p0, rcs)
    its = [[ref.one_iteration(v[k][0], v[k][1], p0[k], pb["lb"], pb["ub"], mu=1e-3, levels=12, cost=rcs[i][k][1]) for k in range(R)]
           for i, v in enumerate(nrm)]
    trials = np.concatenate([np.asarray(its[0][k]["trial"], float) for k in range(R)])            # [R * 12, P], row-major by problem
    rc_t = _residuals_at(eng, pb, trials, np.repeat(rows, 12))[0]
    picks = [None if its[0][k]["done"] else ref.pick(rcs[0][k][1], [rc_t[k * 12 + lv][1] for lv in range(12)], its[0][k]["pred"]) for k in range(R)]
    return p0, rcs, nrm, its, picks


@pytest.mark.parametrize("case,R", NORMAL_PARAMS)
def test_normal_equations_and_first_iterate(eng, ms, case, R):
    """max_iter = 1.  (b) JTJ is J^T J at clip(P0) (the first Jacobian phase sees every row, in order, in one chunk): against
    normal_equations() of one solve_ode_sens_batch call, per entry within (F + 8) 2^-53 sum_f |Jw_fi Jw_fj| -- each Jw entry carries the
    chain-rule product, the reciprocal of sigma and its product (3 u), a term of the sum twice that and its own product (7 u), the
    sequential sum over the tiles F u more, the ridge entry d^2 counted among the terms -- plus 6 u d^2 for the three operations that form
    d, squared; and JTJ[k] == JTJ[k].T bit for bit.
    (c) The returned p equals the reference's trial point of the level pick() chooses, within P cond 2^-52 |step| (cond of the reference's
    damped matrix), trial costs from one solve_ode_batch call at the reference's trial points; rows done at once have p == clip(P0); the
    returned r and cost are those of the returned p.  Under log space the spread of the reference over exp's neighbours is added.
    The seed was checked on the CPU first with pm.solve_exact_lti / pm.sens_exact_lti standing in for the library's solves (no row's
    decision margin was narrow) and then on the GPU: no row of any case is excused.
    Measured on MI355X (ratios to the bounds; level = the damping level pick() chose for each row; no row excused anywhere):
      case   R   JTJ      p        r      cost     levels          |  case   R   JTJ      p        r      cost     levels
      F24    1   0.106    2.2e-3   0.125  1.1e-3   0               |  F24    5   0.135    2.4e-3   0.125  3.0e-3   0 0 0 1 0
      F32    1   0.092    8.2e-4   0.125  4.9e-4   0               |  F32    5   0.107    5.2e-3   0.125  3.6e-3   0 0 4 0 4
      F65    1   0.096    4.7e-3   0      6.5e-3   5               |  F65    5   0.136    1.3e-2   0.125  5.5e-3   0 0 0 0 0
      P26    1   0.100    3.9e-4   0.125  7.8e-4   0               |  P26    5   0.138    2.5e-3   0.125  6.4e-3   0 0 0 0 0
      succ6  1   0.085    1.2e-3   0.125  9.6e-3   0               |  succ6  5   0.157    4.7e-3   0.125  9.0e-3   6 0 5 6 2
      rand2  1   0.013    1.1e-4   0.23   2.9e-5   6               |  rand2  5   0.045    2.0e-4   0.35   1.6e-3   0 7 1 0 1
      n62    2   0.078    1.8e-5   0.125  1.6e-3   0 0
    (rand2: the spread over exp's neighbours is up to 3.8e-10 of sum |terms| in JTJ and 4.7e-9 relative in r: it dominates those bounds.)"""
    pb, fit = _one_iteration_case(eng, ms, case, R)
    Pn, Fn = pb["P"], pb["F"]
    p0, rcs, nrm, its, picks = _reference_iteration(eng, pb)
    # (b)
    assert np.array_equal(fit.JTJ, fit.JTJ.transpose(0, 2, 1))
    worst_b = spread_b = 0.0
    for k in range(R):
        A, _, absA, d2 = nrm[0][k]
        spread = np.max([np.abs(v[k][0] - A) for v in nrm], axis=0).astype(float)
        bound = (Fn + 8) * U * absA.astype(float) + np.diag(6.0 * U * d2.astype(float)) + spread
        err = np.abs(fit.JTJ[k] - A).astype(float)
        assert np.all(np.diag(fit.JTJ[k]) > 0.0)
        worst_b = max(worst_b, float(np.max(err / np.maximum(bound, 1e-300))))
        spread_b = max(spread_b, float(np.max(spread / np.maximum(absA.astype(float), 1e-300))))
    print(f"[b {case} R={R}] F {Fn} P {Pn}: max |JTJ - ref| / bound {worst_b:.3e}  (exp spread {spread_b:.3e} of sum |terms|)", flush=True)
    assert worst_b <= 1.0
    # (c)
    excused, worst_c, levels = 0, 0.0, []
    for k in range(R):
        it = its[0][k]
        if it["done"]:
            assert fit.reason[k] == 1 and np.array_equal(fit.p[k], p0[k])
            levels.append("done")
            continue
        L, margins = picks[k]
        levels.append(L)
        if any(abs(m[0]) < 1e-6 or abs(m[1]) < 1e-9 for m in margins):
            excused += 1
            continue
        if L < 0:
            assert fit.reason[k] == 2 and np.array_equal(fit.p[k], p0[k])
            continue
        want = np.asarray(it["trial"][L], float)
        spread = max(float(np.linalg.norm((v[k]["trial"][L] - it["trial"][L]).astype(float))) for v in its)
        tol = Pn * it["cond"][L] * 2.0 * U * float(np.linalg.norm(it["step"][L].astype(float))) + spread
        err = float(np.linalg.norm(fit.p[k] - want))
        worst_c = max(worst_c, err / tol)
        assert np.all(fit.p[k] >= pb["lb"]) and np.all(fit.p[k] <= pb["ub"])
    print(f"[c {case} R={R}] levels {levels}  excused {excused}  max |p - trial_ref| / (P cond 2^-52 |step| + spread) {worst_c:.3e}  reasons {fit.reason}", flush=True)
    assert excused <= R // 10
    assert worst_c <= 1.0
    assert fit.counters["jacobian_phases"] == 1 and fit.counters["iterations"] == 1
    _check_r_and_cost(f"c {case} R={R} belonging", eng, pb, fit)


@pytest.mark.parametrize("trial_levels", [1, 3])
@pytest.mark.parametrize("case", ["F65", "succ6", "rand2"])
def test_returned_p_r_and_cost_belong_together(eng, ms, case, trial_levels):
    """max_iter = 6: after several accepted and rejected levels, with the pending list shrinking, r is residual() of flat(p returned) and
    cost is 0.5 |r|^2 within the bounds of (a).  A slot of another row or another level would give a plausible residual of another problem.
    Measured on MI355X (ratios to the bounds, equal for one and three levels per launch): F65 r 0 (bit-equal), cost 9.7e-3; succ6 r 0,
    cost 9.4e-3; rand2 r 0.45, cost 1.7e-3 (spread over exp's neighbours 1.1e-8 relative in r)."""
    model, n, t, _, _, kw = NORMAL_CASES[case]
    pb = _shared(eng, model, n, 9, 41, t=t, **kw)
    fit = _fit(ms, pb, max_iter=6, trial_levels=trial_levels)
    assert fit.counters["trial_rounds"] >= 6 and np.any(fit.p != np.clip(pb["P0"], pb["lb"], pb["ub"]))
    _check_r_and_cost(f"belong {case} K={trial_levels}", eng, pb, fit)


# ------------------------------------------------------------------------------------------------------------------ (d) per-row layouts

LAYOUT_CASES = {"distmod3": ("distmod", 3, 7, False), "succmod6": ("succmod", 6, 5, False), "randmod2": ("randmod", 2, 5, True)}


@pytest.mark.parametrize("sigma", [None, "shared", "rows"])
@pytest.mark.parametrize("case", list(LAYOUT_CASES))
def test_per_row_layouts(eng, ms, case, sigma):
    """Every row its own y0, target, box and lam (_per_row); sigma absent, [Nr] and [R, Nr]; max_iter = 6 with three levels per launch
    (slot = lv m + q with m < R once rows leave the pending list) and with one.
    (i) bit for bit what R one-row calls give, each handed that row's arguments in the SHARED form, and the same for the reversed batch;
    (ii) the steps of the Python host driver given the same batched arguments (the limits of _same_steps);
    (iii) lb batched with ub shared, and the reverse, equal both batched bit for bit;
    (iv) any two rows' one-row results differ in p, cost and r, so a wrong row index cannot pass (i).
    Measured on MI355X, Python host driver against native as fractions of the limits of _same_steps (p: 1e-7 + 1e-5 |p|; JTJ: 1e-9 max|JTJ|
    + 1e-5 |JTJ|), sigma None / [Nr] / [R, Nr], the same for one and three levels per launch:
      distmod n = 3   p 2.3e-6 / 2.2e-6 / 1.9e-6   JTJ 1.1e-5 / 4.3e-6 / 1.6e-5   solves (K = 3) 193 / 196 / 202, full rounds would take 280 / 301 / 280
      succmod n = 6   p 2.1e-4 / 7.7e-5 / 2.5e-5   JTJ 4.6e-3 / 1.4e-4 / 5.0e-5   solves 140 / 137 / 134, full rounds 185 / 170 / 155
      randmod n = 2   p 4.5e-4 / 8.4e-4 / 6.8e-4   JTJ 3.2e-5 / 8.1e-5 / 3.1e-4   solves 137 / 128 / 134, full rounds 185 / 140 / 170
    Every row of every case ends with a variable on its box; every row runs its six iterations (reason 3)."""
    model, n, R, ridge = LAYOUT_CASES[case]
    pb = _per_row(eng, model, n, R, 51, ridge, sigma)
    for K in (3, 1):
        kw = dict(max_iter=6, trial_levels=K)
        full = _fit(ms, pb, **kw)
        ones = [_fit(ms, pb, rows=slice(k, k + 1), shared_form=True, **kw) for k in range(R)]
        for k in range(R):
            assert _same_bits(ones[k], full, slice(k, k + 1)) == [], (K, k)                 # (i)
        for a in range(R):
            for b in range(a + 1, R):
                assert all(not np.array_equal(getattr(ones[a], f), getattr(ones[b], f)) for f in ("p", "cost", "r", "JTJ")), (a, b)    # (iv)
        rev = np.arange(R)[::-1]
        assert _same_bits(_fit(ms, pb, rows=rev, **kw), full, rev) == [], K
        on_box = (full.p == pb["lb"]) | (full.p == pb["ub"])
        assert on_box.any() and not on_box.all()
        host = _fit(ms, pb, driver="python", **kw)
        _report(f"d {case} sigma={sigma} K={K}: python host / native", host, full)
        print(f"   rows with a variable on the box {int(on_box.any(axis=1).sum())} of {R}  reasons {full.reason}  counters {full.counters}", flush=True)
        _same_steps(host, full)                                                            # (ii)
        if K == 3:                                                                         # some round ran with m < R: fewer solves than full rounds take
            c = full.counters
            assert c["solves"] < R + R * c["jacobian_phases"] + 3 * R * c["trial_rounds"]
    # (iii): one bound shared, the other per row
    for shared in ("ub", "lb"):
        one = pb[shared].max(axis=0) if shared == "ub" else pb[shared].min(axis=0)
        mixed = _fit(ms, dict(pb, **{shared: one}), max_iter=6, trial_levels=3)
        both = _fit(ms, dict(pb, **{shared: np.tile(one, (R, 1))}), max_iter=6, trial_levels=3)
        assert _same_bits(mixed, both) == [], shared


# ------------------------------------------------------------------------------------------------------------------ (e) optional outputs

def _raw_fit(eng, pb, want_r=True, want_JTJ=True, want_reason=True, **fit_kw):
    """pk_fit_protein_rows_batch on the context's library handle, as batch.fit_rows_native calls it, with NULL for the outputs not wanted."""
    import torch
    from phoskintime_amd import _capi
    ctx = eng.get_context()
    dev = torch.device("cuda", ctx.device)
    d = lambda x: eng._dev_f64(x, dev)
    R, P, Nr = pb["R"], pb["P"], pb["Nr"]
    ins = dict(P0=d(pb["P0"]), y0=d(pb["y0"]), t=d(pb["t"]), target=d(pb["target"]), sigma=d(pb["sigma"]), lam=d(pb["lam"]), lb=d(pb["lb"]), ub=d(pb["ub"]))
    out = dict(p=torch.empty((R, P), dtype=torch.float64, device=dev), cost=torch.empty((R,), dtype=torch.float64, device=dev),
               r=torch.empty((R, Nr), dtype=torch.float64, device=dev) if want_r else None,
               JTJ=torch.zeros((R, P, P), dtype=torch.float64, device=dev) if want_JTJ else None,
               reason=torch.zeros((R,), dtype=torch.int32, device=dev) if want_reason else None)
    opts = _capi.default_opts(kernel="group")
    fopts = _capi.default_fit_opts(log_space=int(pb["log_space"]), use_reg=int(pb["ridge"]), **fit_kw)
    cnt = (C.c_int64 * 6)()
    ptr = eng._ptr
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ctx.check(ctx.lib.pk_fit_protein_rows_batch(ctx.handle, pm.MODEL_IDS[pb["model"]], pb["n"], R, ptr(ins["P0"]), ptr(ins["y0"]), int(pb["y0"].ndim == 2),
                                                ptr(ins["t"]), pb["t"].size, ptr(ins["target"]), int(pb["target"].ndim == 2), ptr(ins["sigma"]),
                                                int(pb["sigma"].ndim == 2), ptr(ins["lam"]), ptr(ins["lb"]), ptr(ins["ub"]), int(pb["lb"].ndim == 2),
                                                C.byref(opts), C.byref(fopts), ptr(out["p"]), ptr(out["cost"]), ptr(out["r"]), ptr(out["JTJ"]),
                                                ptr(out["reason"]), C.byref(cnt)))
    ctx.synchronize()
    res = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    res["counters"] = [int(v) for v in cnt]
    return res


def test_optional_outputs_through_the_c_abi(eng, ms):
    """r = NULL, JTJ = NULL, reason = NULL, each alone and all together (distmod n = 3, ridge rows, per-row sigma, 6 rows, max_iter = 6):
    p, cost, the counters and the outputs that remain are bit-equal to the all-outputs call, which is bit-equal to fit_rows_native's; the
    context's workspace_stats() is unchanged and a following ordinary fit reproduces its earlier bits."""
    pb = _shared(eng, "distmod", 3, 6, 61, ridge=True, sigma="rows")
    kw = dict(max_iter=6, trial_levels=3)
    before = _fit(ms, pb, **kw)
    stats = eng.get_context().workspace_stats()
    full = _raw_fit(eng, pb, **kw)
    for f in FIELDS:
        assert np.array_equal(full[f], getattr(before, f)), f
    assert full["counters"] == list(before.counters.values()) and before.counters["trial_rounds"] >= 6
    for drop in (("r",), ("JTJ",), ("reason",), ("r", "JTJ", "reason")):
        got = _raw_fit(eng, pb, **{f"want_{f}": False for f in drop}, **kw)
        for f in FIELDS:
            if f in drop:
                assert got[f] is None
            else:
                assert np.array_equal(got[f], full[f]), (drop, f)
        assert got["counters"] == full["counters"], drop
    assert eng.get_context().workspace_stats() == stats
    after = _fit(ms, pb, **kw)
    assert _same_bits(after, before) == [] and after.counters == before.counters


# ------------------------------------------------------------------------------------------------------------------ (f) stationarity

def _projected_gradient(p, y0, n, t, target, lb, ub):
    """|P(g)| with g = J^T (flat - target) from the oracle's exact derivative (pm.sens_exact_lti, pm.flat_and_jacobian), the components that
    point out of an active bound dropped."""
    sol, dsol = pm.sens_exact_lti(0, p, y0, n, t)
    flat, dflat = pm.flat_and_jacobian(0, sol, dsol, y0, n)
    g = dflat.T @ (flat - target)
    keep = ~(((p <= lb) & (g > 0)) | ((p >= ub) & (g < 0)))
    return float(np.linalg.norm(g[keep]))


def test_stationarity_at_convergence(eng, ms):
    """The setting of test_convergence_in_data_space (distmod n = 4, 12 rows, noise-free target, max_iter = 200): for the rows the native fit
    ends for ftol / xtol or the gradient, the projected gradient of the cost at the returned p, formed from the oracle's exact derivative and
    never from the library's own g, against the same quantity at the Python driver's result for the same row.
    Measured on MI355X: all 12 rows end with reason 0 or 1 (ten and two); the figure is 3.409e-10 for every row of BOTH drivers (at the
    starts it is 0.53 .. 11.9): at the common minimum it is what the integrator's error in the target leaves of J^T (flat_exact - target),
    not a distance from stationarity.  Margin: the native figure may be at most twice the Python figure of the same row -- room for last
    iterates that differ below the integrator's error, none for a row that stops early (nine orders above)."""
    model, n = "distmod", 4
    S, P = pm.n_states(0, n), pm.n_params(0, n)
    rng = np.random.default_rng(11)
    truth = rng.uniform(0.5, 1.5, size=P)
    y0 = np.ones(S); t = pm.TIME_POINTS
    target = eng.solve_ode_batch(model, truth[None], y0, n, t, want_sol=False, kernel="group").flat.cpu().numpy()[0]
    P0 = truth * rng.uniform(0.7, 1.4, size=(12, P))
    lb, ub = np.full(P, 1e-3), np.full(P, 10.0)
    kw = dict(bounds=(lb, ub), max_iter=200, kernel="group")
    nat = ms.fit_rows_batch(model, n, t, P0, y0, target, driver="native", **kw)
    py = ms.fit_rows_batch(model, n, t, P0, y0, target, jacobian="sens", **kw)
    rows = np.where(np.isin(nat.reason, (0, 1)))[0]
    assert rows.size >= 6
    g_nat = np.array([_projected_gradient(nat.p[k], y0, n, t, target, lb, ub) for k in rows])
    g_py = np.array([_projected_gradient(py.p[k], y0, n, t, target, lb, ub) for k in rows])
    g_0 = np.array([_projected_gradient(np.clip(P0[k], lb, ub), y0, n, t, target, lb, ub) for k in rows])
    print(f"[f] rows {rows} reasons {nat.reason}\n    |Pg| native {np.array2string(g_nat, precision=3)}\n    |Pg| python {np.array2string(g_py, precision=3)}\n"
          f"    |Pg| start  {np.array2string(g_0, precision=3)}\n    max native {g_nat.max():.3e}  max python {g_py.max():.3e}  max native / python {np.max(g_nat / g_py):.3e}", flush=True)
    assert np.all(g_nat <= 2.0 * g_py)
