"""GPU: the bounded Levenberg-Marquardt polish of network candidates on the device (``NetworkEngine.fit_batch`` ->
``pk_network_fit_batch``, csrc/pk_net_fit.hip) on the four ``network_m*_small`` fixtures (S = 20 .. 32), loss data, ``cols`` (K = 8) and
``defaults`` of tests/net_objgrad_reference.py::fixture_data, rtol = 1e-8 / atol = 1e-10, B = 3 .. 6 -- and one call at ``netlarge_m0``.
Physical candidates unless stated; obj_w = (1, 0.6, 1.7), lambdas = (1, 0.5, 2, 0.7).

Operation counts behind the rounding bounds (u = 2^-53; ``norm_m`` is taken as the library forms it, a sequential sum, and is data):
    scale_i  = sqrt(((obj_w norm) lambda) w_i)                three products, one root                  4 u
    Jw_ik    = scale_i dpred_ik                                                                         5 u
    r_i      = scale_i (pred_i - obs_i)                       the difference, the product               6 u
    A_kl     = sum_i Jw_ik Jw_il                              two entries (10 u), their product, n_obs terms in sequence
               + d_k^2 on the diagonal, d = sqrt(sum obj_w lambda_prior / (5 N)) / (d_c + 1e-6) [softplus']: <= 10 u, squared 21 u
                                                              -> (n_obs + 1 + OPS_A) u sum |products|,  OPS_A = 22
    g_k      = sum_i Jw_ik r_i + d_k rp_k                     5 + 6 + 1 per term; the prior term 10 + 12 + 1 -> OPS_G = 24
    1/2 sum_m obj_w[m] dF[m, k]                               og.OPS["dF"] per term of dsums, three products and two sums more
                                                              -> (n_obs + OPS_G + og.OPS["dF"] + 5) u sum |products| between the two
The step: x after one iteration equals the reference's trial point of the level ``pick`` chooses within K cond 2^-52 |step| (cond of the
reference's damped matrix M: the figure tests/test_gpu_fit_native_exact.py derives for the protein fit) plus |M^-1| |bound of g|, because
the reference is fed the device's JTJ but the host twin's g (the entry point does not return g).

Measured on an MI355X: see DESIGN 5.13."""
import numpy as np
import pytest

import lm_reference as lmr
import net_objgrad_reference as og
import net_sens_reference as ref

pytestmark = pytest.mark.gpu
RTOL, ATOL = ref.RTOL_GPU, ref.ATOL_GPU
OPT = dict(rtol=RTOL, atol=ATOL)
LAM = og.LAM
OBJ_W = (1.0, 0.6, 1.7)
U = 2.0 ** -53
LD = np.longdouble
OPS_A, OPS_G = 22, 24
TWIN = 1e-5                         # tests/test_gpu_fit_native.py: native against the host twin
_CACHE = {}


def _setup(name):
    if name not in _CACHE:
        from phoskintime_amd.global_model import NetworkEngine
        s = dict(og.fixture_data(name))
        s["eng"] = eng = NetworkEngine.from_npz(s["g"])
        s["cols"] = s["gold"]["cols"].astype(np.int32)
        s["t"], s["y0"] = s["g"]["t_eval"], s["g"]["y0"]
        s["loss"] = eng.make_loss(s["ld"], s["t"].size)
        s["n_obs"] = sum(s["ld"][k].size for k in ("w_prot", "w_rna", "w_pho"))
        _CACHE[name] = s
    return _CACHE[name]


def _starts(s, B, cols=None, seed=0, lo=0.8, hi=1.25):
    """B start candidates: the fixture's three (cycled) with the fitted entries scaled by U(lo, hi); a box 0.25 .. 4 x the fixture's
    entries, per row, which cuts the first fitted entry of row 0 (its start lies outside: clip(x0) != x0)."""
    cols = s["cols"] if cols is None else cols
    rng = np.random.default_rng([seed, B, len(cols)])
    X = s["X"][np.arange(B) % s["X"].shape[0]].copy()
    base = X[:, cols].copy()
    X[:, cols] = base * rng.uniform(lo, hi, size=base.shape)
    lb, ub = 0.25 * base, 4.0 * base
    X[0, cols[0]] = 5.0 * base[0, 0]
    return X, lb, ub


def _np(t):
    return None if t is None else t.cpu().numpy()


def _fit(s, x0, lb, ub, cols=None, loss=None, **kw):
    kw = dict(dict(OPT, obj_w=OBJ_W, defaults=s["defaults"], lambdas=LAM, y0=s["y0"]), **kw)
    x, cost, F, JTJ, reason, status, counters = s["eng"].fit_batch(s["loss"] if loss is None else loss, x0, s["t"], s["cols"] if cols is None else cols,
                                                                  lb=lb, ub=ub, **kw)
    return dict(x=_np(x), cost=_np(cost), F=_np(F), JTJ=_np(JTJ), reason=_np(reason), status=_np(status), counters=counters)


def _twin(s, x0, lb, ub, cols=None, loss=None, ld=None, **kw):
    from phoskintime_amd.global_model import polish
    kw = dict(dict(OPT, obj_w=OBJ_W, defaults=s["defaults"], lambdas=LAM, y0=s["y0"]), **kw)
    return polish.polish_batch(s["eng"], s["loss"] if loss is None else loss, s["ld"] if ld is None else ld, x0, s["t"],
                               s["cols"] if cols is None else cols, lb=lb, ub=ub, driver="python", **kw)


def _plain(s, X, loss=None, kernel="lds", **kw):
    out = s["eng"].simulate_objective_batch(s["loss"] if loss is None else loss, X, s["t"], y0=s["y0"], defaults=s["defaults"], lambdas=LAM,
                                            method="rosw", kernel=kernel, **dict(OPT, **kw))
    assert out is not None
    return out[1].cpu().numpy(), out[2].cpu().numpy()


def _tangent(s, X, cols=None, loss=None, raw=False, **kw):
    out = s["eng"].simulate_objective_grad_batch(s["loss"] if loss is None else loss, X, s["t"], s["cols"] if cols is None else cols, y0=s["y0"],
                                                 defaults=s["defaults"], lambdas=LAM, want_pred=True, raw=raw, **dict(OPT, **kw))
    assert out is not None
    return {k: v.cpu().numpy() for k, v in out.items()}


def _clip(x0, cols, lb, ub):
    x = x0.copy()
    x[:, cols] = np.minimum(np.maximum(x[:, cols], lb), ub)
    return x


def _reference_normal(s, tg, k, xrow, cols, ld=None, raw=False):
    """Long-double A, g with the sums of magnitudes, from row k of a tangent launch."""
    from phoskintime_amd.global_model import polish
    ld = s["ld"] if ld is None else ld
    scl, obs = polish.residual_rows(ld, OBJ_W, LAM)
    Jw = lmr.weighted_jacobian(tg["dpred"][k], None, scl, False)
    r = LD(scl) * (LD(tg["pred"][k]) - LD(obs))
    A, g, absA, absg = lmr.normal_equations(Jw, r, None, 0.0, None, False)
    eng = s["eng"]
    pr, pd = polish.prior_rows(xrow[cols], cols, s["defaults"], OBJ_W, LAM[3], (eng.n_K, eng.N, eng.total_sites), raw)
    A = A + np.diag(LD(pd) * LD(pd)); absA = absA + np.diag(LD(pd) * LD(pd))
    g = g + LD(pd) * LD(pr); absg = absg + np.abs(LD(pd) * LD(pr))
    return A, g, absA, absg


def _check_normal(s, fit, tg, xc, cols, what):
    n_obs, worst = tg["pred"].shape[1], 0.0
    assert np.array_equal(fit["JTJ"], fit["JTJ"].transpose(0, 2, 1))
    for k in range(xc.shape[0]):
        A, _, absA, _ = _reference_normal(s, tg, k, xc[k], cols)
        bound = (n_obs + 1 + OPS_A) * U * absA.astype(float)
        err = np.abs(LD(fit["JTJ"][k]) - A).astype(float)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(np.diag(fit["JTJ"][k]) > 0.0)
    print(f"[{what}] K {len(cols)} n_obs {n_obs}: max |JTJ - ref| / bound {worst:.3e}", flush=True)
    assert worst <= 1.0


@pytest.mark.parametrize("name", ref.NAMES)
def test_normal_equations_gradient_and_first_iterate(name):
    """Checks 1, 3 and 4 of one max_iter = 1 call (B = 3, K = 8): JTJ against the long-double normal equations of a separate tangent
    launch at clip(x0); the twin's g against 1/2 sum_m obj_w[m] dF[b, m, :] of that launch; x, cost and reason against
    lm_reference.one_iteration + pick fed the device's JTJ, that g, and trial costs from plain launches at the reference's trial points."""
    from phoskintime_amd.global_model import polish
    s = _setup(name)
    cols, n_obs = s["cols"], s["n_obs"]
    x0, lb, ub = _starts(s, 3)
    xc = _clip(x0, cols, lb, ub)
    assert not np.array_equal(xc, x0)
    fit = _fit(s, x0, lb, ub, max_iter=1)
    tg = _tangent(s, xc)
    assert not tg["status"].any()
    _check_normal(s, fit, tg, xc, cols, name)                                                               # 1
    tw = _twin(s, x0, lb, ub, max_iter=1, want_g=True)
    F0, _ = _plain(s, xc)
    cost0 = polish.cost_of(F0, OBJ_W)
    worst_g = worst_x = 0.0
    for k in range(3):
        A, g, absA, absg = _reference_normal(s, tg, k, xc[k], cols)
        half = 0.5 * np.sum(np.asarray(OBJ_W)[:, None] * tg["dF"][k], axis=0)
        gb = (n_obs + OPS_G + og.OPS["dF"] + 5) * U * absg.astype(float)
        worst_g = max(worst_g, float(np.max(np.abs(tw.g[k] - half) / gb)), float(np.max(np.abs(LD(tw.g[k]) - g).astype(float) / gb)))      # 3
        it = lmr.one_iteration(fit["JTJ"][k], tw.g[k], xc[k, cols], lb[k], ub[k], mu=1e-3, levels=12, cost=cost0[k])                       # 4
        assert not it["done"]
        Xt = np.repeat(xc[k][None], 12, axis=0)
        Xt[:, cols] = it["trial"].astype(float)
        Ft, stt = _plain(s, Xt)
        assert not stt.any()
        cn = polish.cost_of(Ft, OBJ_W)
        L, margins = lmr.pick(cost0[k], cn, it["pred"])
        assert L >= 0 and not any(abs(m[0]) < 1e-6 or abs(m[1]) < 1e-9 for m in margins), (k, margins)
        free = it["free"]
        M = np.where(free[:, None] & free[None, :], fit["JTJ"][k], 0.0)
        M[np.arange(8), np.arange(8)] = np.where(free, np.diag(fit["JTJ"][k]) + 1e-3 * 4.0 ** L * it["DD"].astype(float) ** 2, 1.0)
        step = float(np.linalg.norm(it["step"][L].astype(float)))
        tol = 8 * it["cond"][L] * 2.0 * U * step + float(np.linalg.norm(np.linalg.inv(M), 2)) * float(np.linalg.norm(gb))
        err = float(np.linalg.norm(fit["x"][k, cols] - it["trial"][L].astype(float)))
        worst_x = max(worst_x, err / tol)
        dx, xn = float(np.linalg.norm(it["dp"][L].astype(float))), float(np.linalg.norm(it["trial"][L].astype(float)))
        conv = (cost0[k] - cn[L]) <= 1e-10 * max(cn[L], 1e-300) or dx <= 1e-10 * (1e-10 + xn)
        assert fit["reason"][k] == (0 if conv else 3) and fit["cost"][k] < cost0[k]
        assert np.all(fit["x"][k, cols] >= lb[k]) and np.all(fit["x"][k, cols] <= ub[k])
    print(f"[{name}] max |g - 1/2 obj_w dF| / bound {worst_g:.3e}   max |x - trial_ref| / tol {worst_x:.3e}", flush=True)
    assert worst_g <= 1.0 and worst_x <= 1.0
    assert fit["counters"]["jacobian_phases"] == 1 and fit["counters"]["iterations"] == 1
    # the twin took the same step
    assert np.array_equal(tw.reason, fit["reason"]) and tw.counters == fit["counters"]
    np.testing.assert_allclose(tw.x, fit["x"], rtol=TWIN, atol=1e-7)


def test_normal_equations_wider_K():
    """Check 2: K = 23, the smallest K whose triangle K (K + 1) / 2 = 276 passes the 256 threads of the kernel (a thread then owns more than
    one entry and the entry map crosses columns inside a wave); n_obs = 270 = 8 tiles of 32 rows + 14."""
    s = _setup("network_m0_small")
    K = 23
    assert (K - 1) * K // 2 <= 256 < K * (K + 1) // 2 and K <= s["eng"].n_var and s["n_obs"] % 32 != 0
    cols = np.concatenate([s["cols"], np.setdiff1d(np.arange(s["eng"].n_var), s["cols"])[: K - 8]]).astype(np.int32)
    x0, lb, ub = _starts(s, 3, cols=cols, seed=2)
    xc = _clip(x0, cols, lb, ub)
    fit = _fit(s, x0, lb, ub, cols=cols, max_iter=1)
    tg = _tangent(s, xc, cols=cols)
    assert not tg["status"].any()
    _check_normal(s, fit, tg, xc, cols, "wider K")


@pytest.mark.parametrize("name", ref.NAMES)
def test_whole_fit_against_the_twin(name):
    """Check 5: both drivers take the same accept / reject sequence (the six counters and the reasons are equal) and agree in x and cost."""
    s = _setup(name)
    x0, lb, ub = _starts(s, 4, seed=1)
    fit = _fit(s, x0, lb, ub, max_iter=4)
    tw = _twin(s, x0, lb, ub, max_iter=4)
    print(f"[{name}] counters native {fit['counters']}  twin {tw.counters}  reasons {fit['reason']} {tw.reason}\n   cost {fit['cost']}\n   twin {tw.cost}", flush=True)
    assert fit["counters"] == tw.counters and np.array_equal(fit["reason"], tw.reason)
    np.testing.assert_allclose(fit["cost"], tw.cost, rtol=TWIN)
    np.testing.assert_allclose(fit["x"], tw.x, rtol=TWIN, atol=1e-7)
    assert np.all(fit["cost"] < _fit(s, x0, lb, ub, max_iter=0)["cost"])                       # every row went down


@pytest.mark.parametrize("name", ref.NAMES)
def test_exact_claims(name):
    """Check 6, bit for bit: F is the plain order-3 fused objective at the returned x and cost its scalarisation; a row alone equals its
    row in the batch, also with trial_levels 1 against 3; max_iter = 0; optional outputs."""
    from phoskintime_amd.global_model import polish
    s = _setup(name)
    cols = s["cols"]
    x0, lb, ub = _starts(s, 4, seed=3)
    fit = _fit(s, x0, lb, ub, max_iter=2, trial_levels=3)
    Fp, stp = _plain(s, fit["x"])
    assert np.array_equal(fit["F"], Fp) and not stp.any() and np.array_equal(fit["cost"], polish.cost_of(Fp, OBJ_W))
    held = np.setdiff1d(np.arange(s["eng"].n_var), cols)
    assert np.array_equal(fit["x"][:, held], x0[:, held])
    for k in (3,):
        alone = _fit(s, x0[k:k + 1], lb[k:k + 1], ub[k:k + 1], max_iter=2, trial_levels=1)
        for key in ("x", "cost", "F", "JTJ", "reason", "status"):
            assert np.array_equal(alone[key][0], fit[key][k]), (key, k)
    zero = _fit(s, x0, lb, ub, max_iter=0)
    xc = _clip(x0, cols, lb, ub)
    F0, _ = _plain(s, xc)
    assert np.array_equal(zero["x"], xc) and np.array_equal(zero["F"], F0) and (zero["reason"] == 3).all() and not zero["JTJ"].any()
    assert zero["counters"] == dict(iterations=0, simulated=4, launches=3, host_waits=0, jacobian_phases=0, trial_rounds=0)
    bare = _fit(s, x0, lb, ub, max_iter=2, trial_levels=3, want_JTJ=False, want_reason=False, want_status=False)
    assert bare["JTJ"] is None and bare["reason"] is None and bare["status"] is None
    for key in ("x", "cost", "F"):
        assert np.array_equal(bare[key], fit[key]), key
    assert bare["counters"] == fit["counters"]


def test_box_rows_end_on_bounds():
    """Check 7a.  Per-row bounds as tests/test_gpu_fit_native_exact.py::_per_row draws them (lb = c U(0.4, 1.05), ub = lb + c U(0.1, 1) around
    the fixture's entries c): entries end exactly on a bound, everything lies inside, and the twin ends on the same bounds."""
    s = _setup("network_m1_small")
    cols = s["cols"]
    rng = np.random.default_rng(17)
    B = 6
    X = s["X"][np.arange(B) % 3].copy()
    base = X[:, cols].copy()
    lb = base * rng.uniform(0.4, 1.05, size=base.shape)
    ub = lb + base * rng.uniform(0.1, 1.0, size=base.shape)
    X[:, cols] = base * rng.uniform(0.2, 4.0, size=base.shape)
    fit = _fit(s, X, lb, ub, max_iter=5)
    z = fit["x"][:, cols]
    on = (z == lb) | (z == ub)
    print(f"[box] entries on a bound per row {on.sum(axis=1)}  reasons {fit['reason']}", flush=True)
    assert np.all(z >= lb) and np.all(z <= ub) and on.sum() >= 3 and (on.sum(axis=1) > 0).sum() >= 2
    tw = _twin(s, X, lb, ub, max_iter=5)
    assert np.array_equal((tw.x[:, cols] == lb) | (tw.x[:, cols] == ub), on)
    np.testing.assert_allclose(fit["cost"], tw.cost, rtol=TWIN)
    np.testing.assert_allclose(fit["x"], tw.x, rtol=TWIN, atol=1e-7)


def _noise_free():
    """network_m0_small with the device's own pred at the truth candidate (the fixture's first) as observations, B = 3 starts -- the
    truth with the K columns scaled by factors in [0.7, 1.4] -- and the native fit from them inside 0.2 .. 5 x the truth; made once."""
    if "noise_free" not in _CACHE:
        s = _setup("network_m0_small")
        eng, cols = s["eng"], s["cols"]
        truth = s["X"][0]
        pred = _tangent(s, truth[None])["pred"][0]
        n = [s["ld"][k].size for k in ("w_prot", "w_rna", "w_pho")]
        ld = dict(s["ld"], obs_prot=pred[:n[0]], obs_rna=pred[n[0]:n[0] + n[1]], obs_pho=pred[n[0] + n[1]:])
        loss = eng.make_loss(ld, s["t"].size)
        x0 = np.repeat(truth[None], 3, axis=0)
        x0[:, cols] *= np.random.default_rng(23).uniform(0.7, 1.4, size=(3, cols.size))
        lb, ub = 0.2 * truth[cols], 5.0 * truth[cols]
        _CACHE["noise_free"] = dict(ld=ld, loss=loss, x0=x0, lb=lb, ub=ub, fit=_fit(s, x0, lb, ub, loss=loss, max_iter=25))
    return _CACHE["noise_free"]


def test_raw_agrees_with_physical():
    """Check 7b: the fit on raw entries from the same starts, the box inactive (the physical fit ends strictly inside its own), reaches
    the physical fit's minimum in physical space within the twin tolerance.  On the noise-free problem both converge (reason 0 or 1)."""
    from phoskintime_amd.global_model import polish
    s, q = _setup("network_m0_small"), _noise_free()
    cols, phys = s["cols"], q["fit"]
    z = phys["x"][:, cols]
    assert np.all(z > q["lb"]) and np.all(z < q["ub"]) and np.all(phys["reason"] <= 1)
    raw = _fit(s, np.log(np.expm1(q["x0"])), None, None, loss=q["loss"], max_iter=25, raw=True)
    print(f"[raw] reasons phys {phys['reason']} raw {raw['reason']}  cost {phys['cost']} {raw['cost']}  iterations {phys['counters']['iterations']} "
          f"{raw['counters']['iterations']}", flush=True)
    assert np.all(raw["reason"] <= 1)
    np.testing.assert_allclose(raw["cost"], phys["cost"], rtol=TWIN)
    np.testing.assert_allclose(polish.softplus(raw["x"]), phys["x"], rtol=TWIN, atol=1e-7)


@pytest.mark.parametrize("k", range(3))
def test_quality_against_scipy_trf(k):
    """Check 8, one row per case, every row of the batch a case.  Observations: the device's own pred at a truth candidate, noise-free;
    starts: the truth with the K columns scaled by factors in [0.7, 1.4]; the row must reach cost_native <= 1.02 cost_scipy + floor against
    scipy.optimize.least_squares(method="trf", bounds=...) fed residual and Jacobian by single-row tangent launches.  cost_scipy is
    1/2 obj_w . F of the tangent launch at scipy's point (the residual it minimised plus the constant prior of the held entries); floor is
    |1/2 obj_w . (F_plain - F_tangent)| at the native point."""
    from scipy.optimize import least_squares
    from phoskintime_amd.global_model import polish
    s, q = _setup("network_m0_small"), _noise_free()
    eng, cols, fit, x0, loss = s["eng"], s["cols"], q["fit"], q["x0"], q["loss"]
    scl, obs = polish.residual_rows(q["ld"], OBJ_W, LAM)
    shape = (eng.n_K, eng.N, eng.total_sites)
    memo = {}

    def both(z):
        key = z.tobytes()
        if key not in memo:
            x = x0[k].copy(); x[cols] = z
            tg = _tangent(s, x[None], loss=loss)
            pr, pd = polish.prior_rows(z, cols, s["defaults"], OBJ_W, LAM[3], shape, False)
            memo[key] = (np.concatenate([scl * (tg["pred"][0] - obs), pr]), np.vstack([scl[:, None] * tg["dpred"][0], np.diag(pd)]), tg["F"][0])
        return memo[key]

    sol = least_squares(lambda z: both(z)[0], x0[k, cols], jac=lambda z: both(z)[1], bounds=(q["lb"], q["ub"]), method="trf", xtol=1e-10, ftol=1e-10, gtol=1e-10)
    assert sol.success, sol.message
    cost_scipy = float(polish.cost_of(both(sol.x)[2], OBJ_W))
    floor = abs(float(polish.cost_of(both(np.ascontiguousarray(fit["x"][k, cols]))[2], OBJ_W)) - fit["cost"][k])
    print(f"[scipy row {k}] native {fit['cost'][k]:.9e} (reason {fit['reason'][k]}, {fit['counters']['iterations']} iterations)  scipy {cost_scipy:.9e} "
          f"({sol.nfev} evaluations)  floor {floor:.2e}", flush=True)
    assert fit["cost"][k] <= 1.02 * cost_scipy + floor


def test_hbm_route_agrees_with_lds():
    """Check 9a: the same fit with state and tangents on HBM slabs; its F is the workspace kernel's fused objective bit for bit."""
    s = _setup("network_m2_small")
    x0, lb, ub = _starts(s, 3, seed=5)
    lds = _fit(s, x0, lb, ub, max_iter=3)
    hbm = _fit(s, x0, lb, ub, max_iter=3, kernel="hbm")
    np.testing.assert_allclose(hbm["cost"], lds["cost"], rtol=TWIN)
    np.testing.assert_allclose(hbm["x"], lds["x"], rtol=TWIN, atol=1e-7)
    assert np.array_equal(hbm["reason"], lds["reason"])
    Fw, _ = _plain(s, hbm["x"], kernel="workspace")
    assert np.array_equal(hbm["F"], Fw)


def test_netlarge_one_iteration():
    """Check 9b: netlarge_m0 (N = 100, S = 552), B = 2, K = 4 -- two column chunks at KC = 3 --, max_iter = 1: the normal equations of
    check 1 and the exact claims of check 6."""
    from phoskintime_amd.global_model import NetworkEngine, polish
    from oracle import network_models as nm
    g = np.load(ref.GOLDEN / "netlarge_m0.npz")
    eng = NetworkEngine.from_npz(g)
    net = nm.Network.from_npz(g)
    assert eng.objective_grad_columns_per_launch() == 3
    X = np.stack([eng.pack_params(*(g[k][b] for k in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale"))) for b in range(2)])
    t = g["t_eval"]
    ld = og.loss_data(net, t)
    sl = ref.slices(net)
    cols = np.array([sl["c_k"][0] + 1, sl["A_i"][0] + 99, sl["Dp_i"][0] + 351, sl["tf_scale"][0]], dtype=np.int32)
    loss = eng.make_loss(ld, t.size)
    s = dict(eng=eng, loss=loss, X=X, t=t, cols=cols, y0=g["y0"], defaults=X[0] * 1.1, ld=ld,
             n_obs=sum(ld[k].size for k in ("w_prot", "w_rna", "w_pho")))
    x0, lb, ub = _starts(s, 2, seed=6)
    xc = _clip(x0, cols, lb, ub)
    fit = _fit(s, x0, lb, ub, max_iter=1)
    tg = _tangent(s, xc)
    assert not tg["status"].any() and not fit["status"].any()
    _check_normal(s, fit, tg, xc, cols, "netlarge_m0")
    Fp, _ = _plain(s, fit["x"])
    assert np.array_equal(fit["F"], Fp) and np.array_equal(fit["cost"], polish.cost_of(Fp, OBJ_W))
    alone = _fit(s, x0[1:], lb[1:], ub[1:], max_iter=1)
    for key in ("x", "cost", "F", "JTJ", "reason"):
        assert np.array_equal(alone[key][0], fit[key][1]), key
    assert np.all(fit["cost"] < polish.cost_of(_plain(s, xc)[0], OBJ_W))
    eng.free_loss(loss); eng.close()


def test_a_flagged_jacobian_launch_stops_its_row():
    """Check 10.  One candidate's held B entries are scaled by 1000: its tangent launch needs 1.9 x the steps of the slowest other row
    (measured: 14 885 against 7 811), and ``max_steps`` = 1.3 x that row's count lies between them -- the solver's own step budget flags the
    candidate (PK_ST_MAXSTEPS; nothing faults): reason 4 at clip(x0), status non-zero; the other rows are bit-equal to the batch without it.
    One iteration: the one Jacobian phase runs at clip(x0), where the step counts were read."""
    s = _setup("network_m0_small")
    cols = s["cols"]
    x0, lb, ub = _starts(s, 4, seed=7)
    x0[0, cols[0]] = s["X"][0, cols[0]]
    sl = ref.slices(s["net"])
    stiff = 2
    held = np.setdiff1d(np.arange(*sl["B_i"]), cols)
    x0[stiff, held] *= 1000.0
    xc = _clip(x0, cols, lb, ub)
    steps = _tangent(s, xc)["n_steps"].sum(axis=1)
    others = np.delete(np.arange(4), stiff)
    print(f"[flag] steps of the tangent launch per row {steps}", flush=True)
    assert steps[stiff] > 1.6 * steps[others].max()
    budget = int(1.3 * steps[others].max())
    fit = _fit(s, x0, lb, ub, max_iter=1, max_steps=budget)
    assert fit["reason"][stiff] == 4 and fit["status"][stiff] != 0 and np.array_equal(fit["x"][stiff], xc[stiff])
    assert (fit["reason"][others] != 4).all() and not fit["status"][others].any()
    rest = _fit(s, x0[others], lb[others], ub[others], max_iter=1, max_steps=budget)
    for key in ("x", "cost", "F", "JTJ", "reason", "status"):
        assert np.array_equal(rest[key], fit[key][others]), key
