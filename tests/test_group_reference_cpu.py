"""CPU: tests/group_reference.py, the numpy restatement of the lane-group integrator, pinned before it judges the kernels
(tests/test_gpu_group_matrix.py): against the C restatement of the distmod throughput kernel, against the closed form, its two RODAS4
forms against each other, the order of every method, and its own rounding in double against long double.

Figures these tests print (pytest -s), as measured:
  * |y64 - yld|_inf / tau on the forced grids, worst over every size and the compared replicas: LRP12 2.76 (succmod n = 31), LRP8 2.63
    (distmod n = 6), RODAS4 resolvent 3.40 (succmod n = 7), RODAS4 stage form 2.63 (randmod n = 4), BDF1 / BDF2 5.79 (distmod n = 6),
    RK4 0.93 (succmod n = 62)
  * largest err on the forced grids over all 37 replicas of every size: LRP12 0.0127, LRP8 0.0179, RODAS4 0.0552 in both forms (all at
    distmod n = 62), BDF2 0.0026 (distmod n = 1); the condition is err <= 0.5
  * accepted / rejected steps with a single- against a double-precision root, largest difference over every size and the compared
    replicas: LRP12 1, LRP8 0, RODAS4 0 in both forms; BDF2 has no single-precision root
  * RODAS4 stage form against resolvent form as one step: 0.63 tau in long double (73.6 tau in double, at distmod n = 30, hs = 1, where
    each form in double is itself 26 to 37 tau from its long-double value: a whole step from y0, far from the steady state)
  * RK4 global error ratio 17.19, BDF2 4.00; LRP12 defect exponents 7.68, 9.51, 10.70, LRP8 7.05, 7.50, 7.74
"""
import numpy as np
import pytest

import group_reference as gr
from oracle import protein_models as pm

LD = np.longdouble
ALL_SIZES = [(model, n) for (model, G), ns in gr.SIZES.items() for n in ns]
#: |y64 - yld|_inf <= R64 tau: the double-precision restatement's own rounding, the figure the GPU file's condition (64 x) starts from.
#: Each of the NS solves is backward stable (row-pivoted LU) and the weighted sum adds one rounding per term, so on these grids, where
#: the rows sit near the steady state and cond(W) does not show, the difference is a few tau.  Measured at most 5.79 (module docstring);
#: 8 is the next power of two.  This pins the restatement's own rounding; it is not a tolerance on any kernel.
R64 = {("lrp12", "resolvent"): 8.0, ("lrp8", "resolvent"): 8.0, ("rodas4", "resolvent"): 8.0, ("rodas4", "stage"): 8.0,
       ("bdf2", "resolvent"): 8.0, ("rk4", "resolvent"): 8.0}


def test_lrp_free_run_agrees_with_the_c_restatement_of_the_throughput_kernel():
    """integrate against oracle/lrp8_dist.c (same method and controller, difference basis, arrow elimination) on distmod: the project's
    limits for two statements of one algorithm, band error 0.02 and accepted steps within 2."""
    from oracle import lrp8_cpu
    rng = np.random.default_rng(5)
    for n in (1, 6, 30):
        theta = rng.uniform(0.0, 20.0, (4, pm.n_params(pm.DIST, n)))
        y0 = rng.uniform(0.2, 2.0, n + 2)
        for method, kw, kw_c in (("lrp12", {}, {}), ("lrp8", dict(rtol=1e-7, atol=1e-9), dict(stages=8, rtol=1e-7, atol=1e-9))):
            sol_c, st_c, ns_c = lrp8_cpu.solve_batch(theta, n, y0, pm.TIME_POINTS, **kw_c)
            assert not st_c.any()
            for b in range(theta.shape[0]):
                sol, st, (acc, rej) = gr.integrate(method, "resolvent", pm.DIST, theta[b], n, y0, pm.TIME_POINTS, **kw)
                assert st == 0
                assert pm.band_error(sol, sol_c[b]) <= 0.02, (n, method, b)
                assert abs(acc - ns_c[b, 0]) <= 2 and abs(rej - ns_c[b, 1]) <= 2, (n, method, b, acc, rej, ns_c[b])


@pytest.mark.parametrize("model,n", [(pm.DIST, 7), (pm.SUCC, 6), (pm.RAND, 3)])
def test_free_run_within_the_band_of_the_closed_form(model, n):
    """Every method at the tolerances and limits tests/test_gpu_parity.py applies to it; RK4 at h = 2e-3 on benign rates, inside the band."""
    theta, y0 = gr.case(model, n)
    for (method, form), (kw, limit) in gr.FREE.items():
        for b in (0, 18):
            sol, st, _ = gr.integrate(method, form, model, theta[b], n, y0[b], pm.TIME_POINTS, **kw)
            assert st == 0
            assert pm.band_error(sol, pm.solve_exact_lti(model, theta[b], y0[b], n, pm.TIME_POINTS)) <= limit, (method, form, b)
    th = np.random.default_rng(1).uniform(0.05, 2.0, pm.n_params(model, n))
    t = pm.TIME_POINTS[:6]
    sol, st, (acc, rej) = gr.integrate("rk4", "resolvent", model, th, n, y0[0], t, rk4_h=2e-3)
    assert st == 0 and (acc, rej) == (sum(gr.rk4_substeps(t, 2e-3)), 0)
    assert pm.band_error(sol, pm.solve_exact_lti(model, th, y0[0], n, t)) <= 1.0
    # the flags: a step budget that runs out, and a rate that is not a number
    sol, st, ns = gr.integrate("lrp12", "resolvent", model, theta[0], n, y0[0], pm.TIME_POINTS, max_steps=5)
    assert st == gr.ST_MAXSTEPS and sum(ns) == 5 and np.isnan(sol[-1]).all() and np.isfinite(sol[0]).all()


def test_rodas4_stage_form_equals_resolvent_form_as_one_step():
    """The models are affine, so the classical six stages and the resolvent weights are the same map.  In long double the two agree within
    one tau: what is left is the rounding of both tables to double (sum |RB_k z_k| 2^-53 is tau itself).  In double each form also
    carries its own rounding, which test_double_against_long_double_on_the_forced_grids bounds per form; the figure is printed."""
    worst = {float: 0.0, LD: 0.0}
    for model, n in ((pm.DIST, 1), (pm.DIST, 30), (pm.SUCC, 14), (pm.SUCC, 62), (pm.RAND, 3), (pm.RAND, 5)):
        theta, y0 = gr.case(model, n)
        for b in gr.COMPARED:
            sys = gr.system(model, theta[b], n)
            for hs in (0.02, 0.2, 1.0):
                for dtype in (float, LD):
                    a, ea, maj = gr.one_step("rodas4", "resolvent", model, theta[b], n, y0[b], hs, dtype=dtype, sys=sys)
                    s, es, _ = gr.one_step("rodas4", "stage", model, theta[b], n, y0[b], hs, dtype=dtype, sys=sys)
                    worst[dtype] = max(worst[dtype], float(np.max(np.abs(a - s))) / gr.tau(maj), float(np.max(np.abs(ea - es))) / gr.tau(maj))
    print(f"RODAS4 stage form against resolvent form, one step: {worst[float]:.2f} tau in double, {worst[LD]:.3f} tau in long double")
    assert worst[LD] <= 1.0


def test_order_of_every_method():
    """Global error of RK4 and BDF2 (constant step, BDF1 start-up) on halving h: ratios 16 and 4.  One-step defect of LRP12 and LRP8 against
    the exact flow: order p = 11 and 7, so the defect falls as h^(p+1)."""
    model, n = pm.DIST, 2
    th = np.array([1.2, 0.6, 0.9, 0.3, 1.5, 0.7, 0.4, 1.1])
    y0 = np.array([0.7, 1.3, 0.4, 1.1])
    sys = gr.system(model, th, n)
    exact = lambda tt: pm.solve_exact_lti(model, th, y0, n, np.array([0.0, tt]))[1]

    def march(method, steps, span):
        y, hist, h = y0.astype(LD), [], span / steps
        for _ in range(steps):
            yn = gr.one_step(method, "resolvent", model, th, n, y, h, history=hist, dtype=LD, sys=sys)[0]
            hist = [(y, h)] + hist[:1]
            y = yn
        return float(np.max(np.abs(y - exact(span))))

    r = march("rk4", 16, 1.0) / march("rk4", 32, 1.0)
    print(f"RK4 global error ratio on halving h: {r:.2f}")
    assert 14.0 <= r <= 18.0
    r = march("bdf2", 200, 1.0) / march("bdf2", 400, 1.0)
    print(f"BDF2 global error ratio on halving h: {r:.2f}")
    assert 3.6 <= r <= 4.4
    # a diagonal affine system, whose flow long double gives to 1e-19: the defect at |h lambda| <= 1 is far below double's reach
    lam, bias, y1 = np.array([-1.0, -0.25], dtype=LD), np.array([0.5, 0.0], dtype=LD), np.array([0.7, 1.3], dtype=LD)
    diag = (np.diag(lam.astype(float)), bias.astype(float))
    flow = lambda hh: np.exp(lam * LD(hh)) * y1 + np.expm1(lam * LD(hh)) / lam * bias
    # The weights are rounded to double, so the defect cannot be seen below tau, and |gamma h lambda| is not small above it: the exponent
    # between successive halvings rises towards p + 1 from below (LRP12: 7.7, 9.5, 10.7; LRP8: 7.0, 7.5, 7.7) and must not pass it
    for method, order, hs in (("lrp12", 11, (4.0, 2.0, 1.0, 0.5)), ("lrp8", 7, (1.0, 0.5, 0.25, 0.125))):
        d = [float(np.max(np.abs(gr.one_step(method, "resolvent", None, None, None, y1, hh, dtype=LD, sys=diag)[0] - flow(hh)))) for hh in hs]
        ex = [float(np.log2(d[i] / d[i + 1])) for i in range(3)]
        print(f"{method} one-step defect at h = {hs}: " + ", ".join("%.3e" % x for x in d) + "; exponents " + ", ".join("%.2f" % x for x in ex))
        assert ex[0] < ex[1] < ex[2] <= order + 1.1 and ex[2] >= order + 1 - 1.5


@pytest.fixture(scope="module")
def forced_runs():
    """integrate on the forced grid of every size, update and replica: {(model, n, method, form): (t, opts, [(sol, status, n_steps, max err)])}."""
    out = {}
    for model, n in ALL_SIZES:
        theta, y0 = gr.case(model, n)
        for method, form in gr.UPDATES:
            t, opts = gr.forced(method, model, theta, n)
            runs = []
            for b in range(gr.B):
                trace = []
                sol, st, ns = gr.integrate(method, form, model, theta[b], n, y0[b], t, trace=trace, **opts)
                runs.append((sol, st, ns, max((e for _, e in trace), default=0.0)))
            out[model, n, method, form] = (t, opts, runs)
    return out


def test_forced_grid_premise_one_step_per_interval_and_err_below_half(forced_runs):
    """A condition on the inputs of the GPU matrix, not a tolerance: on every size, update and replica the restatement accepts exactly one
    step per interval (RK4: the planned sub-steps) and its error estimate stays below 0.5, so no kernel close to it can reject a step."""
    worst = {}
    for (model, n, method, form), (t, opts, runs) in forced_runs.items():
        want = (sum(gr.rk4_substeps(t, opts["rk4_h"])) if method == "rk4" else t.size - 1, 0)
        if method == "rk4":
            assert 1 <= min(gr.rk4_substeps(t, opts["rk4_h"])) and max(gr.rk4_substeps(t, opts["rk4_h"])) == 3
        if method == "bdf2":
            assert (np.diff(t)[1:] / np.diff(t)[:-1]).max() < 2.0
        for b, (sol, st, ns, err) in enumerate(runs):
            assert st == 0 and ns == want and np.isfinite(sol).all(), (model, n, method, form, b, st, ns)
            if err > worst.get((method, form), (0.0,))[0]:
                worst[method, form] = (err, pm.MODEL_NAMES[model], n, b)
    for k, v in worst.items():
        print("forced grid, largest err:", k, "%.4f at %s n = %d replica %d" % v)
    assert max(v[0] for v in worst.values()) <= 0.5


def test_double_against_long_double_on_the_forced_grids(forced_runs):
    """one_step in double against long double, restarted from each row of the double run: the restatement's own rounding, in units of tau."""
    worst = {}
    for (model, n, method, form), (t, opts, runs) in forced_runs.items():
        theta, _ = gr.case(model, n)
        for b in gr.COMPARED:
            sys = gr.system(model, theta[b], n)
            sol = runs[b][0]
            for k in range(1, t.size):
                y64, t64 = gr.interval_reference(method, form, sys, sol, t, k, opts.get("rk4_h"), dtype=float)
                yld, tt = gr.interval_reference(method, form, sys, sol, t, k, opts.get("rk4_h"))
                assert abs(t64 - tt) <= 1e-6 * tt
                r = float(np.max(np.abs(y64 - yld))) / tt
                if r > worst.get((method, form), (0.0,))[0]:
                    worst[method, form] = (r, pm.MODEL_NAMES[model], n, b)
    for k, v in worst.items():
        print("double against long double:", k, "%.2f tau at %s n = %d replica %d" % v)
    for k, v in worst.items():
        assert v[0] <= R64[k], (k, v)


_KERNEL_RUNS = {}


def _kernel_forced_run(case):
    """integrate on the forced grid of one (model, n, batch, method) of gr.KERNEL_CASES, every replica: (t, [(sol, status, n_steps, max err)])."""
    if case not in _KERNEL_RUNS:
        model, n, batch, method = case
        theta, y0 = gr.case(model, n, batch)
        t, opts = gr.forced(method, model, theta, n)
        runs = []
        for b in range(batch):
            trace = []
            sol, st, ns = gr.integrate(method, "resolvent", model, theta[b], n, y0[b], t, trace=trace, **opts)
            runs.append((sol, st, ns, max(e for _, e in trace)))
        _KERNEL_RUNS[case] = (t, runs)
    return _KERNEL_RUNS[case]


_case_id = lambda c: "%s-n%d-B%d-%s" % (pm.MODEL_NAMES[c[0]], c[1], c[2], c[3])


def test_batch_argument_of_case_leaves_the_37_replica_draws_alone():
    for model, n in ((pm.RAND, 4), (pm.DIST, 62)):
        a, b = gr.case(model, n), gr.case(model, n, 37)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        rng = np.random.default_rng(20261020 + 1000 * model + n)                       # the draw as it was written before `batch` existed
        P = pm.n_params(model, n)
        np.testing.assert_array_equal(a[0][:18], rng.uniform(0.0, 20.0, (18, P)))
        np.testing.assert_array_equal(a[0][18:], np.exp(rng.uniform(np.log(1e-3), np.log(20.0), (19, P))))
        np.testing.assert_array_equal(a[1], rng.uniform(0.2, 2.0, (37, pm.n_states(model, n))))
    th, y0 = gr.case(pm.RAND, 7, 1024)
    assert th.shape == (1024, pm.n_params(pm.RAND, 7)) and y0.shape == (1024, 129) and gr.compared(1024) == (0, 512, 1023) and gr.compared() == gr.COMPARED


@pytest.mark.parametrize("case", gr.KERNEL_CASES, ids=_case_id)
def test_kernel_table_forced_grid_is_single_step_and_the_restatement_within_its_cap(case):
    """The inputs of tests/test_gpu_rand_matrix.py, on every replica of the batch: the restatement accepts exactly one step per interval,
    rejects none, and its error estimate stays below 0.5 (measured: at most 0.085, distmod n = 255; below 0.007 on randmod) -- so the GPU
    file's n_steps == (T - 1, 0) is never where this is first learned.  And the double restatement's own |y64 - yld| / tau on the compared
    replicas stays below the figure recorded in gr.KERNEL_R64, from which the GPU file's finding threshold L x R64 is defined, itself
    under the cap of 8 that R64 above argues for."""
    model, n, batch, method = case
    t, runs = _kernel_forced_run(case)
    for b, (sol, st, ns, err) in enumerate(runs):
        assert st == 0 and ns == (t.size - 1, 0) and np.isfinite(sol).all() and err <= 0.5, (case, b, st, ns, err)
    theta, _ = gr.case(model, n, batch)
    worst = 0.0
    for b in gr.compared(batch):
        sys = gr.system(model, theta[b], n)
        for k in range(1, t.size):
            y64, _ = gr.interval_reference(method, "resolvent", sys, runs[b][0], t, k, dtype=float)
            yld, tt = gr.interval_reference(method, "resolvent", sys, runs[b][0], t, k)
            worst = max(worst, float(np.max(np.abs(y64 - yld))) / tt)
    print("kernel table, forced grid:", _case_id(case), "largest err %.4f" % max(r[3] for r in runs), "double against long double %.3f tau" % worst)
    assert worst <= gr.KERNEL_R64[case] <= R64[method, "resolvent"], (case, worst)


def test_kernel_table_step_counts_do_not_hang_on_the_precision_of_the_root():
    """As test_step_counts_do_not_hang_on_the_precision_of_the_root, at the sizes of gr.KERNEL_CASES: the spread is within ROOT_SPREAD
    (measured: 1 accepted step of LRP12 at distmod n = 127, 0 everywhere else)."""
    spread = {m: 0 for m in gr.ROOT_SPREAD}
    for model, n, batch, method in gr.KERNEL_CASES:
        theta, y0 = gr.case(model, n, batch)
        kw = gr.FREE[method, "resolvent"][0]
        for b in gr.compared(batch):
            _, s32, n32 = gr.integrate(method, "resolvent", model, theta[b], n, y0[b], pm.TIME_POINTS, root=np.float32, **kw)
            _, s64, n64 = gr.integrate(method, "resolvent", model, theta[b], n, y0[b], pm.TIME_POINTS, root=np.float64, **kw)
            assert s32 == 0 and s64 == 0
            spread[method] = max(spread[method], abs(n32[0] - n64[0]), abs(n32[1] - n64[1]))
    print("kernel table, steps with a single- against a double-precision root, largest difference:", spread)
    assert all(spread[m] <= gr.ROOT_SPREAD[m] for m in spread), spread


def test_text_of_tpr_rand_kernel_1_in_correctly_rounded_double():
    """The finding of tests/test_gpu_rand_matrix.py: csrc/pk_tpr_rand.hpp at NB = 1, operation for operation (the 2 x 2 in-place Gauss-Jordan
    inverse, the mRNA row as a scalar, FMA dot products and FMA stage sums), each operation correctly rounded (exact rational arithmetic,
    rounded once; the kernel's refined reciprocal taken as 1 / x rounded), on the forced grid from the restatement's rows, against the
    long-double step.  Measured 1.11 tau where the restatement's LAPACK solve gives 0.59: the figure of this elimination order, recorded
    as gr.TPR1_TEXT_R64, from which the GPU file's condition for that kernel is defined."""
    from fractions import Fraction as F
    fma = lambda a, b, c: float(F(a) * F(b) + F(c))
    rcp = lambda x: float(1 / F(x))
    model, n = pm.RAND, 1
    theta, y0 = gr.case(model, n)
    t, opts = gr.forced("lrp12", model, theta, n)
    T = gr.TAB["lrp12"]
    worst = 0.0
    for b in gr.COMPARED:
        th = theta[b]
        sol, st, _ = gr.integrate("lrp12", "resolvent", model, th, n, y0[b], t, **opts)
        sys = gr.system(model, th, n)
        cA, cB, cC, cD, S0, Dd = th
        dg, ci = [cD + (0.0 + S0), (0.0 + 1.0) + Dd], [0.0, S0]
        for k in range(1, t.size):
            hs = t[k] - t[k - 1]
            yR, y = sol[k - 1][0], list(sol[k - 1][1:])
            q = T["GAM"] * hs
            winvR, qC = rcp(fma(q, cB, 1.0)), q * cC
            a = [[fma(q, dg[0], 1.0), -q * 1.0], [-q * ci[1], fma(q, dg[1], 1.0)]]
            for kk in range(2):
                rp, i = rcp(a[kk][kk]), 1 - kk
                ml = a[i][kk] * rp
                a[i][i] = fma(-ml, a[kk][i], a[i][i])
                a[i][kk] = -ml
                a[kk][i] *= rp
                a[kk][kk] = rp

            def solve(r, rR):
                zR = rR * winvR
                rr = [fma(qC, zR, r[0]), r[1]]
                return [fma(a[i][1], rr[1], a[i][0] * rr[0]) for i in range(2)], zR

            f = [fma(cC, yR, fma(1.0, y[1], -dg[0] * y[0])) * hs, fma(ci[1], y[0], -dg[1] * y[1]) * hs]
            z, zR = solve(f, hs * fma(-cB, yR, cA))
            ynR, yn = fma(T["B"][0], zR, yR), [fma(T["B"][0], z[m], y[m]) for m in range(2)]
            for s in range(1, len(T["B"])):
                z, zR = solve(z, zR)
                ynR, yn = fma(T["B"][s], zR, ynR), [fma(T["B"][s], z[m], yn[m]) for m in range(2)]
            ref, tt = gr.interval_reference("lrp12", "resolvent", sys, sol, t, k)
            worst = max(worst, float(np.max(np.abs(np.array([ynR] + yn) - ref.astype(float)))) / tt)
    print("text of tpr_rand_kernel<1> in correctly rounded double against long double: %.3f tau" % worst)
    assert gr.KERNEL_R64[model, n, gr.B, "lrp12"] < worst <= gr.TPR1_TEXT_R64 <= R64["lrp12", "resolvent"]


def _with_clamps(lo, hi, call):
    """call() with step_fac's clamps [lo, hi] in group_reference.integrate."""
    orig = gr.step_fac
    gr.step_fac = lambda root, lo_=lo, safety_inv=1.0 / 0.9: max(lo_, min(hi, root * safety_inv))
    try:
        return call()
    finally:
        gr.step_fac = orig


def test_clamp_runs_are_set_by_the_clamps_and_not_by_the_precision_of_the_root():
    """The GROWTH and SHRINK runs of tests/test_gpu_rand_matrix.py on the restatement, at every LRP12 case of the table with up to 129
    states and on the first replica of the larger ones (what the GPU file compares).  GROWTH: the same count with a single- and a
    double-precision root, and a growth clamp of 8 instead of 6 takes at least 2 steps fewer -- so the GPU file's equality sees it.  SHRINK:
    at least 9 rejected steps, the spread between the two roots within SHRINK_SPREAD, and a shrink clamp of 10 instead of 5 rejects at
    least 2 fewer -- beyond the GPU file's allowance of SHRINK_SPREAD[1] = 1."""
    spread = [0, 0]
    for model, n, batch, method in gr.KERNEL_CASES:
        if method != "lrp12":
            continue
        theta, y0 = gr.case(model, n, batch)
        for b in gr.compared(batch) if pm.n_states(model, n) <= 129 else (0,):
            run = lambda t, kw, **more: gr.integrate("lrp12", "resolvent", model, theta[b], n, y0[b], t, **kw, **more)[1:]
            g32, g64 = run(pm.TIME_POINTS, gr.GROWTH), run(pm.TIME_POINTS, gr.GROWTH, root=np.float64)
            assert g32 == g64 and g32[0] == 0 and g32[1][1] == 0, (model, n, b, g32, g64)
            s32, s64 = run(gr.SHRINK_T, gr.SHRINK), run(gr.SHRINK_T, gr.SHRINK, root=np.float64)
            assert s32[0] == 0 and s64[0] == 0 and s32[1][1] >= 9, (model, n, b, s32)
            for i in (0, 1):
                spread[i] = max(spread[i], abs(s32[1][i] - s64[1][i]))
            if pm.n_states(model, n) <= 65:
                g8 = _with_clamps(1.0 / 8.0, 5.0, lambda: run(pm.TIME_POINTS, gr.GROWTH))
                s10 = _with_clamps(1.0 / 6.0, 10.0, lambda: run(gr.SHRINK_T, gr.SHRINK))
                assert g8[1][0] <= g32[1][0] - 2 and s10[1][1] <= s32[1][1] - 2, (model, n, b, g32, g8, s32, s10)
    print("SHRINK run, single- against double-precision root, largest difference (accepted, rejected):", tuple(spread))
    assert spread[0] <= gr.SHRINK_SPREAD[0] and spread[1] <= gr.SHRINK_SPREAD[1], spread


def test_kernel_table_names_every_kernel_of_the_issue_once():
    names = [(k.name, k.n) for k in gr.KERNELS]
    assert len(set(names)) == len(names) == 29
    assert all(k.env in gr.ENV_GROUPS and "lrp12" == k.methods[0] for k in gr.KERNELS)
    assert [k.B for k in gr.KERNELS if k.B != gr.B] == [1024]
    for k in gr.KERNELS:                                                              # wide_chain_lds_bytes of csrc/pk_wide.hpp against the 160 KB of LDS
        if k.plan == "WideChain":
            assert (15 * k.S + 2 + k.n + 24) * 8 <= 160 * 1024


def test_step_counts_do_not_hang_on_the_precision_of_the_root():
    """The controller's root err^(1/Q) is taken in single precision on the device.  integrate with a single- and with a double-precision
    root on the free-running inputs of the GPU matrix: the spread in accepted / rejected steps is what the GPU file allows the device (plus
    2), and it stays below a tenth of the step count.  BDF2 takes sqrt / cbrt in double in the kernel and here: no spread by construction."""
    spread = {m: 0 for m in gr.ROOT_SPREAD}
    for model, n in ALL_SIZES:
        theta, y0 = gr.case(model, n)
        for (method, form), (kw, _) in gr.FREE.items():
            if method == "bdf2":
                continue
            for b in gr.COMPARED:
                _, s32, n32 = gr.integrate(method, form, model, theta[b], n, y0[b], pm.TIME_POINTS, root=np.float32, **kw)
                _, s64, n64 = gr.integrate(method, form, model, theta[b], n, y0[b], pm.TIME_POINTS, root=np.float64, **kw)
                assert s32 == 0 and s64 == 0
                d = max(abs(n32[0] - n64[0]), abs(n32[1] - n64[1]))
                assert d <= 0.1 * n32[0], (model, n, method, form, b, n32, n64)
                spread[method] = max(spread[method], d)
    print("steps with a single- against a double-precision root, largest difference:", spread)
    assert spread == gr.ROOT_SPREAD
