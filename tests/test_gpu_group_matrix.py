"""GPU: every lane-group kernel (solve_kernel, steady_kernel, rhs_kernel, jac_kernel of csrc/pk_solve_kernel.hpp) against the numpy
restatement tests/group_reference.py, which tests/test_group_reference_cpu.py pins first.  An explicit `linsolve` routes all three models
to these kernels (tests/test_protein_plan_cpu.py holds protein_plan to that for every size used here).

Sizes: both sides of every lane-group width and the minimum (distmod / succmod n = 1, 6 | 7, 14 | 15, 30 | 31, 62, i.e. S = 3, 8 | 9, 16 |
17, 32 | 33, 64; randmod n = 1 .. 5, S = 3, 5, 9, 17, 33: idle lanes at every width), B = 37 (a ragged last block at 32, 16, 8 and 4
replicas per block), per-replica y0, theta half U(0, 20) and half log-uniform.

a. Forced grid.  With rtol = atol = 1 and h0 above every spacing the kernel takes exactly one step per interval, which n_steps == (T - 1, 0)
   proves on all 37 replicas; each output row is then one step from the kernel's own previous rows, and is compared with that step in long
   double: |y_gpu - y_ref|_inf <= C tau, tau = |majorant|_inf 2^-53.
   Worst ratio measured per solver and update (MI355X; worst over every size, the compared replicas and every row), and C:
                 LRP12        LRP8         RODAS4       RODAS4 stage  BDF1 / BDF2   RK4
     DenseInv    3.48 -> 16   3.32 -> 16   9.71 -> 64   3.80 -> 16    4.23 -> 32
     Arrow       1.14 ->  8   2.03 -> 16   5.36 -> 32   3.13 -> 16    4.23 -> 32
     Tridiag     3.48 -> 16   2.98 -> 16   3.26 -> 16   1.91 ->  8    4.22 -> 32
     (no solve)                                                                     1.29 -> 8
   (DenseInv 9.71: distmod n = 62, the first row; every other figure of that column is below 5.4.)
   C is 4 x the worst ratio of the solver and update, rounded up to a power of two (the allowance is for rounding variation across
   inputs).  Condition: no ratio above 64 x the double-precision restatement's own (tests/test_group_reference_cpu.py: LRP12 2.76, LRP8
   2.63, RODAS4 3.40 / 2.63 stage form, BDF2 5.79, RK4 0.93) -- 64 is the longest dot product in the kernel, DenseInvSolver<64>::solve.
b. Free-running on the 14-point grid at the tolerances and limits of tests/test_gpu_parity.py, with accepted and rejected steps against
   group_reference.integrate: within 2 for LRP12 / LRP8; for RODAS4 and BDF2 within 2 plus the spread between a single- and a
   double-precision root measured on the CPU (group_reference.ROOT_SPREAD: 0 for both).  Measured on the MI355X: the counts are equal
   on every size, solver and compared replica but for one accepted step of LRP12; worst band error 0.034 (LRP12), 0.024 (LRP8), 0.029
   (RODAS4, both forms), 1.90 (BDF2); up to 21 576 steps (BDF2).
c. steady_kernel, rhs_kernel and jac_kernel, which share load_row and the solvers, at the same sizes.

Template instantiations this file launches that no test launched before: ArrowSolver<64>; DenseInvSolver<DIST, 64>, DenseInvSolver<SUCC,
32> and <SUCC, 64>; TridiagSolver<32> and <64> under LRP8, RODAS4 (both forms) and BDF2; every BDF2 and RK4 kernel wider than 16 lanes;
the classical RODAS4 stage form wider than 32 lanes and on succmod beyond 16; steady / rhs / jac kernels of 64 lanes for distmod and succmod."""
import numpy as np
import pytest

import group_reference as gr
from oracle import protein_models as pm

pytestmark = pytest.mark.gpu

ALL_SIZES = [(model, n) for (model, G), ns in gr.SIZES.items() for n in ns]
GROUPS = list(gr.SIZES)
#: the double-precision restatement's own |y64 - yld| / tau (tests/test_group_reference_cpu.py); 64 x this is where a ratio becomes a finding
R64 = {("lrp12", "resolvent"): 2.76, ("lrp8", "resolvent"): 2.63, ("rodas4", "resolvent"): 3.40, ("rodas4", "stage"): 2.63,
       ("bdf2", "resolvent"): 5.79, ("rk4", "resolvent"): 0.93}
#: C per (solver, update): 4 x the measured worst ratio, rounded up to a power of two (module docstring)
_UPD = (("lrp12", "resolvent"), ("lrp8", "resolvent"), ("rodas4", "resolvent"), ("rodas4", "stage"), ("bdf2", "resolvent"))
C_BOUND = {("none", ("rk4", "resolvent")): 8.0}
C_BOUND.update({("DenseInv", u): c for u, c in zip(_UPD, (16.0, 16.0, 64.0, 16.0, 32.0))})
C_BOUND.update({("Arrow", u): c for u, c in zip(_UPD, (8.0, 16.0, 32.0, 16.0, 32.0))})
C_BOUND.update({("Tridiag", u): c for u, c in zip(_UPD, (16.0, 16.0, 16.0, 8.0, 32.0))})
WORST = {}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()          # raises loudly if libphoskin_hip.so is missing
    return batch


def _np(x):
    return x.detach().cpu().numpy()


def _solver(model, linsolve, method):
    if method == "rk4":
        return "none"
    return "DenseInv" if linsolve == "dense" or model == pm.RAND else ("Arrow" if model == pm.DIST else "Tridiag")


@pytest.mark.parametrize("model,G", GROUPS)
def test_forced_grid_every_step_against_long_double(eng, model, G):
    for n in gr.SIZES[model, G]:
        theta, y0 = gr.case(model, n)
        metric = pm.METRICS[ALL_SIZES.index((model, n)) % len(pm.METRICS)]
        systems = {b: gr.system(model, theta[b], n) for b in gr.COMPARED}
        for method, form in gr.UPDATES:
            t, opts = gr.forced(method, model, theta, n)
            want = (sum(gr.rk4_substeps(t, opts["rk4_h"])) if method == "rk4" else t.size - 1, 0)
            sols = {}
            for linsolve in ("dense", "structured"):
                where = (pm.MODEL_NAMES[model], n, method, form, linsolve)
                r = eng.solve_ode_batch(model, theta, y0, n, t, method=method, linsolve=linsolve, stage_form=int(form == "stage"), clip_nonneg=False,
                                        metric=metric, **opts)
                sol, flat, met = _np(r.sol), _np(r.flat), _np(r.metric)
                sols[linsolve] = sol
                assert not _np(r.status).any(), where
                assert (_np(r.n_steps) == np.array(want)).all(), (where, _np(r.n_steps))          # the steps the comparison assumes, on all 37
                key = (_solver(model, linsolve, method), (method, form))
                for b in gr.COMPARED:
                    np.testing.assert_array_equal(sol[b, 0], y0[b])
                    for k in range(1, t.size):
                        ref, tt = gr.interval_reference(method, form, systems[b], sol[b], t, k, opts.get("rk4_h"))
                        ratio = float(np.max(np.abs(sol[b, k] - ref.astype(float)))) / tt
                        if ratio > WORST.get(key, (0.0,))[0]:
                            WORST[key] = (ratio, where, b, k)
                        assert ratio <= 64.0 * R64[method, form], (where, b, k, ratio)             # beyond this: a finding, not a tolerance
                        assert ratio <= C_BOUND[key], (where, b, k, ratio)
                    assert met[b] == pytest.approx(pm.compute_Y(sol[b], n, metric), rel=1e-10, abs=1e-12), (where, metric, b)
                    np.testing.assert_array_equal(flat[b], pm.flatten_observables(model, sol[b], n))
            if model == pm.RAND:                                                                   # no structured solve: the same kernel, the same bits
                np.testing.assert_array_equal(sols["structured"], sols["dense"])
        t, opts = gr.forced("lrp12", model, theta, n)
        r = eng.solve_ode_batch(model, theta, y0, n, t, method="lrp12", linsolve="dense", clip_nonneg=False, normalize=True, **opts)
        p = eng.solve_ode_batch(model, theta, y0, n, t, method="lrp12", linsolve="dense", clip_nonneg=False, **opts)
        np.testing.assert_allclose(_np(r.sol), _np(p.sol) * (1.0 / y0)[:, None, :], rtol=1e-15)
    for key in sorted(WORST):
        print("forced grid, worst |y_gpu - y_ref| / tau so far:", key, "%.2f at %s replica %d row %d" % WORST[key])


@pytest.mark.parametrize("update", list(gr.FREE), ids=lambda u: "-".join(u))
@pytest.mark.parametrize("model,n", ALL_SIZES)
def test_free_running_band_and_step_counts(eng, model, n, update):
    method, form = update
    kw, limit = gr.FREE[update]
    theta, y0 = gr.case(model, n)
    allow = 2 if method in ("lrp12", "lrp8") else gr.ROOT_SPREAD[method] + 2      # measured spread (CPU): 0 for RODAS4, none for BDF2
    ref = {b: gr.integrate(method, form, model, theta[b], n, y0[b], pm.TIME_POINTS, **kw) for b in gr.COMPARED}
    for linsolve in ("dense", "structured"):
        where = (pm.MODEL_NAMES[model], n, method, form, linsolve)
        r = eng.solve_ode_batch(model, theta, y0, n, pm.TIME_POINTS, method=method, linsolve=linsolve, stage_form=int(form == "stage"),
                                clip_nonneg=False, **kw)
        assert not _np(r.status).any(), where
        sol, ns = _np(r.sol), _np(r.n_steps)
        for b in gr.COMPARED:
            e = pm.band_error(sol[b], pm.solve_exact_lti(model, theta[b], y0[b], n, pm.TIME_POINTS))
            _, st, (acc, rej) = ref[b]
            print("free-running", where, "replica", b, "band error %.4f" % e, "steps gpu", tuple(ns[b]), "restatement", (acc, rej))
            assert e <= limit, (where, b, e)
            assert st == 0 and abs(int(ns[b, 0]) - acc) <= allow and abs(int(ns[b, 1]) - rej) <= allow, (where, b, tuple(ns[b]), (acc, rej))


@pytest.mark.parametrize("model,G", GROUPS)
def test_steady_rhs_and_jacobian_kernels(eng, model, G):
    for n in gr.SIZES[model, G]:
        theta, y0 = gr.case(model, n)
        where = (pm.MODEL_NAMES[model], n)
        y, st = eng.steady_state_batch(model, theta, n)
        y, st = _np(y), _np(st)
        assert not st.any(), where
        for b in range(gr.B):
            np.testing.assert_allclose(y[b], pm.steady_state(model, theta[b], n), rtol=1e-11, atol=1e-14, err_msg=str((where, b)))
        bad = theta.copy()
        bad[5, 1] = 0.0                                                  # B = 0: the mRNA never degrades, no steady state
        yb, sb = eng.steady_state_batch(model, bad, n)
        yb, sb = _np(yb), _np(sb)
        assert sb[5] == 1 and np.isnan(yb[5]).all() and not np.delete(sb, 5).any(), where
        np.testing.assert_array_equal(np.delete(yb, 5, axis=0), np.delete(y, 5, axis=0))
        J = _np(eng.jacobian_batch(model, theta, n))
        dy = _np(eng.rhs_batch(model, theta, y0, n))
        Jref = np.stack([pm.jacobian_analytic(model, theta[b], n) for b in range(gr.B)])
        assert (np.abs(J - Jref) <= 4e-15 * max(np.abs(Jref).max(), 1.0)).all(), where
        ref = np.stack([pm.rhs(model, y0[b], 0.0, theta[b], n) for b in range(gr.B)])
        scale = np.abs(Jref).max(axis=(1, 2))[:, None] * np.abs(y0).max() * y0.shape[1]
        assert (np.abs(dy - ref) <= 4e-16 * np.maximum(scale, 1.0) * 4).all(), where
