"""The step-size controller of the distributive throughput kernels (csrc/pk_dist_fast.hpp) takes its maxima and minima as single
v_max_f64 / v_min_f64 instructions (csrc/pk_wave.hpp: max_abs, max_raw, min_raw -- in both error norms, the controller and the loop head)
and multiplies the step by a clamped growth factor, hnew = hs * step_growth(err^(-1/Q)) (csrc/pk_step.hpp), where it divided by a clamped
divisor through a full-precision reciprocal.  The C restatement (oracle/lrp8_dist.c through oracle/lrp8_cpu.py) and its statement-for-
statement numpy port with an initial step (tests/test_gpu_dist_fast_sitesum.py) keep hnew = hs / fac and are the yardstick, at the project's
limits: band error <= 0.02, accepted and rejected steps within 2.

Every case runs the four output classes (tests/test_gpu_dist_fast_resolvent.py: _classes) on the five lane layouts below, in batches of
17-48 replicas that leave a wave partial:
  * growth at the cap: slow systems from a first step of 1e-6, which the controller multiplies by six step after step;
  * shrink at the cap and the rule after a reject: a first step of 10, which every replica rejects;
  * landings shorter than the step the controller asked for (the grid's outputs at 0.75 and 1.0);
  * the specialised kernels against the run-time kernel (DistAny) through integer views, on a healthy batch and on the batch of
    tests/test_gpu_dist_fast_norm.py with NaN, inf and negative parameters: max_abs keeps fmax's NaN behaviour in both norms.
Each case states on the REFERENCE's step counts that it is about what it names.  LRP8 runs at n = 30 (the port states LRP12: no forced
first step there)."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lrp8_cpu
from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_dist_fast_norm as tn  # noqa: E402  (_poisoned: replicas with NaN, inf and negative parameters)
import test_gpu_dist_fast_resolvent as tr  # noqa: E402  (_theta, _classes, _np, _bits, _bitwise)
import test_gpu_dist_fast_sitesum as ts  # noqa: E402  (the numpy port of the C restatement with an initial step)

T = pm.TIME_POINTS
# n: (G x RPL, layout, replicas)
SIZES = {2: ("4 x 1", "resident", 17), 14: ("4 x 4", "resident, registers", 33), 30: ("4 x 8", "resident, parked", 48),
         32: ("4 x 8", "shadowed", 37), 38: ("8 x 5", "resident, parked", 19)}
H_SMALL, H_LARGE = 1e-6, 10.0


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


_REF = {}


def _frozen(key, make):
    """A reference computed once, shared, never written to."""
    if key not in _REF:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _port(theta, n, t, h0):
    out = [ts._lrp12_with_h0(th, n, np.ones(n + 2), t, h0=h0) for th in theta]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([[o[2], o[3]] for o in out])


# ---------------------------------------------------------------- growth at the cap
def _fewest_steps(cap, span, h0):
    """The fewest steps in which a controller that multiplies the step by at most `cap` covers `span` from a first step h0: the smallest m
    with h0 (1 + cap + ... + cap^(m-2)) + 1.0001 h0 cap^(m-1) >= span (the last step is a landing: it may be 1.0001 steps long)."""
    m, done, h = 1, 0.0, h0
    while done + 1.0001 * h < span:
        done, h, m = done + h, h * cap, m + 1
    return m


def _growth(n):
    """theta ~ U(0, 0.05), h0 = 1e-6: (theta, sol, status, steps) of the port on the whole grid, and its steps up to the first output."""
    def make():
        theta = tr._theta(n, SIZES[n][2], 19000 + n, hi=0.05)
        sol, st, ns = _port(theta, n, T, H_SMALL)
        _, st1, ns1 = _port(theta, n, T[:2], H_SMALL)
        return theta, sol, st, ns, st1, ns1
    return _frozen(("growth", n), make)


def test_the_restatement_grows_at_the_cap():
    """CPU.  From h0 = 1e-6 to the first output at 0.5: nine steps are the fewest a sixfold cap allows, and a fivefold cap allows no fewer
    than ten.  The restatement takes nine in every replica, so its steps grow beyond fivefold -- at the cap -- on the way."""
    six, five = _fewest_steps(6.0, float(T[1] - T[0]), H_SMALL), _fewest_steps(5.0, float(T[1] - T[0]), H_SMALL)
    assert (six, five) == (9, 10)
    for n in SIZES:
        _, _, st, ns, st1, ns1 = _growth(n)
        assert not st.any() and not st1.any(), n
        assert (ns1[:, 0] == six).all() and not ns1[:, 1].any(), (n, ns1)
        assert ns[:, 0].min() > 20, n


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_growth_at_the_cap(eng, n):
    theta, raw, st, ns, _, ns1 = _growth(n)
    assert not st.any()
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "%s %s, growth from h0 = 1e-6" % SIZES[n][:2], rejected=True, h0=H_SMALL)
    # The kernel's own way to the first output.  It cannot take fewer steps than the fewest its cap allows, and it takes that many only
    # if it multiplies by more than five on the way (test_the_restatement_grows_at_the_cap): a cap of 5, 1 / 6 for 6 or the two clamps
    # exchanged would show here, inside the +-2 that the whole grid is held to.  Both kernels: the specialised one and the run-time one.
    for kw in (dict(), dict(clip_nonneg=False)):
        r = eng.solve_ode_batch(pm.DIST, theta, np.ones(n + 2), n, T[:2], want_flat=False, h0=H_SMALL, **tr.KW, **kw)
        steps = tr._np(r.n_steps)
        print(n, kw, "steps to the first output", sorted(set(map(tuple, steps.tolist()))), "reference", sorted(set(map(tuple, ns1.tolist()))))
        assert not tr._np(r.status).any()
        assert np.array_equal(steps, ns1), (n, kw, "steps to the first output")


# ---------------------------------------------------------------- shrink at the cap, and the rule after a reject
def _shrink(n):
    def make():
        theta = tr._theta(n, SIZES[n][2], 19100 + n)
        return (theta,) + _port(theta, n, T, H_LARGE)
    return _frozen(("shrink", n), make)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_forced_first_reject(eng, n):
    """h0 = 10: the error of the first step is beyond 5^11, so the step shrinks fivefold (the cap) and the accepted step after it may
    not grow.  The reference must reject too, or the test is not about rejects."""
    theta, raw, st, ns = _shrink(n)
    assert not st.any() and ns[:, 1].min() >= 1, (n, "the restatement does not reject the forced first step")
    out = tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "%s %s, h0 = 10" % SIZES[n][:2], rejected=True, h0=H_LARGE)
    for what, r in out.items():
        assert tr._np(r.n_steps)[:, 1].min() >= 1, (n, what, "a replica rejected nothing")
        assert np.array_equal(tr._np(r.n_steps), tr._np(out["raw"].n_steps)), (n, what)


# ---------------------------------------------------------------- landings shorter than the step
def _landings(n):
    """The benchmark's distribution on the library's grid: (theta, sol, steps) of the C restatement, and its accepted steps up to the
    outputs at 0.5, 0.75 and 1.0 (the step sequence up to an output does not depend on the outputs after it)."""
    def make():
        theta = tr._theta(n, SIZES[n][2], 19200 + n)
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), T)
        assert not st.any()
        upto = np.stack([lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), T[:k])[2][:, 0] for k in (2, 3, 4)], axis=1)
        return theta, sol, ns, upto
    return _frozen(("landings", n), make)


def test_the_restatement_lands_short_of_its_step():
    """CPU.  An interval of 0.25 covered in one or two steps ends in a landing cut short of h, where h = max(hnew, h) keeps the step the
    controller had asked for.  One step: it lands, so 1.0001 h >= 0.25 = hs.  Two steps by the halving rule (h < 0.25 < 2 h): two steps of
    0.125 < h.  Two steps otherwise: the first is h <= 0.125 and the second lands, hs = 0.25 - h <= 1.0001 h_2.  In each case hs < h but
    for a sliver of relative width 1e-4.  Every replica of every batch does that at both outputs."""
    for n in SIZES:
        _, _, _, upto = _landings(n)
        per = np.diff(upto, axis=1)
        print(n, "steps from 0.5 to 0.75 and from 0.75 to 1.0:", dict(zip(*map(np.ndarray.tolist, np.unique(per, return_counts=True)))))
        assert per.min() >= 1 and per.max() <= 2, n


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_landings_shorter_than_the_step(eng, n):
    theta, raw, ns, _ = _landings(n)
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "%s %s, U(0, 20)" % SIZES[n][:2], rejected=True)


# ---------------------------------------------------------------- LRP8
def _lrp8(hi):
    def make():
        theta = tr._theta(30, 29, 19300 + int(hi), hi=hi)
        sol, st, ns = lrp8_cpu.solve_batch(theta, 30, np.ones(32), T, stages=8, rtol=1e-7, atol=1e-9)
        assert not st.any()
        return theta, sol, ns
    return _frozen(("lrp8", hi), make)


@pytest.mark.gpu
@pytest.mark.parametrize("hi", (20.0, 0.05))
def test_lrp8(eng, hi):
    """Q = 7 on the 8 x 4 shadowed table; the slow systems grow from the library's first step at or near the cap"""
    theta, raw, ns = _lrp8(hi)
    tr._classes(eng, theta, np.ones(32), 30, raw, ns, "lrp8, U(0, %g)" % hi, rejected=True, method="lrp8", rtol=1e-7, atol=1e-9)


# ---------------------------------------------------------------- the four output classes against DistAny, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_healthy_batch_has_the_bits_of_the_run_time_kernel(eng, n):
    tr._bitwise(eng, n)


def _poisoned_two_sites(B=40):
    """tests/test_gpu_dist_fast_norm.py: _poisoned names sites 1 to 3 and so needs four of them; the same defects on the two sites of n = 2"""
    n = 2
    rng = np.random.default_rng(4200 + n)
    theta = rng.uniform(0.05, 5.0, (B, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (B, n + 2))
    bad = {1: ("th", 4, np.nan), 4: ("th", 0, np.nan), 6: ("th", 4 + n + 1, np.inf), 9: ("th", 4 + 1, np.inf), 13: ("th", 4 + 1, 1e308),
           18: ("th", 3, -1e308), 21: ("th", 4 + n + 1, 1e200), 25: ("y", 2 + 1, np.nan), 29: ("y", 1, np.inf), 33: ("th", 1, -np.inf),
           38: ("th", 4 + n, 1e308)}
    for r, (where, i, v) in bad.items():
        (theta if where == "th" else y0)[r, i] = v
    theta[14, 4] = theta[14, 5] = 1e308                                # two rates whose sum is inf
    return theta, y0, np.array(sorted(list(bad) + [14]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_nonfinite_batch_has_the_bits_of_the_run_time_kernel(eng, n):
    """NaN, inf, overflowing and negative parameters and initial values beside healthy replicas: err_norm (specialised kernels) and
    group_max (DistAny) both go through max_abs, and must still drop and surface the same NaNs -- same status, same steps, same 64-bit
    patterns in every output, NaN rows included."""
    theta, y0, bad = tn._poisoned(n) if n >= 4 else _poisoned_two_sites()
    kw = dict(max_steps=400)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric="total_signal", **kw)                      # sol + flat + sum: DistAny
    a = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **kw)                             # DistSolOnly
    c = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **kw)                              # DistFlatOnly
    d = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **kw)      # DistSolSum
    st = tr._np(ref.status)
    ok = np.setdiff1d(np.arange(len(theta)), bad)
    assert st[bad].any() and not st[ok].any(), (n, st)
    for what, r in (("sol only", a), ("flat only", c), ("sol + sum", d)):
        assert np.array_equal(tr._np(r.status), st) and np.array_equal(tr._np(r.n_steps), tr._np(ref.n_steps)), (n, what)
    assert np.array_equal(tr._bits(a.sol), tr._bits(ref.sol)) and np.array_equal(tr._bits(d.sol), tr._bits(ref.sol)), n
    assert np.array_equal(tr._bits(c.flat), tr._bits(ref.flat)), n
    failed = st != 0
    assert np.array_equal(tr._bits(d.metric)[~failed], tr._bits(ref.metric)[~failed]), n
    assert np.isnan(tr._np(d.metric)[failed]).all() and np.isnan(tr._np(ref.metric)[failed]).all(), n
