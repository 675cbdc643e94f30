"""The first LRP12 stage formed from the state rows, the single-chain stage dot product and the P slot's fix-ups as arithmetic
(csrc/pk_dist_fast.hpp: dist_stage1_state(), gdot(), dist_pslot_arith()), one size per layout the three touch, against the C restatement
(oracle/lrp8_dist.c through oracle/lrp8_cpu.py) at the project's limits: status 0, band error <= 0.02, accepted and rejected steps within 2.

    n = 30   4 x 8 resident (the benchmark's)     first stage from the state, one chain, P slot as arithmetic
    n = 22   4 x 6 resident                       the same (the flat-output kernel keeps the P slot's selects)
    n = 62   8 x 8 resident                       the same
    n = 24, 28   4 x 6 / 4 x 7 shadowed           first stage from the state, one chain
    n = 20, 40   4 x 5 / 8 x 5 shadowed           one chain (five shadowed rows keep rho_j = y_j ic_j: no registers for winv_j)
    n = 18   4 x 5 resident, plain units          the P slot as arithmetic in the flat-output and run-time kernels only

Batches: those of tests/test_gpu_dist_fast_scaled.py, whose references are shared and never written to -- 29-41 replicas (a partial wave) of
theta ~ U(0, 20) and U(0, 1) from y0 = 1, the edge rates of the scale rule, and a forced first step of 1e-9 at n = 22, 28, 30.  The four
output classes of a layout agree bit for bit; a replica with a NaN or an infinite site rate ends as PK_ST_NONFINITE with NaN rows from the
landing it failed at, and leaves its wave mates' bits alone."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_dist_fast_resolvent as tr  # noqa: E402  (_classes: the four output classes against the restatement's trajectories)
import test_gpu_dist_fast_scaled as sc  # noqa: E402  (the batches and their references, computed once per process)

T = pm.TIME_POINTS
SIZES = (18, 20, 22, 24, 28, 30, 40, 62)
H0_SIZES = (22, 28, 30)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def test_the_restatement_finishes_every_batch():
    """CPU: the references of the tests below end with status 0 after a run of steps."""
    for n in SIZES:
        for hi in (20.0, 1.0):
            _, _, st, ns = sc._random(n, hi)
            assert not st.any() and ns[:, 0].min() > 10, (n, hi)
        _, _, _, st, ns = sc._edge(n)
        assert not st.any() and ns[:, 0].min() > 10, (n, "edge")
    for n in H0_SIZES:
        _, _, st, ns = sc._with_h0(n)
        assert not st.any() and ns[:, 0].min() > 10, (n, "h0")


@pytest.mark.gpu
@pytest.mark.parametrize("hi", (20.0, 1.0))
@pytest.mark.parametrize("n", SIZES)
def test_random_rates_against_the_c_restatement(eng, n, hi):
    theta, raw, st, ns = sc._random(n, hi)
    assert not st.any()
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, sc._tag(n, "theta ~ U(0, %g)" % hi), rejected=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_edge_rates_against_the_c_restatement(eng, n):
    """A rate exactly 0, every rate 0, rates of 1e-300, 1e-12 and 1e6, rates over eight decades (kappa_j = d_j / s_j from 1e-6 to 2^600
    d_j), and the zero-rate site that starts at 0: +0.0 in every output row of every class (kappa_j = 0, every value of the row 0 w_j)."""
    theta, y0, raw, st, ns = sc._edge(n)
    assert not st.any()
    out = tr._classes(eng, theta, y0, n, raw, ns, sc._tag(n, "edge rates"), rejected=True)
    for what, r in out.items():
        if r.sol is not None:
            assert not tr._bits(r.sol)[7, :, 2 + sc.ZERO_SITE].any(), (n, what, "the zero row is not +0.0")


@pytest.mark.gpu
@pytest.mark.parametrize("n", H0_SIZES)
def test_small_first_step(eng, n):
    """h0 = 1e-9: q kappa_j y_j is nine decades below xq on the first steps"""
    theta, raw, st, ns = sc._with_h0(n)
    assert not st.any()
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, sc._tag(n, "h0 = 1e-9"), rejected=True, h0=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_the_four_classes_agree_bit_for_bit(eng, n):
    """sol alone, flat alone and sol + total_signal against sol + flat + total_signal, which runs on DistAny: every output through its
    integer view, on the random and the edge rates in one batch.  The classes of a layout share its first stage and its dot product; they
    differ in how the P slot is fixed up (dist_pslot_arith()), which moves no bit."""
    th_r, _, _, _ = sc._random(n, 20.0)
    th_e, y0_e, _, _, _ = sc._edge(n)
    theta = np.concatenate([th_r, th_e])
    y0 = np.concatenate([np.ones((len(th_r), n + 2)), y0_e])
    kw = tr.KW
    a = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **kw)
    c = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **kw)
    d = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **kw)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric="total_signal", **kw)
    assert np.isfinite(tr._np(ref.sol)).all() and not tr._np(ref.status).any() and tr._np(ref.n_steps)[:, 0].min() > 10, n
    assert np.array_equal(tr._bits(a.sol), tr._bits(ref.sol)) and np.array_equal(tr._bits(d.sol), tr._bits(ref.sol)), n
    assert np.array_equal(tr._bits(c.flat), tr._bits(ref.flat)), n
    assert np.array_equal(tr._bits(d.metric), tr._bits(ref.metric)), n
    for other in (a, c, d):
        assert np.array_equal(tr._np(other.status), tr._np(ref.status)) and np.array_equal(tr._np(other.n_steps), tr._np(ref.n_steps)), n


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_site_rates(eng, n):
    """Replica 5 has a NaN rate at site 3, replica 22 an infinite one at the last site (kappa_j and the scale are then NaN or 0 / inf; the
    rate has reached Dsum): both end as PK_ST_NONFINITE with NaN rows from the first landing on, in every class; all other replicas, their
    wave mates among them, keep the bits of a launch in which the two are ordinary."""
    from phoskintime_amd._capi import ST_NONFINITE
    plain, _, _, _ = sc._random(n, 20.0)
    theta = plain.copy()
    odd = np.array([5, 22])
    theta[5, 4 + 3] = np.nan
    theta[22, 4 + n - 1] = np.inf
    mates = np.setdiff1d(np.arange(len(theta)), odd)
    y0 = np.ones(n + 2)
    for name, extra in (("sol + sum", dict(want_flat=False, metric="total_signal")), ("sol only", dict(want_flat=False)),
                        ("flat only", dict(want_sol=False)), ("run-time", dict(metric="total_signal"))):
        r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, **extra, **tr.KW)
        p = eng.solve_ode_batch(pm.DIST, plain, y0, n, T, **extra, **tr.KW)
        st = tr._np(r.status)
        assert (st[odd] == ST_NONFINITE).all() and not st[mates].any() and not tr._np(p.status).any(), (n, name, st)
        assert np.array_equal(tr._np(r.n_steps)[mates], tr._np(p.n_steps)[mates]), (n, name, "wave mates' steps")
        if r.sol is not None:
            sol = tr._np(r.sol)
            assert np.isnan(sol[odd, 1:]).all() and np.isfinite(sol[odd, 0]).all(), (n, name, "NaN rows from the failed landing on")
            assert np.array_equal(tr._bits(r.sol)[mates], tr._bits(p.sol)[mates]), (n, name, "wave mates")
        if r.flat is not None:
            assert np.array_equal(tr._bits(r.flat)[mates], tr._bits(p.flat)[mates]), (n, name, "wave mates, flat")
        if r.metric is not None:
            assert np.isnan(tr._np(r.metric)[odd]).all() and np.array_equal(tr._bits(r.metric)[mates], tr._bits(p.metric)[mates]), (n, name, "metric")
