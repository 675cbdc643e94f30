"""The distributive throughput kernel (csrc/pk_dist_fast.hpp) is compiled once per combination of launch-uniform choices the library's
callers produce (DistSolSum: trajectories + running-sum metric; DistSolOnly: trajectories; DistFlatOnly: flat observables) and once with
every choice read at run time (DistAny).  The choices change control flow, addressing and which bookkeeping exists -- not one floating-point
operation of the solve, the controller or the emitted values -- so wherever two instantiations compute the same thing they must agree
EXACTLY (np.array_equal), on every layout of the LRP12 table and at batch sizes that do not fill a wave or a workgroup."""
import numpy as np
import pytest

from oracle import protein_models as pm

pytestmark = pytest.mark.gpu

SIZES = (17, 24, 30, 32, 40, 62)            # 4x5, 4x6, 4x8, 4x8 (full), 8x5, 8x8 parked layouts
BATCHES = (1, 15, 17, 65)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _np(x):
    return x.detach().cpu().numpy()


def _inputs(n, B, seed=0):
    rng = np.random.default_rng(1000 * n + B + seed)
    theta = rng.uniform(0.05, 5.0, (B, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (B, n + 2))
    return theta, y0


def _flat_of(sol):
    """The flat observable vector laid out from trajectories [B, T, S]: R from the sixth time point on, P, then every site, time-major."""
    B, T, S = sol.shape
    T5 = max(T - 5, 0)
    return np.concatenate([sol[:, 5:, 0].reshape(B, T5), sol[:, :, 1], sol[:, :, 2:].transpose(0, 2, 1).reshape(B, (S - 2) * T)], axis=1)


@pytest.mark.parametrize("n", SIZES)
def test_sol_and_flat_agree_exactly_across_instantiations(eng, n):
    """sol alone (DistSolOnly), sol + flat (DistAny), flat alone (DistFlatOnly), sol + total_signal (DistSolSum): same bits, same steps."""
    for B in BATCHES:
        theta, y0 = _inputs(n, B)
        t = pm.TIME_POINTS
        a = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False)
        b = eng.solve_ode_batch(pm.DIST, theta, y0, n, t)
        c = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_sol=False)
        d = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, metric="total_signal")
        sol = _np(a.sol)
        assert sol.shape == (B, t.size, n + 2) and np.isfinite(sol).all()
        assert not _np(a.status).any()
        for other in (b, d):
            assert np.array_equal(sol, _np(other.sol)), (n, B)
        assert np.array_equal(_np(b.flat), _np(c.flat)), (n, B)
        assert np.array_equal(_np(b.flat), _flat_of(sol)), (n, B)
        for other in (b, c, d):
            assert np.array_equal(_np(a.n_steps), _np(other.n_steps)) and not _np(other.status).any(), (n, B)


@pytest.mark.parametrize("metric", pm.METRICS)
def test_each_metric_with_and_without_sol(eng, metric):
    """A metric with trajectories (DistSolSum for the running-sum metrics, DistAny for the others) and without (DistAny): the same scalar,
    bit for bit, and the one the oracle computes from the trajectories."""
    for n in (17, 30, 40):
        theta, y0 = _inputs(n, 33, seed=7)
        a = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, metric=metric)
        b = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_sol=False, want_flat=False, metric=metric)
        c = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, metric=metric)
        assert np.array_equal(_np(a.metric), _np(b.metric)), (n, metric)
        assert np.array_equal(_np(a.metric), _np(c.metric)), (n, metric)
        assert np.array_equal(_np(a.sol), _np(c.sol)), (n, metric)
        sol = _np(a.sol)
        for r in range(0, 33, 8):
            ref = pm.compute_Y(sol[r], n, metric)
            assert abs(_np(a.metric)[r] - ref) <= 1e-9 * max(1.0, abs(ref)), (n, metric, r)


@pytest.mark.parametrize("n", (24, 30, 62))
def test_clip_and_normalize_against_the_run_time_instantiation(eng, n):
    """clip off and normalize on run on DistAny; clipping / scaling its raw output on the host is the very operation the specialised
    kernels apply to the same raw values."""
    theta, y0 = _inputs(n, 65, seed=3)
    on = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False).sol)
    off = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, clip_nonneg=False).sol)
    assert np.array_equal(on, np.where(off < 0.0, 0.0, off))
    norm = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, normalize=True).sol)
    assert np.array_equal(norm, on * (1.0 / y0)[:, None, :])
    both = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, normalize=True)
    assert np.array_equal(_np(both.sol), norm) and np.array_equal(_np(both.flat), _flat_of(norm))


def test_a_failed_replica_leaves_its_wave_mates_untouched(eng):
    """max_steps too small for the slowest replica of a wave: NaN rows from the landing it
    failed at, finite rows before, a non-zero status; the other replicas of the wave bit-identical to a run without the limit."""
    from phoskintime_amd._capi import ST_MAXSTEPS
    n, B = 30, 17
    theta, y0 = _inputs(n, B, seed=11)
    free = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, metric="total_signal")
    steps = _np(free.n_steps).sum(axis=1)
    limit = int(steps.max()) - 1                                          # enough for every replica but the one(s) needing the most steps
    bad = steps > limit
    assert bad.any() and not bad.all()
    r = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, metric="total_signal", max_steps=limit)
    st, sol = _np(r.status), _np(r.sol)
    for slow in np.flatnonzero(bad):
        assert st[slow] & ST_MAXSTEPS
        bad_rows = np.isnan(sol[slow]).all(axis=1)
        assert bad_rows[-1] and not bad_rows[0]
        first = int(np.argmax(bad_rows))
        assert bad_rows[first:].all() and np.isfinite(sol[slow, :first]).all()
        assert np.array_equal(sol[slow, :first], _np(free.sol)[slow, :first])
        assert np.isnan(_np(r.metric)[slow])
    ok = ~bad
    assert not st[ok].any()
    assert np.array_equal(sol[ok], _np(free.sol)[ok]) and np.array_equal(_np(r.metric)[ok], _np(free.metric)[ok])


@pytest.mark.parametrize("n", (24, 40))
def test_against_the_c_restatement_of_the_same_algorithm(eng, n):
    """The comparison of test_gpu_parity (oracle/lrp8_dist.c, same method and controller: band <= 0.02, accepted steps within 2) on two
    more layouts."""
    from oracle import lrp8_cpu
    rng = np.random.default_rng(20260515 + n)
    theta = rng.uniform(0.0, 20.0, (64, pm.n_params(pm.DIST, n)))
    y0 = np.ones(n + 2)
    r = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, clip_nonneg=False)
    sol_c, st_c, ns_c = lrp8_cpu.solve_batch(theta, n, y0, pm.TIME_POINTS)
    assert not st_c.any() and not _np(r.status).any()
    assert pm.band_error(_np(r.sol), sol_c) <= 0.02
    assert np.abs(_np(r.n_steps)[:, 0] - ns_c[:, 0]).max() <= 2
