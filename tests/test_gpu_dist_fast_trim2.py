"""The specialised distributive kernels (csrc/pk_dist_fast.hpp: DistSolSum, DistSolOnly, DistFlatOnly) carry their step count, their time
and their non-finite exit differently from the run-time kernel (DistAny), and clip a landing's row only when a sign bit is set somewhere
in the wave.  None of that may change a bit of what a replica returns: here the three are held to DistAny, which keeps the literal code,
through int64 views of every output -- on healthy batches of four layouts, at the controller's corners (a first landing shorter than the
step estimate, rejected steps, an exhausted step budget), next to replicas with non-finite parameters, and on states that are exact zeros
of either sign or negative before the clip."""
import numpy as np
import pytest

from oracle import protein_models as pm

pytestmark = pytest.mark.gpu

SIZES = (4, 17, 30, 62)             # 4 x 1 in registers, 4 x 5 parked, 4 x 8 parked, 8 x 8 parked
B = 256                             # four waves of the 4-lane layouts, eight of the 8-lane one


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    """The 64-bit patterns of a float64 array (NaN payloads and the sign of a zero included)."""
    return np.ascontiguousarray(_np(x), dtype=np.float64).view(np.int64)


def _four(eng, n, theta, y0, t, **kw):
    """The same batch through DistAny (trajectories + flat + metric) and the three specialised configurations."""
    kw = dict(kernel="group", **kw)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, metric="total_signal", **kw)
    msum = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, metric="total_signal", **kw)
    only = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, **kw)
    flat = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_sol=False, **kw)
    return ref, msum, only, flat


def _assert_identical(ref, msum, only, flat, what):
    for name, r in (("sol + sum", msum), ("sol only", only), ("flat only", flat)):
        assert np.array_equal(_np(ref.status), _np(r.status)), (what, name, "status")
        assert np.array_equal(_np(ref.n_steps), _np(r.n_steps)), (what, name, "n_steps")
    assert np.array_equal(_bits(ref.sol), _bits(msum.sol)), (what, "sol + sum", "sol")
    assert np.array_equal(_bits(ref.sol), _bits(only.sol)), (what, "sol only", "sol")
    assert np.array_equal(_bits(ref.metric), _bits(msum.metric)), (what, "sol + sum", "metric")
    assert np.array_equal(_bits(ref.flat), _bits(flat.flat)), (what, "flat only", "flat")


@pytest.mark.parametrize("n", SIZES)
def test_specialised_kernels_match_the_run_time_kernel_bit_for_bit(eng, n):
    rng = np.random.default_rng(5100 + n)
    theta = rng.uniform(0.0, 20.0, (B, pm.n_params(pm.DIST, n)))
    y0 = np.ones(n + 2)
    ref, msum, only, flat = _four(eng, n, theta, y0, pm.TIME_POINTS)
    assert not _np(ref.status).any() and np.isfinite(_np(ref.sol)).all()
    _assert_identical(ref, msum, only, flat, n)


@pytest.mark.parametrize("n", (17, 30))
def test_controller_corners(eng, n):
    """A first output time far below the first step (the first step lands with hs < h and the controller keeps the larger step), a first
    step (h0 = 10) far too long for the tolerance, so that the step after that landing is rejected with the growth factor at its clamp,
    and a step budget that about half of the replicas exhaust."""
    from phoskintime_amd._capi import ST_MAXSTEPS
    rng = np.random.default_rng(5200 + n)
    theta = rng.uniform(0.0, 20.0, (B, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (B, n + 2))
    t = np.concatenate([[0.0, 1e-9], pm.TIME_POINTS[1:]])
    kw = dict(rtol=1e-10, atol=1e-12, h0=10.0)
    free = _four(eng, n, theta, y0, t, **kw)
    steps = _np(free[0].n_steps)
    assert not _np(free[0].status).any()
    assert steps[:, 1].sum() > 0, "no rejected step in the batch: the case would pass vacuously"
    _assert_identical(*free, (n, "free"))
    limit = int(np.median(steps.sum(axis=1)))
    capped = _four(eng, n, theta, y0, t, max_steps=limit, **kw)
    st = _np(capped[0].status)
    assert (st & ST_MAXSTEPS).any() and not st.all()
    _assert_identical(*capped, (n, "capped"))
    ok = st == 0
    assert np.array_equal(_bits(capped[1].sol)[ok], _bits(free[1].sol)[ok])
    assert np.isnan(_np(capped[1].sol)[~ok, -1]).all() and np.isnan(_np(capped[1].metric)[~ok]).all()


def _poisoned(n, nb=48):
    """Replicas with NaN, inf and overflowing parameters among healthy wave mates (the pattern of test_gpu_dist_fast_norm.py)."""
    rng = np.random.default_rng(5300 + n)
    theta = rng.uniform(0.05, 5.0, (nb, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (nb, n + 2))
    last = n - 1
    bad = {
        1: lambda th, y: th.__setitem__(4 + 2, np.nan),                 # NaN site rate
        4: lambda th, y: th.__setitem__(0, np.nan),                     # NaN production rate A
        6: lambda th, y: th.__setitem__(4 + n + last, np.inf),          # inf site degradation on the last site
        9: lambda th, y: th.__setitem__(4 + last, np.inf),              # inf site rate
        13: lambda th, y: th.__setitem__(4 + 1, 1e308),                 # a rate whose products overflow
        14: lambda th, y: (th.__setitem__(4, 1e308), th.__setitem__(5, 1e308)),   # two of them: their sum is inf
        18: lambda th, y: th.__setitem__(3, -1e308),                    # D so negative that the factors overflow
        21: lambda th, y: th.__setitem__(4 + n + 3, 1e200),             # huge but finite: stiff, must solve or fail the same way
        25: lambda th, y: y.__setitem__(2 + last, np.nan),              # NaN initial value in one site row only
        29: lambda th, y: y.__setitem__(1, np.inf),                     # inf initial P
        33: lambda th, y: th.__setitem__(1, -np.inf),                   # -inf mRNA degradation
        38: lambda th, y: th.__setitem__(4 + n, 1e308),                 # 1 + D_1 overflows the factor
        42: lambda th, y: th.__setitem__(2, 1e308),                     # C R overflows in the right-hand side only
    }
    for r, f in bad.items():
        f(theta[r], y0[r])
    return theta, y0, np.array(sorted(bad))


@pytest.mark.parametrize("n", (17, 30, 62))
def test_nonfinite_exit_below_the_step_loop_decides_as_the_loop_did(eng, n):
    from phoskintime_amd._capi import ST_NONFINITE
    theta, y0, bad = _poisoned(n)
    kw = dict(max_steps=400)
    ref, msum, only, flat = _four(eng, n, theta, y0, pm.TIME_POINTS, **kw)
    for name, r in (("sol + sum", msum), ("sol only", only), ("flat only", flat)):
        assert np.array_equal(_np(ref.status), _np(r.status)), (n, name)
        assert np.array_equal(_np(ref.n_steps), _np(r.n_steps)), (n, name)
    for r in (msum, only):
        assert np.array_equal(np.isnan(_np(ref.sol)), np.isnan(_np(r.sol))), n
        assert np.array_equal(_np(ref.sol), _np(r.sol), equal_nan=True), n
    assert np.array_equal(_np(ref.flat), _np(flat.flat), equal_nan=True), n
    st = _np(ref.status)
    for r in (1, 4, 9, 25, 29, 33):
        assert st[r] & ST_NONFINITE, (n, r, st[r])
    failed = st != 0
    assert np.isnan(_np(msum.sol)[failed, -1]).all() and np.isnan(_np(msum.metric)[failed]).all()
    # the healthy wave mates: finite, bit for bit the run-time kernel's, and what they are without the bad replicas beside them
    ok = np.setdiff1d(np.arange(theta.shape[0]), bad)
    assert not st[ok].any() and np.isfinite(_np(msum.sol)[ok]).all()
    assert np.array_equal(_bits(ref.sol)[ok], _bits(msum.sol)[ok]) and np.array_equal(_bits(ref.metric)[ok], _bits(msum.metric)[ok]), n
    clean = eng.solve_ode_batch(pm.DIST, theta[ok], y0[ok], n, pm.TIME_POINTS, want_flat=False, metric="total_signal", kernel="group", **kw)
    assert np.array_equal(_bits(clean.sol), _bits(msum.sol)[ok]) and np.array_equal(_bits(clean.metric), _bits(msum.metric)[ok]), n
    assert np.array_equal(_np(clean.n_steps), _np(msum.n_steps)[ok]), n


@pytest.mark.parametrize("n", (17, 30, 62))
def test_clip_keeps_the_bits_of_the_literal_form(eng, n):
    """Rows that are exact zeros (zero initial value, zero rate), an mRNA row pinned at zero (A = 0, R(0) = 0), and fast-decaying sites
    at a loose tolerance (candidates for a negative value before the clip): the clipped outputs have the run-time kernel's bit
    patterns, and they are its unclipped values with `x < 0 ? 0 : x` applied -- which leaves a -0 and a positive value alone."""
    rng = np.random.default_rng(5400 + n)
    theta = rng.uniform(0.0, 20.0, (B, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (B, n + 2))
    y0[::3, 2 + 1] = 0.0; theta[::3, 4 + 1] = 0.0                         # a site that stays an exact zero
    y0[::5, 2 + n - 1] = 0.0; theta[::5, 4 + n - 1] = 0.0                 # the last site (last lane, last row) too
    y0[::7, 0] = 0.0; theta[::7, 0] = 0.0                                 # R = 0 for ever; P and the sites then decay
    theta[::4, 4 + 2] = 0.0; theta[::4, 4 + n + 2] = 1e4                  # no inflow, fast decay: heads for zero from above
    for kw in (dict(), dict(rtol=1e-3, atol=1e-5)):
        ref, msum, only, flat = _four(eng, n, theta, y0, pm.TIME_POINTS, **kw)
        assert not _np(ref.status).any()
        _assert_identical(ref, msum, only, flat, (n, kw))
        raw = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, clip_nonneg=False, kernel="group", **kw).sol)
        assert (raw == 0.0).any()
        want = np.where(raw < 0.0, 0.0, raw)
        assert np.array_equal(want.view(np.int64), _bits(msum.sol)), (n, kw)
