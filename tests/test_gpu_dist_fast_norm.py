"""The error norm of the LRP12 step loop in the specialised distributive kernels (csrc/pk_dist_fast.hpp: err_norm) takes the maximum of the
per-row ratios with v_max_f64, which drops a NaN, and surfaces a NaN ratio separately as +inf.  The run-time kernel (DistAny) keeps the
NaN-propagating maximum of the parent (group_max).  On replicas whose parameters, rates or initial values are non-finite or overflow, both
must take the same path: same status bits, same step counts, NaN rows from the same landing on, identical finite rows before it -- and the
healthy replicas that share a wave with them must not notice."""
import numpy as np
import pytest

from oracle import protein_models as pm

pytestmark = pytest.mark.gpu

SIZES = (14, 30, 32, 40)            # 4x4 in registers, 4x8 parked with two idle rows, 4x8 full, 8x5 parked (three DPP levels)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _np(x):
    return x.detach().cpu().numpy()


def _poisoned(n, B=40):
    """theta [B, P] (A, B, C, D, S_1..n, D_1..n) and y0 [B, n + 2] with a bad replica every few rows, healthy ones in between."""
    rng = np.random.default_rng(4200 + n)
    theta = rng.uniform(0.05, 5.0, (B, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (B, n + 2))
    last = n - 1
    bad = {
        1: lambda th, y: th.__setitem__(4 + 2, np.nan),                 # NaN site rate
        4: lambda th, y: th.__setitem__(0, np.nan),                     # NaN production rate A
        6: lambda th, y: th.__setitem__(4 + n + last, np.inf),          # inf site degradation on the last site (last lane / last row)
        9: lambda th, y: th.__setitem__(4 + last, np.inf),              # inf site rate
        13: lambda th, y: th.__setitem__(4 + 1, 1e308),                 # a rate whose products overflow
        14: lambda th, y: (th.__setitem__(4, 1e308), th.__setitem__(5, 1e308)),   # two of them: their sum is inf
        18: lambda th, y: th.__setitem__(3, -1e308),                    # D so negative that the factors overflow
        21: lambda th, y: th.__setitem__(4 + n + 3, 1e200),             # huge but finite: stiff, must still solve or fail the same way
        25: lambda th, y: y.__setitem__(2 + last, np.nan),              # NaN initial value in one site row only
        29: lambda th, y: y.__setitem__(1, np.inf),                     # inf initial P
        33: lambda th, y: th.__setitem__(1, -np.inf),                   # -inf mRNA degradation
        38: lambda th, y: th.__setitem__(4 + n, 1e308),                 # 1 + D_1 overflows the factor
    }
    for r, f in bad.items():
        f(theta[r], y0[r])
    return theta, y0, np.array(sorted(bad))


def _same_fate(a, b, what):
    sa, sb = _np(a.sol), _np(b.sol)
    assert np.array_equal(_np(a.status), _np(b.status)), what
    assert np.array_equal(_np(a.n_steps), _np(b.n_steps)), what
    assert np.array_equal(np.isnan(sa), np.isnan(sb)), what
    assert np.array_equal(sa, sb, equal_nan=True), what


@pytest.mark.parametrize("n", SIZES)
def test_nonfinite_parameters_take_the_same_path_as_the_nan_propagating_norm(eng, n):
    theta, y0, bad = _poisoned(n)
    t = pm.TIME_POINTS
    kw = dict(max_steps=400)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, **kw)                                    # sol + flat: DistAny, group_max
    only = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, **kw)                  # DistSolOnly, err_norm
    msum = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, metric="total_signal", **kw)   # DistSolSum, err_norm
    flat = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_sol=False, **kw)                   # DistFlatOnly, err_norm
    _same_fate(ref, only, (n, "sol only"))
    _same_fate(ref, msum, (n, "sol + sum"))
    assert np.array_equal(_np(ref.status), _np(flat.status)) and np.array_equal(_np(ref.n_steps), _np(flat.n_steps)), n
    assert np.array_equal(_np(ref.flat), _np(flat.flat), equal_nan=True), n
    st = _np(ref.status)
    from phoskintime_amd._capi import ST_NONFINITE
    # the replicas with a NaN / inf parameter fail as non-finite; every failed replica ends in NaN rows and a NaN metric
    for r in (1, 4, 9, 25, 29, 33):
        assert st[r] & ST_NONFINITE, (n, r, st[r])
    failed = st != 0
    assert np.isnan(_np(ref.sol)[failed, -1]).all() and np.isnan(_np(msum.metric)[failed]).all()
    # healthy wave mates: untouched, bit for bit, by what fails beside them
    ok = np.setdiff1d(np.arange(theta.shape[0]), bad)
    assert not st[ok].any()
    clean_theta, clean_y0 = theta[ok], y0[ok]
    clean = eng.solve_ode_batch(pm.DIST, clean_theta, clean_y0, n, t, want_flat=False, metric="total_signal", **kw)
    assert np.array_equal(_np(clean.sol), _np(msum.sol)[ok]) and np.array_equal(_np(clean.metric), _np(msum.metric)[ok]), n
    assert np.array_equal(_np(clean.n_steps), _np(msum.n_steps)[ok]), n


@pytest.mark.parametrize("n", (30, 32))
def test_zero_absolute_tolerance_keeps_its_fate(eng, n):
    """atol = 0: a row that is exactly zero with a zero error has the ratio 0 * inf = NaN -- a NaN born in the norm itself, in one row, with
    every input finite (the idle rows of a padded layout; at n = 32 there are none).  Both norms must see it."""
    rng = np.random.default_rng(77 + n)
    theta = rng.uniform(0.05, 5.0, (19, pm.n_params(pm.DIST, n)))
    y0 = rng.uniform(0.5, 2.0, (19, n + 2))
    y0[3, 2 + 5] = 0.0; theta[3, 4 + 5] = 0.0                                                    # a real site that stays exactly zero
    kw = dict(rtol=1e-6, atol=0.0, max_steps=300)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, **kw)
    only = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, **kw)
    msum = eng.solve_ode_batch(pm.DIST, theta, y0, n, pm.TIME_POINTS, want_flat=False, metric="total_signal", **kw)
    _same_fate(ref, only, n)
    _same_fate(ref, msum, n)
    assert _np(ref.status)[3] != 0
