"""The distributive throughput kernels (csrc/pk_dist_fast.hpp) invert the RPL + 1 independent arrow pivots of a lane, 1 + q B and
1 + q d_j, through shared reciprocals (chain_rcp, csrc/pk_linsolve.hpp): one reciprocal of the product of up to five pivots and three
multiplies per further pivot; one chain up to five pivots, two even ones above.  Held here against the C restatement of the algorithm
(oracle/lrp8_dist.c through oracle/lrp8_cpu.py, which divides by every pivot) at the project's limits -- band error <= 0.02, accepted
steps within 2, statuses equal -- at one size per chain shape, through each specialised kernel and the run-time one, on a lane whose
pivots span many decades, and next to one very large pivot.  The CPU test holds the numpy statement of the chain
(tools/pivot_chain_sensitivity.py) to its error bound."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lrp8_cpu
from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import pivot_chain_sensitivity as pcs  # noqa: E402

BAND, STEPS = 0.02, 2               # the project's limits against the C restatement (tests/test_gpu_parity.py)
RTOL, ATOL = 1e-6, 1e-8
T = pm.TIME_POINTS                  # the 14-point grid
B = 40                              # n <= 32: sixteen replicas per wave, two whole waves and half a one; above: five waves of eight
# n -> (lanes, rows per lane, chain lengths): every chain shape of the two launch tables
SHAPES = {4: (4, 1, (2, 0)), 16: (4, 4, (5, 0)), 20: (4, 5, (3, 3)), 30: (4, 8, (5, 4)), 40: (8, 5, (3, 3)), 62: (8, 8, (5, 4))}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _np(x):
    return x.detach().cpu().numpy()


def _theta(n, nb, seed):
    return np.random.default_rng(seed).uniform(0.0, 20.0, (nb, pm.n_params(pm.DIST, n)))


# ---------------------------------------------------------------- CPU: the chain against 1 / x
def test_split_rule():
    for n, (G, RPL, chains) in SHAPES.items():
        assert G * RPL >= n and pcs.chain_split(RPL) == chains, n
    assert pcs.chain_split(6) == (4, 3) and pcs.chain_split(7) == (4, 4) and pcs.chain_split(2) == (3, 0) and pcs.chain_split(3) == (4, 0)


@pytest.mark.parametrize("m", (2, 3, 4, 5))
def test_chain_is_within_its_bound_of_the_reciprocal(m):
    """1e5 factor sets, log-uniform over 1 ... 1e12.  A reciprocal of the chain is 1 / a_i times at most 2 m - 1 roundings (the multiplies
    of the prefix products from a_i on, the reciprocal, the multiplies of the walk back down to a_i), and 1 / x of numpy is rounded
    once: 2 m half-ulps between them, inside the stated bound 2 (m + 1) 2^-53."""
    a = 10.0 ** np.random.default_rng(8000 + m).uniform(0.0, 12.0, (100000, m))
    inv, ref = pcs.chain_inverse(a), 1.0 / a
    rel = float(np.max(np.abs(inv - ref) / ref))
    print("m", m, "largest relative difference", rel, "bound", 2 * (m + 1) * 2.0 ** -53)
    assert rel <= 2 * (m + 1) * 2.0 ** -53
    # one factor of 1e200 beside ordinary ones is inside the range; five of 1e62 are not
    big = np.array([3.0, 1e200, 7.0, 1e4, 11.0])[:m]
    assert np.max(np.abs(pcs.chain_inverse(big) * big - 1.0)) <= 2 * (m + 1) * 2.0 ** -53
    with np.errstate(all="ignore"):
        assert not (np.abs(pcs.chain_inverse(np.full(5, 1e62)) * 1e62 - 1.0) < 0.5).any()


# ---------------------------------------------------------------- parity against the oracle at every chain shape
_ORACLE = {}


def _oracle(n):
    """The C restatement on the shared batch of size n: computed once, never written to."""
    if n not in _ORACLE:
        theta = _theta(n, B, 7100 + n)
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), T, rtol=RTOL, atol=ATOL)
        assert not st.any()
        for a in (theta, sol, ns):
            a.setflags(write=False)
        _ORACLE[n] = (theta, sol, ns)
    return _ORACLE[n]


def _check(r, ref, ns_ref, what):
    assert not _np(r.status).any(), what
    steps = _np(r.n_steps)
    d = int(np.abs(steps[:, 0] - ns_ref[:, 0]).max())
    e = pm.band_error(_np(r.sol), ref, RTOL, ATOL) if r.sol is not None else None
    print(what, "accepted steps differ by at most", d, "band error", e)
    assert d <= STEPS, (what, "accepted steps", d)
    if e is not None:
        assert e <= BAND, (what, "band error", e)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_parity_against_the_c_restatement(eng, n):
    theta, raw, ns = _oracle(n)
    y0 = np.ones(n + 2)
    clipped = np.clip(raw, 0.0, None)
    kw = dict(kernel="group", rtol=RTOL, atol=ATOL)
    # DistSolSum: trajectories and the running-sum metric
    r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **kw)
    _check(r, clipped, ns, (n, "sol + sum"))
    width = ATOL + RTOL * np.abs(clipped)
    want = clipped.sum(axis=(1, 2))
    assert (np.abs(_np(r.metric) - want) <= BAND * width.sum(axis=(1, 2)) + 1e-13 * np.abs(want)).all(), (n, "total_signal")
    # DistSolOnly: trajectories alone
    _check(eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **kw), clipped, ns, (n, "sol only"))
    # DistFlatOnly: the flat observable vector alone
    r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **kw)
    _check(r, None, ns, (n, "flat only"))
    want = np.stack([pm.flatten_observables(pm.DIST, c, n) for c in clipped])
    e = pm.band_error(_np(r.flat), want, RTOL, ATOL)
    assert e <= BAND, (n, "flat only", e)
    # DistAny: trajectories as integrated (no clip)
    _check(eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, clip_nonneg=False, **kw), raw, ns, (n, "raw, run-time kernel"))


# ---------------------------------------------------------------- prefix products that run through many decades
@pytest.mark.gpu
def test_pivots_of_very_different_size_in_one_lane(eng):
    """n = 30 (4 lanes x 8 rows).  Replica 5 has, in every one of its lanes, the site degradations 1e-3 ... 1e6 log-spaced over the
    lane's eight rows (row j of lane l is site l + 4 j), so the pivots 1 + q (1 + D_i) of a chain differ by up to six decades and its
    prefix products run through twelve.  Its wave mates are ordinary.  The C restatement solves the full 1e-3 ... 1e6 spread with
    status 0 in 65 accepted steps (default budget 100 000; its mates take 36 - 41), so the whole spread is run."""
    n, odd = 30, 5
    theta = _theta(n, 16, 7200)
    theta[odd, 4 + n:4 + 2 * n] = np.logspace(-3.0, 6.0, 8)[np.arange(n) // 4]
    y0 = np.ones(n + 2)
    raw, st, ns = lrp8_cpu.solve_batch(theta, n, y0, T, rtol=RTOL, atol=ATOL)
    assert not st.any()
    kw = dict(kernel="group", rtol=RTOL, atol=ATOL, want_flat=False)
    for what, r, ref in (("sol + sum", eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric="total_signal", **kw), np.clip(raw, 0.0, None)),
                         ("raw, run-time kernel", eng.solve_ode_batch(pm.DIST, theta, y0, n, T, clip_nonneg=False, **kw), raw)):
        _check(r, ref, ns, what)
        e = pm.band_error(_np(r.sol)[odd], ref[odd], RTOL, ATOL)
        print(what, "replica", odd, "band error", e, "steps", _np(r.n_steps)[odd], "restatement", ns[odd])
        assert e <= BAND


# ---------------------------------------------------------------- one very large pivot beside ordinary ones
@pytest.mark.gpu
@pytest.mark.parametrize("big, empty", ((1e55, True), (1e14, False)))
def test_one_very_large_pivot(eng, big, empty):
    """n = 30, replica 5, site 9 (lane 1, row 2: inside the five-pivot chain).  Checked on the CPU when this test was written: with every
    initial value 1 the C restatement returns status 0 up to D_9 = 1e15 (68 accepted steps) and PK_ST_HMIN from 1e16 on -- its first
    step, 0.01 / D, falls under the smallest step it takes, 1e-17, and at 1e15 it equals that limit to fourteen digits, which tests the
    rounding of the initial step and not the pivots: that start runs at 1e14 (67 accepted steps).  With site 9 starting empty the
    restatement returns status 0 at every power of ten tried up to 1e55 (44 accepted steps), close to the 1e61 per pivot up to which
    the product of a five-pivot chain stays finite.  Both are run.  The GPU returns the restatement's status, stays inside the
    band on that replica, and its healthy wave mates have the bits of a run in which replica 5 is ordinary."""
    n, odd, site = 30, 5, 9
    plain = _theta(n, 16, 7300)
    theta = plain.copy()
    theta[odd, 4 + n + site] = big
    y0 = np.ones((16, n + 2))
    if empty:
        y0[odd, 2 + site] = 0.0
    raw, st_c, ns = lrp8_cpu.solve_batch(theta[odd:odd + 1], n, y0[odd], T, rtol=RTOL, atol=ATOL)
    assert st_c[0] == 0
    mates = np.setdiff1d(np.arange(16), [odd])
    kw = dict(kernel="group", rtol=RTOL, atol=ATOL, want_flat=False)
    for what, extra, ref in (("sol + sum", dict(metric="total_signal"), np.clip(raw[0], 0.0, None)), ("raw, run-time kernel", dict(clip_nonneg=False), raw[0])):
        r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, **extra, **kw)
        sol, st, steps = _np(r.sol).copy(), _np(r.status).copy(), _np(r.n_steps).copy()
        assert st[odd] == st_c[0] and not st.any(), (what, st)
        e = pm.band_error(sol[odd], ref, RTOL, ATOL)
        print(what, "D = %g" % big, "band error", e, "steps", steps[odd], "restatement", ns[0])
        assert e <= BAND and abs(int(steps[odd, 0]) - int(ns[0, 0])) <= STEPS, (what, e, steps[odd])
        q = eng.solve_ode_batch(pm.DIST, plain, y0, n, T, **extra, **kw)
        assert np.array_equal(sol[mates].view(np.int64), _np(q.sol)[mates].view(np.int64)), (what, "wave mates")
        assert np.array_equal(steps[mates], _np(q.n_steps)[mates]), (what, "wave mates' steps")
