"""The LRP12 launch table of the distributive throughput kernel (csrc/pk_inst_dist_fast12.hip) runs a size in the RESIDENT layout
(csrc/pk_dist_fast.hpp) exactly when its G x RPL slots hold the whole state, G * RPL >= n + 2: R in slot 0 (lane 0, row 0), P in slot 1
(lane 1, row 0), site i in slot i + 2, nothing shadowed.  Held here against the C restatement of the algorithm (oracle/lrp8_dist.c
through oracle/lrp8_cpu.py) at the project's limits -- band error <= 0.02, accepted steps within 2 -- at resident sizes of every shape
(no spare slot left, one idle slot, 4 and 8 lanes) and at the neighbours that stay shadowed; the specialised kernels against the
run-time one bit for bit; the rows that share lanes with R and P; rejected first steps (R and P come back from their parked slots);
and non-finite inputs in the R / P slots and the last site.  The CPU test holds the numpy statement of the resident step
(tools/inslot_sensitivity.py) to the shadowed port and to the C restatement."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lrp8_cpu
from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import inslot_sensitivity as ins  # noqa: E402
import test_gpu_dist_fast_sitesum as ts  # noqa: E402  (the numpy port of the C restatement with an initial step)

BAND, STEPS = 0.02, 2               # the project's limits against the C restatement (tests/test_gpu_parity.py)
RTOL, ATOL = 1e-6, 1e-8
T = pm.TIME_POINTS                  # the 14-point grid
B = 48
RESIDENT = (2, 6, 13, 14, 29, 30, 33, 38, 62)      # 4 x 1 full; 4 x 2; 4 x 4 with one idle slot and full; 4 x 8 with one idle slot and full; 8 x 5; 8 x 5 full; 8 x 8 full
SHADOWED = (4, 31, 32, 39, 40)                     # G * RPL < n + 2: these stay shadowed
BITWISE = (2, 14, 30, 38, 62)
KW = dict(kernel="group", rtol=RTOL, atol=ATOL)


def _layout(n):
    """(G, RPL) of the LRP12 table."""
    return (4, (n + 3) // 4) if n <= 32 else (8, (n + 7) // 8)


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
    return _np(x).view(np.int64) if _np(x).dtype == np.float64 else _np(x)


def _theta(n, nb, seed):
    return np.random.default_rng(seed).uniform(0.0, 20.0, (nb, pm.n_params(pm.DIST, n)))


def _band_rows(sol, ref):
    return pm.band_error(sol, ref, RTOL, ATOL)


# ---------------------------------------------------------------- CPU: the selection rule and the numpy port
def test_selection_rule():
    res = [n for n in range(1, 65) if ins.resident_fits(n, *_layout(n))]
    assert res == [n for n in range(1, 31) if n % 4 in (1, 2)] + [n for b in (33, 41, 49, 57) for n in range(b, b + 6)]
    assert all(n in res for n in RESIDENT) and not any(n in res for n in SHADOWED)


def test_resident_port_against_the_shadowed_port_and_the_c_restatement():
    """n = 30 on 4 x 8, the benchmark's parameter distribution, 24 replicas: the resident step moves the trajectories of the shadowed port
    by rounding only (the two rounding-level changes before this one measured 1.9e-4 and 6.7e-3 band widths on the same batch; the limit
    is the project's 0.02), and takes the C restatement's steps."""
    shift, moved, vs_c, dsteps = ins.compare(24)
    print("band shift resident vs shadowed: max", max(shift), "median", float(np.median(shift)), "replicas with another step count", moved,
          "| vs the C restatement: band", vs_c, "accepted steps differ by at most", dsteps)
    assert max(shift) <= BAND and vs_c <= BAND and dsteps <= STEPS


# ---------------------------------------------------------------- parity against the oracle, every output class
_ORACLE = {}


def _oracle(n):
    """The C restatement on the shared batch of size n: computed once, never written to."""
    if n not in _ORACLE:
        theta = _theta(n, B, 8100 + n)
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
    e = _band_rows(_np(r.sol), ref) if r.sol is not None else None
    print(what, "accepted steps differ by at most", d, "band error", e)
    assert d <= STEPS, (what, "accepted steps", d)
    if e is not None:
        assert e <= BAND, (what, "band error", e)


def _four_classes(eng, theta, y0, n, raw, ns, tag, **extra):
    """sol + total_signal, sol only, flat only and the raw run-time kernel against the restatement's trajectories `raw`."""
    clipped = np.clip(raw, 0.0, None)
    kw = dict(KW, **extra)
    out = {}
    r = out["sol + sum"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **kw)
    _check(r, clipped, ns, (n, tag, "sol + sum"))
    width = ATOL + RTOL * np.abs(clipped)
    want = clipped.sum(axis=(1, 2))
    assert (np.abs(_np(r.metric) - want) <= BAND * width.sum(axis=(1, 2)) + 1e-13 * np.abs(want)).all(), (n, tag, "total_signal")
    r = out["sol only"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **kw)
    _check(r, clipped, ns, (n, tag, "sol only"))
    r = out["flat only"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **kw)
    _check(r, None, ns, (n, tag, "flat only"))
    want = np.stack([pm.flatten_observables(pm.DIST, c, n) for c in clipped])
    e = pm.band_error(_np(r.flat), want, RTOL, ATOL)
    print((n, tag, "flat only"), "band error", e)
    assert e <= BAND, (n, tag, "flat only", e)
    r = out["raw"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, clip_nonneg=False, **kw)
    _check(r, raw, ns, (n, tag, "raw, run-time kernel"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", RESIDENT + SHADOWED)
def test_parity_against_the_c_restatement(eng, n):
    theta, raw, ns = _oracle(n)
    _four_classes(eng, theta, np.ones(n + 2), n, raw, ns, "resident" if n in RESIDENT else "shadowed")


# ---------------------------------------------------------------- the specialised kernels against DistAny, bit for bit
def _inputs(n, nb, seed=0):
    rng = np.random.default_rng(1000 * n + nb + seed)
    return rng.uniform(0.05, 5.0, (nb, pm.n_params(pm.DIST, n))), rng.uniform(0.5, 2.0, (nb, n + 2))


def _flat_of(sol):
    """The flat observable vector laid out from trajectories [B, T, S]: R from the sixth time point on, P, then every site, time-major."""
    nb, nt, S = sol.shape
    t5 = max(nt - 5, 0)
    return np.concatenate([sol[:, 5:, 0].reshape(nb, t5), sol[:, :, 1], sol[:, :, 2:].transpose(0, 2, 1).reshape(nb, (S - 2) * nt)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BITWISE)
def test_specialised_kernels_have_the_bits_of_the_run_time_kernel(eng, n):
    """sol alone (DistSolOnly), flat alone (DistFlatOnly), sol + total_signal (DistSolSum) against sol + flat (+ total_signal), which runs
    on DistAny: sol, flat, metric, status and n_steps through their integer views; one replica and a partial wave; one, two and fourteen
    output times (at one and two, R has no entry in the flat vector)."""
    for nb in (1, 17):
        theta, y0 = _inputs(n, nb)
        for nt in (1, 2, 14):
            t = T[:nt]
            a = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, **KW)
            c = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_sol=False, **KW)
            d = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, want_flat=False, metric="total_signal", **KW)
            ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, t, metric="total_signal", **KW)
            what = (n, nb, nt)
            assert _np(ref.sol).shape == (nb, nt, n + 2) and np.isfinite(_np(ref.sol)).all() and not _np(ref.status).any(), what
            assert np.array_equal(_np(ref.sol)[:, 0], np.clip(y0, 0.0, None)), what
            assert np.array_equal(_bits(a.sol), _bits(ref.sol)) and np.array_equal(_bits(d.sol), _bits(ref.sol)), what
            assert np.array_equal(_bits(c.flat), _bits(ref.flat)), what
            assert np.array_equal(_bits(d.metric), _bits(ref.metric)), what
            for other in (a, c, d):
                assert np.array_equal(_np(other.status), _np(ref.status)) and np.array_equal(_np(other.n_steps), _np(ref.n_steps)), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", BITWISE)
def test_normalize_and_every_metric(eng, n):
    """normalize runs on DistAny and indexes y0 by slot: its output is the clipped output of the specialised kernel times 1 / y0, bit for
    bit, and its flat vector is laid out from it.  Every metric with trajectories (DistSolSum for the running-sum class, DistAny for the
    full-moment class) and without (DistAny): the same scalar bit for bit, and the one the oracle computes from the trajectories."""
    theta, y0 = _inputs(n, 17, seed=3)
    on = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **KW).sol)
    norm = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, normalize=True, **KW)
    assert np.array_equal(_np(norm.sol).view(np.int64), (on * (1.0 / y0)[:, None, :]).view(np.int64)), n
    assert np.array_equal(_np(norm.flat).view(np.int64), _flat_of(_np(norm.sol)).view(np.int64)), n
    for metric in pm.METRICS:
        a = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric=metric, **KW)
        b = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, want_flat=False, metric=metric, **KW)
        c = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric=metric, **KW)
        assert np.array_equal(_bits(a.metric), _bits(b.metric)) and np.array_equal(_bits(a.metric), _bits(c.metric)), (n, metric)
        assert np.array_equal(_bits(a.sol), _bits(c.sol)) and np.array_equal(_np(a.sol), on), (n, metric)
        for r in (0, 8, 16):
            ref = pm.compute_Y(on[r], n, metric)
            assert abs(_np(a.metric)[r] - ref) <= 1e-9 * max(1.0, abs(ref)), (n, metric, r)


# ---------------------------------------------------------------- flat against sol
@pytest.mark.gpu
@pytest.mark.parametrize("n", BITWISE)
def test_flat_is_the_flattened_sol_and_the_total_is_the_sum_of_the_rows(eng, n):
    theta, y0 = _inputs(n, 17, seed=5)
    sol = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **KW).sol)
    flat = _np(eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **KW).flat)
    want = np.stack([pm.flatten_observables(pm.DIST, s, n) for s in sol])
    assert flat.shape == want.shape and np.array_equal(flat.view(np.int64), want.view(np.int64)), n
    r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **KW)
    assert np.array_equal(_np(r.sol).view(np.int64), sol.view(np.int64)), n
    tot = np.array([float(np.sum(s)) for s in sol])
    assert (np.abs(_np(r.metric) - tot) <= 1e-13 * np.abs(tot)).all(), (n, np.abs(_np(r.metric) - tot).max())


# ---------------------------------------------------------------- the rows that share lanes with R and P, and the last slot
def _corners(n, seed):
    """Four replicas per corner: (name, theta [4, P], y0 [S])."""
    S = n + 2
    out = []
    for i, name in enumerate(("C = 0", "B = 0", "A = 0", "y0[R] = 0", "y0[P] = 0", "all site rates 0", "site 0 alone", "site n - 1 alone")):
        th = _theta(n, 4, seed + i)
        y0 = np.ones(S)
        if name == "C = 0":
            th[:, 2] = 0.0
        elif name == "B = 0":
            th[:, 1] = 0.0
        elif name == "A = 0":
            th[:, 0] = 0.0
        elif name == "y0[R] = 0":
            y0[0] = 0.0
        elif name == "y0[P] = 0":
            y0[1] = 0.0
        elif name == "all site rates 0":
            th[:, 4:4 + n] = 0.0
        elif name == "site 0 alone":
            th[:, 5:4 + n] = 0.0
        else:
            th[:, 4:3 + n] = 0.0
        out.append((name, th, y0))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 38))
def test_row_role_corners(eng, n):
    """Site 0 and site 1 sit in row 1 of lanes 0 and 1 at n = 30 (slots 2, 3 are row 0 of lanes 2, 3) and site n - 1 in the last slot; a zero
    C, B or A removes a term of row 0 in lane 0 or 1.  One batch of 32 replicas, initial values per replica."""
    cases = _corners(n, 8300 + 10 * n)
    theta = np.concatenate([c[1] for c in cases])
    y0 = np.concatenate([np.tile(c[2], (4, 1)) for c in cases])
    raw = np.empty((theta.shape[0], len(T), n + 2)); ns = np.empty((theta.shape[0], 2), int)
    for i, (name, th, y) in enumerate(cases):
        sol, st, steps = lrp8_cpu.solve_batch(th, n, y, T, rtol=RTOL, atol=ATOL)
        assert not st.any(), name
        raw[4 * i:4 * i + 4], ns[4 * i:4 * i + 4] = sol, steps
    out = _four_classes(eng, theta, y0, n, raw, ns, "corners")
    for i, (name, _, _) in enumerate(cases):
        e = _band_rows(_np(out["raw"].sol)[4 * i:4 * i + 4], raw[4 * i:4 * i + 4])
        print(n, name, "band error", e)
        assert e <= BAND, (n, name, e)


# ---------------------------------------------------------------- a rejected first step: R and P come back from their slots
@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 38))
def test_forced_first_reject(eng, n):
    nb = 32
    theta = _theta(n, nb, 8400 + n)
    y0 = np.ones(n + 2)
    # the initial step is chosen on the CPU: the first value at which the restatement itself rejects a step of every replica
    for h0 in (1.0, 10.0, 100.0):
        raw, st, ns = ts._port_batch(theta, n, y0, h0)
        if ns[:, 1].min() >= 1:
            break
    assert ns[:, 1].min() >= 1 and not st.any(), "no initial step makes the restatement reject in every replica"
    out = _four_classes(eng, theta, y0, n, raw, ns, "h0 = %g" % h0, h0=h0)
    first = out["raw"]
    for what, r in out.items():
        steps = _np(r.n_steps)
        assert steps[:, 1].min() >= 1, (n, what, "a replica rejected nothing")
        assert np.abs(steps[:, 1] - ns[:, 1]).max() <= STEPS, (n, what, "rejected steps")
        # identical fate across the four output classes
        assert np.array_equal(steps, _np(first.n_steps)) and np.array_equal(_np(r.status), _np(first.status)), (n, what)
    clipped = np.where(_np(first.sol) < 0.0, 0.0, _np(first.sol))
    assert np.array_equal(_bits(out["sol only"].sol), clipped.view(np.int64)) and np.array_equal(_bits(out["sol + sum"].sol), clipped.view(np.int64))
    assert np.array_equal(_bits(out["flat only"].flat), _flat_of(clipped).view(np.int64))


# ---------------------------------------------------------------- non-finite inputs in the R / P slots and the last site
@pytest.mark.gpu
@pytest.mark.parametrize("what", ("NaN A", "NaN C", "-inf B", "inf y0[P]", "NaN y0 in the last site"))
def test_nonfinite_inputs(eng, what):
    """n = 30, one wave of sixteen replicas, replica 5 spoiled.  It ends ST_NONFINITE with NaN rows from its failing landing on and a NaN
    metric, status and step counts equal DistAny's, and its fifteen wave mates have the bits of a run in which it is ordinary."""
    from phoskintime_amd._capi import ST_NONFINITE
    n, nb, odd = 30, 16, 5
    plain_th = _theta(n, nb, 8500)
    plain_y0 = np.ones((nb, n + 2))
    theta, y0 = plain_th.copy(), plain_y0.copy()
    if what == "NaN A":
        theta[odd, 0] = np.nan
    elif what == "NaN C":
        theta[odd, 2] = np.nan
    elif what == "-inf B":
        theta[odd, 1] = -np.inf
    elif what == "inf y0[P]":
        y0[odd, 1] = np.inf
    else:
        y0[odd, n + 1] = np.nan
    mates = np.setdiff1d(np.arange(nb), [odd])
    kw = dict(KW, want_flat=False)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric="total_signal", **KW)                     # sol + flat: DistAny
    for name, extra in (("sol + sum", dict(metric="total_signal")), ("sol only", dict())):
        r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, **extra, **kw)
        q = eng.solve_ode_batch(pm.DIST, plain_th, plain_y0, n, T, **extra, **kw)
        st, sol, steps = _np(r.status), _np(r.sol), _np(r.n_steps)
        print(what, name, "status", st[odd], "steps", steps[odd])
        assert st[odd] == ST_NONFINITE and not st[mates].any(), (what, name, st)
        assert np.array_equal(st, _np(ref.status)) and np.array_equal(steps, _np(ref.n_steps)), (what, name, "against DistAny")
        assert np.isnan(sol[odd, 1:]).all(), (what, name, "NaN rows from the failing landing on")
        row0 = np.where(y0[odd] < 0.0, 0.0, y0[odd])
        assert np.array_equal(sol[odd, 0].view(np.int64), row0.view(np.int64)), (what, name, "row 0 is the initial state")
        if r.metric is not None:
            assert np.isnan(_np(r.metric)[odd]) and np.array_equal(_bits(r.metric)[mates], _bits(q.metric)[mates]), (what, name, "metric")
        assert np.array_equal(sol[mates].view(np.int64), _np(q.sol)[mates].view(np.int64)), (what, name, "wave mates")
        assert np.array_equal(steps[mates], _np(q.n_steps)[mates]) and not _np(q.status).any(), (what, name, "wave mates' steps")
        assert np.array_equal(sol.view(np.int64), _np(ref.sol).view(np.int64)), (what, name, "sol against DistAny")
    f = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **KW)
    assert np.array_equal(_np(f.status), _np(ref.status)) and np.array_equal(_np(f.n_steps), _np(ref.n_steps)), (what, "flat only")
    assert np.array_equal(_bits(f.flat), _bits(ref.flat)), (what, "flat only against DistAny")
