"""The step loop of the distributive throughput kernels (csrc/pk_dist_fast.hpp) forms its first resolvent stage without a right-hand
side.  f(y) = J y + b is affine (b = A in row R, zero elsewhere) and J = (I - M) / q with M = I - q J, q = gamma h, so

    M^-1 h f(y) = (1 / gamma) (M^-1 (y + q b) - y):

the same solve() on the state itself with q A added to row R, one subtraction per row, and 1 / gamma folded into the tableau weights.
The C restatement (oracle/lrp8_dist.c through oracle/lrp8_cpu.py) keeps its direct right-hand side and is the yardstick, at the
project's limits -- band error <= 0.02, accepted steps within 2, status 0: resident and shadowed layouts, LRP12 / LRP8 / RODAS4, the
specialised kernels against the run-time one bit for bit (in both layouts), first steps so small that the subtraction cancels nearly
everything, forced rejects, and non-finite inputs (the loop carries no site sum any more; the non-finite test forms it from the
accepted rows).  The CPU test holds the identity itself in numpy.

RODAS4 has no C restatement (oracle/lrp8_dist.c states LRP12 and LRP8).  Its independent reference is the generic solve_kernel
(linsolve = "structured"), which this change does not touch and which forms the right-hand side directly: same method, same
controller, held at the same limits (band error <= 0.02, accepted and rejected steps within 2)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lrp8_cpu
from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_dist_fast_sitesum as ts  # noqa: E402  (the numpy port of the C restatement with an initial step)

ROOT = Path(__file__).resolve().parents[1]
BAND, STEPS = 0.02, 2               # the project's limits against the C restatement (tests/test_gpu_parity.py)
RTOL, ATOL = 1e-6, 1e-8
T = pm.TIME_POINTS                  # the 14-point grid
B = 64
RESIDENT = (2, 14, 30, 38)          # 4 x 1, 4 x 4, 4 x 8 parked, 8 x 5 parked
SHADOWED = (3, 28, 32)              # their neighbours with G * RPL < n + 2
KW = dict(kernel="group", rtol=RTOL, atol=ATOL)
U = 2.0 ** -53


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


def _theta(n, nb, seed, hi=20.0):
    return np.random.default_rng(seed).uniform(0.0, hi, (nb, pm.n_params(pm.DIST, n)))


# ---------------------------------------------------------------- CPU: the identity in numpy
def _arrow(r, q, th, n):
    """M^-1 r for a batch [nb, n + 2], the arrow elimination of the C restatement in numpy."""
    Bc, Cc, D = th[:, 1], th[:, 2], th[:, 3]
    Sr, dg = th[:, 4:4 + n], 1.0 + th[:, 4 + n:4 + 2 * n]
    w = 1.0 / (1.0 + q[:, None] * dg)
    xR = r[:, 0] / (1.0 + q * Bc)
    tt = r[:, 2:] * w
    cw = q[:, None] * Sr * w
    xP = (r[:, 1] + q * (Cc * xR + tt.sum(axis=1))) / (1.0 + q * (D + Sr.sum(axis=1) - cw.sum(axis=1)))
    return np.concatenate([xR[:, None], xP[:, None], tt + cw * xP[:, None]], axis=1)


def test_the_identity_in_numpy():
    """gamma solve(h f(y)) against solve(y + q b) - y on 1e4 random factor sets: n = 30, theta ~ U(0, 20), y ~ U(0, 2), q = gamma h
    log-uniform over 1e-12 .. 1e2.

    Tolerance per entry: K 2^-53 Y with K = 4 (n + 12) = 168 and Y = max(|y|, |M^-1 (y + q b)|) in the maximum norm.  (The issue
    writes the bound as a multiple of 2^-53 |y| / min(1, q |J|); what the derivation yields is an absolute error that does not grow as q
    shrinks, so the division is dropped -- the asserted bound is the tighter one -- and Y takes the solved vector beside |y| because
    that is what the rounding of the solve is relative to; the two differ by at most q A, and M^-1 does not enlarge a vector by more
    than the factor the sum below allows for.)
    Where K comes from.  Side one, solve(y + q b) - y: every term of the solve is non-negative (theta, y >= 0), nothing cancels, and
    an entry carries the relative rounding of its longest chain: the n-term site sum (n - 1 additions) and at most eleven further
    operations (pivot, reciprocal, t_i, q S_i w_i, the denominator's sum and division, C x_R, the two additions and the multiply of
    x_P, the row's own multiply-add): (n + 10) 2^-53 Y.  The subtraction rounds once more, a result no larger than Y: + 1.
    Side two, gamma solve(h f(y)): f is rounded with (n + 3) 2^-53 (|J| |y| + b) per entry (row P has n + 2 terms of mixed sign), and
    the solve adds its own (n + 10) 2^-53 relative to its non-negative majorant M^-1 q (|J| |y| + b).  That majorant is taken as at
    most 2 Y: q |J| = 2 q D - (M - I) with D the magnitude of J's diagonal, so M^-1 q |J| y = 2 M^-1 q D y - y + M^-1 y, which is
    below 2 Y where q D <= 1 and, for larger q, as long as M^-1 q D y stays of the size of y (the stage is then y itself to leading
    order).  This step is an estimate, not a proof; the factor 2 is the allowance named above.  Side two: 2 (n + 3) + (n + 10).
    Sum: (n + 10) + 1 + 2 (n + 3) + (n + 10) = 4 n + 27 <= 4 (n + 12) = K."""
    n, nb, gam = 30, 10000, 0.16
    rng = np.random.default_rng(20261)
    th = rng.uniform(0.0, 20.0, (nb, 4 + 2 * n))
    y = rng.uniform(0.0, 2.0, (nb, n + 2))
    q = 10.0 ** rng.uniform(-12.0, 2.0, nb)
    h = q / gam
    A, Bc, Cc, D = th[:, 0], th[:, 1], th[:, 2], th[:, 3]
    Sr, dg = th[:, 4:4 + n], 1.0 + th[:, 4 + n:4 + 2 * n]
    Dsum = D + Sr.sum(axis=1)
    f = np.concatenate([(A - Bc * y[:, 0])[:, None], (Cc * y[:, 0] - Dsum * y[:, 1] + y[:, 2:].sum(axis=1))[:, None],
                        Sr * y[:, 1:2] - dg * y[:, 2:]], axis=1)
    old = gam * _arrow(h[:, None] * f, q, th, n)
    r = y.copy(); r[:, 0] = q * A + y[:, 0]
    u = _arrow(r, q, th, n)
    new = u - y
    normJ = np.maximum(np.maximum(Bc, Cc + Dsum + n), (Sr + dg).max(axis=1))
    Y = np.maximum(np.abs(y).max(axis=1), np.abs(u).max(axis=1))
    K = 4 * (n + 12)
    diff = np.abs(new - old).max(axis=1)
    small = q * normJ < 1e-6
    print("largest |difference| / (K 2^-53 Y): %.3f over all samples, %.3f over the %d with q |J| < 1e-6"
          % ((diff / (K * U * Y)).max(), (diff[small] / (K * U * Y[small])).max(), small.sum()))
    assert small.sum() > 1000
    assert (diff <= K * U * Y).all()


# ---------------------------------------------------------------- parity against the C restatement
_ORACLE = {}


def _oracle(n, **kw):
    """The C restatement on the shared batch of size n: computed once, never written to."""
    key = (n, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        theta = _theta(n, B, 9700 + n)
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), T, **{"rtol": RTOL, "atol": ATOL, **kw})
        assert not st.any()
        for a in (theta, sol, ns):
            a.setflags(write=False)
        _ORACLE[key] = (theta, sol, ns)
    return _ORACLE[key]


def _check(r, ref, ns_ref, what, rtol=RTOL, atol=ATOL, rejected=False):
    assert not _np(r.status).any(), what
    steps = _np(r.n_steps)
    d = int(np.abs(steps[:, 0] - ns_ref[:, 0]).max())
    dr = int(np.abs(steps[:, 1] - ns_ref[:, 1]).max())
    e = pm.band_error(_np(r.sol), ref, rtol, atol) if r.sol is not None else None
    print(what, "accepted / rejected steps differ by at most", d, "/", dr, "band error", e)
    assert d <= STEPS, (what, "accepted steps", d)
    if rejected:
        assert dr <= STEPS, (what, "rejected steps", dr)
    if e is not None:
        assert e <= BAND, (what, "band error", e)


def _classes(eng, theta, y0, n, raw, ns, tag, rejected=False, **extra):
    """DistSolSum, DistSolOnly, DistFlatOnly and the run-time kernel against the restatement's trajectories `raw`."""
    clipped = np.clip(raw, 0.0, None)
    kw = dict(KW, **extra)
    rtol, atol = kw["rtol"], kw["atol"]
    out = {}
    r = out["sol + sum"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **kw)
    _check(r, clipped, ns, (n, tag, "sol + sum"), rtol, atol, rejected)
    width = atol + rtol * np.abs(clipped)
    want = clipped.sum(axis=(1, 2))
    assert (np.abs(_np(r.metric) - want) <= BAND * width.sum(axis=(1, 2)) + 1e-13 * np.abs(want)).all(), (n, tag, "total_signal")
    r = out["sol only"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **kw)
    _check(r, clipped, ns, (n, tag, "sol only"), rtol, atol, rejected)
    r = out["flat only"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **kw)
    _check(r, None, ns, (n, tag, "flat only"), rtol, atol, rejected)
    want = np.stack([pm.flatten_observables(pm.DIST, c, n) for c in clipped])
    e = pm.band_error(_np(r.flat), want, rtol, atol)
    print((n, tag, "flat only"), "band error", e)
    assert e <= BAND, (n, tag, "flat only", e)
    r = out["raw"] = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, clip_nonneg=False, **kw)
    _check(r, raw, ns, (n, tag, "raw, run-time kernel"), rtol, atol, rejected)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", RESIDENT + SHADOWED)
def test_lrp12_against_the_c_restatement(eng, n):
    theta, raw, ns = _oracle(n)
    _classes(eng, theta, np.ones(n + 2), n, raw, ns, "resident" if n in RESIDENT else "shadowed")


@pytest.mark.gpu
def test_lrp8_against_the_c_restatement(eng):
    n = 30
    theta, raw, ns = _oracle(n, stages=8, rtol=1e-7, atol=1e-9)
    _classes(eng, theta, np.ones(n + 2), n, raw, ns, "lrp8", method="lrp8", rtol=1e-7, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 32))
def test_rodas4_against_the_generic_kernel(eng, n):
    """B_1 / gamma is not 1 for this tableau and E_k / gamma differs from E_k by a factor 4, so a wrong fold moves the step sizes.  The
    reference is the generic solve_kernel with the arrow solver (linsolve = "structured"): RODAS4 in resolvent form with a directly
    formed right-hand side, the same controller and initial step.  n = 30 runs resident-sized on the shadowed RODAS4 table's 4 x 8,
    n = 32 its neighbour; with and without a forced first reject."""
    nb = 32
    theta = _theta(n, nb, 9800 + n)
    y0 = np.ones(n + 2)
    for h0 in (None, 10.0):
        kw = dict(method="rodas4", want_flat=False, clip_nonneg=False, rtol=1e-7, atol=1e-9, h0=h0)
        ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, linsolve="structured", **kw)
        assert not _np(ref.status).any() and _np(ref.n_steps)[:, 0].min() > 10
        if h0:
            assert _np(ref.n_steps)[:, 1].min() >= 1, "the forced first step is not rejected"
        r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, kernel="group", **kw)
        _check(r, _np(ref.sol), _np(ref.n_steps), (n, "rodas4", "h0", h0), 1e-7, 1e-9, rejected=True)
        assert not np.array_equal(_bits(r.sol), _bits(ref.sol)), "the reference ran the kernel under test"


# ---------------------------------------------------------------- the specialised kernels against DistAny, bit for bit
def _bitwise(eng, n, **extra):
    """sol alone (DistSolOnly), flat alone (DistFlatOnly), sol + total_signal (DistSolSum) against sol + flat + total_signal, which runs on
    DistAny: every output through its integer view; a partial wave; initial values per replica."""
    nb = 17
    rng = np.random.default_rng(1000 * n + 7)
    theta, y0 = rng.uniform(0.05, 5.0, (nb, pm.n_params(pm.DIST, n))), rng.uniform(0.5, 2.0, (nb, n + 2))
    KW = dict(globals()["KW"], **extra)
    a = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, **KW)
    c = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **KW)
    d = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_flat=False, metric="total_signal", **KW)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric="total_signal", **KW)
    assert np.isfinite(_np(ref.sol)).all() and not _np(ref.status).any() and _np(ref.n_steps)[:, 0].min() > 0, n
    assert np.array_equal(_bits(a.sol), _bits(ref.sol)) and np.array_equal(_bits(d.sol), _bits(ref.sol)), n
    assert np.array_equal(_bits(c.flat), _bits(ref.flat)), n
    assert np.array_equal(_bits(d.metric), _bits(ref.metric)), n
    for other in (a, c, d):
        assert np.array_equal(_np(other.status), _np(ref.status)) and np.array_equal(_np(other.n_steps), _np(ref.n_steps)), n


@pytest.mark.gpu
@pytest.mark.parametrize("n", RESIDENT + SHADOWED)
def test_specialised_kernels_have_the_bits_of_the_run_time_kernel(eng, n):
    _bitwise(eng, n)


@pytest.mark.gpu
@pytest.mark.parametrize("method", ("lrp8", "rodas4"))
def test_specialised_kernels_have_the_bits_of_the_run_time_kernel_other_methods(eng, method):
    """The other two instantiations of the folded weights, at n = 30 and at the tolerances these methods run at."""
    _bitwise(eng, 30, method=method, rtol=1e-7, atol=1e-9)


_SHADOW_SCRIPT = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_dist_fast_resolvent as t
from phoskintime_amd import batch
batch.get_context()
for n in t.RESIDENT:
    t._bitwise(batch, n)
print("shadowed layout: bit for bit at", t.RESIDENT)
"""


@pytest.mark.gpu
def test_bits_in_the_shadowed_layout_of_the_resident_sizes():
    """PK_DIST_LAYOUT is read once per process, so the shadowed kernels of the resident sizes run in a child."""
    r = subprocess.run([sys.executable, "-c", _SHADOW_SCRIPT, str(ROOT)], env={**os.environ, "PK_DIST_LAYOUT": "shadow"},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "bit for bit" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- first steps at which the subtraction cancels nearly everything
def _corner_batches(n):
    """(name, theta, y0 [S], h0): q |J| is about 1e-7 ... 1e-13 at the first step of these."""
    nb = 12
    out = []
    for h0 in (1e-9, 1e-12):
        out.append(("U(0, 20), h0 = %g" % h0, _theta(n, nb, 9900 + n), np.ones(n + 2), h0))
        out.append(("U(0, 0.05), h0 = %g" % h0, _theta(n, nb, 9910 + n, hi=0.05), np.ones(n + 2), h0))
    th = _theta(n, nb, 9920 + n); th[:, 0] = 0.0
    out.append(("A = 0, h0 = 1e-9", th, np.ones(n + 2), 1e-9))
    y0 = np.ones(n + 2); y0[0] = 0.0
    out.append(("y0[R] = 0, h0 = 1e-9", _theta(n, nb, 9930 + n), y0, 1e-9))
    return out


_CORNER_REF = {}


def _corner_ref(n):
    if n not in _CORNER_REF:
        _CORNER_REF[n] = [(name, th, y0, h0) + ts._port_batch(th, n, y0, h0) for name, th, y0, h0 in _corner_batches(n)]
    return _CORNER_REF[n]


def test_the_restatement_finishes_the_cancellation_corners():
    """CPU: the inputs of the next test are ones on which the C restatement's algorithm (with the same initial step) ends with status 0."""
    for n in (30, 32):
        for name, _, _, _, _, st, ns in _corner_ref(n):
            assert not st.any(), (n, name)
            assert ns[:, 0].min() > 10, (n, name)         # the step really starts small and has to grow


@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 32))
def test_cancellation_corners(eng, n):
    for name, th, y0, h0, raw, st, ns in _corner_ref(n):
        assert not st.any(), (n, name)
        _classes(eng, th, y0, n, raw, ns, name, rejected=True, h0=h0)


# ---------------------------------------------------------------- forced rejects
@pytest.mark.gpu
@pytest.mark.parametrize("n", (14, 30, 32))
def test_forced_first_reject(eng, n):
    nb = 32
    theta = _theta(n, nb, 9940 + n)
    y0 = np.ones(n + 2)
    # the initial step is chosen on the CPU: the first value at which the restatement itself rejects a step of every replica
    for h0 in (1.0, 10.0, 100.0):
        raw, st, ns = ts._port_batch(theta, n, y0, h0)
        if ns[:, 1].min() >= 1:
            break
    assert ns[:, 1].min() >= 1 and not st.any(), "no initial step makes the restatement reject in every replica"
    out = _classes(eng, theta, y0, n, raw, ns, "h0 = %g" % h0, rejected=True, h0=h0)
    for what, r in out.items():
        assert _np(r.n_steps)[:, 1].min() >= 1, (n, what, "a replica rejected nothing")
        assert np.array_equal(_np(r.n_steps), _np(out["raw"].n_steps)), (n, what)


# ---------------------------------------------------------------- non-finite inputs
NONFINITE = ("inf A", "NaN B", "inf C", "NaN D_3", "NaN y0[R]", "inf y0[P]", "NaN y0 in a site")


@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 32))
@pytest.mark.parametrize("what", NONFINITE)
def test_nonfinite_inputs(eng, what, n):
    """One wave of sixteen replicas, replica 5 spoiled (ordinary arithmetic NaNs and infs).  Status, NaN rows and step counts are
    DistAny's, and the fifteen wave mates have the bits of a launch in which replica 5 is ordinary."""
    from phoskintime_amd._capi import ST_NONFINITE
    nb, odd = 16, 5
    plain_th = _theta(n, nb, 9950 + n)
    plain_y0 = np.ones((nb, n + 2))
    theta, y0 = plain_th.copy(), plain_y0.copy()
    if what == "inf A":
        theta[odd, 0] = np.inf
    elif what == "NaN B":
        theta[odd, 1] = np.nan
    elif what == "inf C":
        theta[odd, 2] = np.inf
    elif what == "NaN D_3":
        theta[odd, 4 + n + 3] = np.nan
    elif what == "NaN y0[R]":
        y0[odd, 0] = np.nan
    elif what == "inf y0[P]":
        y0[odd, 1] = np.inf
    else:
        y0[odd, 2 + n // 2] = np.nan
    mates = np.setdiff1d(np.arange(nb), [odd])
    kw = dict(KW, want_flat=False)
    ref = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, metric="total_signal", **KW)                     # sol + flat: DistAny
    assert _np(ref.status)[odd] == ST_NONFINITE and not _np(ref.status)[mates].any(), (what, _np(ref.status))
    for name, extra in (("sol + sum", dict(metric="total_signal")), ("sol only", dict())):
        r = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, **extra, **kw)
        p = eng.solve_ode_batch(pm.DIST, plain_th, plain_y0, n, T, **extra, **kw)
        st, sol, steps = _np(r.status), _np(r.sol), _np(r.n_steps)
        print(n, what, name, "status", st[odd], "steps", steps[odd])
        assert np.array_equal(st, _np(ref.status)) and np.array_equal(steps, _np(ref.n_steps)), (what, name, "against DistAny")
        assert np.isnan(sol[odd, 1:]).all(), (what, name, "NaN rows from the failing landing on")
        assert np.array_equal(sol.view(np.int64), _np(ref.sol).view(np.int64)), (what, name, "sol against DistAny")
        if r.metric is not None:
            assert np.isnan(_np(r.metric)[odd]) and np.array_equal(_bits(r.metric)[mates], _bits(p.metric)[mates]), (what, name, "metric")
        assert not _np(p.status).any()
        assert np.array_equal(sol[mates].view(np.int64), _np(p.sol)[mates].view(np.int64)), (what, name, "wave mates")
        assert np.array_equal(steps[mates], _np(p.n_steps)[mates]), (what, name, "wave mates' steps")
    # the run-time kernel and the flat-only kernel against launches without the bad replica, so that a leak they share cannot pass
    pref = eng.solve_ode_batch(pm.DIST, plain_th, plain_y0, n, T, metric="total_signal", **KW)
    assert not _np(pref.status).any()
    assert np.array_equal(_bits(ref.sol)[mates], _bits(pref.sol)[mates]) and np.array_equal(_bits(ref.flat)[mates], _bits(pref.flat)[mates]), (what, "DistAny wave mates")
    assert np.array_equal(_bits(ref.metric)[mates], _bits(pref.metric)[mates]) and np.array_equal(_np(ref.n_steps)[mates], _np(pref.n_steps)[mates]), (what, "DistAny wave mates")
    f = eng.solve_ode_batch(pm.DIST, theta, y0, n, T, want_sol=False, **KW)
    pf = eng.solve_ode_batch(pm.DIST, plain_th, plain_y0, n, T, want_sol=False, **KW)
    assert np.array_equal(_bits(f.flat)[mates], _bits(pf.flat)[mates]) and np.array_equal(_np(f.n_steps)[mates], _np(pf.n_steps)[mates]), (what, "flat only wave mates")
    assert np.array_equal(_np(f.status), _np(ref.status)) and np.array_equal(_np(f.n_steps), _np(ref.n_steps)), (what, "flat only")
    assert np.array_equal(_bits(f.flat), _bits(ref.flat)), (what, "flat only against DistAny")
