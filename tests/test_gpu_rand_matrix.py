"""GPU: every randmod kernel outside the lane groups, and the wide-chain kernels, against the numpy restatement tests/group_reference.py --
the kernels that repeat the step loop of solve_kernel in their own text and that tests/test_gpu_group_matrix.py does not reach.  The table
is group_reference.KERNELS (29 rows); tests/test_protein_plan_cpu.py holds protein_plan to its routing and
tests/test_group_reference_cpu.py proves its forced grids single-step and measures the restatement's own rounding on them.  B = 37, per-replica
y0, theta half U(0, 20) and half log-uniform (group_reference.case); compared replicas: first, middle, last.

Switches are read once per process, so the kernels that need one run in a child process per switch group (three children, one after
another, 120 s each, none retried; a child that dies or runs into its limit ends every later launch of this module) and write an .npz;
every comparison is made here.  Default-routed kernels and kernel="tpr" run in this process.

  kernel (csrc)                 n    selected by                     L    worst ratio -> C   (LRP12; LRP8; RODAS4)
  rand_fast_kernel<1>           1    default                         2    0.287 -> 2;  1.463 -> 8;  2.152 -> 16
  rand_fast_kernel<2>           2    default                         4    1.221 -> 8;  1.202 -> 8;  1.867 -> 8
  rand_fast_kernel<3>           3    PK_RAND_ROWS=1                  8    1.466 -> 8;  2.932 -> 16; 1.716 -> 8
  rand_fast_kernel<4>           4    PK_RAND_ROWS=1                  16   4.838 -> 32; 0.976 -> 4;  2.322 -> 16
  rand_fast_kernel<6>           6    PK_RAND_PARITY56=0              64   1.098 -> 8;  1.548 -> 8;  2.598 -> 16   (three units; LRP8 / RODAS4 also by default)
  rand_fastr_kernel<3,2>        3    default                         8    1.466 -> 8;  2.932 -> 16; 1.717 -> 8
  rand_fastr_kernel<4,4>        4    default                         16   4.838 -> 32; 0.976 -> 4;  3.251 -> 16
  rand_fastr_kernel<5,2>        5    default                         32   1.893 -> 8;  1.956 -> 8;  3.920 -> 16
  tpr_rand_kernel<1>, <2>, <3>  1-3  kernel="tpr"                    2^n  1.421 -> 8 | 1.221 -> 8 | 1.466 -> 8
  rand_parity_kernel<6,8>       6    default                         32   0.621 -> 4
  rand_parity_kernel<7,16>      7    default, B < 1024               64   1.463 -> 8
  rand_parity_kernel<7,8>       7    default, B = 1024               64   1.528 -> 8
  rand_parity_kernel<8,16,16>   8    default                         128  0.626 -> 4
  rand_parity_kernel<5,4>       5    PK_RAND_PARITY56=1              16   1.893 -> 8
  rand_parity_kernel<6,16>      6    PK_RAND_PARITY6_TB=16           32   0.472 -> 2
  rand_parity_kernel<8,16,32>   8    PK_RAND_PARITY8_GRID=512        128  0.724 -> 4
  rand_level_kernel<6>          6    PK_RAND_LEVEL6=1                20   0.693 -> 4
  rand_level_kernel<8>          8    PK_WIDE_RAND_EXACT=2            70   0.513 -> 4
  rand_dense_kernel<7>          7    PK_WIDE_RAND_EXACT=2            128  1.463 -> 8
  wide_chain_kernel<M_DIST>     63, 126, 127, 255   default          S    0.418, 0.496, 0.395, 0.372 -> 2 each
  wide_chain_kernel<M_SUCC>     63, 126, 127, 255   default          2 ceil(log2 S) + 1   0.735, 0.609, 0.718, 0.622 -> 4 each
  (MI355X; each figure the worst over the compared replicas and every row of the forced grid and of the T = 2 grid.  The wide-chain sizes:
  the first past the lane groups, S = 128 | 129 where the launcher goes from 128 to 256 threads, and S = 257, the first at which a thread
  strides over two rows.)

a. Forced grid (group_reference.forced: rtol = atol = 1, h0 twice the largest spacing).  Status 0 and n_steps == (T - 1, 0) on every
   replica, row 0 bit-equal to y0, and on the compared replicas every row against one long-double step from the kernel's own previous row:
   |y_gpu - y_ref|_inf <= C tau.  C is 4 x the worst measured ratio of that instantiation and method, rounded up to a power of two (the margin of
   the group matrix).  The fused metric cycles over pm.METRICS against pm.compute_Y, flat is bit-equal to flatten_observables, normalize
   scales by 1 / y0 at rtol 1e-15, clip_nonneg equals numpy.clip bit for bit.
   Condition, not a measurement: no ratio above L x the double restatement's own ratio at that size and method (group_reference.KERNEL_R64).
   L is the longest accumulation of the kernel's solve, read from its code: the 2^n-term dot product with a row of the in-register inverse
   (rand_fast, rand_fastr, tpr_rand, rand_dense: solve()); the order 2^(n-1) of the even Schur complement whose inverse rand_parity's solve
   multiplies by; the widest level block C(n, n/2) of rand_level's mat-vecs; for the chains the S terms the arrow solve sums over the site
   rows and the two pivots (distmod) and the two terms parallel cyclic reduction adds to a row at each of its ceil(log2 S) levels (succmod).
   Finding.  tpr_rand_kernel<1> measures 1.42 where L x R64 = 2 x 0.6 = 1.2.  Its text at n = 1 is a 2 x 2 Gauss-Jordan inverse with
   refined reciprocals and FMA dot products; tests/test_group_reference_cpu.py evaluates exactly those operations in correctly rounded
   double on the same grid and finds 1.11 against long double, twice the 0.59 of the LAPACK solve the restatement makes: at this size the
   figure depends on the elimination order, and the kernel's order is the one that applies to it.  The kernel is held to L x that figure,
   2 x 1.2 = 2.4 (group_reference.TPR1_TEXT_R64), and to C = 8.  The draw stays.
b. Free-running on pm.TIME_POINTS at the tolerances and limits of group_reference.FREE: status 0, band error against the closed form
   within the limit, accepted and rejected steps on the compared replicas within 2 + ROOT_SPREAD of group_reference.integrate.  Measured:
   the counts are EQUAL to the restatement's on every kernel, method and compared replica but for one accepted step at distmod and
   succmod n = 127 (LRP12 23 to 53 steps, LRP8 35 to 84, RODAS4 102 to 402, none rejected); worst band error 0.099 (LRP12, on the B = 1024 draw
   at randmod n = 7; 0.062 on the 37-replica draw there, 0.046 at succmod n = 63, at most 0.033 elsewhere; limit 0.1), 0.024 (LRP8), 0.029
   (RODAS4).
   Those runs hardly meet the controller's clamps (none rejects a step; with the growth clamp at 12 instead of 6 the restatement's
   count moves by one step on two of the compared replicas), so two more LRP12 runs per kernel are set by them (group_reference.GROWTH,
   SHRINK).  GROWTH starts from h0 = 1e-13 at rtol = atol = 1: err ~ 0, every step grows by the growth clamp's factor, and the count (30
   or 31) must EQUAL the restatement's -- the root is the clamped 1e-30^(1/11) in any precision; a clamp of 8 gives 2 to 3 steps fewer, 12
   gives 4 to 5.  SHRINK starts at h0 = 1e7 on (0, 1e6, 2e6) at rtol = 1e-12, atol = 1e-14: the first 9 to 14 steps are rejected, finite,
   at the shrink clamp's factor 5, and the steps after them pass through the after-reject rule; rejected steps within 1 and accepted
   within 2 + 2 of the restatement's (SHRINK_SPREAD: what the precision of the root moves on the CPU); a shrink clamp of 10 rejects 2 to 4
   steps fewer, one of 7 rejects 1 to 2 fewer (so a clamp of 7 is seen only where it makes 2).  On the 257-state systems the SHRINK run is
   compared on the first replica alone (its restatement takes 140 steps of twelve 257 x 257 solves).
c. Exits and edges, every kernel: a NaN in theta of replica 5 (inside the first wave of every kernel that packs 4, 16 or 64 replicas into
   one) gives NONFINITE, NaN rows after t0 and every other replica bit-equal to the clean run; a step budget one short of the quickest
   replica gives MAXSTEPS everywhere, the reached rows bit-equal to the unrestricted run and NaN after them; T = 1, 2, 5 (shapes, row 0,
   the same bits as the first rows of the full grid, flat without an mRNA block; T = 2 held as in a.); a permuted batch and single
   replicas cut out of it give the same bits (every row but B = 1024, where a cut-out replica runs on the kernel of smaller batches).

Template instantiations this file launches that no test launched before: rand_fast_kernel<3, .> and <4, .> under all three methods
(PK_RAND_ROWS=1), rand_parity_kernel<5,4>, <6,16>, <8,16,32> and, at B >= 1024, <7,8>; wide_chain_kernel with a thread striding over two
rows was launched before (n up to 1276) but never compared step by step."""
import functools
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import group_reference as gr
from oracle import protein_models as pm

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
NAN_REPLICA = 5            # inside the first wave of every kernel that packs replicas into one (4, 16 or 64 of them), live neighbours on both sides
CHILD_TIMEOUT = 120        # seconds; the import dominates
#: C per instantiation and method (LRP12, LRP8, RODAS4): 4 x the measured worst ratio, rounded up to a power of two (module docstring)
C_BOUND = {("rand_fast_kernel<1>", 1): (2.0, 8.0, 16.0), ("rand_fast_kernel<2>", 2): (8.0, 8.0, 8.0), ("rand_fast_kernel<3>", 3): (8.0, 16.0, 8.0),
           ("rand_fast_kernel<4>", 4): (32.0, 4.0, 16.0), ("rand_fast_kernel<6>", 6): (8.0, 8.0, 16.0), ("rand_fastr_kernel<3,2>", 3): (8.0, 16.0, 8.0),
           ("rand_fastr_kernel<4,4>", 4): (32.0, 4.0, 16.0), ("rand_fastr_kernel<5,2>", 5): (8.0, 8.0, 16.0), ("tpr_rand_kernel<1>", 1): (8.0,),
           ("tpr_rand_kernel<2>", 2): (8.0,), ("tpr_rand_kernel<3>", 3): (8.0,), ("rand_parity_kernel<6,8>", 6): (4.0,), ("rand_parity_kernel<7,16>", 7): (8.0,),
           ("rand_parity_kernel<7,8>", 7): (8.0,), ("rand_parity_kernel<8,16,16>", 8): (4.0,), ("rand_parity_kernel<5,4>", 5): (8.0,),
           ("rand_parity_kernel<6,16>", 6): (2.0,), ("rand_parity_kernel<8,16,32>", 8): (4.0,), ("rand_level_kernel<6>", 6): (4.0,),
           ("rand_level_kernel<8>", 8): (4.0,), ("rand_dense_kernel<7>", 7): (8.0,)}
C_BOUND.update({("wide_chain_kernel<M_DIST>", n): (2.0,) for n in gr.CHAIN_SIZES})
C_BOUND.update({("wide_chain_kernel<M_SUCC>", n): (4.0,) for n in gr.CHAIN_SIZES})
#: where the restatement's LAPACK solve is not the double-precision evaluation that applies (module docstring, "Finding"): L x the figure
#: of the kernel's own elimination order in correctly rounded double
DERIVED = {("tpr_rand_kernel<1>", "lrp12"): 2 * gr.TPR1_TEXT_R64}
_FIELDS = dict(sol="sol", flat="flat", met="metric", st="status", ns="n_steps")


def _np(x):
    return x.detach().cpu().numpy()


def _solve(eng, k, theta, y0, t, method, **kw):
    kw.setdefault("clip_nonneg", False)
    if k.kernel:
        kw["kernel"] = k.kernel
    return eng.solve_ode_batch(k.model, theta, y0, k.n, t, method=method, **kw)


def collect(eng, k):
    """Every launch the three tests need of kernel `k`, as {tag.field: array}.  Runs in this process for the default-routed kernels and
    kernel="tpr", in a child process (which imports this module) for the kernels an environment switch selects."""
    theta, y0 = gr.case(k.model, k.n, k.B)
    idx = gr.KERNELS.index(k)
    out = {}

    def put(tag, r, fields="sol st ns"):
        for f in fields.split():
            out["%s.%s" % (tag, f)] = _np(getattr(r, _FIELDS[f]))

    for mi, method in enumerate(k.methods):
        t, opts = gr.forced(method, k.model, theta, k.n)
        put("forced-" + method, _solve(eng, k, theta, y0, t, method, metric=pm.METRICS[(idx + mi) % len(pm.METRICS)], **opts), "sol flat met st ns")
        put("free-" + method, _solve(eng, k, theta, y0, pm.TIME_POINTS, method, **gr.FREE[method, "resolvent"][0]))
    put("growth", _solve(eng, k, theta, y0, pm.TIME_POINTS, "lrp12", **gr.GROWTH), "st ns")
    put("shrink", _solve(eng, k, theta, y0, gr.SHRINK_T, "lrp12", **gr.SHRINK), "st ns")
    t, opts = gr.forced("lrp12", k.model, theta, k.n)
    put("norm", _solve(eng, k, theta, y0, t, "lrp12", normalize=True, **opts), "sol")
    put("clip", _solve(eng, k, theta, y0, t, "lrp12", clip_nonneg=True, **opts), "sol")
    bad = theta.copy()
    bad[NAN_REPLICA, 5] = np.nan
    put("nan", _solve(eng, k, bad, y0, pm.TIME_POINTS, "lrp12"), "sol st")
    budget = int(out["free-lrp12.ns"].sum(axis=1).min()) - 1            # one step short of the quickest replica: every replica runs out, on different rows
    out["maxsteps.budget"] = np.array(budget)
    put("maxsteps", _solve(eng, k, theta, y0, pm.TIME_POINTS, "lrp12", max_steps=budget))
    for T in (1, 2, 5):
        put("short%d" % T, _solve(eng, k, theta, y0, t[:T], "lrp12", **opts), "sol flat st ns")
    if k.B == gr.B:          # (at B = 1024 a cut-out replica would run on the kernel of B < 1024)
        perm = np.random.default_rng(7).permutation(k.B)
        put("perm", _solve(eng, k, theta[perm], y0[perm], t, "lrp12", **opts), "sol")
        for b in gr.compared(k.B):
            put("single%d" % b, _solve(eng, k, theta[b:b + 1], y0[b:b + 1], t, "lrp12", **opts), "sol")
    return out


_CHILD_SCRIPT = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from phoskintime_amd import batch
import group_reference as gr
import test_gpu_rand_matrix as m
out = {}
for i in map(int, sys.argv[3].split(",")):
    for key, v in m.collect(batch, gr.KERNELS[i]).items():
        out["%d.%s" % (i, key)] = v
np.savez(sys.argv[2], **out)
"""
_DATA = {}        # kernel index -> {tag.field: array}
_GROUPS = {}      # index of the switch group -> its child's .npz, loaded
_STOP = []        # why nothing more is started on the GPU: a child died or ran into its limit


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()          # raises loudly if libphoskin_hip.so is missing
    return batch


@pytest.fixture
def data(eng, tmp_path_factory):
    """data(k) -> get(tag.field).  At most three child processes, one per switch group, one after another, each started only when the
    one before it returned 0; a child that dies or runs into its limit is not tried again and ends every later launch of this module."""
    def of(k):
        i, g = gr.KERNELS.index(k), gr.ENV_GROUPS.index(k.env)
        assert not _STOP, "nothing more is started on the GPU: " + _STOP[0]
        if g == 0:
            if i not in _DATA:
                try:
                    _DATA[i] = collect(eng, k)
                except Exception as e:          # a launch that raised (a refusal, a HIP error): no later launch may follow it
                    _STOP.append("%r raised %r" % (k, e))
                    raise
            return _DATA[i].__getitem__
        if g not in _GROUPS:
            f = tmp_path_factory.mktemp("rand_matrix") / ("group%d.npz" % g)
            members = ",".join(str(j) for j, kk in enumerate(gr.KERNELS) if kk.env is k.env)
            try:
                rc = subprocess.run([sys.executable, "-c", _CHILD_SCRIPT, str(ROOT), str(f), members], env={**os.environ, **k.env},
                                    timeout=CHILD_TIMEOUT).returncode
            except subprocess.TimeoutExpired:
                rc = "its limit of %d s" % CHILD_TIMEOUT
            if rc != 0:
                _STOP.append("the child of %s ended with %s" % (k.env, rc))
                pytest.fail(_STOP[0])
            _GROUPS[g] = np.load(f)
        return lambda key: _GROUPS[g]["%d.%s" % (i, key)]
    return of


def _one_step_ratios(k, method, theta, sol, t):
    """[(|y_gpu - y_ref|_inf / tau, replica, row)] of every row of the compared replicas, y_ref one long-double step from the kernel's own row before."""
    out = []
    for b in gr.compared(k.B):
        sys_b = gr.system(k.model, theta[b], k.n)
        for row in range(1, t.size):
            ref, tt = gr.interval_reference(method, "resolvent", sys_b, sol[b], t, row)
            out.append((float(np.max(np.abs(sol[b, row] - ref.astype(float)))) / tt, b, row))
    return out


def _hold(k, method, ratios, what):
    worst = max(ratios)
    r64 = gr.KERNEL_R64[k.model, k.n, k.B, method]
    finding = DERIVED.get((k.name, method), k.L * r64)
    print("%s: %s %s, worst |y_gpu - y_ref| / tau %.3f at replica %d row %d (S = %d); L x R64 = %d x %.1f, finding above %.1f"
          % (what, k, method, worst[0], worst[1], worst[2], k.S, k.L, r64, finding))
    assert worst[0] <= finding, (k, method, worst)                                # beyond this: a finding, not a tolerance
    assert worst[0] <= C_BOUND[k.name, k.n][k.methods.index(method)], (k, method, worst)


@pytest.mark.parametrize("k", gr.KERNELS, ids=repr)
def test_forced_grid_every_step_against_long_double(data, k):
    get = data(k)
    theta, y0 = gr.case(k.model, k.n, k.B)
    idx = gr.KERNELS.index(k)
    held = []
    for mi, method in enumerate(k.methods):
        t, opts = gr.forced(method, k.model, theta, k.n)
        sol, flat, met, st, ns = (get("forced-%s.%s" % (method, f)) for f in ("sol", "flat", "met", "st", "ns"))
        assert sol.shape == (k.B, t.size, k.S) and not st.any(), (k, method)
        assert (ns == np.array((t.size - 1, 0))).all(), (k, method, ns)                    # the steps the comparison assumes, on every replica
        np.testing.assert_array_equal(sol[:, 0], y0)
        held.append((method, _one_step_ratios(k, method, theta, sol, t)))
        metric = pm.METRICS[(idx + mi) % len(pm.METRICS)]
        for b in gr.compared(k.B):
            assert met[b] == pytest.approx(pm.compute_Y(sol[b], k.n, metric), rel=1e-10, abs=1e-12), (k, method, metric, b)
            np.testing.assert_array_equal(flat[b], pm.flatten_observables(k.model, sol[b], k.n))
    for method, ratios in held:
        _hold(k, method, ratios, "forced grid")
    plain = get("forced-lrp12.sol")
    np.testing.assert_allclose(get("norm.sol"), plain * (1.0 / y0)[:, None, :], rtol=1e-15)
    np.testing.assert_array_equal(get("clip.sol"), np.clip(plain, 0.0, None))


@functools.lru_cache(maxsize=None)
def _free_reference(model, n, batch, b, method):
    """(accepted, rejected) of the restatement and the closed form, once per replica however many kernels integrate it."""
    theta, y0 = gr.case(model, n, batch)
    _, st, steps = gr.integrate(method, "resolvent", model, theta[b], n, y0[b], pm.TIME_POINTS, **gr.FREE[method, "resolvent"][0])
    assert st == 0
    grown = steps
    if method == "lrp12":
        _, st, grown = gr.integrate(method, "resolvent", model, theta[b], n, y0[b], pm.TIME_POINTS, **gr.GROWTH)
        assert st == 0
    return steps, pm.solve_exact_lti(model, theta[b], y0[b], n, pm.TIME_POINTS), grown


@functools.lru_cache(maxsize=None)
def _shrink_reference(model, n, batch, b):
    theta, y0 = gr.case(model, n, batch)
    _, st, steps = gr.integrate("lrp12", "resolvent", model, theta[b], n, y0[b], gr.SHRINK_T, **gr.SHRINK)
    assert st == 0 and steps[1] >= 9                          # the run the comparison is about: rejected steps at the shrink clamp
    return steps


@pytest.mark.parametrize("k", gr.KERNELS, ids=repr)
def test_free_running_band_and_step_counts(data, k):
    get = data(k)
    for method in k.methods:
        limit = gr.FREE[method, "resolvent"][1]
        allow = 2 + gr.ROOT_SPREAD[method]
        sol, st, ns = (get("free-%s.%s" % (method, f)) for f in ("sol", "st", "ns"))
        assert not st.any(), (k, method)
        for b in gr.compared(k.B):
            (acc, rej), exact, grown = _free_reference(k.model, k.n, k.B, b, method)
            e = pm.band_error(sol[b], exact)
            print("free-running", k, method, "replica", b, "band error %.4f" % e, "steps gpu", tuple(map(int, ns[b])), "restatement", (acc, rej))
            assert e <= limit, (k, method, b, e)
            assert abs(int(ns[b, 0]) - acc) <= allow and abs(int(ns[b, 1]) - rej) <= allow, (k, method, b, tuple(ns[b]), (acc, rej))
            if method == "lrp12":                       # growth from h0 = 1e-13 at the clamp: the restatement's count
                gs = tuple(map(int, get("growth.ns")[b]))
                print("clamped growth", k, "replica", b, "steps gpu", gs, "restatement", grown)
                assert not get("growth.st").any() and gs == tuple(grown), (k, b, gs, grown)
                if k.S <= 129 or b == 0:                # rejected steps at the shrink clamp, then the after-reject rule
                    ss, want = tuple(map(int, get("shrink.ns")[b])), _shrink_reference(k.model, k.n, k.B, b)
                    print("clamped shrinking", k, "replica", b, "steps gpu", ss, "restatement", want)
                    assert not get("shrink.st").any(), k
                    assert abs(ss[0] - want[0]) <= 2 + gr.SHRINK_SPREAD[0] and abs(ss[1] - want[1]) <= gr.SHRINK_SPREAD[1], (k, b, ss, want)


@pytest.mark.parametrize("k", gr.KERNELS, ids=repr)
def test_exits_short_grids_and_replica_independence(data, k):
    get = data(k)
    theta, y0 = gr.case(k.model, k.n, k.B)
    T = pm.TIME_POINTS.size
    free, free_st = get("free-lrp12.sol"), get("free-lrp12.st")
    others = np.arange(k.B) != NAN_REPLICA
    # a NaN in one replica's theta: flagged, NaN after t0, and nobody else touched
    sol, st = get("nan.sol"), get("nan.st")
    assert st[NAN_REPLICA] & gr.ST_NONFINITE and np.isnan(sol[NAN_REPLICA, 1:]).all(), (k, st[NAN_REPLICA])
    np.testing.assert_array_equal(sol[NAN_REPLICA, 0], y0[NAN_REPLICA])
    np.testing.assert_array_equal(st[others], free_st[others])
    np.testing.assert_array_equal(sol[others], free[others])
    # a step budget one short of the quickest replica: every replica runs out, the rows it reached are those of the unrestricted run
    sol, st, ns, budget = get("maxsteps.sol"), get("maxsteps.st"), get("maxsteps.ns"), int(get("maxsteps.budget"))
    assert (st & gr.ST_MAXSTEPS).all() and (ns.sum(axis=1) == budget).all(), (k, budget, st, ns)
    reached = np.array([int(np.isfinite(sol[b]).all(axis=1).sum()) for b in range(k.B)])
    assert reached.min() >= 1 and reached.max() >= 2 and reached.max() < T, (k, reached)
    for b in range(k.B):
        np.testing.assert_array_equal(sol[b, :reached[b]], free[b, :reached[b]])
        assert np.isnan(sol[b, reached[b]:]).all(), (k, b)
    # T = 1, 2, 5: shapes, row 0, the layout of flat without an mRNA block; T = 2 is one forced step, held as in the forced-grid test
    t, _ = gr.forced("lrp12", k.model, theta, k.n)
    plain = get("forced-lrp12.sol")
    for Ts in (1, 2, 5):
        sol, flat, st, ns = (get("short%d.%s" % (Ts, f)) for f in ("sol", "flat", "st", "ns"))
        assert sol.shape == (k.B, Ts, k.S) and not st.any() and (ns == np.array((Ts - 1, 0))).all(), (k, Ts, sol.shape, ns)
        np.testing.assert_array_equal(sol[:, 0], y0)
        np.testing.assert_array_equal(sol, plain[:, :Ts])                                 # the same steps as the first rows of the full grid
        want = np.stack([pm.flatten_observables(k.model, sol[b], k.n) for b in range(k.B)])
        assert flat.shape == want.shape == (k.B, Ts * (1 + min(k.n, k.S - 2))), (k, Ts, flat.shape)
        np.testing.assert_array_equal(flat, want)
    _hold(k, "lrp12", _one_step_ratios(k, "lrp12", theta, get("short2.sol"), t[:2]), "T = 2")
    # a permuted batch and single replicas cut out of it: the same bits
    if k.B == gr.B:
        perm = np.random.default_rng(7).permutation(k.B)
        np.testing.assert_array_equal(get("perm.sol"), plain[perm])
        for b in gr.compared(k.B):
            np.testing.assert_array_equal(get("single%d.sol" % b)[0], plain[b])
