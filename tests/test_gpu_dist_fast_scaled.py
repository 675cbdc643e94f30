"""The scaled stages of the distributive throughput kernel (csrc/pk_dist_fast.hpp, dist_scaled()): the LRP12 layouts that carry their site
rows in units of the rows' coupling weight -- c_j = winv_j s_j, three FMAs per row and difference stage, the state entering as
rho_j = y_j ic_j and leaving once per step -- against the C restatement (oracle/lrp8_dist.c through oracle/lrp8_cpu.py), which keeps plain
units and its weighted sums over twelve solves, at the project's limits: band error <= 0.02, steps within 2.

Sizes: the four the scaling was asked for -- n = 30 (4 x 8 resident, the benchmark's), 32 (4 x 8 shadowed), 18 (4 x 5 resident), 38 (8 x 5
resident); of these only 4 x 8 resident is scaled (the others would lose a wave per SIMD to the registers that hold 1 / s_j and keep plain
units; they stay here as the neighbours that must agree) -- and one size for every other scaled layout: 22 and 46 (4 x 6 and 8 x 6
resident), 62 (8 x 8 resident), 20, 24, 28 (4 x 5, 4 x 6, 4 x 7 shadowed), 40, 48, 56 (8 x 5, 8 x 6, 8 x 7 shadowed).  Batches of 29-41
replicas leave a wave partial.

Batches: theta ~ U(0, 20) and U(0, 1) from y0 = 1; the edge rates of the scale rule (tools/scaled_stage_sensitivity.py: edge_thetas) --
one site rate exactly 0 with y0 = 1, every site rate 0, rates of 1e-300, 1e-12 and 1e6, site rates log-spread over eight decades, and a
site with rate 0 that starts at 0 --; a forced first step h0 = 1e-9 (reference: the numpy port of the C code with an initial step,
tests/test_gpu_dist_fast_sitesum.py).  LRP8 keeps plain units (its table has no parked layout): nothing to hold here."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lrp8_cpu
from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_dist_fast_resolvent as tr  # noqa: E402  (_classes: the four output classes against the restatement's trajectories)
import test_gpu_dist_fast_sitesum as ts  # noqa: E402  (the numpy port of the C restatement with an initial step)

ROOT = Path(__file__).resolve().parents[1]
T = pm.TIME_POINTS
# n: (G x RPL, layout, scaled, replicas)
SIZES = {18: ("4 x 5", "resident", False, 29), 20: ("4 x 5", "shadowed", True, 30), 22: ("4 x 6", "resident", True, 33), 24: ("4 x 6", "shadowed", True, 31),
         28: ("4 x 7", "shadowed", True, 35), 30: ("4 x 8", "resident", True, 41), 32: ("4 x 8", "shadowed", False, 37), 38: ("8 x 5", "resident", False, 29),
         40: ("8 x 5", "shadowed", True, 29), 46: ("8 x 6", "resident", True, 31), 48: ("8 x 6", "shadowed", True, 29), 56: ("8 x 7", "shadowed", True, 29),
         62: ("8 x 8", "resident", True, 33)}
H0_SIZES = (22, 28, 30, 32)         # the forced first step (the port is Python: 9 replicas each)
ZERO_SITE = 3                       # edge replicas 0 and 7: this site's rate is exactly 0
_REF = {}


def _tool():
    name = "scaled_stage_sensitivity"
    if name not in sys.modules:
        sys.path.insert(0, str(ROOT / "tools"))
        spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _frozen(key, make):
    """A reference computed once, shared, never written to."""
    if key not in _REF:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _random(n, hi):
    def make():
        theta = tr._theta(n, SIZES[n][3], 20000 + n + int(hi), hi=hi)
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), T)
        return theta, sol, st, ns
    return _frozen(("random", n, hi), make)


def _edge(n):
    """(theta [8, P], y0 [8, S], sol, status, n_steps) of the edge rates; replica 7 starts its zero-rate site at 0"""
    def make():
        theta = _tool().edge_thetas(n)
        y0 = np.ones((len(theta), n + 2))
        y0[7, 2 + ZERO_SITE] = 0.0
        res = [lrp8_cpu.solve_batch(theta[b:b + 1], n, y0[b], T) for b in range(len(theta))]
        return (theta, y0) + tuple(np.concatenate([r[i] for r in res]) for i in range(3))
    return _frozen(("edge", n), make)


def _with_h0(n):
    def make():
        theta = tr._theta(n, 9, 20300 + n)
        sol, st, ns = ts._port_batch(theta, n, np.ones(n + 2), 1e-9)
        return theta, sol, st, ns
    return _frozen(("h0", n), make)


def test_the_restatement_finishes_every_batch():
    """CPU: every input of the tests below is one the C restatement (or its port) ends with status 0 after a run of steps -- asserted, not
    assumed; and the edge batch holds what it is said to hold."""
    for n in sorted(SIZES):
        for hi in (20.0, 1.0):
            _, _, st, ns = _random(n, hi)
            assert not st.any() and ns[:, 0].min() > 10, (n, hi)
        theta, y0, sol, st, ns = _edge(n)
        assert not st.any() and ns[:, 0].min() > 10, (n, "edge")
        S = theta[:, 4:4 + n]
        assert S[0, ZERO_SITE] == 0.0 and y0[0, 2 + ZERO_SITE] == 1.0 and not S[1].any() and S[7, ZERO_SITE] == 0.0 and y0[7, 2 + ZERO_SITE] == 0.0
        assert (S[2, 5], S[3, 5], S[4, 5]) == (1e-300, 1e-12, 1e6) and S[5].max() / S[5].min() == pytest.approx(1e8)
        assert sol[0, -1, 2 + ZERO_SITE] < 1.0 and (sol[7, :, 2 + ZERO_SITE] == 0.0).all()
    for n in H0_SIZES:
        _, _, st, ns = _with_h0(n)
        assert not st.any() and ns[:, 0].min() > 10, (n, "h0")


def _tag(n, what):
    return "%s %s%s, %s" % (SIZES[n][0], SIZES[n][1], ", scaled" if SIZES[n][2] else "", what)


@pytest.mark.gpu
@pytest.mark.parametrize("hi", (20.0, 1.0))
@pytest.mark.parametrize("n", sorted(SIZES))
def test_random_rates_against_the_c_restatement(eng, n, hi):
    theta, raw, st, ns = _random(n, hi)
    assert not st.any()
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, _tag(n, "theta ~ U(0, %g)" % hi))


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_edge_rates_against_the_c_restatement(eng, n):
    """The scale rule's cases in all four output classes; and the site with rate 0 that starts at 0 is 0.0 in every output row of every
    class, bit for bit, at atol = 1e-8."""
    theta, y0, raw, st, ns = _edge(n)
    assert not st.any()
    out = tr._classes(eng, theta, y0, n, raw, ns, _tag(n, "edge rates"), rejected=True)
    for what, r in out.items():
        if r.sol is not None:
            assert not tr._bits(r.sol)[7, :, 2 + ZERO_SITE].any(), (n, what, "the zero row is not +0.0")
        else:
            F = tr._np(r.flat).reshape(len(theta), -1)
            want = pm.flatten_observables(pm.DIST, np.clip(raw[7], 0.0, None), n)
            assert not F[7].view(np.int64)[want == 0.0].any(), (n, what, "the zero row is not +0.0 in the flat vector")


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_the_four_classes_agree_bit_for_bit_on_the_edge_rates(eng, n):
    theta, y0, _, _, _ = _edge(n)
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
@pytest.mark.parametrize("n", sorted(SIZES))
def test_a_replica_does_not_depend_on_its_wave_mates(eng, n):
    """The scale of a row is the replica's own decision: sol, metric and n_steps of a replica keep their bits when the batch is permuted
    (other lane group, other wave mates) and when the edge replicas are taken out of it."""
    th_r, _, _, _ = _random(n, 20.0)
    th_e, y0_e, _, _, _ = _edge(n)
    theta = np.concatenate([th_r[:12], th_e, th_r[12:]])
    y0 = np.concatenate([np.ones((12, n + 2)), y0_e, np.ones((len(th_r) - 12, n + 2))])
    edge = np.zeros(len(theta), bool)
    edge[12:12 + len(th_e)] = True

    def run(idx):
        r = eng.solve_ode_batch(pm.DIST, theta[idx], y0[idx], n, T, want_flat=False, metric="total_signal", **tr.KW)
        assert not tr._np(r.status).any()
        return tr._bits(r.sol), tr._bits(r.metric), tr._np(r.n_steps)
    every = np.arange(len(theta))
    base = run(every)
    perm = np.random.default_rng(20500 + n).permutation(len(theta))
    assert (perm != every).sum() > len(theta) // 2
    for name, idx in (("permuted", perm), ("without the edge replicas", every[~edge])):
        got = run(idx)
        for x, y in zip(got, base):
            assert np.array_equal(x, y[idx]), (n, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", H0_SIZES)
def test_small_first_step(eng, n):
    """h0 = 1e-9: q d_j ~ 1e-9 and q s_j ~ 1e-9 on the first steps, the step has to grow through nine decades"""
    theta, raw, st, ns = _with_h0(n)
    assert not st.any()
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, _tag(n, "h0 = 1e-9"), rejected=True, h0=1e-9)
