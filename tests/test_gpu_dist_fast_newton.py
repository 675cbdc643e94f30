"""The step loop of the distributive throughput kernels (csrc/pk_dist_fast.hpp) takes the LRP8 / LRP12 error estimate as a repeated
difference: two solves, then NS - 2 stages v <- v - M^-1 v whose group sum comes from a sum carried from stage to stage (lam), with
omw_j = 1 - winv_j formed as (q winv_j) d_j; y_new is summed in that basis (ResolventTab::BN) and the estimate is the last v times
E_2 / gamma.  The C restatement (oracle/lrp8_dist.c through oracle/lrp8_cpu.py) keeps its weighted sums over twelve solves and is the
yardstick, at the project's limits: band error <= 0.02, accepted steps within 2, rejected steps within 2 where rejects are forced.

Every branch of the new stage runs here, in all four output classes (tests/test_gpu_dist_fast_resolvent.py: _classes): one row per lane
(no tracked sum in the resident layout, one element in the shadowed one), the register and the parked layouts, four and eight lanes, an idle
slot, both layouts side by side at n = 30 / 32, LRP8 on its 8 x 4 shadowed table.  Batches of 17-48 replicas leave a wave partial.  Two
batches aim at the tracked sum (rows and coefficients spread over nine and six decades), and the first steps h0 = 1e-9, 1e-12 at omw.

The forced first reject (h0 = 10) and the small first steps need a reference that takes an initial step: the statement-for-statement
numpy port of the C code (tests/test_gpu_dist_fast_sitesum.py, held to the C code's bits there).  It states LRP12; LRP8 runs without a
forced step."""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lrp8_cpu
from oracle import protein_models as pm

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_gpu_dist_fast_resolvent as tr  # noqa: E402  (_classes: the four output classes against the restatement's trajectories)
import test_gpu_dist_fast_sitesum as ts  # noqa: E402  (the numpy port of the C restatement with an initial step)

T = pm.TIME_POINTS
# n: (G x RPL, layout, replicas)
SIZES = {2: ("4 x 1", "resident", 17), 4: ("4 x 1", "shadowed", 23), 14: ("4 x 4", "resident", 33), 29: ("4 x 8", "resident, one idle slot", 41),
         30: ("4 x 8", "resident", 48), 32: ("4 x 8", "shadowed", 37), 38: ("8 x 5", "resident", 19), 64: ("8 x 8", "shadowed", 29)}
NREJ = 17                           # replicas of the forced-reject and first-step runs (the port is Python)


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


def _plain(n, **kw):
    def make():
        theta = tr._theta(n, SIZES[n][2], 18000 + n)
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), T, **kw)
        assert not st.any()
        return theta, sol, ns
    return _frozen(("plain", n, tuple(sorted(kw.items()))), make)


def _with_h0(n, h0, seed):
    def make():
        theta = tr._theta(n, NREJ, seed + n)
        sol, st, ns = ts._port_batch(theta, n, np.ones(n + 2), h0)
        return theta, sol, st, ns
    return _frozen(("h0", n, h0), make)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_lrp12_against_the_c_restatement(eng, n):
    theta, raw, ns = _plain(n)
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "%s %s" % SIZES[n][:2])


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(SIZES))
def test_forced_first_reject(eng, n):
    """h0 = 10: the first step of every replica is rejected (the reference must reject it too, or the test is not about rejects)."""
    theta, raw, st, ns = _with_h0(n, 10.0, 18100)
    assert not st.any() and ns[:, 1].min() >= 1, (n, "the restatement does not reject the forced first step")
    out = tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "%s %s, h0 = 10" % SIZES[n][:2], rejected=True, h0=10.0)
    for what, r in out.items():
        assert tr._np(r.n_steps)[:, 1].min() >= 1, (n, what, "a replica rejected nothing")


@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 32))
def test_lrp8_against_the_c_restatement(eng, n):
    """8 x 4 shadowed (the LRP8 table has no resident half): six difference stages, BN of LRP8"""
    theta, raw, ns = _plain(n, stages=8, rtol=1e-7, atol=1e-9)
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "lrp8", rejected=True, method="lrp8", rtol=1e-7, atol=1e-9)


# ---------------------------------------------------------------- batches that aim at the tracked sum
def _tracked_batches(n):
    """(name, theta [nb, P], y0 [nb, S]).  lam = sum v_j is carried through ten stages by lam' = sum p_j - x_P Cl: rows of very different
    size and cw_j of very different size are where a slip in it (a row left out, Cl over the wrong rows) or its rounding would show.

    Batch one: the replicas' initial values are spread over 1e-6 .. 1e3 as one scale per replica (times U(0.5, 2) per state), so that both
    terms of the band, atol and rtol |y|, are met; rates and D_i spread over four decades then pull the site rows of a replica up to eight
    decades apart (x_i -> S_i P / (1 + D_i)).  Spreading the initial values over nine decades WITHIN a replica as well is not a case these
    limits can be held on: the restatement's own rounding (weights up to 240, 2^-53 of a row near 1e3, against a band of 1e-8 on a row
    near 1e-6, every step) then puts the restatement itself 0.04 .. 0.12 band widths from the closed form, and two weighted-sum
    implementations that differ in summation order alone 0.028 apart (measured with the CPU ports of tools/)."""
    nb = 17
    rng = np.random.default_rng(18200 + n)
    th = rng.uniform(0.0, 20.0, (nb, pm.n_params(pm.DIST, n)))
    th[:, 4:4 + 2 * n] = 10.0 ** rng.uniform(-3.0, np.log10(20.0), (nb, 2 * n))
    y0 = 10.0 ** np.linspace(-6.0, 3.0, nb)[:, None] * rng.uniform(0.5, 2.0, (nb, n + 2))
    out = [("y0 over 1e-6 .. 1e3, rates and D_i over 1e-3 .. 20", th, y0)]
    th = rng.uniform(0.0, 20.0, (nb, pm.n_params(pm.DIST, n)))
    th[:, 4:4 + n] = 1e-3 * rng.uniform(0.5, 2.0, (nb, n))
    hot = rng.integers(0, n, nb)                                   # any row of any lane, row 0 of the resident layout included
    th[np.arange(nb), 4 + hot] *= 1e6
    out.append(("one site rate 1e6 times the others", th, np.ones((nb, n + 2))))
    return out


def _tracked_ref(n):
    def make():
        out = []
        for name, th, y0 in _tracked_batches(n):
            res = [lrp8_cpu.solve_batch(th[b:b + 1], n, y0[b], T) for b in range(len(th))]
            out.append((name, th, y0, np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), np.concatenate([r[2] for r in res])))
        return out
    return _frozen(("tracked", n), make)


def test_the_restatement_finishes_the_tracked_sum_batches():
    """CPU: the inputs of the next test are ones the C restatement ends with status 0, after a run of steps."""
    for n in (30, 32):
        for name, _, _, _, st, ns in _tracked_ref(n):
            assert not st.any(), (n, name)
            assert ns[:, 0].min() > 10, (n, name)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (30, 32))
def test_tracked_sum_batches(eng, n):
    for name, th, y0, raw, st, ns in _tracked_ref(n):
        assert not st.any(), (n, name)
        tr._classes(eng, th, y0, n, raw, ns, name, rejected=True)


# ---------------------------------------------------------------- first steps at which 1 - winv keeps no digits
def test_the_restatement_finishes_the_small_first_steps():
    for n in (30, 32):
        for h0 in (1e-9, 1e-12):
            _, _, st, ns = _with_h0(n, h0, 18300)
            assert not st.any() and ns[:, 0].min() > 10, (n, h0)   # the step really starts small and has to grow


@pytest.mark.gpu
@pytest.mark.parametrize("h0", (1e-9, 1e-12))
@pytest.mark.parametrize("n", (30, 32))
def test_small_first_steps(eng, n, h0):
    """q d_j is 1e-7 .. 1e-13 on the first steps: omw_j = (q winv_j) d_j holds its digits there, 1 - winv_j would not"""
    theta, raw, st, ns = _with_h0(n, h0, 18300)
    assert not st.any(), (n, h0)
    tr._classes(eng, theta, np.ones(n + 2), n, raw, ns, "h0 = %g" % h0, rejected=True, h0=h0)
