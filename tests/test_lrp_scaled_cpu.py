"""CPU tests of the scaled stages of the LRP12 step (csrc/pk_dist_fast.hpp: site rows carried in units of their coupling weight), on the
numpy model of tools/scaled_stage_sensitivity.py (the kernel's lane layouts and operation order):

  * one step in the scaled form is as close to the long-double weighted sums as the current difference form is, within a factor of two
    (both distances are a few roundings of differing order; a wrong derivation moves y_new by band widths);
  * the scale rule: a zero-rate row that starts at zero stays zero bit for bit, one that starts at 1 decays as in the unscaled port;
  * c_j ic_j = 1 to 4 ulp, over steps from 1e-13 to 300."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    sys.path.insert(0, str(ROOT / "tools"))
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", (30, 32))
def test_one_scaled_step_is_as_close_to_long_double_as_the_current_form(n):
    """one_step_forms' 4 000 random steps (theta ~ U(0, 20), y ~ U(0, 2), h log-uniform over 1e-5 .. 300), 4 x 8 resident at n = 30 and
    shadowed at n = 32: the largest distance of y_new to the long-double weighted sums, in band widths 1e-8 + 1e-6 |y|, and the largest
    relative distance of the error norm to the long-double one, are at most twice those of the current difference form.  y_new is judged
    over all steps, the error norm on the steps a controller could take or narrowly reject (norm in 0.01 .. 10, at least 150 of them, as
    in tests/test_lrp_newton_cpu.py).  Measured: y_new 2.00e-7 (scaled) against 1.88e-7 (current) band widths at n = 30, 2.25e-7 against
    1.83e-7 at n = 32; error norm 4.97e-7 and 5.10e-7 in both forms."""
    ss = _load("scaled_stage_sensitivity")
    cur = ss.nss.one_step_forms(n, nb=4000)
    scl = ss.one_step_scaled(n, nb=4000)
    assert np.array_equal(cur["y"], scl["y"]) and np.array_equal(np.asarray(cur["yl"], float), np.asarray(scl["yl"], float))
    width = 1e-8 + 1e-6 * np.abs(cur["yw"])

    def dist(r):
        y = float(np.max(np.asarray(np.abs(r["yd"] - r["yl"]) / width, float)))
        el = np.asarray(r["errl"], float)
        judged = (el > 0.01) & (el < 10.0)
        assert judged.sum() >= 150
        e = float(np.max(np.abs(np.asarray(r["errd"] / r["errl"], float) - 1.0)[judged]))
        return y, e
    (yc, ec), (ys, es) = dist(cur), dist(scl)
    print("n = %d: y_new against long double: scaled %.3e, current %.3e band widths; error norm: scaled %.3e, current %.3e relative"
          % (n, ys, yc, es, ec))
    assert ys <= 2.0 * yc
    assert es <= 2.0 * ec


@pytest.mark.parametrize("n,resident", ((30, True), (32, False)))
def test_the_scale_rule(n, resident):
    """Whole integrations, 4 x 8: site 3 has rate 0.  Started at 0 its trajectory is 0.0 in every output, bit for bit (scale 0: every
    value of the row is 0 w_j); started at 1 it decays under the scale 2^-600 as in the unscaled port, to 1e-13 absolute, with the same
    statuses and step counts.  A rate of 1e-300 and of 1e-12 likewise."""
    ss = _load("scaled_stage_sensitivity")
    ts, _ = ss.nss._old_tabs()
    tabs = ss.nss.header_tables(12)
    th = ss.edge_thetas(n)
    for b, y3 in ((7, 0.0), (0, 1.0), (1, 1.0), (2, 1.0), (3, 1.0)):
        y0 = np.ones(n + 2)
        y0[2 + 3] = y3
        a = ss.lrp12_scaled(th[b], n, 4, 8, y0, ts.T, tabs, resident)
        o = ss.nss.lrp12_newton(th[b], n, 4, 8, y0, ts.T, tabs, resident)
        d = float(np.max(np.abs(a[0] - o[0])))
        print("n = %d replica %d (y0_3 = %g): status %d / %d, steps %s / %s, max |scaled - unscaled| = %.2e" % (n, b, y3, a[1], o[1], a[2:], o[2:], d))
        assert a[1] == 0 and a[1:] == o[1:]
        assert d <= 1e-13
        if y3 == 0.0:
            assert (a[0][:, 2 + 3] == 0.0).all() and not np.signbit(a[0][:, 2 + 3]).any()
        if b == 0:
            assert a[0][-1, 2 + 3] < 1.0 and a[0][-1, 2 + 3] == pytest.approx(o[0][-1, 2 + 3], abs=1e-13)


@pytest.mark.parametrize("n,resident", ((30, True), (32, False)))
def test_c_times_ic_is_one(n, resident):
    """c_j = winv_j s_j and ic_j = piv_j / s_j of every scaled row with a positive scale: their product within 4 ulp of 1 (two roundings
    of the products, the chain's reciprocal, 1 / s_j), q from 1e-13 to 50; rates from U(0, 20) and the edge rates down to 2^-600."""
    ss = _load("scaled_stage_sensitivity")
    rng = np.random.default_rng(404)
    nb = 2000
    th = rng.uniform(0.0, 20.0, (nb, 4 + 2 * n))
    th[:8] = ss.edge_thetas(n)
    q = 10.0 ** rng.uniform(-13.0, np.log10(50.0), nb)
    L = ss.ScaledLanes(th, n, 4, 8, resident)
    L.load(np.ones((nb, n + 2)))
    L.factor(q)
    J0 = L.J0
    live = L.s[..., J0:] != 0.0
    assert live.sum() >= nb * (n - 4)
    prod = (L.c[..., J0:] * L.ic[..., J0:])[live]
    worst = float(np.max(np.abs(prod - 1.0))) / np.finfo(float).eps
    print("n = %d: largest |c ic - 1| = %.2f ulp over %d rows" % (n, worst, live.sum()))
    assert worst <= 4.0
    assert (L.c[..., J0:][~live] == 0.0).all() and (L.ic[..., J0:][~live] == 0.0).all()
