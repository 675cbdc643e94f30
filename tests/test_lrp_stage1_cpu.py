"""CPU tests of the first LRP12 stage formed from the state itself and of the single-chain stage dot product (csrc/pk_dist_fast.hpp,
DESIGN 4.3), on the numpy model of tools/stage1_form_sensitivity.py (Stage1Lanes: ScaledLanes with t_j = kappa_j y_j, the dot term
fma(winv_j, y_j, .) and zeta_j = fma(-q, t_j, xq) in the first stage, and one FMA chain per dot product):

  * one step is as close to the long-double weighted sums as the scaled form it replaces, within the margin of tests/test_lrp_scaled_cpu.py
    (a factor of two on y_new and on the error norm);
  * whole integrations on the tool's six settings stay within the project's limits of the scaled form: band shift <= 0.02, steps within 2;
  * the edge rates of the scale rule end with equal statuses and step counts, and the zero-rate row that starts at zero is +0.0 throughout;
  * the P-slot fix-ups of factor() as arithmetic on two per-lane constants give the bits of the selects they replace."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
BAND, STEPS = 0.02, 2
REPLICAS = 24


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
def test_one_step_is_as_close_to_long_double_as_the_current_form(n):
    """one_step_forms' 4 000 random steps, 4 x 8 resident at n = 30 and shadowed at n = 32, judged as in tests/test_lrp_scaled_cpu.py: the
    largest distance of y_new to the long-double weighted sums in band widths 1e-8 + 1e-6 |y| over all steps, and the largest relative
    distance of the error norm to the long-double one over the steps a controller could take or narrowly reject (norm in 0.01 .. 10, at
    least 150 of them), are at most twice those of the current (scaled) form.  Measured: y_new 2.36e-7 (new) against 2.00e-7 (current) band
    widths at n = 30, 2.45e-7 against 2.25e-7 at n = 32; error norm 4.97e-7 and 5.10e-7 in both forms."""
    s1 = _load("stage1_form_sensitivity")
    cur = s1.sss.one_step_scaled(n, nb=4000)
    new = s1.one_step_stage1(n, nb=4000)
    assert np.array_equal(cur["y"], new["y"]) and np.array_equal(np.asarray(cur["yl"], float), np.asarray(new["yl"], float))
    assert not np.array_equal(cur["yd"], new["yd"]), "the new form ran the current one"
    width = 1e-8 + 1e-6 * np.abs(cur["yw"])

    def dist(r):
        y = float(np.max(np.asarray(np.abs(r["yd"] - r["yl"]) / width, float)))
        el = np.asarray(r["errl"], float)
        judged = (el > 0.01) & (el < 10.0)
        assert judged.sum() >= 150
        e = float(np.max(np.abs(np.asarray(r["errd"] / r["errl"], float) - 1.0)[judged]))
        return y, e
    (yc, ec), (yn, en) = dist(cur), dist(new)
    print("n = %d: y_new against long double: new %.3e, current %.3e band widths; error norm: new %.3e, current %.3e relative"
          % (n, yn, yc, en, ec))
    assert yn <= 2.0 * yc
    assert en <= 2.0 * ec


@pytest.mark.parametrize("setting", range(6))
def test_whole_integrations_against_the_current_form(setting):
    """The tool's six settings (n = 30 resident and n = 32 shadowed on 4 x 8; theta ~ U(0, 20), U(0, 1), and U(0, 20) from a forced first
    step of 1e-9), 24 replicas each: status 0 in both forms, band shift at most 0.02, accepted and rejected steps within 2.  Measured: the
    largest shift over the six settings is 8.0e-9, no step count moves."""
    s1 = _load("stage1_form_sensitivity")
    ins = _load("inslot_sensitivity")
    ts, _ = s1.nss._old_tabs()
    tabs = s1.nss.header_tables(12)
    n, resident, what, hi, h0 = s1.SETTINGS[setting]
    theta = np.random.default_rng(20260515).uniform(0.0, hi, (REPLICAS, 4 + 2 * n))
    y0 = np.ones(n + 2)
    worst = 0.0
    for b, th in enumerate(theta):
        a = s1.lrp12_stage1(th, n, 4, 8, y0, ts.T, tabs, resident, h0=h0)
        o = s1.sss.lrp12_scaled(th, n, 4, 8, y0, ts.T, tabs, resident, h0=h0)
        assert a[1] == 0 and o[1] == 0, (n, what, b)
        assert abs(a[2] - o[2]) <= STEPS and abs(a[3] - o[3]) <= STEPS, (n, what, b, a[2:], o[2:])
        worst = max(worst, ins.band(o[0], a[0]))
    print("n = %d %s, %s: largest band shift against the current form %.3e" % (n, "resident" if resident else "shadowed", what, worst))
    assert worst <= BAND


@pytest.mark.parametrize("n,resident", ((30, True), (32, False)))
def test_the_edge_replicas(n, resident):
    """edge_thetas (a rate exactly 0, every rate 0, rates of 1e-300, 1e-12 and 1e6, rates over eight decades, a healthy replica, and a
    zero-rate site that starts at 0): statuses and step counts equal those of the current form, and the zero-rate-from-zero row is +0.0
    in every output."""
    s1 = _load("stage1_form_sensitivity")
    ts, _ = s1.nss._old_tabs()
    tabs = s1.nss.header_tables(12)
    th = s1.sss.edge_thetas(n)
    for b in range(8):
        y0 = np.ones(n + 2)
        if b == 7:
            y0[2 + 3] = 0.0
        a = s1.lrp12_stage1(th[b], n, 4, 8, y0, ts.T, tabs, resident)
        o = s1.sss.lrp12_scaled(th[b], n, 4, 8, y0, ts.T, tabs, resident)
        assert a[1] == 0 and a[1:] == o[1:], (n, b, a[1:], o[1:])
        assert ins_band(o[0], a[0]) <= BAND, (n, b)
        if b == 7:
            assert (a[0][:, 2 + 3] == 0.0).all() and not np.signbit(a[0][:, 2 + 3]).any()


def ins_band(a, b):
    return _load("inslot_sensitivity").band(a, b)


def test_the_p_slot_fixups_as_arithmetic_have_the_bits_of_the_selects():
    """factor() ends the P slot (row 0 of lane 1) with four selects on isP; with selP = 1 in that lane and 0 elsewhere, notP = 1 - selP, and
    the P lane's diagonal slot rewritten to 1.0, they are one changed addend and three operations.  10 000 random finite
    (q, dg0, winv0, cw0, omw0), both values of isP: the same 64 bits in all four.  q = gamma h is positive; dg0, cw0 and omw0 take both
    signs, and so does winv0 in a lane that is not P; in the P lane cw0 is 0 (its rate slot is 0) and winv0 is positive, being the chain's
    1 / q.  The sign matters in one place: winv0 * notP is a zero of winv0's sign in the P lane, -0.0 for a negative winv0 where the select
    gave +0.0 (asserted below, so that the restriction is on record; no step has a negative q).
    numpy has no fused multiply-add; every product here has a factor 0 or 1 or an addend 0, so the unfused form rounds once, as the FMA
    does -- except q dg0 + 1 in the other lanes, which is the same expression on both sides."""
    rng = np.random.default_rng(20261021)
    nb = 10000

    def draw(signed):
        mag = 10.0 ** rng.uniform(-12.0, 6.0, nb)
        return mag * rng.choice([-1.0, 1.0], nb) if signed else mag

    def bits(x):
        return np.asarray(x, float).view(np.int64)
    q, dg0, cw0, omw0 = draw(False), draw(True), draw(True), draw(True)
    for isP in (False, True):
        winv0 = draw(not isP)
        selP = np.full(nb, 1.0 if isP else 0.0)
        notP = 1.0 - selP
        dgs = np.ones(nb) if isP else dg0                       # the P lane's diagonal slot is 1.0 after the prologue
        cw = np.zeros(nb) if isP else cw0
        assert np.array_equal(bits(q * dgs + notP), bits(q if isP else q * dg0 + 1.0)), isP
        assert np.array_equal(bits(winv0 * selP + cw), bits(winv0 if isP else cw)), isP
        assert np.array_equal(bits(winv0 * notP), bits(np.zeros(nb) if isP else winv0)), isP
        assert np.array_equal(bits(omw0 * notP + selP), bits(np.ones(nb) if isP else omw0)), isP
    assert np.signbit(-draw(False) * 0.0).all()
