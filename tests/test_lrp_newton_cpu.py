"""CPU tests of the difference form of the LRP8 / LRP12 step (csrc/pk_dist_fast.hpp; tables in csrc/pk_solve_kernel.hpp).

  * the estimator's weights E in the header ARE E[1] times a signed row of Pascal's triangle (what lets the kernel take the estimate as a
    repeated difference), read from the literals;
  * BN, the weights of y_new in the difference basis, against the exact rational change of basis of the header's B, and expanded back to
    powers of M^-1 against the order conditions solved afresh (what tests/test_integrator_tables.py asks of B);
  * a numpy model of one step in the kernel's lane layouts and operation order (tools/newton_stage_sensitivity.py): difference form with
    the tracked sum against the weighted sums in double and in long double;
  * omw_j = (q winv_j) d_j keeps its relative accuracy where 1 - winv_j has no digits left."""
import importlib.util
import re
import sys
from fractions import Fraction
from math import comb
from pathlib import Path

import mpmath as mp
import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
METHODS = [(8, "0.22"), (12, "0.16")]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _header(stages):
    """{name: [literal strings]} of ResolventTab<LRP stages>, and its DIFFERENCE flag"""
    src = (ROOT / "phoskintime_amd" / "csrc" / "pk_solve_kernel.hpp").read_text()
    blk = src[src.index("struct ResolventTab<PK_METHOD_LRP%d>" % stages):]
    blk = blk[:blk.index("\n};")]
    out = {}
    for name in ("B", "E", "BN"):
        m = re.search(r"\b%s\[(\d+)\]\s*=\s*\{([^}]*)\}" % name, blk)
        out[name] = [x.strip() for x in m.group(2).split(",")]
        assert len(out[name]) == int(m.group(1))
    out["GAM"] = re.search(r"\bGAM\s*=\s*([0-9.]+)", blk).group(1)
    out["DIFFERENCE"] = re.search(r"\bDIFFERENCE\s*=\s*(\w+)", blk).group(1)
    return out


@pytest.mark.parametrize("stages,gam", METHODS)
def test_the_estimator_is_a_repeated_difference(stages, gam):
    """E[k] = E[1] (-1)^(k-1) C(NS - 2, k - 1), k = 1 .. NS - 1 (0-based), to 1e-15 relative; E[0] = 0; the table says so."""
    h = _header(stages)
    E = [Fraction(x) for x in h["E"]]
    assert len(E) == stages and E[0] == 0 and h["DIFFERENCE"] == "true" and h["GAM"] == gam
    worst = max(abs(E[k] - E[1] * (-1) ** (k - 1) * comb(stages - 2, k - 1)) / abs(E[k]) for k in range(1, stages))
    print("LRP%d: largest relative deviation of E from E[1] x Pascal's row: %.2e" % (stages, float(worst)))
    assert worst <= Fraction(1, 10 ** 15)
    src = (ROOT / "phoskintime_amd" / "csrc" / "pk_solve_kernel.hpp").read_text()
    r4 = src[src.index("struct ResolventTab<PK_METHOD_RODAS4>"):]
    assert re.search(r"\bDIFFERENCE\s*=\s*(\w+)", r4[:r4.index("\n};")]).group(1) == "false"


@pytest.mark.parametrize("stages,gam", METHODS)
def test_bn_is_the_change_of_basis_of_b(stages, gam):
    """BN[m] = (-1)^m sum_{k >= m+1} B[k] C(k - 1, m) (0-based k) in rational arithmetic from the header's literals, to 1e-14; the last
    one is E[1], the same double."""
    h = _header(stages)
    B, BN = [Fraction(x) for x in h["B"]], [Fraction(x) for x in h["BN"]]
    assert len(BN) == stages - 1
    for m in range(stages - 1):
        want = (-1) ** m * sum(B[k] * comb(k - 1, m) for k in range(m + 1, stages))
        assert abs(BN[m] - want) <= Fraction(1, 10 ** 14) * max(1, abs(want)), (m, float(BN[m]), float(want))
    assert float(h["BN"][-1]) == float(h["E"][1]) == float(h["B"][-1])
    # and the tool prints what the header holds
    mp.mp.dps = 60
    rp = _load("restricted_pade")
    bn = rp.newton_weights(rp.solve_weights(stages, mp.mpf(gam), stages - 1))
    assert all(abs(mp.mpf(x) - y) <= mp.mpf("1e-19") * max(1, abs(y)) for x, y in zip(h["BN"], bn))


@pytest.mark.parametrize("stages,gam", METHODS)
def test_bn_satisfies_the_order_conditions(stages, gam):
    """Expanded back to powers, v_m = sum_j (-1)^j C(m, j) z_{2+j}, the weights are the ones the order conditions give: order NS - 1,
    L-stable, as tests/test_integrator_tables.py asks of B (same tolerances)."""
    mp.mp.dps = 60
    h = _header(stages)
    rp = _load("restricted_pade")
    g = mp.mpf(gam)
    BN = [mp.mpf(x) for x in h["BN"]]
    back = [mp.mpf(h["B"][0])] + [(-1) ** j * sum(BN[m] * mp.binomial(m, j) for m in range(j, stages - 1)) for j in range(stages - 1)]
    beta = rp.solve_weights(stages, g, stages - 1)
    for k in range(stages):
        assert abs(back[k] - beta[k]) < mp.mpf("2e-15") * max(1, abs(beta[k])), k
    z = mp.mpf("0.05")
    assert abs(rp.R(back, g, z) - mp.e ** z) < 1e-3 * z ** stages * 100
    assert abs(rp.R(back, g, mp.mpf("-1e12"))) < mp.mpf("1e-10")
    # the estimate E[1] v_{NS-2} expanded the same way is the header's E: the embedded method of order NS - 2
    e1 = mp.mpf(h["E"][1])
    bh = [beta[0]] + [beta[k] - e1 * (-1) ** (k - 1) * mp.binomial(stages - 2, k - 1) for k in range(1, stages)]
    assert abs(rp.R(bh, g, z) - mp.e ** z) < 1e-2 * z ** (stages - 1) * 100 and abs(bh[-1]) < mp.mpf("1e-18")


@pytest.mark.parametrize("n", (30, 32))
def test_one_step_in_the_difference_form(n):
    """4 000 random steps (theta ~ U(0, 20), y ~ U(0, 2), h log-uniform over 1e-5 .. 300) in the 4 x 8 layout, resident at n = 30 and shadowed at
    n = 32; judged on the steps a controller could take or narrowly reject, error norm in 0.01 .. 10 (at least 150 of them).
      * y_new within 1e-5 band widths (1e-8 + 1e-6 |y|) of the weighted-sum form: 50 times below the per-step share, 0.02 / 40 steps, of
        the project's band, and far above rounding (1.8e-7 measured) -- a wrong weight or a slip in the tracked sum moves y_new by
        band widths;
      * the error norm within 1e-4 relative of the long-double value (measured 5e-7; the weighted sums in double: 1.2e-6)."""
    ns = _load("newton_stage_sensitivity")
    r = ns.one_step_forms(n, nb=4000)
    use = (r["errl"] > 0.01) & (r["errl"] < 10.0)
    assert use.sum() >= 150, use.sum()
    width = 1e-8 + 1e-6 * np.abs(r["yw"])
    shift = (np.abs(r["yd"] - r["yw"]) / width).max(axis=1)[use]
    vs_l = np.asarray((np.abs(r["yd"] - r["yl"]) / width).max(axis=1), float)[use]
    w_l = np.asarray((np.abs(r["yw"] - r["yl"]) / width).max(axis=1), float)[use]
    rel = np.abs(r["errd"] / r["errl"] - 1.0)[use]
    rel_w = np.abs(r["errw"] / r["errl"] - 1.0)[use]
    print("n = %d, %d steps: y_new shift max %.2e median %.2e band widths; against long double: difference form %.2e, weighted sums %.2e; "
          "error norm relative to long double: difference form %.2e, weighted sums %.2e"
          % (n, use.sum(), shift.max(), np.median(shift), vs_l.max(), w_l.max(), rel.max(), rel_w.max()))
    assert shift.max() <= 1e-5
    assert rel.max() <= 1e-4


@pytest.mark.parametrize("n,resident", ((30, True), (32, False)))
def test_omw_keeps_its_digits(n, resident):
    """omw_j = (q winv_j) d_j against q d_j / (1 + q d_j) in long double, q d_j from 1 down to 1e-13: 1e-12 relative.  1 - winv_j, the
    form not taken, is off by more than 1e-6 there (the test would see it)."""
    ns = _load("newton_stage_sensitivity")
    rng = np.random.default_rng(181)
    nb = 2000
    th = rng.uniform(0.05, 20.0, (nb, 4 + 2 * n))
    q = 10.0 ** rng.uniform(-14.5, 0.0, nb)
    L = ns.Lanes(th, n, 4, 8, resident)
    ld = np.longdouble
    qd = q.astype(ld)[:, None, None] * L.dg.astype(ld)
    want = qd / (1 + qd)
    if resident:
        want[:, 1, 0] = 1                                       # the P slot: v' = v - x_P
    assert float(np.abs(qd).min()) < 1e-13

    def worst(cancelling):
        L.factor(q, cancelling_omw=cancelling)
        w = float(np.max(np.abs(L.omw.astype(ld) - want) / np.abs(want)))
        if not resident:
            qb = (q * th[:, 1]).astype(ld)[:, None]
            w = max(w, float(np.max(np.abs(L.omwR.astype(ld) - qb / (1 + qb)) / (qb / (1 + qb)))))
        return w
    good, bad = worst(False), worst(True)
    print("n = %d: largest relative error of omw: (q winv) d %.2e, 1 - winv %.2e" % (n, good, bad))
    assert good <= 1e-12
    assert bad > 1e-6
