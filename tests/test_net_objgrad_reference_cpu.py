"""CPU: the plain-loop reference chain the GPU objective gradient is held to (tests/net_objgrad_reference.py) against differences of the
oracle, on the stored exact ``Y`` / ``dY`` of tests/golden/net_sens_m*_small.npz (three candidates, eight columns per fixture).

Loss data: every protein / site at every time, rna from t = 4 on (``rna_base_idx`` > 0); observations are candidate 0's reference
predictions times exp(0.2 N(0, 1)), weights U(0.5, 2), seed 3.

``dsums[m, c]`` is the derivative of ``nm.loss_function`` along the direction ``dY[..., c]`` of the trajectory: it is compared with
R = (4 D(e / 2) - D(e)) / 3 of the central differences D(e) = (L(Y + e dY_c) - L(Y - e dY_c)) / 2e, e = 1e-3 / max|dY_c| and half of
it.  As in test_net_sens_reference_cpu.py the consistency of the two step sizes is the tolerance (MARGIN = 2), plus the rounding of a
difference quotient that the consistency of an exactly quadratic loss does not show: two sums of n terms, each within
(n + 17) 2^-53 of its ``mag``, divided by e.  Mode 2 is NaN where a residual is negative: NaN positions must agree with the oracle (with these
observations every modality has such an entry, so mode 2's sums are NaN throughout and its formula is held entry by entry in
test_net_loss_grad_cpu.py).  The
prior term is checked against central differences of ``nm.objectives`` in x (a quadratic: the difference is exact up to rounding).

Conditions on the inputs, asserted: no floor of the fold change is active on the stored trajectories, and every objective's largest
gradient entry is non-zero on every fixture and candidate.  The rna objective has structurally zero columns (a parameter that reaches
no observed mRNA): five on network_m1_small's candidate 2, one on every candidate of network_m4_small; no others are excused."""
import numpy as np
import pytest

import net_objgrad_reference as og
import net_sens_reference as ref
from oracle import network_models as nm

MARGIN = 2.0
ZERO_RNA_COLUMNS = {("network_m1_small", 2): 5, ("network_m4_small", 0): 1, ("network_m4_small", 1): 1, ("network_m4_small", 2): 1}
LAM, LAMD = og.LAM, og.LAMD
_setup = og.fixture_data


@pytest.mark.parametrize("name", ref.NAMES)
def test_conditions_on_the_inputs(name):
    s = _setup(name)
    for k in range(ref.N_CAND):
        r = og.chain(s["net"], s["gold"]["Y"][k], s["gold"]["dY"][k], s["ld"], 0, s["X"][k], s["defaults"], LAM, s["gold"]["cols"])
        assert r["floors"] == 0
        assert (np.abs(r["dsums"]).max(axis=1) > 0).all() and (np.abs(r["dF"]).max(axis=1) > 0).all()
        zeros = (r["dsums"] == 0).sum(axis=1)
        assert zeros[0] == 0 and zeros[2] == 0 and zeros[1] == ZERO_RNA_COLUMNS.get((name, k), 0), (name, k, zeros)


@pytest.mark.parametrize("mode", range(8))
@pytest.mark.parametrize("name", ref.NAMES)
def test_sums_and_dsums_against_directional_differences_of_the_oracle(name, mode):
    s = _setup(name)
    net, gold, ld, ldo = s["net"], s["gold"], s["ld"], s["ldo"]
    worst = 0.0
    for k in range(ref.N_CAND):
        Y, dY = gold["Y"][k], gold["dY"][k]
        r = og.chain(net, Y, dY, ld, mode, s["X"][k], s["defaults"], LAM, gold["cols"])
        L0 = np.array(nm.loss_function(net.model, Y, ldo, mode))
        nanpos = np.isnan(L0)
        assert np.array_equal(np.isnan(r["sums"]), nanpos) and (mode == 2 or not nanpos.any())
        ok = ~nanpos
        assert (np.abs(r["sums"][ok] - L0[ok]) <= og.bound(r, "sums")[ok]).all()
        F0 = nm.objectives(net, s["X"][k], s["defaults"], Y, ldo, mode, LAMD)
        assert (np.abs(r["F"][ok] - F0[ok]) <= og.bound(r, "F")[ok]).all()
        assert np.array_equal(np.isnan(r["dsums"]).any(axis=1), nanpos)
        for c in range(dY.shape[2]):
            e = 1e-3 / np.abs(dY[:, :, c]).max()
            D = [(np.array(nm.loss_function(net.model, Y + h * dY[:, :, c], ldo, mode)) - np.array(nm.loss_function(net.model, Y - h * dY[:, :, c], ldo, mode))) / (2 * h)
                 for h in (e, e / 2)]
            R = (4.0 * D[1] - D[0]) / 3.0
            cons = np.abs(D[0] - D[1])
            floor = 2.0 * (r["n"]["sums"] + og.OPS["sums"]) * og.U * r["mag"]["sums"] / e
            tol = MARGIN * cons + floor
            err = np.abs(r["dsums"][:, c] - R)
            assert (err[ok] <= tol[ok]).all(), (name, mode, k, c, err, tol)
            worst = max(worst, float(np.max(err[ok] / tol[ok])) if ok.any() else 0.0)
    print(f"{name} mode {mode}: worst |dsums - R| / (MARGIN |D(e) - D(e/2)| + rounding) = {worst:.3f}")


@pytest.mark.parametrize("name", ref.NAMES)
def test_prior_term_against_differences_of_the_objectives_in_x(name):
    s = _setup(name)
    net, gold = s["net"], s["gold"]
    cols = gold["cols"]
    kinds = [str(n).rsplit("_", 1)[0] for n in gold["names"]]
    for k in range(ref.N_CAND):
        Y, x = gold["Y"][k], s["X"][k]
        r = og.chain(net, Y, gold["dY"][k], s["ld"], 0, x, s["defaults"], LAM, cols)
        norm = np.array([1.0 / max(1e-6, float(np.sum(s["ld"][w]))) for w in ("w_prot", "w_rna", "w_pho")])
        dprior = r["dF"] - r["dsums"] * (norm * np.array(LAM[:3]))[:, None]
        for q, c in enumerate(cols):
            h = 1e-4 * x[c]
            xp = x.copy(); xp[c] += h
            xm = x.copy(); xm[c] -= h
            fd = (nm.objectives(net, xp, s["defaults"], Y, s["ldo"], 0, LAMD) - nm.objectives(net, xm, s["defaults"], Y, s["ldo"], 0, LAMD)) / (2 * h)
            # F ~ 1e2 .. 1e4 here: rounding 2^-53 |F| / h on both sides, and the cancellation in dF - dsums norm lambda
            tol = 8 * og.U * (np.abs(r["F"]) / h + np.abs(r["dF"][:, q]) + np.abs(r["mag"]["dF"][:, q]))
            assert (np.abs(dprior[:, q] - fd) <= tol).all(), (k, q, dprior[:, q], fd)
            assert (fd != 0).all() == (kinds[q] in ("A_i", "B_i", "C_i", "D_i", "E_i")), kinds[q]
            # a scale factor on the prior term multiplies it, as softplus' does for raw candidates
            r2 = og.chain(net, Y, gold["dY"][k], s["ld"], 0, x, s["defaults"], LAM, cols, scl=np.full(cols.size, 0.25))
            assert np.allclose(r2["dF"][:, q] - r2["dsums"][:, q] * norm * np.array(LAM[:3]), 0.25 * dprior[:, q], rtol=0, atol=tol.max())
