"""CPU: the exact sensitivity reference the GPU kernels are held to (tests/net_sens_reference.py, stored in
tests/golden/net_sens_m*_small.npz) agrees with Richardson-extrapolated central differences of the oracle's ``simulate_odeint``.

On the four ``network_m*_small`` fixtures, candidate 0 (candidates 1 and 2: the c_k and E_i columns), one column per parameter kind (c_k, A_i, B_i, C_i, D_i, Dp_i, E_i, tf_scale):
D(h) = (Y(x + h) - Y(x - h)) / 2h with h = 2e-3 x_c and 1e-3 x_c at rtol = atol = 1e-12, extrapolated R = (4 D(h / 2) - D(h)) / 3.
The differences carry the integration noise of two LSODA runs divided by 2h (the adaptive steps and the 14 kinase-bucket edges make
the differenced trajectory noisy) and an O(h^2) truncation term; |D(h) - D(h / 2)| measures both (it is 3/4 of the truncation term of D(h)
plus the noise).  The bound per column is

    max |ref - R| <= MARGIN max |D(h) - D(h / 2)| + self_err,         MARGIN = 2

-- R's own error is the noise of D(h / 2) amplified by 4/3 plus that of D(h) by 1/3, i.e. at most 5/3 of the larger noise, and its
truncation remainder is O(h^4); 2 covers both.  Measured here with the columns the stored references use (entry 1 of each group), the
consistency max |D(h) - D(h / 2)| is 3.1e-9 .. 3.0e-6 of the column maximum and max |ref - R| is 8.4e-10 .. 3.4e-7 of it: the reference,
not the differences, is what the GPU is held to.

The reference's own tolerance-halving self-consistency (LSODA at 1e-12 against 1e-10, stored as ``self_err``), worst over the three stored
candidates and the eight columns, relative to the column maximum: 3.5e-10 (distributive), 4.9e-10 (sequential), 3.3e-10 (combinatorial),
5.0e-10 (saturating); SELF_ERR_MAX = 1e-8 is asserted on the stored data.  A second test integrates one column of the
reference afresh and compares it with the stored values, so stale fixtures cannot pass."""
import numpy as np
import pytest

import net_sens_reference as ref
from oracle import network_models as nm

MARGIN = 2.0
SELF_ERR_MAX = 1e-8


@pytest.mark.parametrize("name", ref.NAMES)
def test_reference_agrees_with_extrapolated_differences(name):
    g, net, X = ref.fixture(name)
    gold = ref.load_golden(name)
    cols, names = ref.columns_one_per_kind(net)
    assert np.array_equal(gold["cols"], cols) and list(gold["names"]) == names and np.array_equal(gold["X"], X)
    sim = lambda row: nm.simulate_odeint(net, ref.row_to_params(net, row), g["t_eval"], 1e-12, 1e-12, 500000, y0=g["y0"])
    # candidate 0: every column; candidates 1 and 2 (whose TF inputs change sign along the way on some fixtures): the c_k and E_i columns
    for k, qs in ((0, range(len(cols))), (1, (0, 6)), (2, (0, 6))):
        assert np.abs(gold["Y"][k] - sim(X[k])).max() <= 1e-9
        for q in qs:
            c = cols[q]
            D = []
            for rel in (2e-3, 1e-3):
                h = rel * X[k][c]
                rp = X[k].copy(); rp[c] += h
                rm = X[k].copy(); rm[c] -= h
                D.append((sim(rp) - sim(rm)) / (2.0 * h))
            R = (4.0 * D[1] - D[0]) / 3.0
            refc = gold["dY"][k][:, :, q]
            cmax = np.abs(refc).max()
            cons, err = np.abs(D[0] - D[1]).max(), np.abs(refc - R).max()
            print(f"{name} candidate {k} {names[q]}: max|col| {cmax:.3e}  |D(h) - D(h/2)| / max {cons / cmax:.2e}  |ref - R| / max {err / cmax:.2e}  "
                  f"self_err / max {gold['self_err'][k][q] / cmax:.2e}")
            assert err <= MARGIN * cons + gold["self_err"][k][q], (k, names[q])


@pytest.mark.parametrize("name", ref.NAMES)
def test_stored_reference_is_self_consistent_and_current(name):
    g, net, X = ref.fixture(name)
    gold = ref.load_golden(name)
    cmax = np.abs(gold["dY"]).max(axis=(1, 2))
    assert gold["dY"].shape == (ref.N_CAND, g["t_eval"].size, net.S, 8) and (cmax > 0).all()
    print(f"{name}: self_err / max|column|, worst {np.max(gold['self_err'] / cmax):.2e}")
    assert (gold["self_err"] <= SELF_ERR_MAX * cmax).all()
    # one column afresh over the first six output times at a looser tolerance (quick): within that tolerance's own error of the stored values
    q = 3
    _, d = ref.tangent_reference(net, X[1], gold["cols"][[q]], g["t_eval"][:6], y0=g["y0"], rtol=1e-9, atol=1e-9)
    assert np.abs(d[:, :, 0] - gold["dY"][1][:6, :, q]).max() <= 1e-5 * cmax[1, q]
