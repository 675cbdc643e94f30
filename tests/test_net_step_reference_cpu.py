"""CPU: tests/net_step_reference.py, the numpy restatement that tests/test_gpu_network_steps.py holds the network integrator kernels to,
pinned before any GPU test relies on it: its right-hand side against the oracle, its block Jacobian against differences of the oracle,
the order of both methods with the exact block and with the approximate factorisation (the licence the kernels rely on), its loop against
the numpy prototypes the kernels were written from, double against long double in units of tau, and the premise of the forced grid."""
import sys
from pathlib import Path

import numpy as np
import pytest

import net_step_reference as nr
from oracle import network_models as nm

LD = np.longdouble
ROOT = Path(__file__).resolve().parents[1]
TAGS = nr.GOLDEN_SMALL + tuple(s[0] for s in nr.SYNTHETIC)


def _operators(net):
    """(method, operator) of every kernel route on this network."""
    if net.model != 2:
        return (("rosw", "exact"), ("ark", "exact"))
    return (("rosw", "sgs"),) + ((("ark", "exact"), ("ark", "sgs")) if int(net.n_sites.max()) <= 3 else ())


def _compared(net):
    return nr.COMPARED if net.N < 50 else nr.COMPARED[:2]


def _golden(tag, k=0):
    g = np.load(nr.GOLDEN / (tag + ".npz"))
    return g, nm.Network.from_npz(g), nm.Params.from_npz(g, k)


@pytest.mark.parametrize("tag", TAGS)
def test_rhs_equals_the_oracle_to_rounding(tag):
    desc, net, X, y0, t = nr.case(tag)
    for c, tt in ((0, 0.0), (2, 0.3), (4, 2.0), (1, 100.0), (3, 2000.0)):
        p = nr.params_of(net, X[c])
        f, ref = nr.rhs(net, p, y0[c], tt), nm.rhs(net, p, y0[c], tt)
        unit = nr.U * nr.rhs(net, p, y0[c], tt, absolute=True)                   # one rounding of the largest addend of each row
        assert (np.abs(f - ref) <= 4 * unit).all(), (tag, c, tt, float(np.max(np.abs(f - ref) / unit)))
        assert (np.abs(np.asarray(nr.rhs(net, p, y0[c], tt, LD), float) - f) <= 8 * unit).all()
        assert (unit >= nr.U * np.abs(f)).all()


def _central(net, p, y, t, h=1e-6):
    J = np.empty((net.S, net.S))
    for c in range(net.S):
        yp, ym = y.copy(), y.copy()
        yp[c] += h; ym[c] -= h
        J[:, c] = (nm.rhs(net, p, yp, t) - nm.rhs(net, p, ym, t)) / (2 * h)
    return J


def _block_mask(net):
    mask = np.zeros((net.S, net.S), bool)
    for _, st, rows in nr._blocks(net):
        mask[st:st + rows, st:st + rows] = True
    return mask


@pytest.mark.parametrize("tag", [t for t in TAGS if t != "m0_wide"])
def test_block_jacobian_is_the_block_diagonal_of_the_oracles_jacobian(tag):
    desc, net, X, y0, t = nr.case(tag)
    mask = _block_mask(net)
    for c, tt in ((0, 0.3), (4, 5.0)):
        p = nr.params_of(net, X[c])
        A, J = nr.block_jacobian(net, p, y0[c], tt), _central(net, p, y0[c], tt)
        assert (A[~mask] == 0.0).all()
        tf = np.zeros_like(mask)                                                  # the TF input: mRNA row of a block against its own protein states
        for i, st, rows in nr._blocks(net):
            tf[st, st + 1:st + rows] = True
            assert A[st, st] == -p.B_i[i] and (A[st, st + 1:st + rows] == 0.0).all()
        cmp = mask & ~tf
        assert np.max(np.abs(A - J)[cmp]) <= 1e-8 * max(1.0, np.abs(A).max()), (tag, c)      # differencing accuracy: h^2 f''' / 6 + eps |f| / h
        assert (A[cmp & (np.abs(J) < 1e-9)] == 0.0).all() and (np.abs(J[cmp & (A == 0.0)]) < 1e-9).all()      # structural zeros are exact zeros
        assert (np.abs(J[cmp]) >= 1e-9).sum() == (A != 0.0).sum()
        assert np.max(np.abs(np.asarray(nr.block_jacobian(net, p, y0[c], tt, LD), float) - A)) <= 4 * nr.U * np.abs(A).max()
        if net.model == 4:                                                        # the saturation factors are taken at y
            P = y0[c][net.offset_y + 1]
            i = int(np.argmax(net.n_sites)); st, ss = int(net.offset_y[i]), int(net.offset_s[i])
            S_all, _ = nm.site_rates(net, p, tt)
            assert abs(A[st + 2, st + 1] - S_all[ss] / (1.0 + P[i]) ** 2) <= 4 * nr.U * abs(A[st + 2, st + 1])
            assert abs(A[st + 1, st] - p.C_i[i] / (1.0 + y0[c][st]) ** 2) <= 4 * nr.U * abs(A[st + 1, st])


def test_block_jacobian_leaves_out_a_proteins_own_tf_input():
    """A protein that feeds its own mRNA row: the oracle's Jacobian has the entry, A does not."""
    import dataclasses
    for tag in ("network_m0_small", "m2_c3", "m4_c4", "m1_c4"):
        desc, net, X, y0, t = nr.case(tag)
        i = next(i for i in range(net.N) if net.TF_indptr[i + 1] > net.TF_indptr[i] and (net.model == 2 or net.driver_map[i] < 0))
        idx = net.TF_indices.copy()
        idx[net.TF_indptr[i]] = i
        loop = dataclasses.replace(net, TF_indices=idx)
        p = nr.params_of(net, X[0])
        st = int(net.offset_y[i])
        J, A = _central(loop, p, y0[0], 0.3), nr.block_jacobian(loop, p, y0[0], 0.3)
        assert abs(J[st, st + 1]) > 1e-6 and A[st, st + 1] == 0.0 and A[st, st] == -p.B_i[i]
        f, ref = nr.rhs(loop, p, y0[0], 0.3), nm.rhs(loop, p, y0[0], 0.3)
        assert np.max(np.abs(f - ref)) <= 8 * nr.U * np.max(np.abs(ref))


def test_sgs_operator_is_the_two_sweeps_of_the_kernels():
    desc, net, X, y0, t = nr.case("m2_c3")
    p = nr.params_of(net, X[1])
    A = nr.block_jacobian(net, p, y0[1], 0.3)
    g = 1.0 / (0.25 * 0.7)
    P = nr.sgs_operator(A, g)
    Dg = g - np.diag(A)
    F, K = np.tril(A, -1), np.triu(A, 1)
    np.testing.assert_allclose(P, (g * np.eye(net.S) - A) + F @ np.diag(1.0 / Dg) @ K, rtol=0, atol=1e-13 * np.abs(P).max())      # g I - A + F D_g^-1 K
    r = np.random.default_rng(3).uniform(-1, 1, net.S)
    u = np.linalg.solve(np.diag(Dg) - F, r)                                       # (D_g - F) u = r, then (D_g - K) x = D_g u
    np.testing.assert_allclose(np.linalg.solve(P, r), np.linalg.solve(np.diag(Dg) - K, Dg * u), rtol=1e-12)
    assert not np.allclose(P, g * np.eye(net.S) - A, rtol=1e-3)                   # and it is not the exact operator


ORDER_CASES = [("network_m0_small", "exact"), ("network_m1_small", "exact"), ("network_m4_small", "exact"), ("network_m2_small", "exact"),
               ("network_m2_small", "sgs")]


@pytest.mark.parametrize("tag,operator", ORDER_CASES)
def test_order_of_both_methods_with_either_operator(tag, operator):
    """Step halving inside the first kinase bucket against the oracle's LSODA at 1e-12: ARK order 4 with an embedded method of order 3
    (error estimate O(h^4)), ROS34PW2-W order 3 (estimate O(h^3)), whichever of the two operators stands in the stage equations."""
    g, net, p = _golden(tag)
    T = float(net.kin_grid[1])
    ref = nm.simulate_odeint(net, p, np.array([0.0, T]), 1e-12, 1e-12, 500000, y0=g["y0"])[1]
    for method, lo, hi in (("ark", 3.7, 4.4), ("rosw", 2.6, 3.4)):
        errs, ests = [], []
        for n in (4, 8, 16):
            y = g["y0"].astype(LD)
            for k in range(n):
                y, ev, _ = nr.STEP[method](net, p, y, 0.0, T / n, operator, LD)
                if k == 0:
                    ests.append(float(np.max(np.abs(ev))))
            errs.append(float(np.max(np.abs(np.asarray(y, float) - ref))))
        slopes = [float(np.log2(a / b)) for a, b in zip(errs[:-1], errs[1:])]
        est = [float(np.log2(a / b)) for a, b in zip(ests[:-1], ests[1:])]
        print(tag, operator, method, "global error", errs, "slopes", slopes, "estimate", ests, "slopes", est)
        assert all(lo <= s <= hi for s in slopes), (method, slopes)
        assert all(lo - 0.4 <= s <= hi + 0.2 for s in est), (method, est)          # the estimate of one step: one order below the local error


@pytest.mark.parametrize("tag", nr.GOLDEN_SMALL)
def test_loop_reproduces_the_numpy_prototypes(tag):
    """tools/proto_ark_network.py and tools/proto_rosw_network.py, which the kernels were written from: the same accepted and rejected
    steps and the same rows up to the prototypes' central-difference Jacobian (they start at h = 1e-3 and know no after_reject rule:
    none of these runs rejects twice in a row, where it would bite)."""
    sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
    try:
        import proto_ark_network as pa
        import proto_rosw_network as rw
    finally:
        del sys.path[:2]
    g, net, p = _golden(tag)
    te = g["t_eval"][:6]
    runs = [(pa.solve, "ark", "exact"), (lambda *a: rw.solve(*a, False), "rosw", "exact")] + ([(pa.solve_sgs, "ark", "sgs")] if net.model == 2 else [])
    for fn, method, operator in runs:
        Yp, steps, rej = fn(net, p, g["y0"], te, 1e-6, 1e-8)
        Y, status, (nacc, nrej) = nr.integrate(method, net, p, g["y0"], te, rtol=1e-6, atol=1e-8, h0=1e-3, operator=operator)
        assert status == 0 and (nacc + nrej, nrej) == (steps, rej), (method, operator, nacc, nrej, steps, rej)
        assert rej >= 1 and np.max(np.abs(Y - Yp) / (1e-8 + np.abs(Yp))) <= 1e-8, (method, operator)


def test_double_against_long_double_in_units_of_tau():
    """R64: how far one step evaluated in double lies from the same step in long double, in units of tau, per method and operator."""
    worst = {}
    for tag in TAGS:
        desc, net, X, y0, t = nr.case(tag)
        for method, operator in _operators(net):
            for c in _compared(net)[:2]:
                p = nr.params_of(net, X[c])
                y = y0[c].astype(LD)
                for k in range(1, t.size):
                    yl, _, maj = nr.STEP[method](net, p, y, t[k - 1], t[k] - t[k - 1], operator, LD)
                    yd, _, majd = nr.STEP[method](net, p, np.asarray(y, float), t[k - 1], t[k] - t[k - 1], operator, float)
                    assert abs(nr.tau(majd) / nr.tau(maj) - 1.0) < 1e-10 and (np.asarray(maj, float) >= np.abs(np.asarray(yl, float)) * (1 - 1e-12)).all()
                    worst[method, operator] = max(worst.get((method, operator), 0.0), float(np.max(np.abs(yd - np.asarray(yl, float)))) / nr.tau(maj))
                    y = yl
    print(worst)
    assert set(worst) == set(nr.R64)
    for key, r in worst.items():
        assert r <= nr.R64[key] <= 4 * r, (key, r)


@pytest.mark.parametrize("tag", TAGS)
def test_forced_grid_premise_holds_for_the_reference_alone(tag):
    """rtol = atol = TOL, h0 = 1e9: the restatement takes one accepted step per stop with an error norm <= 0.5 on every step, for both
    methods (the order-4 one at ARK_TOLFAC x TOL, as the library hands it to the kernel), every operator and every compared candidate --
    so that n_steps == (n_stops, 0) on the GPU is a proof."""
    desc, net, X, y0, t = nr.case(tag)
    assert 10 <= t.size <= 15 and set(net.kin_grid[net.kin_grid <= t[-1]]) <= set(t)
    worst = 0.0
    for method, operator in _operators(net):
        f = nr.ARK_TOLFAC if method == "ark" else 1.0
        for c in _compared(net):
            trace = []
            Y, status, counts = nr.integrate(method, net, nr.params_of(net, X[c]), y0[c], t, rtol=f * nr.TOL, atol=f * nr.TOL, h0=nr.H0, operator=operator, trace=trace)
            assert status == 0 and counts == (t.size - 1, 0) and len(trace) == t.size - 1 and np.isfinite(Y).all(), (method, operator, c, counts)
            assert [hs for _, hs, _ in trace] == list(np.diff(t))
            worst = max(worst, max(e for _, _, e in trace))
    print(tag, "worst error norm", worst)
    assert worst <= nr.FORCED_WORST <= 0.5
