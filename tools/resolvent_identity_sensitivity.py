"""Dev tool (CPU): how far forming the first resolvent stage from M^-1 y moves the LRP12 trajectories of the distributive model
(csrc/pk_dist_fast.hpp).

The right-hand side is affine, f(y) = J y + b with b = A in row R and zero elsewhere, and J = (I - M) / q with M = I - q J, q = gamma h:

    M^-1 h f(y) = (1 / gamma) (M^-1 (y + q b) - y)

so the step loop solves the state itself with q A added to row R, subtracts y, carries w_k = gamma z_k through the stages and uses the
weights B_k / gamma, E_k / gamma.  The numpy ports of the kernel's step (tools/inslot_sensitivity.py: resident layout;
tools/pivot_chain_sensitivity.py: shadowed layout) take `resolvent=True` for that form and `False` for the earlier solve(h f(y)).

Prints, per setting, the largest band shift |dy| / (1e-8 + 1e-6 |y|) and the step-count changes of the new first stage against the
earlier port and against the C restatement: 4 x 8 resident at n = 30 and 4 x 8 shadowed at n = 32, on the benchmark's distribution
theta ~ U(0, 20) and on theta ~ U(0, 1), and one run with a forced first step h0 = 1e-9, where q |J| is smallest and the subtraction
cancels most (reference there: the statement-for-statement port of the C code with an initial step, tests/test_gpu_dist_fast_sitesum.py).
A band shift above 0.02 or a step count off by more than 2 would mean the derivation is wrong, not rounding.
usage: resolvent_identity_sensitivity.py [replicas = 24]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import inslot_sensitivity as ins  # noqa: E402
import pivot_chain_sensitivity as pcs  # noqa: E402


def run(n, theta, resident, resolvent, h0=0.0, G=4, RPL=8):
    """[(sol, status, accepted, rejected)] of the port in the layout and first-stage form asked for."""
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import test_gpu_dist_fast_sitesum as ts
    tables, y0 = ts._tables(), np.ones(n + 2)
    if resident:
        return [ins.lrp12_resident(th, n, G, RPL, y0, ts.T, tables, h0=h0, resolvent=resolvent)[:4] for th in theta]
    return [pcs.lrp12_lanes(th, n, G, RPL, y0, ts.T, tables, True, h0=h0, resolvent=resolvent)[:4] for th in theta]


def restatement(n, theta, h0=0.0):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import test_gpu_dist_fast_sitesum as ts
    from oracle import lrp8_cpu
    if h0 > 0.0:
        sol, st, ns = ts._port_batch(theta, n, np.ones(n + 2), h0)
    else:
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, np.ones(n + 2), ts.T)
    return [(sol[b], int(st[b]), int(ns[b, 0]), int(ns[b, 1])) for b in range(len(theta))]


def against(new, old):
    """(largest band shift, median band shift, largest accepted-step difference, largest rejected-step difference)"""
    assert not any(r[1] for r in new) and not any(r[1] for r in old), "a replica ended with a status"
    shift = [ins.band(o[0], r[0]) for o, r in zip(old, new)]
    return max(shift), float(np.median(shift)), max(abs(o[2] - r[2]) for o, r in zip(old, new)), max(abs(o[3] - r[3]) for o, r in zip(old, new))


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    worst = 0.0
    for n, resident in ((30, True), (32, False)):
        for what, hi, h0 in (("theta ~ U(0, 20)", 20.0, 0.0), ("theta ~ U(0, 1)", 1.0, 0.0), ("theta ~ U(0, 20), h0 = 1e-9", 20.0, 1e-9)):
            theta = np.random.default_rng(20260515).uniform(0.0, hi, (B, 4 + 2 * n))
            new, old, ref = run(n, theta, resident, True, h0), run(n, theta, resident, False, h0), restatement(n, theta, h0)
            a, b = against(new, old), against(new, ref)
            worst = max(worst, a[0], b[0])
            print("n = %d, 4 x 8 %s, %s, %d replicas:" % (n, "resident" if resident else "shadowed", what, B))
            print("  solve(y + q b) - y against solve(h f(y)), same port: band shift max %.3e median %.3e; accepted / rejected steps differ by at most %d / %d"
                  % a)
            print("  solve(y + q b) - y against the C restatement:        band max %.3e median %.3e; accepted / rejected steps differ by at most %d / %d"
                  % b)
            assert max(a[2], a[3], b[2], b[3]) <= 2 and max(a[0], b[0]) <= 0.02, "beyond rounding: the derivation or the port is wrong"
    print("largest band over all settings: %.3e (limit 0.02)" % worst)


if __name__ == "__main__":
    main()
