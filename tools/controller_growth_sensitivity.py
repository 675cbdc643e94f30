"""Dev tool (CPU): how far the reciprocal-free controller moves the LRP12 trajectories of the distributive model (the step loop of
csrc/pk_dist_fast.hpp).

The kernel took  fac = clamp(err^(1/Q) / 0.9, 1/6, 5), hnew = hs / fac  with err^(1/Q) through v_log_f32 / v_exp_f32 and 1 / fac as a
full-precision reciprocal; it now takes  finv = clamp(0.9 err^(-1/Q), 1/5, 6), hnew = hs finv  (pk_step.hpp: step_growth), the exponent
negated.  Both are stated here with the single-precision part in numpy float32 (log2, the product with the rounded exponent, exp2) and
everything else in double, around the whole-integration port of tools/newton_stage_sensitivity.py.

Prints, for the six settings of that tool, the largest and median band shift |dy| / (1e-8 + 1e-6 |y|) of the new rule against the old one
and every replica whose step count changes.  The limit is the project's: 0.02, steps within 2.
usage: controller_growth_sensitivity.py [replicas = 24]"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import inslot_sensitivity as ins  # noqa: E402
import newton_stage_sensitivity as nss  # noqa: E402

f32 = np.float32


def _pow32(err, expo):
    """exp2f(log2f((float) clamp(err)) * (float) expo) as a double"""
    e = f32(min(max(err, 1e-30), 1e30))
    return float(np.exp2(f32(np.log2(e) * f32(expo))))


def by_divisor(hs, err, Q):
    fac = max(1.0 / 6.0, min(5.0, _pow32(err, 1.0 / Q) * (1.0 / 0.9)))
    return hs / fac


def by_growth(hs, err, Q):
    return hs * min(6.0, max(0.2, _pow32(err, -1.0 / Q) * 0.9))


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    ts, _ = nss._old_tabs()
    tabs = nss.header_tables(12)
    G, RPL = 4, 8
    worst = 0.0
    # one factor against the other over the controller's whole range
    errs = 10.0 ** np.linspace(-32.0, 32.0, 200001)
    rel = np.array([abs(by_growth(1.0, e, 11.0) / by_divisor(1.0, e, 11.0) - 1.0) for e in errs[::20]])
    print("hnew by the growth factor against hnew by the divisor, err over 1e-32 .. 1e32 (Q = 11): largest relative difference %.2e" % rel.max())
    for n, resident in ((30, True), (32, False)):
        for what, hi, h0 in (("theta ~ U(0, 20)", 20.0, 0.0), ("theta ~ U(0, 1)", 1.0, 0.0), ("theta ~ U(0, 20), h0 = 1e-9", 20.0, 1e-9)):
            theta = np.random.default_rng(20260515).uniform(0.0, hi, (B, 4 + 2 * n))
            y0 = np.ones(n + 2)
            old = [nss.lrp12_newton(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0, controller=by_divisor) for th in theta]
            new = [nss.lrp12_newton(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0, controller=by_growth) for th in theta]
            assert not any(r[1] for r in new) and not any(r[1] for r in old), "a replica ended with a status"
            shift = [ins.band(o[0], r[0]) for o, r in zip(old, new)]
            moved = [(b, o[2], o[3], r[2], r[3]) for b, (o, r) in enumerate(zip(old, new)) if (o[2], o[3]) != (r[2], r[3])]
            print("n = %d, 4 x 8 %s, %s, %d replicas: band shift max %.3e median %.3e; step counts changed in %d replicas%s"
                  % (n, "resident" if resident else "shadowed", what, B, max(shift), float(np.median(shift)), len(moved),
                     "".join("\n    replica %d: accepted / rejected %d / %d -> %d / %d" % m for m in moved)))
            worst = max(worst, max(shift))
            assert max(shift) <= 0.02 and all(abs(m[1] - m[3]) <= 2 and abs(m[2] - m[4]) <= 2 for m in moved), "beyond the project's limit"
    print("largest band over all settings: %.3e (limit 0.02)" % worst)


if __name__ == "__main__":
    main()
