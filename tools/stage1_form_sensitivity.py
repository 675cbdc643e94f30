"""Dev tool (CPU): how far forming the first LRP12 stage of the scaled layouts from the state itself, and summing the stage dot product on
one chain, moves the trajectories (csrc/pk_dist_fast.hpp).

The scaled form (tools/scaled_stage_sensitivity.py) lets the state enter the first solve as rho_j = y_j ic_j with ic_j = piv_j / s_j, and
then uses g_j rho_j in the dot product and fma(-omw_j, rho_j, xq) as the stage.  c_j ic_j = 1, so both products are known without ic_j:
    g_j rho_j   = winv_j y_j
    omw_j rho_j = q (d_j / s_j) y_j = q kappa_j y_j         kappa_j = d_j (1 / s_j), fixed per replica
and the first stage of a scaled row is
    t_j = kappa_j y_j ;  dot term fma(winv_j, y_j, .) ;  zeta_j = fma(-q, t_j, xq)
three operations per row where the scaled form has four (ic_j, rho_j, the dot term, the stage), and two roundings fewer (piv_j / s_j and
y_j ic_j).  A row with s_j = 0 has kappa_j = 0, zeta_j = xq, and every value of the row is 0 w_j as before.  The dot product of every stage
runs on one FMA chain (resident: seeded by row 0's explicit term; shadowed: by g_0 v_0) instead of two chains joined by an add.

`Stage1Lanes` subclasses ScaledLanes with exactly these two changes; everything from the second solve on is ScaledLanes' own.  Prints, per
setting, the band shift |dy| / (1e-8 + 1e-6 |y|) and every step-count change against the scaled form as it stands (ScaledLanes) and against
the C restatement, on the six settings of scaled_stage_sensitivity.main(), and its edge rates.  Project limits: band <= 0.02, steps +- 2.
usage: stage1_form_sensitivity.py [replicas = 24]"""
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import scaled_stage_sensitivity as sss  # noqa: E402

nss = sss.nss


class Stage1Lanes(sss.ScaledLanes):
    """ScaledLanes with the first stage formed from the state rows and the single-chain dot product."""

    def load(self, y):
        first = self.s is None
        v = super().load(y)
        if first:
            self.kappa = self.dg * self.si                        # d_j / s_j; 0 where s_j is 0 (and in row 0 of the resident layout: unused)
        return v

    def _gdot(self, v, coef=None):
        c = self.g if coef is None else coef
        a = v[..., 0] * self.ws0 if self.res else c[..., 0] * v[..., 0]
        for j in range(1, self.RPL):
            a = c[..., j] * v[..., j] + a
        return a

    def _xq(self, v, coef=None):
        R = self.RPL
        St = self._gdot(v, coef).sum(axis=-1, keepdims=True)
        if self.res:
            return St * self.qs, None, None
        xR = v[..., R] * self.winvR
        xP = (self.q1 * (self.C * xR + St) + v[..., R + 1]) * self.sinv[..., None]
        return self.q1 * xP, xR, xP

    def solve(self, r, first=False):
        """first: r holds the state rows themselves (plus q A in row R); the scaled rows come back as zeta_j = xq - q (kappa_j y_j)"""
        if not first:
            return super().solve(r)
        R, J0 = self.RPL, self.J0
        xq, xR, xP = self._xq(r, self.winv)
        u = np.empty_like(r)
        u[..., J0:R] = xq[..., None] - self.q1[..., None] * (self.kappa[..., J0:] * r[..., J0:R])
        if self.res:
            u[..., 0] = self.c[..., 0] * xq + r[..., 0] * self.winv[..., 0]
        else:
            u[..., R], u[..., R + 1] = xR, xP
        return u

    def step(self, y, q, tabs, cancelling_omw=False):
        GAM, LB, LE, BN = tabs
        R, J0 = self.RPL, self.J0
        sc = slice(J0, R)                                         # the scaled rows
        self.factor(q)
        z = self.solve(self.first_rhs(y), first=True)
        plain = y.copy(); plain[..., sc] = 0.0
        z = z - plain
        acc = y.copy(); acc[..., sc] = 0.0
        acc = acc + (LB[0] / GAM) * z
        z = self.solve(z)
        acc = acc + (BN[0] / GAM) * z
        for m in range(1, len(LB) - 1):
            z = self.diff(z)
            acc = acc + (BN[m] / GAM) * z
        yn, e = acc, z.copy()
        yn[..., sc] = self.c[..., J0:] * acc[..., sc] + y[..., sc]
        e[..., sc] = self.c[..., J0:] * z[..., sc]
        return yn, (abs(LE[1]) / GAM) * e


@contextmanager
def stage1():
    """newton_stage_sensitivity with Stage1Lanes in the place of Lanes, for the length of the block"""
    old = nss.Lanes
    nss.Lanes = Stage1Lanes
    try:
        yield nss
    finally:
        nss.Lanes = old


def lrp12_stage1(th, n, G, RPL, y0, t, tabs, resident, **kw):
    with stage1():
        return nss.lrp12_newton(th, n, G, RPL, y0, t, tabs, resident, **kw)


def one_step_stage1(n, **kw):
    with stage1():
        return nss.one_step_forms(n, **kw)


SETTINGS = tuple((n, resident, what, hi, h0) for n, resident in ((30, True), (32, False))
                 for what, hi, h0 in (("theta ~ U(0, 20)", 20.0, 0.0), ("theta ~ U(0, 1)", 1.0, 0.0), ("theta ~ U(0, 20), h0 = 1e-9", 20.0, 1e-9)))


def compare_setting(n, resident, hi, h0, B, ts, tabs, G=4, RPL=8):
    """(new, current, reference) of one setting: lists of (sol, status, accepted, rejected) per replica"""
    from oracle import lrp8_cpu
    theta = np.random.default_rng(20260515).uniform(0.0, hi, (B, 4 + 2 * n))
    y0 = np.ones(n + 2)
    new = [lrp12_stage1(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0) for th in theta]
    cur = [sss.lrp12_scaled(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0) for th in theta]
    if h0 > 0.0:
        sol, st, ns = ts._port_batch(theta, n, y0, h0)
    else:
        sol, st, ns = lrp8_cpu.solve_batch(theta, n, y0, ts.T)
    ref = [(sol[b], int(st[b]), int(ns[b, 0]), int(ns[b, 1])) for b in range(B)]
    return new, cur, ref


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    ts, _ = nss._old_tabs()
    import inslot_sensitivity as ins
    tabs = nss.header_tables(12)
    G, RPL = 4, 8
    worst = 0.0
    for n, resident, what, hi, h0 in SETTINGS:
        new, cur, ref = compare_setting(n, resident, hi, h0, B, ts, tabs)
        print("n = %d, 4 x 8 %s, %s, %d replicas:" % (n, "resident" if resident else "shadowed", what, B))
        for name, other in (("the current form", cur), ("the C restatement", ref)):
            assert not any(r[1] for r in new) and not any(r[1] for r in other), "a replica ended with a status"
            shift = [ins.band(o[0], r[0]) for o, r in zip(other, new)]
            moved = [(b, o[2], o[3], r[2], r[3]) for b, (o, r) in enumerate(zip(other, new)) if (o[2], o[3]) != (r[2], r[3])]
            print("  new first stage against %s: band shift max %.3e median %.3e; step counts changed in %d replicas%s"
                  % (name, max(shift), float(np.median(shift)), len(moved),
                     "".join("\n    replica %d: accepted / rejected %d / %d -> %d / %d" % m for m in moved)))
            worst = max(worst, max(shift))
            assert max(shift) <= 0.02 and all(abs(m[1] - m[3]) <= 2 and abs(m[2] - m[4]) <= 2 for m in moved), \
                "beyond rounding: the derivation or the port is wrong"
    print("largest band over all settings: %.3e (limit 0.02)" % worst)
    n = 30
    th = sss.edge_thetas(n)
    for b in range(8):
        y0 = np.ones(n + 2)
        if b == 7:
            y0[2 + 3] = 0.0
        a = lrp12_stage1(th[b], n, G, RPL, y0, ts.T, tabs, True)
        o = sss.lrp12_scaled(th[b], n, G, RPL, y0, ts.T, tabs, True)
        print("edge replica %d: status %d / %d, steps %d+%d / %d+%d, max |new - current| = %.3e%s"
              % (b, a[1], o[1], a[2], a[3], o[2], o[3], float(np.max(np.abs(a[0] - o[0]))),
                 ", site 3 identically zero: %s" % bool((a[0][:, 5] == 0.0).all()) if b == 7 else ""))
        assert a[1:] == o[1:] and np.max(np.abs(a[0] - o[0])) <= 1e-13
    for n in (30, 32):
        cur, new = sss.one_step_scaled(n, nb=4000), one_step_stage1(n, nb=4000)
        width = 1e-8 + 1e-6 * np.abs(cur["yw"])
        print("one step, n = %d: y_new against long double %.3e band widths (new) / %.3e (current)"
              % (n, *(float(np.max(np.asarray(np.abs(r["yd"] - r["yl"]) / width, float))) for r in (new, cur))))


if __name__ == "__main__":
    main()
