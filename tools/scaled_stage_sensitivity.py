"""Dev tool (CPU): how far carrying the site rows of the distributive model in units of their coupling weight moves the LRP12 trajectories
(the scaled stages of csrc/pk_dist_fast.hpp).

A difference stage in plain units costs four operations per site row: p_j = omw_j v_j, the tree that sums p_j, v'_j = fma(-cw_j, x_P, p_j) and
the accumulation.  The multiply exists only because x_P enters each row with its own coefficient cw_j.  With c_j = winv_j s_j (= cw_j / q; s_j
the row's scale, its rate), v_j = c_j w_j and xq = q x_P:
    difference stage   w'_j = fma(omw_j, w_j, -xq)
    solve              upsilon_j = winv_j rho_j + xq = (rho_j + xq) - omw_j rho_j   (r_j = c_j rho_j; the state enters as rho_j = y_j ic_j,
                       ic_j = piv_j / s_j; the first stage upsilon_j - rho_j is fma(-omw_j, rho_j, xq), without its cancellation)
    group-sum input    sum winv_j v_j = sum g_j w_j, g_j = winv_j c_j     (an FMA dot product on two chains; no tracked sum)
    accumulator        A_j += BN_m w'_j;  y_new_j = fma(c_j, A_j, y_j) and e_j = c_j w_last,j once per step.
The scale of a row is decided once per replica: S_j where |S_j| >= 2^-600 (NaN and inf included); 0 for an idle row and for a site with rate 0
that starts at 0 (every value of the row is then 0 w_j, exactly zero); 2^-600 for any other rate below that floor.

`ScaledLanes` is a numpy port of the scaled factor(), solve() and diff() in the kernel's lane layouts and operation order (plain numpy
arithmetic standing in for the FMAs, `1 / x` for the reciprocals), a subclass of newton_stage_sensitivity.Lanes, which holds the current form.
Resident: rows 1 .. RPL - 1 are scaled, row 0 (R slot, P slot, two sites) keeps plain units; shadowed: every site row is scaled, the shadow
rows stay as they are.  `scaled()` runs any function of newton_stage_sensitivity with ScaledLanes in the place of Lanes.

Prints, per setting, the largest and median band shift |dy| / (1e-8 + 1e-6 |y|) and every step-count change of the scaled form against the
current form and against the C restatement, on the six settings of newton_stage_sensitivity.main(), and the edge rates of the scale rule.
Project limits: band <= 0.02, steps +- 2.
usage: scaled_stage_sensitivity.py [replicas = 24]"""
import sys
from contextlib import contextmanager
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import newton_stage_sensitivity as nss  # noqa: E402

SCALE_MIN = 2.0 ** -600


def row_scale(Sr, y):
    """(s_j, 1 / s_j) of the kernel's prologue for rates Sr and initial values y of the same shape."""
    with np.errstate(invalid="ignore"):
        s = np.where(~(np.abs(Sr) < SCALE_MIN), Sr, np.where((Sr == 0.0) & (y == 0.0), 0.0, SCALE_MIN))
    with np.errstate(divide="ignore"):
        return s, np.where(s != 0.0, 1.0 / np.where(s != 0.0, s, 1.0), 0.0)


class ScaledLanes(nss.Lanes):
    """The scaled stages.  Vectors are laid out as in Lanes; a scaled row of a stage vector is in units of c_j, every other row (row 0 of
    the resident layout, the shadow rows) in plain units.  The scale is decided by the first load(), from the state it is given."""

    def __init__(self, th, n, G, RPL, resident):
        super().__init__(th, n, G, RPL, resident)
        self.J0 = 1 if resident else 0
        self.s = None

    def load(self, y):
        v = super().load(y)
        if self.s is None:
            s, si = row_scale(self.Sr, v[..., :self.RPL])
            if self.res:                                          # row 0 keeps its rate: it is not scaled
                s[..., 0], si[..., 0] = self.Sr[..., 0], 0.0
            self.s, self.si = s, si
        return v

    def factor(self, q, cancelling_omw=False):
        q = np.asarray(q, float)
        J0 = self.J0
        self.q1 = q[..., None]
        q2 = q[..., None, None]
        piv = 1.0 + q2 * self.dg
        if self.res:
            piv[..., 1, 0] = q
            self.winv = self._chains(piv)
        else:
            inv = self._chains(np.concatenate([np.broadcast_to(1.0 + self.q1 * self.B, piv.shape[:-1])[..., None], piv], axis=-1))
            self.winvR, self.winv = inv[..., 0], inv[..., 1:]
            self.omwR = self.q1 * self.winvR * self.B
        self.c = self.winv * self.s
        self.g = self.winv * self.c
        self.ic = piv * self.si
        self.omw = (q2 * self.winv) * self.dg
        Scw = q * self.c.sum(axis=(-1, -2))
        self.Scw = Scw
        self.sinv = 1.0 / (1.0 + q * (self.Dsum - Scw))
        if self.res:
            self.qs = ((q * self.sinv) * q)[..., None]
            self.ws0 = self.winv[..., 0] * self.w0
            self.c[..., 1, 0] = self.winv[..., 1, 0]
            self.winv[..., 1, 0] = 0.0
            self.omw[..., 1, 0] = 1.0

    def _gdot(self, v):
        R, J0 = self.RPL, self.J0
        H = (R + J0) // 2
        a = v[..., 0] * self.ws0 if self.res else self.g[..., 0] * v[..., 0]
        for j in range(1, H):
            a = self.g[..., j] * v[..., j] + a
        b = self.g[..., H] * v[..., H]
        for j in range(H + 1, R):
            b = self.g[..., j] * v[..., j] + b
        return a + b

    def _xq(self, v):
        """(xq, x_R, x_P) per lane; resident: x_R and x_P are rows of the vector, None here"""
        R = self.RPL
        St = self._gdot(v).sum(axis=-1, keepdims=True)
        if self.res:
            return St * self.qs, None, None
        xR = v[..., R] * self.winvR
        xP = (self.q1 * (self.C * xR + St) + v[..., R + 1]) * self.sinv[..., None]
        return self.q1 * xP, xR, xP

    def solve(self, r, first=False):
        """first: the scaled rows come back as upsilon_j - rho_j = xq - omw_j rho_j, the first stage itself (no cancellation);
        otherwise upsilon_j = rho_j - omw_j rho_j + xq, as (rho_j + xq) - omw_j rho_j: winv_j is not used after factor()"""
        R, J0 = self.RPL, self.J0
        xq, xR, xP = self._xq(r)
        u = np.empty_like(r)
        if first:
            u[..., J0:R] = xq[..., None] - self.omw[..., J0:] * r[..., J0:R]
        else:
            u[..., J0:R] = (r[..., J0:R] + xq[..., None]) - self.omw[..., J0:] * r[..., J0:R]
        if self.res:
            u[..., 0] = self.c[..., 0] * xq + r[..., 0] * self.winv[..., 0]
        else:
            u[..., R], u[..., R + 1] = xR, xP
        return u

    def diff(self, v):
        R, J0 = self.RPL, self.J0
        xq, xR, xP = self._xq(v)
        u = np.empty_like(v)
        u[..., J0:R] = self.omw[..., J0:] * v[..., J0:R] - xq[..., None]
        if self.res:
            u[..., 0] = self.omw[..., 0] * v[..., 0] - self.c[..., 0] * xq
        else:
            u[..., R], u[..., R + 1] = v[..., R] * self.omwR, v[..., R + 1] - xP
        return u

    def step(self, y, q, tabs, cancelling_omw=False):
        GAM, LB, LE, BN = tabs
        R, J0 = self.RPL, self.J0
        sc = slice(J0, R)                                         # the scaled rows
        self.factor(q)
        r = self.first_rhs(y)
        r[..., sc] = y[..., sc] * self.ic[..., J0:]
        z = self.solve(r, first=True)
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
def scaled():
    """newton_stage_sensitivity with ScaledLanes in the place of Lanes, for the length of the block (the module's own text stays as it is)"""
    old = nss.Lanes
    nss.Lanes = ScaledLanes
    try:
        yield nss
    finally:
        nss.Lanes = old


def lrp12_scaled(th, n, G, RPL, y0, t, tabs, resident, **kw):
    with scaled():
        return nss.lrp12_newton(th, n, G, RPL, y0, t, tabs, resident, **kw)


def one_step_scaled(n, **kw):
    with scaled():
        return nss.one_step_forms(n, **kw)


def edge_thetas(n, seed=20261020):
    """theta [8, 4 + 2 n] on U(0, 20) with, in different replicas: site 3's rate exactly 0; every site rate 0; a rate of 1e-300, of 1e-12, of 1e6
    (site 5); the site rates log-spread over eight decades; a healthy replica; site 3's rate 0 again (for a start at y0_3 = 0)."""
    th = np.random.default_rng(seed).uniform(0.0, 20.0, (8, 4 + 2 * n))
    th[0, 4 + 3] = 0.0
    th[1, 4:4 + n] = 0.0
    th[2, 4 + 5], th[3, 4 + 5], th[4, 4 + 5] = 1e-300, 1e-12, 1e6
    th[5, 4:4 + n] = 10.0 ** np.linspace(-5.0, 3.0, n)
    th[7, 4 + 3] = 0.0
    return th


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    ts, _ = nss._old_tabs()
    from oracle import lrp8_cpu
    import inslot_sensitivity as ins
    tabs = nss.header_tables(12)
    G, RPL = 4, 8
    worst = 0.0
    for n, resident in ((30, True), (32, False)):
        for what, hi, h0 in (("theta ~ U(0, 20)", 20.0, 0.0), ("theta ~ U(0, 1)", 1.0, 0.0), ("theta ~ U(0, 20), h0 = 1e-9", 20.0, 1e-9)):
            theta = np.random.default_rng(20260515).uniform(0.0, hi, (B, 4 + 2 * n))
            y0 = np.ones(n + 2)
            new = [lrp12_scaled(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0) for th in theta]
            old = [nss.lrp12_newton(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0) for th in theta]
            if h0 > 0.0:
                sol, st, ns = ts._port_batch(theta, n, y0, h0)
            else:
                sol, st, ns = lrp8_cpu.solve_batch(theta, n, y0, ts.T)
            ref = [(sol[b], int(st[b]), int(ns[b, 0]), int(ns[b, 1])) for b in range(B)]
            print("n = %d, 4 x 8 %s, %s, %d replicas:" % (n, "resident" if resident else "shadowed", what, B))
            for name, other in (("the current form", old), ("the C restatement", ref)):
                assert not any(r[1] for r in new) and not any(r[1] for r in other), "a replica ended with a status"
                shift = [ins.band(o[0], r[0]) for o, r in zip(other, new)]
                moved = [(b, o[2], o[3], r[2], r[3]) for b, (o, r) in enumerate(zip(other, new)) if (o[2], o[3]) != (r[2], r[3])]
                print("  scaled form against %s: band shift max %.3e median %.3e; step counts changed in %d replicas%s"
                      % (name, max(shift), float(np.median(shift)), len(moved),
                         "".join("\n    replica %d: accepted / rejected %d / %d -> %d / %d" % m for m in moved)))
                worst = max(worst, max(shift))
                assert max(shift) <= 0.02 and all(abs(m[1] - m[3]) <= 2 and abs(m[2] - m[4]) <= 2 for m in moved), \
                    "beyond rounding: the derivation or the port is wrong"
    print("largest band over all settings: %.3e (limit 0.02)" % worst)
    # the scale rule on its edge rates, 4 x 8 resident at n = 30, y0 = 1 and y0 = 1 with site 3 starting at 0
    n = 30
    th = edge_thetas(n)
    for b in range(8):
        y0 = np.ones(n + 2)
        if b == 7:
            y0[2 + 3] = 0.0
        a = lrp12_scaled(th[b], n, G, RPL, y0, ts.T, tabs, True)
        o = nss.lrp12_newton(th[b], n, G, RPL, y0, ts.T, tabs, True)
        print("edge replica %d: status %d / %d, steps %d+%d / %d+%d, max |scaled - current| = %.3e%s"
              % (b, a[1], o[1], a[2], a[3], o[2], o[3], float(np.max(np.abs(a[0] - o[0]))),
                 ", site 3 identically zero: %s" % bool((a[0][:, 5] == 0.0).all()) if b == 7 else ""))
        assert a[1:] == o[1:] and np.max(np.abs(a[0] - o[0])) <= 1e-13


if __name__ == "__main__":
    main()
