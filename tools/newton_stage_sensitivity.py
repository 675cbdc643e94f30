"""Dev tool (CPU): how far taking the LRP error estimate as a repeated difference moves the LRP12 trajectories of the distributive model
(the step loop of csrc/pk_dist_fast.hpp).

The estimator's weights are E_2 times a signed row of Pascal's triangle, so err = (E_2 / gamma) (I - M^-1)^(NS-2) w_2.  The step loop takes
two solves w_1, w_2 and then NS - 2 difference stages v_0 = w_2, v_{m+1} = v_m - M^-1 v_m; y_new = y + (B_1 w_1 + sum_m BN_m v_m) / gamma with
BN the weights of ResolventTab in that basis, and the estimate is the last v.  A difference stage is cheaper than a solve: every row obeys
v'_j = omw_j v_j - cw_j x_P (omw_j = 1 - winv_j, formed as (q winv_j) d_j), and the group sum that feeds x_P is lam - sum omw_j v_j with
lam = sum v_j carried from stage to stage, lam' = sum omw_j v_j - x_P Cl (Cl = sum cw_j over the same rows).

`Lanes` is a numpy port of factor(), solve() and diff() in the kernel's lane layouts (G lanes x RPL rows; resident: R and P in slots 0 and 1,
row 0 outside the tracked sum; shadowed: every lane carries its own R and P) and operation order, plain numpy arithmetic standing in for the
FMAs, `1 / x` for fast_rcp and pairwise numpy sums for the trees.  `lrp12_newton` runs whole integrations with it; `one_step_forms` is the one-step model
of tests/test_lrp_newton_cpu.py (weighted sums in double and in long double against the difference form).

Prints, per setting, the largest and median band shift |dy| / (1e-8 + 1e-6 |y|) and every step-count change of the new form against the
weighted-sum port of the same layout (tools/inslot_sensitivity.py, tools/pivot_chain_sensitivity.py) and against the C restatement:
4 x 8 resident at n = 30 and 4 x 8 shadowed at n = 32, on the benchmark's distribution theta ~ U(0, 20), on theta ~ U(0, 1), and with a
forced first step h0 = 1e-9 (where q d_j ~ 1e-9 and 1 - winv_j would keep seven digits).
usage: newton_stage_sensitivity.py [replicas = 24]"""
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import inslot_sensitivity as ins  # noqa: E402
import pivot_chain_sensitivity as pcs  # noqa: E402

RTOL, ATOL = 1e-6, 1e-8


def header_tables(stages=12):
    """(GAM, B, E, BN) of ResolventTab<LRP8 | LRP12>, read from the literals of csrc/pk_solve_kernel.hpp."""
    src = (ROOT / "phoskintime_amd" / "csrc" / "pk_solve_kernel.hpp").read_text()
    blk = src[src.index("struct ResolventTab<PK_METHOD_LRP%d>" % stages):]
    blk = blk[:blk.index("\n};")]

    def lit(name):
        body = re.search(r"\b%s\[\d+\]\s*=\s*\{([^}]*)\}" % name, blk).group(1)
        return np.array([float(x) for x in body.split(",")])
    return float(re.search(r"\bGAM\s*=\s*([0-9.]+)", blk).group(1)), lit("B"), lit("E"), lit("BN")


class Lanes:
    """factor(), solve() and diff() of dist_fast_kernel for vectors [..., G, RPL] (resident) or [..., G, RPL + 2] (shadowed: the last two
    columns are the lane's copies of R and P).  th [..., 4 + 2 n]; leading axes are a batch."""

    def __init__(self, th, n, G, RPL, resident):
        th = np.asarray(th, float)
        self.n, self.G, self.RPL, self.res = n, G, RPL, resident
        self.A, self.B, self.C = (th[..., i, None] for i in range(3))                 # [..., 1]: one value per lane
        slot = np.arange(G)[:, None] + G * np.arange(RPL)[None, :]
        self.slot = slot
        site = slot - (2 if resident else 0)
        ok = (site >= 0) & (site < n)
        idx = np.where(ok, site, 0)
        self.live = (slot < n + 2) if resident else ok
        self.Sr = np.where(ok, th[..., 4:4 + n][..., idx], 0.0)
        self.dg = np.where(ok, 1.0 + th[..., 4 + n:4 + 2 * n][..., idx], 1.0)
        if resident:
            assert G * RPL >= n + 2
            self.dg[..., 0, 0] = th[..., 1]
            self.dg[..., 1, 0] = -th[..., 2]
            self.w0 = np.ones(th.shape[:-1] + (G,)); self.w0[..., 0] = th[..., 2]
            self.k3 = np.zeros(th.shape[:-1] + (G,)); self.k3[..., 0] = th[..., 0]
        self.Dsum = th[..., 3] + self.Sr.sum(axis=(-1, -2))

    def load(self, y):
        """state vector(s) [..., n + 2] -> the lanes' rows"""
        y = np.asarray(y, float)
        if self.res:
            return np.where(self.live, y[..., np.where(self.live, self.slot, 0)], 0.0)
        s = np.where(self.live, y[..., 2:][..., np.where(self.live, self.slot, 0)], 0.0)
        sh = np.broadcast_to(y[..., None, :2], s.shape[:-1] + (2,))
        return np.concatenate([s, sh], axis=-1)

    def emit(self, v):
        """the lanes' rows -> state vector(s) [..., n + 2] as the kernel stores them (shadowed: R and P from lane 0)"""
        order = np.argsort(self.slot[self.live])
        if self.res:
            return v[..., self.live][..., order]
        return np.concatenate([v[..., 0, self.RPL:], v[..., :self.RPL][..., self.live][..., order]], axis=-1)

    def _chains(self, piv):
        m = piv.shape[-1]
        m0 = m if m <= 5 else (m + 1) // 2
        inv = np.empty_like(piv)
        inv[..., :m0] = pcs.chain_inverse(piv[..., :m0])
        if m > m0:
            inv[..., m0:] = pcs.chain_inverse(piv[..., m0:])
        return inv

    def factor(self, q, cancelling_omw=False):
        """cancelling_omw: form omw as 1 - winv (what the kernel does NOT do), to show what that costs"""
        q = np.asarray(q, float)
        self.q1 = q[..., None]                                    # per lane
        q2 = q[..., None, None]                                   # per row
        piv = 1.0 + q2 * self.dg
        if self.res:
            piv[..., 1, 0] = q
            self.winv = self._chains(piv)
        else:
            inv = self._chains(np.concatenate([np.broadcast_to(1.0 + self.q1 * self.B, piv.shape[:-1])[..., None], piv], axis=-1))
            self.winvR, self.winv = inv[..., 0], inv[..., 1:]
            self.omwR = (1.0 - self.winvR) if cancelling_omw else self.q1 * self.winvR * self.B
        qw = q2 * self.winv
        self.cw = qw * self.Sr
        self.omw = (1.0 - self.winv) if cancelling_omw else qw * self.dg
        if self.res:
            self.Cl = self.cw[..., 1:].sum(axis=-1)
            Scw = (self.Cl + self.cw[..., 0]).sum(axis=-1)
        else:
            self.Cl = self.cw.sum(axis=-1)
            Scw = self.Cl.sum(axis=-1)
        self.sinv = 1.0 / (1.0 + q * (self.Dsum - Scw))
        if self.res:
            self.qs = (q * self.sinv)[..., None]
            self.ws0 = self.winv[..., 0] * self.w0
            self.winv[..., 1, 0] = 0.0
            self.cw[..., 1, 0] = 1.0
            self.omw[..., 1, 0] = 1.0

    def first_rhs(self, y):
        """y + q b: q A joins row R"""
        r = y.copy()
        if self.res:
            r[..., 0] = self.q1 * self.k3 + y[..., 0]
        else:
            r[..., self.RPL] = self.q1 * self.A + y[..., self.RPL]
        return r

    def solve(self, r):
        R = self.RPL
        if self.res:
            t = r * self.winv
            tsum = t[..., 1:].sum(axis=-1)
            xP = (r[..., 0] * self.ws0 + tsum).sum(axis=-1, keepdims=True) * self.qs
            self.lam = xP * self.Cl + tsum
            return self.cw * xP[..., None] + t
        xR = r[..., R] * self.winvR
        t = r[..., :R] * self.winv
        tsum = t.sum(axis=-1)
        St = tsum.sum(axis=-1, keepdims=True)
        xP = (self.q1 * (self.C * xR + St) + r[..., R + 1]) * self.sinv[..., None]
        self.lam = xP * self.Cl + tsum
        return np.concatenate([self.cw * xP[..., None] + t, xR[..., None], xP[..., None]], axis=-1)

    def diff(self, v):
        """v - M^-1 v; reads and advances the tracked sum of the solve or difference stage before it"""
        R = self.RPL
        p = self.omw * v[..., :R]
        if self.res:
            psum = p[..., 1:].sum(axis=-1)
            xP = (v[..., 0] * self.ws0 + (self.lam - psum)).sum(axis=-1, keepdims=True) * self.qs
            self.lam = psum - xP * self.Cl
            return p - self.cw * xP[..., None]
        psum = p.sum(axis=-1)
        xR = v[..., R] * self.winvR
        St = (self.lam - psum).sum(axis=-1, keepdims=True)
        xP = (self.q1 * (self.C * xR + St) + v[..., R + 1]) * self.sinv[..., None]
        self.lam = psum - xP * self.Cl
        return np.concatenate([p - self.cw * xP[..., None], (v[..., R] * self.omwR)[..., None], (v[..., R + 1] - xP)[..., None]], axis=-1)

    def step(self, y, q, tabs, cancelling_omw=False):
        """(y_new, error vector) of one step in the difference form, lanes' rows"""
        GAM, LB, LE, BN = tabs
        self.factor(q, cancelling_omw)
        z = self.solve(self.first_rhs(y)) - y
        yn = y + (LB[0] / GAM) * z
        z = self.solve(z)
        yn = yn + (BN[0] / GAM) * z
        for m in range(1, len(LB) - 1):
            z = self.diff(z)
            yn = yn + (BN[m] / GAM) * z
        return yn, (abs(LE[1]) / GAM) * z


def lrp12_newton(th, n, G, RPL, y0, t, tabs, resident, rtol=RTOL, atol=ATOL, max_steps=100000, h0=0.0, controller=None):
    """One replica, whole integration, the step loop's controller around Lanes.step.  (sol [T, n + 2], status, accepted, rejected)
    controller(hs, err, Q) -> hnew replaces the double-precision rule (tools/controller_growth_sensitivity.py)"""
    GAM, NS = tabs[0], len(tabs[1])
    L = Lanes(th, n, G, RPL, resident)
    y = L.load(y0)
    nT = len(t)
    sol = np.zeros((nT, n + 2)); sol[0] = L.emit(y)
    acc = rej = status = 0
    after_reject = False
    tc = float(t[0])
    # initial step: |y| / sc and |f(y)| / sc in state order (the prologue is not what this tool is about)
    ys = np.asarray(y0, float)
    A, Bc, Cc, D = (float(v) for v in th[:4])
    Sr, dg = np.asarray(th[4:4 + n], float), 1.0 + np.asarray(th[4 + n:4 + 2 * n], float)
    f = np.concatenate([[A - Bc * ys[0], Cc * ys[0] - (D + Sr.sum()) * ys[1] + ys[2:].sum()], Sr * ys[1] - dg * ys[2:]])
    sc = atol + rtol * np.abs(ys)
    d0, d1 = float(np.max(np.abs(ys) / sc)), float(np.max(np.abs(f) / sc))
    h = 0.01 * d0 / d1 if (d0 > 1e-5 and d1 > 1e-5) else 1e-6
    if h0 > 0.0:
        h = h0
    for k in range(1, nT):
        te = float(t[k])
        while True:
            if acc + rej >= max_steps:
                status |= 2; break
            last = tc + 1.0001 * h >= te
            hs = te - tc if last else (0.5 * (te - tc) if tc + 2.0 * h > te else h)
            if not hs > 1e-14 * max(abs(tc), 1e-3):
                status |= 4; break
            yn, e = L.step(y, GAM * hs, tabs)
            v = np.abs(e) / (atol + rtol * np.maximum(np.abs(y), np.abs(yn)))
            bad = bool(np.isnan(v).any())
            err = 0.0 if bad else float(v.max())
            if bad or err > 1e300:
                rej += 1; after_reject = True; h = 0.1 * hs
                if not (np.isfinite(y).all() and np.isfinite(th[:4 + 2 * n]).all()):
                    status |= 1; break
                continue
            if controller is not None:
                hnew = controller(hs, err, NS - 1.0)
            else:
                fac = min(max(err, 1e-30), 1e30) ** (1.0 / (NS - 1.0)) / 0.9
                fac = max(1.0 / 6.0, min(5.0, fac))
                hnew = hs / fac
            if err <= 1.0:
                acc += 1
                y = yn; tc += hs
                if after_reject:
                    hnew = min(hnew, hs)
                after_reject = False
                if last:
                    tc = te; h = max(hnew, h) if hs < h else hnew
                    break
                h = hnew
            else:
                rej += 1; after_reject = True; h = hnew
        if status:
            sol[k:] = np.nan
            break
        sol[k] = L.emit(y)
    return sol, status, acc, rej


# ---------------------------------------------------------------- the one-step model
def arrow(r, q, th, n):
    """M^-1 r for a batch [nb, n + 2] in state order and in the arrays' own precision (double or long double)."""
    Bc, Cc, D = th[:, 1], th[:, 2], th[:, 3]
    Sr, dg = th[:, 4:4 + n], 1 + th[:, 4 + n:4 + 2 * n]
    w = 1 / (1 + q[:, None] * dg)
    xR = r[:, 0] / (1 + q * Bc)
    tt = r[:, 2:] * w
    cw = q[:, None] * Sr * w
    xP = (r[:, 1] + q * (Cc * xR + tt.sum(axis=1))) / (1 + q * (D + Sr.sum(axis=1) - cw.sum(axis=1)))
    return np.concatenate([xR[:, None], xP[:, None], tt + cw * xP[:, None]], axis=1)


def weighted_step(y, q, th, n, tabs):
    """(y_new, error vector) by the weighted sums over the NS solves, in the precision of y, q, th (tables GAM, B, E in the same)"""
    GAM, LB, LE = tabs[:3]
    r = y.copy(); r[:, 0] = q * th[:, 0] + y[:, 0]
    z = arrow(r, q, th, n) - y
    yn = y + (LB[0] / GAM) * z
    e = 0 * y
    for k in range(1, len(LB)):
        z = arrow(z, q, th, n)
        yn = yn + (LB[k] / GAM) * z
        e = e + (LE[k] / GAM) * z
    return yn, e


def one_step_forms(n, nb=4000, seed=20261019, stages=12, G=4, RPL=8, rtol=RTOL, atol=ATOL):
    """nb random steps of the distributive model at n sites: theta ~ U(0, 20), y ~ U(0, 2), h log-uniform over 1e-5 .. 300.
    Returns a dict: y, y_new and error norm of the weighted sums in double ('w') and long double ('l') and of the difference form in the
    kernel's lane layout ('d': resident when G RPL >= n + 2, shadowed otherwise), all in state order."""
    tabs = header_tables(stages)
    rng = np.random.default_rng(seed)
    th = rng.uniform(0.0, 20.0, (nb, 4 + 2 * n))
    y = rng.uniform(0.0, 2.0, (nb, n + 2))
    h = 10.0 ** rng.uniform(-5.0, np.log10(300.0), nb)
    q = tabs[0] * h

    def nrm(e, yn, yy):
        return np.asarray((np.abs(e) / (atol + rtol * np.maximum(np.abs(yy), np.abs(yn)))).max(axis=1), float)
    yw, ew = weighted_step(y, q, th, n, tabs)
    ld = np.longdouble
    tl = tuple(np.asarray(x, ld) for x in tabs)
    yl, el = weighted_step(y.astype(ld), q.astype(ld), th.astype(ld), n, tl)
    L = Lanes(th, n, G, RPL, G * RPL >= n + 2)
    yv = L.load(y)
    ydv, edv = L.step(yv, q, tabs)
    yd, ed = L.emit(ydv), L.emit(edv)
    return dict(y=y, h=h, yw=yw, yl=yl, yd=yd, errw=nrm(ew, yw, y), errl=nrm(el, yl, y.astype(ld)), errd=nrm(ed, yd, y))


# ---------------------------------------------------------------- whole integrations
def _old_tabs():
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import test_gpu_dist_fast_sitesum as ts
    return ts, ts._tables()


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    ts, old_tabs = _old_tabs()
    from oracle import lrp8_cpu
    tabs = header_tables(12)
    G, RPL = 4, 8
    worst = 0.0
    for n, resident in ((30, True), (32, False)):
        for what, hi, h0 in (("theta ~ U(0, 20)", 20.0, 0.0), ("theta ~ U(0, 1)", 1.0, 0.0), ("theta ~ U(0, 20), h0 = 1e-9", 20.0, 1e-9)):
            theta = np.random.default_rng(20260515).uniform(0.0, hi, (B, 4 + 2 * n))
            y0 = np.ones(n + 2)
            new = [lrp12_newton(th, n, G, RPL, y0, ts.T, tabs, resident, h0=h0) for th in theta]
            if resident:
                old = [ins.lrp12_resident(th, n, G, RPL, y0, ts.T, old_tabs, h0=h0, resolvent=True)[:4] for th in theta]
            else:
                old = [pcs.lrp12_lanes(th, n, G, RPL, y0, ts.T, old_tabs, True, h0=h0, resolvent=True)[:4] for th in theta]
            if h0 > 0.0:
                sol, st, ns = ts._port_batch(theta, n, y0, h0)
            else:
                sol, st, ns = lrp8_cpu.solve_batch(theta, n, y0, ts.T)
            ref = [(sol[b], int(st[b]), int(ns[b, 0]), int(ns[b, 1])) for b in range(B)]
            print("n = %d, 4 x 8 %s, %s, %d replicas:" % (n, "resident" if resident else "shadowed", what, B))
            for name, other in (("the weighted-sum port", old), ("the C restatement", ref)):
                assert not any(r[1] for r in new) and not any(r[1] for r in other), "a replica ended with a status"
                shift = [ins.band(o[0], r[0]) for o, r in zip(other, new)]
                moved = [(b, o[2], o[3], r[2], r[3]) for b, (o, r) in enumerate(zip(other, new)) if (o[2], o[3]) != (r[2], r[3])]
                print("  difference form against %s: band shift max %.3e median %.3e; step counts changed in %d replicas%s"
                      % (name, max(shift), float(np.median(shift)), len(moved),
                         "".join("\n    replica %d: accepted / rejected %d / %d -> %d / %d" % m for m in moved)))
                worst = max(worst, max(shift))
                assert max(shift) <= 0.02 and all(abs(m[1] - m[3]) <= 2 and abs(m[2] - m[4]) <= 2 for m in moved), \
                    "beyond rounding: the derivation or the port is wrong"
    print("largest band over all settings: %.3e (limit 0.02)" % worst)


if __name__ == "__main__":
    main()
