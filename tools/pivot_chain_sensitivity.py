"""Dev tool (CPU): how far inverting the arrow pivots of a distmod step through shared reciprocals (chain_rcp, csrc/pk_linsolve.hpp)
moves the LRP12 trajectories of the distributive model.

A numpy port of the throughput kernel's step in its lane layout (G lanes x RPL rows, site i = lane + G * row; every lane carries its own
copy of the shadow rows R and P, as the kernel does) runs the benchmark's parameter distribution (n = 30 on 4 x 8, theta ~ U(0, 20),
y0 = 1, the 14-point grid, rtol 1e-6 / atol 1e-8) twice: once with every pivot 1 + q B, 1 + q d_j divided on its own, once with the
pivots of a lane inverted by the kernel's chain sequence and split rule, `1 / x` standing in for fast_rcp.  Prints the largest band
difference |dy| / (1e-8 + 1e-6 |y|) between the two, the step-count differences, the largest relative difference between a chained and
a direct reciprocal against the bound 2 (m + 1) 2^-53, and how far the lanes' copies of P drift apart (each lane's chain holds other
pivots, so 1 / (1 + q B) is no longer the same bits in every lane of a group).
usage: pivot_chain_sensitivity.py [replicas = 24]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -53


def chain_inverse(a):
    """The reciprocals of a[..., 0:m] by the kernel's sequence: prefix products, one reciprocal, the walk back.  Plain multiplies."""
    a = np.asarray(a, float)
    m = a.shape[-1]
    p = np.empty_like(a)
    p[..., 0] = a[..., 0]
    for i in range(1, m):
        p[..., i] = p[..., i - 1] * a[..., i]
    inv = np.empty_like(a)
    r = 1.0 / p[..., m - 1]
    for i in range(m - 1, 0, -1):
        inv[..., i] = r * p[..., i - 1]
        r = r * a[..., i]
    inv[..., 0] = r
    return inv


def chain_split(rpl):
    """(m0, m1): the lengths of the chains over the rpl + 1 pivots of a lane (one chain up to five pivots, two even ones above)."""
    m = rpl + 1
    m0 = m if m <= 5 else (m + 1) // 2
    return m0, m - m0


def pivot_inverses(piv, chained):
    """piv [G, RPL + 1] (column 0: 1 + q B) -> reciprocals, and the largest |chain - direct| / direct in units of the bound of its chain."""
    direct = 1.0 / piv
    if not chained:
        return direct, 0.0
    m0, m1 = chain_split(piv.shape[1] - 1)
    inv = np.empty_like(piv)
    inv[:, :m0] = chain_inverse(piv[:, :m0])
    worst = float(np.max(np.abs(inv[:, :m0] - direct[:, :m0]) / direct[:, :m0])) / (2 * (m0 + 1) * U)
    if m1:
        inv[:, m0:] = chain_inverse(piv[:, m0:])
        worst = max(worst, float(np.max(np.abs(inv[:, m0:] - direct[:, m0:]) / direct[:, m0:])) / (2 * (m1 + 1) * U))
    return inv, worst


def lrp12_lanes(th, n, G, RPL, y0, t, tables, chained, rtol=1e-6, atol=1e-8, max_steps=100000, h0=0.0, resolvent=False):
    """One replica on G lanes x RPL rows.  (sol [T, n + 2] as lane 0 and the site rows emit it, status, accepted, rejected,
    worst chain error in units of its bound, largest relative spread of P over the lanes)
    resolvent = True forms the first stage as the step loop of csrc/pk_dist_fast.hpp does: gamma z_1 =
    solve(y + q b) - y with the weights B_k / gamma, E_k / gamma; False keeps the earlier solve(h f(y))."""
    GAM, LB, LE = tables
    NS = 12
    WB, WE = (LB / GAM, LE / GAM) if resolvent else (LB, LE)
    A, Bc, Cc, D = (float(v) for v in th[:4])
    site = np.arange(G)[:, None] + G * np.arange(RPL)[None, :]
    ok = site < n
    idx = np.where(ok, site, 0)
    Sr = np.where(ok, np.asarray(th[4:4 + n], float)[idx], 0.0)
    dg = np.where(ok, 1.0 + np.asarray(th[4 + n:4 + 2 * n], float)[idx], 1.0)
    Dsum = D + float(Sr.sum())
    R = np.full(G, float(y0[0])); P = np.full(G, float(y0[1]))
    s = np.where(ok, np.asarray(y0[2:], float)[idx], 0.0)
    worst = spread = 0.0

    def emit(R, P, s):
        row = np.empty(n + 2)
        row[0], row[1] = R[0], P[0]
        row[2:] = s[ok][np.argsort(site[ok])]
        return row

    def rhs(R, P, s):
        return A - Bc * R, Cc * R - Dsum * P + float(s.sum()), Sr * P[:, None] - dg * s

    def norm(eR, eP, es, R, P, s, Rn, Pn, sn):
        v = [np.abs(eR) / (atol + rtol * np.maximum(np.abs(R), np.abs(Rn))), np.abs(eP) / (atol + rtol * np.maximum(np.abs(P), np.abs(Pn))),
             (np.abs(es) / (atol + rtol * np.maximum(np.abs(s), np.abs(sn)))).ravel()]
        v = np.concatenate(v)
        return (True, 0.0) if np.isnan(v).any() else (False, float(v.max()))

    nT = len(t)
    sol = np.zeros((nT, n + 2)); sol[0] = emit(R, P, s)
    acc = rej = status = 0
    after_reject = False
    tc = float(t[0])
    fR, fP, fs = rhs(R, P, s)
    d0 = max(float(np.max(np.abs(R) / (atol + rtol * np.abs(R)))), float(np.max(np.abs(P) / (atol + rtol * np.abs(P)))),
             float(np.max(np.abs(s) / (atol + rtol * np.abs(s)))))
    d1 = max(float(np.max(np.abs(fR) / (atol + rtol * np.abs(R)))), float(np.max(np.abs(fP) / (atol + rtol * np.abs(P)))),
             float(np.max(np.abs(fs) / (atol + rtol * np.abs(s)))))
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
            q = GAM * hs
            piv = np.concatenate([np.full((G, 1), 1.0 + q * Bc), 1.0 + q * dg], axis=1)
            inv, w = pivot_inverses(piv, chained)
            worst = max(worst, w)
            winvR, winv = inv[:, 0], inv[:, 1:]
            cw = q * Sr * winv
            sinv = 1.0 / (1.0 + q * (Dsum - float(cw.sum())))

            def solve(rR, rP, rs):
                xR = rR * winvR
                tt = rs * winv
                xP = (rP + q * (Cc * xR + float(tt.sum()))) * sinv
                return xR, xP, cw * xP[:, None] + tt

            if resolvent:
                zR, zP, zs = solve(q * A + R, P, s)
                zR, zP, zs = zR - R, zP - P, zs - s
            else:
                fR, fP, fs = rhs(R, P, s)
                zR, zP, zs = solve(hs * fR, hs * fP, hs * fs)
            Rn, Pn, sn = R + WB[0] * zR, P + WB[0] * zP, s + WB[0] * zs
            eR, eP, es = np.zeros(G), np.zeros(G), np.zeros((G, RPL))
            for st in range(1, NS):
                zR, zP, zs = solve(zR, zP, zs)
                Rn, Pn, sn = Rn + WB[st] * zR, Pn + WB[st] * zP, sn + WB[st] * zs
                eR, eP, es = eR + WE[st] * zR, eP + WE[st] * zP, es + WE[st] * zs
            bad, err = norm(eR, eP, es, R, P, s, Rn, Pn, sn)
            if bad or err > 1e300:
                rej += 1; after_reject = True; h = 0.1 * hs
                if not (np.isfinite(R).all() and np.isfinite(P).all() and np.isfinite(s).all() and np.isfinite(th[:4 + 2 * n]).all()):
                    status |= 1; break
                continue
            fac = min(max(err, 1e-30), 1e30) ** (1.0 / (NS - 1.0)) / 0.9
            fac = max(1.0 / 6.0, min(5.0, fac))
            hnew = hs / fac
            if err <= 1.0:
                acc += 1
                R, P, s = Rn, Pn, sn; tc += hs
                spread = max(spread, float((P.max() - P.min()) / max(np.abs(P).max(), 1e-300)))
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
        sol[k] = emit(R, P, s)
    return sol, status, acc, rej, worst, spread


def main():
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import test_gpu_dist_fast_sitesum as ts
    from oracle import lrp8_cpu
    n, G, RPL = 30, 4, 8
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    theta = np.random.default_rng(20260515).uniform(0.0, 20.0, (B, 4 + 2 * n))
    y0 = np.ones(n + 2)
    tables = ts._tables()
    direct = [lrp12_lanes(th, n, G, RPL, y0, ts.T, tables, False) for th in theta]
    chain = [lrp12_lanes(th, n, G, RPL, y0, ts.T, tables, True) for th in theta]
    ref = lrp8_cpu.solve_batch(theta, n, y0, ts.T)

    def band(a, b):
        return float(np.max(np.abs(a - b) / (1e-8 + 1e-6 * np.abs(a))))
    print("lane-layout port against the C restatement (direct pivots): band max %.3e, accepted steps differ in %d of %d"
          % (max(band(r, d[0]) for r, d in zip(ref[0], direct)), sum(int(r[0]) != d[2] for r, d in zip(ref[2], direct)), B))
    bs = [band(d[0], c[0]) for d, c in zip(direct, chain)]
    print("chained against direct pivots (4 x 8: chains of %d + %d): band shift max %.3e median %.3e; replicas with another step count: %d of %d"
          % (*chain_split(RPL), max(bs), float(np.median(bs)), sum((d[2], d[3]) != (c[2], c[3]) for d, c in zip(direct, chain)), B))
    print("largest |chain - direct| / direct over all steps, as a fraction of its chain's bound 2 (m + 1) 2^-53: %.3f" % max(c[4] for c in chain))
    print("largest relative spread of P over the four lanes of a replica: chained %.2e, direct %.2e"
          % (max(c[5] for c in chain), max(d[5] for d in direct)))


if __name__ == "__main__":
    main()
