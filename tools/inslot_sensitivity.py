"""Dev tool (CPU): how far carrying R and P in spare slots of the lane layout (the resident layout of csrc/pk_dist_fast.hpp) moves the
LRP12 trajectories of the distributive model against the shadowed layout.

`lrp12_resident` is a numpy port of the throughput kernel's step in the resident layout: G lanes x RPL rows, slot s = lane + G * row
holds state s (R in slot 0, P in slot 1, site i in slot i + 2, the rest idle); R is a row with pivot 1 + q B, the P slot's chain factor
is q itself, row 0 enters the one group sum of a solve as r_0 ws0 (ws0 = C / (1 + q B) | 1 / q | winv_0), x_P is that sum times q sinv,
and lane 1 carries winv_0 = 0, cw_0 = 1 so that its row 0 comes out as x_P; the right-hand side of row 0 is
fma(k1, P, fma(-dg0, X, k3)) per lane.  The pivots of a lane are inverted by the kernel's chain sequence (RPL pivots: one chain up to
five, two even ones above), `1 / x` standing in for fast_rcp; plain numpy arithmetic stands in for the FMAs.

It runs the benchmark's parameter distribution (n = 30 on 4 x 8, theta ~ U(0, 20), y0 = 1, the 14-point grid, rtol 1e-6 / atol 1e-8)
against the shadowed port (tools/pivot_chain_sensitivity.py, chained pivots) and the C restatement, and prints the largest band shift
|dy| / (1e-8 + 1e-6 |y|) and the step-count differences.
usage: inslot_sensitivity.py [replicas = 24]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import pivot_chain_sensitivity as pcs  # noqa: E402


def chain_split_resident(rpl):
    """(m0, m1): the chains over the rpl pivots of a resident lane (one chain up to five pivots, two even ones above)."""
    m0 = rpl if rpl <= 5 else (rpl + 1) // 2
    return m0, rpl - m0


def resident_fits(n, G, RPL):
    return G * RPL >= n + 2


def lrp12_resident(th, n, G, RPL, y0, t, tables, rtol=1e-6, atol=1e-8, max_steps=100000, h0=0.0, resolvent=False):
    """One replica on G lanes x RPL rows, resident layout.  (sol [T, n + 2], status, accepted, rejected)
    resolvent = True forms the first stage as the step loop of csrc/pk_dist_fast.hpp does: gamma z_1 =
    solve(y + q b) - y with the weights B_k / gamma, E_k / gamma; False keeps the earlier solve(h f(y))."""
    assert resident_fits(n, G, RPL)
    GAM, LB, LE = tables
    NS = 12
    S = n + 2
    A, Bc, Cc, D = (float(v) for v in th[:4])
    slot = np.arange(G)[:, None] + G * np.arange(RPL)[None, :]
    live = slot < S
    site = live & (slot >= 2)
    idx = np.where(site, slot - 2, 0)
    Sr = np.where(site, np.asarray(th[4:4 + n], float)[idx], 0.0)
    dg = np.where(site, 1.0 + np.asarray(th[4 + n:4 + 2 * n], float)[idx], 1.0)
    dg[0, 0], dg[1, 0] = Bc, -Cc
    Dsum = D + float(Sr.sum())
    w0 = np.ones(G); w0[0] = Cc
    k3c = np.zeros(G); k3c[0] = A
    y = np.where(live, np.asarray(y0, float)[np.where(live, slot, 0)], 0.0)
    m0, m1 = chain_split_resident(RPL)
    WB, WE = (LB / GAM, LE / GAM) if resolvent else (LB, LE)

    def sites_only(v):
        w = v.copy(); w[0, 0] = 0.0; w[1, 0] = 0.0
        return float(w.sum())

    def emit(v):
        return v[live][np.argsort(slot[live])]

    def rhs(v, sg):
        Rb, Pb = v[0, 0], v[1, 0]
        f = Sr * Pb - dg * v
        k1 = Sr[:, 0].copy(); k1[1] = -Dsum
        X = v[:, 0].copy(); X[1] = Rb
        k3 = k3c.copy(); k3[1] = sg
        f[:, 0] = k1 * Pb + (-dg[:, 0] * X + k3)
        return f

    def norm(e, a, b):
        v = (np.abs(e) / (atol + rtol * np.maximum(np.abs(a), np.abs(b)))).ravel()
        return (True, 0.0) if np.isnan(v).any() else (False, float(v.max()))

    nT = len(t)
    sol = np.zeros((nT, S)); sol[0] = emit(y)
    sg = sites_only(y)
    acc = rej = status = 0
    after_reject = False
    tc = float(t[0])
    f = rhs(y, sg)
    sc = atol + rtol * np.abs(y)
    d0, d1 = float(np.max(np.abs(y) / sc)), float(np.max(np.abs(f) / sc))
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
            piv = 1.0 + q * dg
            piv[1, 0] = q
            winv = np.empty_like(piv)
            winv[:, :m0] = pcs.chain_inverse(piv[:, :m0])
            if m1:
                winv[:, m0:] = pcs.chain_inverse(piv[:, m0:])
            cw = q * Sr * winv
            sinv = 1.0 / (1.0 + q * (Dsum - float(cw.sum())))
            qs = q * sinv
            ws0 = winv[:, 0] * w0
            winv[1, 0] = 0.0
            cw[1, 0] = 1.0

            def solve(r):
                tt = r * winv
                xP = float((r[:, 0] * ws0 + tt[:, 1:].sum(axis=1)).sum()) * qs
                return cw * xP + tt

            if resolvent:
                r = y.copy(); r[:, 0] = q * k3c + y[:, 0]
                z = solve(r) - y
            else:
                z = solve(hs * rhs(y, sg))
            yn = y + WB[0] * z
            e = np.zeros_like(y)
            for st in range(1, NS):
                z = solve(z)
                yn = yn + WB[st] * z
                e = e + WE[st] * z
            bad, err = norm(e, y, yn)
            if bad or err > 1e300:
                rej += 1; after_reject = True; h = 0.1 * hs
                if not (np.isfinite(y).all() and np.isfinite(th[:4 + 2 * n]).all()):
                    status |= 1; break
                continue
            fac = min(max(err, 1e-30), 1e30) ** (1.0 / (NS - 1.0)) / 0.9
            fac = max(1.0 / 6.0, min(5.0, fac))
            hnew = hs / fac
            if err <= 1.0:
                acc += 1
                y, sg = yn, sites_only(yn); tc += hs
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
        sol[k] = emit(y)
    return sol, status, acc, rej


def band(a, b, rtol=1e-6, atol=1e-8):
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(a))))


def compare(B=24, n=30, G=4, RPL=8, seed=20260515):
    """(band shift per replica resident vs shadowed, replicas with another step count, band resident vs C restatement,
    largest accepted-step difference resident vs C restatement)"""
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import test_gpu_dist_fast_sitesum as ts
    from oracle import lrp8_cpu
    theta = np.random.default_rng(seed).uniform(0.0, 20.0, (B, 4 + 2 * n))
    y0 = np.ones(n + 2)
    tables = ts._tables()
    shadow = [pcs.lrp12_lanes(th, n, G, RPL, y0, ts.T, tables, True) for th in theta]
    res = [lrp12_resident(th, n, G, RPL, y0, ts.T, tables) for th in theta]
    ref = lrp8_cpu.solve_batch(theta, n, y0, ts.T)
    assert not any(r[1] for r in res) and not any(s[1] for s in shadow) and not ref[1].any()
    shift = [band(s[0], r[0]) for s, r in zip(shadow, res)]
    moved = sum((s[2], s[3]) != (r[2], r[3]) for s, r in zip(shadow, res))
    vs_c = max(band(c, r[0]) for c, r in zip(ref[0], res))
    dsteps = max(abs(int(c[0]) - r[2]) for c, r in zip(ref[2], res))
    return shift, moved, vs_c, dsteps


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    shift, moved, vs_c, dsteps = compare(B)
    print("resident against shadowed port (4 x 8, n = 30, chains of %d + %d): band shift max %.3e median %.3e; replicas with another step count: %d of %d"
          % (*chain_split_resident(8), max(shift), float(np.median(shift)), moved, B))
    print("resident port against the C restatement: band max %.3e, accepted steps differ by at most %d" % (vs_c, dsteps))


if __name__ == "__main__":
    main()
