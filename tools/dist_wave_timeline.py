"""Dev tool (GPU): the wave timeline of the benchmark's distmod launch, SIMD by SIMD ("Pacing the waves of a SIMD").

Runs bench.py's batch (same seed, theta ~ U(0, 20)^64, n = 30, B = 65 536, trajectories + total_signal) on the traced build of its kernel
(PK_DIST_TRACE=1, set here before the library reads it): a few hundred untraced-buffer launches for the clock ramp, then one launch
with the record buffer attached.  Every wave (one per workgroup) leaves {blockIdx, s_memrealtime at entry and exit, HW_ID, XCC_ID,
iterations}; the records are grouped by SIMD and summarised.  The policy is whatever PK_DIST_SCHED says (unset: the default).

usage: PK_DIST_SCHED=off python tools/dist_wave_timeline.py [--out profiles/NAME.txt] [--replicas B] [--ramp N] [--records FILE.npy]"""
import argparse
import collections
import os
import sys
from pathlib import Path

os.environ["PK_DIST_TRACE"] = "1"
import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
TGRID = np.array([0.0, 0.5, 0.75, 1.0, 2.0, 4.0, 8.0, 16.0, 30.0, 60.0, 120.0, 240.0, 480.0, 960.0])
TICK_US = 0.01                          # s_memrealtime: 100 MHz


def collect(B, ramp):
    import torch
    from phoskintime_amd import batch, _capi
    n, S, P = 30, 32, 64
    theta = torch.as_tensor(np.random.default_rng(20260515 + 2).uniform(0.0, 20.0, (B, P)), device="cuda")
    y0 = torch.ones(S, dtype=torch.float64, device="cuda")
    tt = torch.as_tensor(TGRID, device="cuda")
    out = batch.BatchResult(sol=torch.empty((B, TGRID.size, S), dtype=torch.float64, device="cuda"), flat=None,
                            metric=torch.empty(B, dtype=torch.float64, device="cuda"), status=torch.zeros(B, dtype=torch.int32, device="cuda"),
                            n_steps=torch.zeros((B, 2), dtype=torch.int32, device="cuda"))
    ctx = batch.get_context()
    run = lambda: batch.solve_ode_batch(_capi.DIST, theta, y0, n, tt, out=out, want_flat=False, metric="total_signal")
    for _ in range(ramp):
        run()
    torch.cuda.synchronize()
    nblk = (B + 15) // 16
    rec = torch.zeros((nblk, 4), dtype=torch.int64, device="cuda")
    ctx.check(ctx.lib.pk_dist_trace_set(ctx.handle, rec.data_ptr(), nblk))
    run()
    torch.cuda.synchronize()
    ctx.check(ctx.lib.pk_dist_trace_set(ctx.handle, None, 0))
    assert int(out.status.abs().sum()) == 0
    return rec.cpu().numpy()


def hist(values):
    c = collections.Counter(int(v) for v in values)
    return "  ".join(f"{k}: {c[k]}" for k in sorted(c))


def q(x):
    x = np.asarray(x, dtype=float)
    return "n/a" if x.size == 0 else f"median {np.median(x):7.2f}  mean {x.mean():7.2f}  min {x.min():7.2f}  max {x.max():7.2f}"


def summarise(rec, B):
    nblk = rec.shape[0]
    w = rec[:, 2:].copy().view(np.uint32).reshape(nblk, 4).astype(np.int64)          # block, hw_id, xcc_id, iterations
    t0 = rec[:, 0].min()
    ent, ext = (rec[:, 0] - t0) * TICK_US, (rec[:, 1] - t0) * TICK_US                  # microseconds from the first wave's entry
    blk, hw, xcc, its = w[:, 0], w[:, 1], w[:, 2] & 0xF, w[:, 3]
    slot, simd, cu, sh, se = hw & 0xF, (hw >> 4) & 3, (hw >> 8) & 0xF, (hw >> 12) & 1, (hw >> 13) & 7
    key = xcc << 12 | (hw >> 4) & 0xFFF
    end = ext.max()
    L = [f"distmod LRP12 wave timeline: B = {B}, {nblk} waves, PK_DIST_SCHED = {os.environ.get('PK_DIST_SCHED', '(default)')}",
         f"launch (first entry to last exit): {end:.2f} us;  iterations per wave: {q(its)}",
         f"distinct XCC {np.unique(xcc).size}  SE {np.unique(se).size}  SH {np.unique(sh).size}  CU ids {np.unique(cu).size}  SIMD ids {np.unique(simd).size}"
         f"  wave slots used: {hist(slot)}"]
    simds = np.unique(key)
    R1 = 3 * simds.size
    L.append(f"SIMDs that received waves: {simds.size}  (three slots each: R1 = {R1})")
    n_waves, order_gap, fourth, lone, resid = [], [], [], [], np.zeros(5)
    first_fin, life_first, life_late, rate_first, rate_late = [[], [], []], [], [], [], []
    lead_slot, lead_block, late_last = [], [], 0
    for s in simds:
        m = np.flatnonzero(key == s)
        m = m[np.argsort(ent[m])]
        n_waves.append(m.size)
        first_exit = ext[m].min()
        first = m[ent[m] < first_exit]                      # the first round: resident before any wave of this SIMD ended
        late = m[ent[m] >= first_exit]
        fin = np.sort(ext[first])
        for i in range(min(3, fin.size)):
            first_fin[i].append(fin[i])
        if fin.size > 1:
            order_gap.append(fin[-1] - fin[0])
        if late.size:
            fourth.append(ent[late[0]])
            late_last += int(ext[late].max() >= ext[m].max())
        life_first += list(ext[first] - ent[first]); life_late += list(ext[late] - ent[late])
        rate_first += list((ext[first] - ent[first]) / np.maximum(its[first], 1)); rate_late += list((ext[late] - ent[late]) / np.maximum(its[late], 1))
        lead_slot.append(int(np.count_nonzero((slot[m] == 0) & (blk[m] < R1))))
        lead_block.append(int(np.count_nonzero(blk[m] < R1 // 3)))
        # residency: sweep the entries (+1) and exits (-1) of this SIMD from the launch's start to its end
        ev = sorted([(ent[i], 1) for i in m] + [(ext[i], -1) for i in m])
        t, c, start1 = 0.0, 0, 0.0
        for tt, d in ev:
            resid[min(c, 4)] += tt - t
            t, c = tt, c + d
            if c == 1:
                start1 = tt                               # one wave resident from here on, whether the others left or this one just arrived
        resid[0] += end - t
        # the final lone phase: from the last moment the SIMD went to exactly one resident wave to that wave's exit
        lone.append(ext[m].max() - start1)
    L += [f"waves per SIMD: {hist(n_waves)}",
          f"first round, finish of the 1st / 2nd / 3rd wave to end [us]:",
          *[f"    {i + 1}: {q(first_fin[i])}" for i in range(3)],
          f"    last minus first finish within the round [us]: {q(order_gap)}",
          f"arrival of the next wave after the round (the fourth) [us]: {q(fourth)}",
          f"SIMDs whose last wave to end is a later-round wave: {late_last} of {simds.size}",
          f"final lone-wave phase per SIMD [us]: {q(lone)}",
          f"    SIMDs with a lone phase > 5 us: {int(np.count_nonzero(np.asarray(lone) > 5.0))}, > 20 us: {int(np.count_nonzero(np.asarray(lone) > 20.0))}, > 40 us: {int(np.count_nonzero(np.asarray(lone) > 40.0))}",
          f"wave lifetime [us]: first round {q(life_first)}",
          f"                    later      {q(life_late)}",
          f"us per iteration:   first round {q(rate_first)}",
          f"                    later      {q(rate_late)}",
          "SIMD-time by resident waves, summed over the SIMDs, as a share of SIMDs x launch:"]
    tot = simds.size * end
    L += [f"    {('4+', '3', '2', '1', '0')[i]} waves: {resid[(4, 3, 2, 1, 0)[i]] / tot * 100:6.2f} %   ({resid[(4, 3, 2, 1, 0)[i]] / simds.size:7.2f} us per SIMD)" for i in range(5)]
    L += [f"mean resident waves per SIMD over the launch: {sum(i * resid[i] for i in range(5)) / tot:.3f}",
          f"lone phase, launch-wide: {np.sum(lone) / tot * 100:.2f} % of SIMD-time",
          "leader rules, waves per SIMD they name (exactly one is the aim):",
          f"    wave slot 0 and blockIdx < R1: {hist(lead_slot)}",
          f"    blockIdx < R1 / 3:             {hist(lead_block)}"]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--replicas", type=int, default=65536)
    ap.add_argument("--ramp", type=int, default=300)
    ap.add_argument("--records", default=None, help="also keep the raw records as .npy")
    a = ap.parse_args()
    rec = collect(a.replicas, a.ramp)
    if a.records:
        np.save(a.records, rec)
    txt = summarise(rec, a.replicas)
    print(txt, end="")
    if a.out:
        Path(a.out).write_text(txt)


if __name__ == "__main__":
    main()
