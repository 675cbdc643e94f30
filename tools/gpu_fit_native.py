"""Time ``fit_rows_batch(driver="native")`` (pk_fit_protein_rows_batch) against the default Python driver on the three shapes of bench.py's
``lm_leg``: 48 starts at distmod n = 8, 480 rows at n = 8 and the 480-row lambda-scan shape at n = 30 -- identical inputs, 2 warm-up runs and
5 timed runs each, wall time around the whole fit with a device synchronisation on both sides, medians reported with the launch and host-wait
counts beside them.  Prints one JSON object; ``--out FILE`` also writes it.

    python tools/gpu_fit_native.py [--out profiles/fit_native_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

TGRID = np.array([0.0, 0.5, 0.75, 1.0, 2.0, 4.0, 8.0, 16.0, 30.0, 60.0, 120.0, 240.0, 480.0, 960.0])
SHAPES = (("multistart_48_starts_distmod_n8", 8, 48, 60), ("rows_480_distmod_n8", 8, 480, 60), ("lambda_scan_480_rows_distmod_n30", 30, 480, 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    from phoskintime_amd import batch
    from phoskintime_amd.paramest import fit_rows_batch, multistart_candidates
    out = {"method": f"wall ms of one whole fit, torch.cuda.synchronize() before and after; {args.warmup} warm-ups, median of {args.runs} runs; "
                     "inputs as bench.py lm_leg; python = fit_rows_batch defaults (jacobian auto -> sens, lm_algebra auto)"}
    for label, n, rows, iters in SHAPES:
        P, S = 4 + 2 * n, n + 2
        rng = np.random.default_rng(20260515 + 9)
        th_true = rng.uniform(0.2, 2.0, P)
        flat = batch.solve_ode_batch("distmod", th_true[None], np.ones(S), n, TGRID, want_sol=False).flat[0].cpu().numpy()
        target = np.abs(flat * (1 + 0.02 * rng.standard_normal(flat.size)))
        lb, ub = np.zeros(P), np.full(P, 20.0)
        P0 = multistart_candidates("BENCH", rng.uniform(lb, ub), lb, ub, n_starts=rows)
        leg = {"rows": rows, "P": P, "residuals": int(flat.size), "max_iter": iters}
        for driver in ("python", "native"):
            ts, fit = [], None
            for k in range(args.warmup + args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fit = fit_rows_batch("distmod", n, TGRID, P0, np.ones(S), target, bounds=(lb, ub), max_iter=iters, driver=driver)
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ts.append(1e3 * (time.perf_counter() - t0))
            leg[driver] = {"wall_ms_median": float(np.median(ts)), "wall_ms_min": float(np.min(ts)), "wall_ms_max": float(np.max(ts)), "iterations": int(fit.n_iter),
                           "solves": int(fit.n_solves), "n_launches": int(fit.n_launches), "best_cost": float(fit.cost.min()), "median_cost": float(np.median(fit.cost))}
            if fit.counters:
                leg[driver].update(host_waits=fit.counters["host_waits"], jacobian_phases=fit.counters["jacobian_phases"], trial_rounds=fit.counters["trial_rounds"])
        leg["native_over_python"] = leg["native"]["wall_ms_median"] / leg["python"]["wall_ms_median"]
        out[label] = leg
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        Path(args.out).write_text(s + "\n")


if __name__ == "__main__":
    main()
