#!/usr/bin/env python3
"""Times d(metric)/d(theta) three ways on one card, HIP events around the launches: gpu_sens_metric_time.py [--out FILE.json]

  (a) solve_ode_sens_batch, then the torch reduction a caller would write today for the flat-visible part (flat.sum, dflat.sum over F);
      the kernel and the reduction are timed separately
  (b) solve_ode_sens_metric_batch with want_dflat=True
  (c) solve_ode_sens_metric_batch with neither flat nor dflat

Shapes: distmod n = 30, succmod n = 30 (B = 480, 4 096), randmod n = 6 (B = 480, 1 024); 14-point grid, default tolerances, metric
total_signal.  One warm-up each, five alternated repeats; prints medians with min / max, mean step counts and the bytes each route
writes (from the shapes), one JSON line per shape.  Route (c) executes the steps of (a)'s kernel and stores less: it must not be
slower than that kernel beyond the spread of the repeats."""
import json, pathlib, statistics, sys
import numpy as np, torch
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from phoskintime_amd import batch
from oracle import protein_models as pm

SHAPES = [("distmod", 30, 480), ("distmod", 30, 4096), ("succmod", 30, 480), ("succmod", 30, 4096), ("randmod", 6, 480), ("randmod", 6, 1024)]
REPEATS = 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b), out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rows = []
    for model, n, B in SHAPES:
        mid = pm.MODEL_IDS[model]; S, P = pm.n_states(mid, n), pm.n_params(mid, n)
        T = pm.TIME_POINTS.size; F = batch.flat_len(model, n, T)
        th = torch.as_tensor(np.random.default_rng(1).uniform(0.2, 2.0, size=(B, P)), device="cuda")
        y0 = torch.ones(S, dtype=torch.float64, device="cuda"); t = torch.as_tensor(pm.TIME_POINTS, device="cuda")
        routes = {
            "a_kernel": lambda: batch.solve_ode_sens_batch(model, th, y0, n, t),
            "b_metric_dflat": lambda: batch.solve_ode_sens_metric_batch(model, th, y0, n, t, want_dflat=True),
            "c_metric_only": lambda: batch.solve_ode_sens_metric_batch(model, th, y0, n, t),
        }
        reduce_a = lambda r: (r.flat.sum(dim=1), r.dflat.sum(dim=1))
        ms = {k: [] for k in list(routes) + ["a_reduce"]}
        steps = {}
        for k, fn in routes.items():                      # one warm-up each
            r = fn()
            if k == "a_kernel":
                reduce_a(r)
            torch.cuda.synchronize()
            steps[k] = float(r.n_steps[:, 0].double().mean()); assert int((r.status != 0).sum()) == 0
            del r
        for _ in range(REPEATS):                           # alternated
            for k, fn in routes.items():
                dt, r = timed(fn)
                ms[k].append(dt)
                if k == "a_kernel":
                    ms["a_reduce"].append(timed(lambda: reduce_a(r))[0])
                del r
        med = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        row = {"model": model, "n_sites": n, "B": B, "P": P, "F": F, "mean_steps": steps,
               "bytes_written": {"a": 8 * B * F * (1 + P) + 12 * B, "b": 8 * B * (1 + P) + 8 * B * F * P + 12 * B, "c": 8 * B * (1 + P) + 12 * B},
               **{k: med(v) for k, v in ms.items()}}
        spread = max(row["a_kernel"]["max_ms"] - row["a_kernel"]["min_ms"], row["c_metric_only"]["max_ms"] - row["c_metric_only"]["min_ms"])
        row["c_minus_a_kernel_ms"] = row["c_metric_only"]["median_ms"] - row["a_kernel"]["median_ms"]
        row["spread_ms"] = spread
        row["c_not_slower_than_a_kernel"] = bool(row["c_minus_a_kernel_ms"] <= spread)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        pathlib.Path(out_path).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
