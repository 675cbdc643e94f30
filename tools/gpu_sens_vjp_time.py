#!/usr/bin/env python3
"""Times the weighted least-squares cost and its gradient J^T r three ways on one card, HIP events around the launches:
gpu_sens_vjp_time.py [--out FILE.json]

  (a) solve_ode_sens_batch, then the contraction a caller writes without the VJP entry point (r = w (flat - target), 0.5 sum r^2 and
      torch.einsum("bf,bfp->bp", w r, dflat)); the kernel and the contraction are timed separately
  (b) solve_ode_vjp_batch in least-squares mode without flat
  (c) solve_ode_vjp_batch in least-squares mode with want_flat=True

Shapes: those of tools/gpu_sens_metric_time.py -- distmod n = 30, succmod n = 30 (B = 480, 4 096), randmod n = 6 (B = 480, 1 024); 14-point
grid, default tolerances, shared w and target.  One warm-up each, five alternated repeats; prints medians with min / max, mean step
counts and the bytes each route writes (from the shapes), one JSON line per shape.  No threshold: the comparison is (b) against
(a)'s kernel + contraction; (b) executes the steps of (a)'s kernel and stores B (1 + P) doubles instead of B F (1 + P)."""
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
        rng = np.random.default_rng(1)
        th = torch.as_tensor(rng.uniform(0.2, 2.0, size=(B, P)), device="cuda")
        y0 = torch.ones(S, dtype=torch.float64, device="cuda"); t = torch.as_tensor(pm.TIME_POINTS, device="cuda")
        w = torch.as_tensor(rng.uniform(0.5, 2.0, size=F), device="cuda"); tg = torch.as_tensor(rng.uniform(0.1, 1.0, size=F), device="cuda")
        routes = {
            "a_kernel": lambda: batch.solve_ode_sens_batch(model, th, y0, n, t),
            "b_vjp": lambda: batch.solve_ode_vjp_batch(model, th, y0, n, t, w, tg),
            "c_vjp_flat": lambda: batch.solve_ode_vjp_batch(model, th, y0, n, t, w, tg, want_flat=True),
        }

        def contract_a(r):
            res = w * (r.flat - tg)
            return 0.5 * (res * res).sum(dim=1), torch.einsum("bf,bfp->bp", w * res, r.dflat)

        ms = {k: [] for k in list(routes) + ["a_contract"]}
        steps = {}
        agree = None
        for k, fn in routes.items():                      # one warm-up each
            r = fn()
            if k == "a_kernel":
                cost_a, grad_a = contract_a(r)
            elif k == "b_vjp":                            # the same numbers, to the chunks' own state values
                agree = float(((r.grad - grad_a).abs().max() / grad_a.abs().max()).item())
            torch.cuda.synchronize()
            steps[k] = float(r.n_steps[:, 0].double().mean()); assert int((r.status != 0).sum()) == 0
            del r
        for _ in range(REPEATS):                           # alternated
            for k, fn in routes.items():
                dt, r = timed(fn)
                ms[k].append(dt)
                if k == "a_kernel":
                    ms["a_contract"].append(timed(lambda: contract_a(r))[0])
                del r
        med = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        row = {"model": model, "n_sites": n, "B": B, "P": P, "F": F, "mean_steps": steps, "max_rel_grad_difference_b_vs_a": agree,
               "bytes_written": {"a": 8 * B * F * (1 + P) + 12 * B, "b": 8 * B * (1 + P) + 12 * B, "c": 8 * B * (1 + P) + 8 * B * F + 12 * B},
               **{k: med(v) for k, v in ms.items()}}
        row["a_total_median_ms"] = row["a_kernel"]["median_ms"] + row["a_contract"]["median_ms"]
        row["b_minus_a_kernel_ms"] = row["b_vjp"]["median_ms"] - row["a_kernel"]["median_ms"]
        row["spread_ms"] = max(row["a_kernel"]["max_ms"] - row["a_kernel"]["min_ms"], row["b_vjp"]["max_ms"] - row["b_vjp"]["min_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        pathlib.Path(out_path).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
