"""Time and memory of the network Morris measurement, fused into the order-3 integrator against the three-step route, one JSON line per
shape (dev tool, run on an MI355X under a timeout; not a test, and bench.py does not call it).

  python tools/gpu_net_measure_scan.py [config4] [union6] [--repeats R] [--rows-union B]

config4 : tests/golden/netlarge_m0.npz (N = 100, S = 552), BASELINE config 4's named shape: 128 x (200 + 1) = 25 728 rows, the fitted
          vector with 200 entries perturbed by +-5 %; method "rosw" on the general LDS kernel
union6  : 6 copies of that network (N = 600, S = 3 312): beyond one workgroup, the default plan (order-3 method, workspace kernel);
          B = 2 048 rows, every entry perturbed by +-5 %

Both at the settings of simulate_and_measure for the order-3 method (rtol 1e-5, atol 1e-7, max_steps 5 000 T), the union grid of
config.TIME_POINTS_* (T = 15), every protein / site at every time of its modality, metric total_signal.  Routes, alternated R times
(default 5) after one warm-up each on the full shape:
  parent : simulate_batch + observables_batch + scalar_metric_batch
  fused  : simulate_measure_batch (metric only)
Reported: wall seconds of every repeat, median, min and max; rows / s at the median; mean accepted / rejected steps; the bytes of the
tensors each route allocates (computed from the shapes) and torch.cuda.max_memory_allocated over one call (which does not see the scratch
arena both routes share); the largest relative difference of the two metrics.
"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from phoskintime_amd.global_model import NetworkEngine, synthetic  # noqa: E402
from phoskintime_amd.global_model import config as gcfg  # noqa: E402
from phoskintime_amd.global_model.sensitivity import scalar_metric_batch  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, torch.cuda.max_memory_allocated()


def leg(case, eng, X, repeats, **opt):
    tp, tr = gcfg.TIME_POINTS_PROTEIN, gcfg.TIME_POINTS_RNA
    t = np.unique(np.concatenate([tp, tr, tp]).astype(np.float64))
    lists, ld = eng.make_index_lists(t, tp, tr, tp)
    n_obs = ld["p_prot"].size + ld["p_rna"].size + ld["p_pho"].size
    B = X.shape[0]
    Xd = torch.as_tensor(X, device="cuda")
    kw = dict(rtol=1e-5, atol=1e-7, max_steps=5000 * t.size, **opt)
    steps = {}

    def parent():
        Y, st, ns = eng.simulate_batch(Xd, t, **kw)
        steps["parent"] = ns
        pred = eng.observables_batch(lists, Y, n_obs, eps=1e-12)
        return scalar_metric_batch(pred, "total_signal"), st

    def fused():
        out = eng.simulate_measure_batch(lists, Xd, t, metric="total_signal", eps=1e-12, **kw)
        if out is None:
            raise RuntimeError("refused: " + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode())
        steps["fused"] = out[3]
        return out[0], out[2]

    routes = (("parent", parent), ("fused", fused))
    for _, fn in routes:                                     # warm-up on the full shape: code objects, scratch arena, allocator pool
        fn()
    torch.cuda.synchronize()
    wall = {k: [] for k, _ in routes}
    peak, val = {}, {}
    for _ in range(repeats):
        for name, fn in routes:
            (val[name], st), dt, peak[name] = _timed(fn)
            wall[name].append(round(dt, 4))
            print(f"{case} {name}: {dt:.3f} s", file=sys.stderr, flush=True)
    a, b = val["fused"].cpu().numpy(), val["parent"].cpu().numpy()
    ok = st.cpu().numpy() == 0
    ns = {k: v.double().mean(dim=0).cpu().numpy() for k, v in steps.items()}
    per_row = 8 + 4 + 8                                      # metric, status, n_steps
    print(json.dumps(dict(
        case=case, B=B, N=eng.N, S=eng.S, T=int(t.size), n_obs=int(n_obs), opts=opt, wall_s=wall,
        median_s={k: float(np.median(v)) for k, v in wall.items()}, min_s={k: min(v) for k, v in wall.items()}, max_s={k: max(v) for k, v in wall.items()},
        rows_per_s={k: round(B / float(np.median(v)), 1) for k, v in wall.items()},
        fused_over_parent=round(float(np.median(wall["fused"]) / np.median(wall["parent"])), 4),
        mean_steps={k: [round(float(v[0]), 2), round(float(v[1]), 2)] for k, v in ns.items()},
        allocated_bytes=dict(parent=B * (t.size * eng.S * 8 + n_obs * 8 + per_row), fused=B * per_row, Y=B * t.size * eng.S * 8, pred=B * n_obs * 8),
        peak_MiB={k: round(v / 2**20, 1) for k, v in peak.items()},
        flagged=int((~ok).sum()), max_rel_diff=float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))))), flush=True)
    eng.free_loss(lists)


def main(argv):
    repeats, rows_union = 5, 2048
    cases = []
    it = iter(argv)
    for a in it:
        if a == "--repeats":
            repeats = int(next(it))
        elif a == "--rows-union":
            rows_union = int(next(it))
        else:
            cases.append(a)
    cases = cases or ["config4", "union6"]
    g = np.load(ROOT / "tests" / "golden" / "netlarge_m0.npz")
    x = np.concatenate([np.ravel(g[n][0]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][0])]])
    if "config4" in cases:
        eng = NetworkEngine.from_npz(g)
        rng = np.random.default_rng(4)
        vary = np.sort(rng.choice(eng.n_var, size=200, replace=False))
        X = np.repeat(x[None, :], 128 * 201, axis=0)
        X[:, vary] *= rng.uniform(0.95, 1.05, size=(X.shape[0], vary.size))
        leg("config4_named_shape_netlarge_m0", eng, X, repeats, method="rosw", kernel="lds")
        eng.close()
    if "union6" in cases:
        d = dict(g)
        eng = NetworkEngine.from_npz(synthetic.tile_network(d, 6))
        rows = x[None, :] * np.random.default_rng(6).uniform(0.95, 1.05, size=(rows_union, x.size))
        X = synthetic.tile_candidate(rows, 6, d)
        X[:, -1] = x[-1]
        leg("union6_netlarge_m0", eng, X, repeats)
        eng.close()


if __name__ == "__main__":
    main(sys.argv[1:])
