"""Throughput of the HBM-workspace network integrator (net_solve_ws_kernel in csrc/pk_network_solve.hpp), one JSON line per case
(dev tool, run on an MI355X).

  python tools/gpu_bench_network_ws.py [case ...]     cases: union, n10k, s1000 (default: these three), fused[:network[:B[:runs]]]

union : 6 copies of tests/golden/netlarge_m0.npz (N = 600, S = 3 312), B = 1 024 and 8 192, rtol = atol = 1e-8
n10k  : synthetic.make_network(N=2000, total_sites=6000, n_K=200, n_tf_edges=5000), S = 10 000, B = 1 024 and 8 192, 1e-8
s1000 : the N = 300 / S = 1 000 synthetic network at B = 8 192: the workspace kernel forced against the LDS kernel (price of HBM over LDS)
fused : the union and the S = 10 000 network at B = 1 024 and 8 192, 1e-8: simulate + loss in ONE launch (simulate_objective_batch(method="rosw"),
        no trajectory) against simulate_batch + objective_batch, `runs` alternated runs each (default 5); candidates / s of every run and
        torch.cuda.max_memory_allocated of both paths.  fused:union:8192:3 runs one network, one B, three runs
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


def run(eng, X, t, reps=2, **kw):
    eng.simulate_batch(X[: min(64, X.shape[0])], t, **kw)          # warm-up: code objects, arena
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        Y, st, ns = eng.simulate_batch(X, t, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    ns = ns.cpu().numpy()
    return dict(B=int(X.shape[0]), S=eng.S, N=eng.N, seconds=round(best, 4), cand_per_s=round(X.shape[0] / best, 1),
                mean_steps=round(float(ns[:, 0].mean()), 1), mean_rejected=round(float(ns[:, 1].mean()), 2),
                state_steps_per_s=float(eng.S * ns.sum() / best), flagged=int((st.cpu().numpy() != 0).sum()),
                workspace_MiB=round(eng.workspace_bytes(X.shape[0]) / 2**20, 1))


def _peak(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, torch.cuda.max_memory_allocated()


def fused_leg(case, eng, X, t, runs, **opt):
    """Alternated runs of the fused launch and of the two-launch path on the same candidates; every protein / site observed at every
    time of its modality (rna from t = 4 on)."""
    lists, ld = eng.make_index_lists(t, t, t[t >= 4.0], t)
    lam = (1.0, 1.0, 1.0, 0.01)
    dflt = X[0]
    Xd = torch.as_tensor(X, device="cuda")

    def one():
        return eng.simulate_objective_batch(lists, Xd, t, defaults=dflt, lambdas=lam, method="rosw", **opt)[1]

    def two():
        Y, st, _ = eng.simulate_batch(Xd, t, **opt)
        return eng.objective_batch(lists, Y, x=Xd, defaults=dflt, lambdas=lam, status=st)[1]

    eng.simulate_objective_batch(lists, Xd[:64], t, defaults=dflt, lambdas=lam, method="rosw", **opt)          # warm-up: code objects, arena
    eng.simulate_batch(Xd[:64], t, **opt)
    rate = {"fused": [], "two_launch": []}
    peak = {}
    F = {}
    for _ in range(runs):
        for name, fn in (("fused", one), ("two_launch", two)):
            F[name], dt, peak[name] = _peak(fn)
            rate[name].append(round(X.shape[0] / dt, 2))
            print(f"{case} B={X.shape[0]} {name}: {dt:.2f} s", file=sys.stderr, flush=True)
    F1, F2 = F["fused"].cpu().numpy(), F["two_launch"].cpu().numpy()
    print(json.dumps(dict(case=case, B=int(X.shape[0]), S=eng.S, N=eng.N, T=int(t.size), cand_per_s=rate,
                          median={k: float(np.median(v)) for k, v in rate.items()},
                          peak_MiB={k: round(v / 2**20, 1) for k, v in peak.items()}, Y_MiB=round(X.shape[0] * t.size * eng.S * 8 / 2**20, 1),
                          max_rel_dF=float(np.max(np.abs(F1 - F2) / np.abs(F2))), failed=int((F2[:, 0] == 1e12).sum()))), flush=True)
    eng.free_loss(lists)


def main(cases):
    opt = dict(rtol=1e-8, atol=1e-8)
    if "union" in cases:
        g = np.load(ROOT / "tests" / "golden" / "netlarge_m0.npz")
        d = dict(g)
        eng = NetworkEngine.from_npz(synthetic.tile_network(d, 6))
        x = np.concatenate([np.ravel(g[n][0]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][0])]])
        for B in (1024, 8192):
            rows = x[None, :] * np.exp(0.2 * np.random.default_rng(B).standard_normal((B, x.size)))
            X = synthetic.tile_candidate(rows, 6, d)
            X[:, -1] = x[-1]
            print(json.dumps(dict(case="union6_netlarge_m0", **run(eng, X, g["t_eval"], **opt))), flush=True)
        eng.close()
    if "n10k" in cases:
        net = synthetic.make_network(N=2000, total_sites=6000, n_K=200, n_tf_edges=5000, model=0, seed=11)
        eng = NetworkEngine(**net)
        t = np.unique(np.concatenate([net["kin_grid"], [15.0]]))
        for B in (1024, 8192):
            X = synthetic.random_candidates(net, B, seed=B, spread=0.3)
            print(json.dumps(dict(case="n10k_m0", **run(eng, X, t, reps=1, **opt))), flush=True)
        eng.close()
    for spec in (c for c in cases if c.split(":")[0] == "fused"):
        part = spec.split(":")
        nets = [part[1]] if len(part) > 1 else ["union", "n10k"]
        Bs = [int(part[2])] if len(part) > 2 else [1024, 8192]
        runs = int(part[3]) if len(part) > 3 else 5
        for which in nets:
            if which == "union":
                g = np.load(ROOT / "tests" / "golden" / "netlarge_m0.npz")
                d = dict(g)
                eng = NetworkEngine.from_npz(synthetic.tile_network(d, 6))
                x = np.concatenate([np.ravel(g[n][0]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][0])]])
                t = g["t_eval"]
            else:
                net = synthetic.make_network(N=2000, total_sites=6000, n_K=200, n_tf_edges=5000, model=0, seed=11)
                eng = NetworkEngine(**net)
                t = np.unique(np.concatenate([net["kin_grid"], [15.0]]))
            for B in Bs:
                if which == "union":
                    rows = x[None, :] * np.exp(0.2 * np.random.default_rng(B).standard_normal((B, x.size)))
                    X = synthetic.tile_candidate(rows, 6, d)
                    X[:, -1] = x[-1]
                else:
                    X = synthetic.random_candidates(net, B, seed=B, spread=0.3)
                fused_leg("fused_union6_netlarge_m0" if which == "union" else "fused_n10k_m0", eng, X, t, runs, **opt)
            eng.close()
    if "s1000" in cases:
        net = synthetic.make_network(N=300, total_sites=400, n_K=60, n_tf_edges=700, model=0, seed=77)
        eng = NetworkEngine(**net)
        t = np.unique(np.concatenate([net["kin_grid"], [15.0]]))
        X = synthetic.random_candidates(net, 8192, seed=2)
        for kernel in ("workspace", "lds"):
            print(json.dumps(dict(case=f"s1000_m0_{kernel}", **run(eng, X, t, kernel=kernel, method="rosw", **opt))), flush=True)
        eng.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["union", "n10k", "s1000"])
