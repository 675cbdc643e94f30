"""Timing of the network fit on the device against its host twin (recorded, not gated; not a test).

Workload: ``netlarge_m0`` (N = 100, S = 552), B = 64 candidates log-normal 0.2 around the fixture's two, K = 6 columns (one of c_k, A, B,
D, Dp, E), rtol = 1e-7 / atol = 1e-9, obj_w = (1, 1, 1), the prior centred on the fixture's first candidate, no box; observations: the
reference predictions of ``net_objgrad_reference.loss_data``.  ``polish_batch(driver="native")`` against ``driver="python"``: one warm-up
of each, then three alternated repetitions; a host clock around work that ends in a device synchronise.  Prints wall times, the six
counters of each driver and the final costs' agreement.

    python tools/gpu_net_fit_time.py [--B 64] [--reps 3] [--max-iter 6] [--only native]

``--only native`` runs the native driver alone (one warm-up, one run): the shape to put under ``rocprofv3 --kernel-trace --stats`` for the
share of time in the four net_fit kernels."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import net_objgrad_reference as og          # noqa: E402
import net_sens_reference as ref            # noqa: E402
from oracle import network_models as nm     # noqa: E402
from phoskintime_amd.global_model import NetworkEngine, polish      # noqa: E402

KINDS = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
OPT = dict(rtol=1e-7, atol=1e-9)


def _row(g, k):
    return np.concatenate([np.ravel(g[n][k]) for n in KINDS[:-1]] + [[float(g["tf_scale"][k])]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=6)
    ap.add_argument("--only", choices=("native",), default=None)
    a = ap.parse_args()
    g = np.load(ref.GOLDEN / "netlarge_m0.npz")
    net = nm.Network.from_npz(g)
    eng = NetworkEngine.from_npz(g)
    t = g["t_eval"]
    rng = np.random.default_rng(0)
    X = np.stack([_row(g, k % 2) for k in range(a.B)]) * np.exp(0.2 * rng.standard_normal((a.B, eng.n_var)))
    sl = ref.slices(net)
    cols = np.array([sl[k][0] + 1 for k in ("c_k", "A_i", "B_i", "D_i", "Dp_i", "E_i")], dtype=np.int32)
    ld = og.loss_data(net, t)
    loss = eng.make_loss(ld, t.size)
    kw = dict(obj_w=(1.0, 1.0, 1.0), defaults=_row(g, 0), lambdas=og.LAM, y0=g["y0"], max_iter=a.max_iter, **OPT)

    def run(driver):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = polish.polish_batch(eng, loss, ld, X, t, cols, driver=driver, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    drivers = ("native",) if a.only else ("native", "python")
    for d in drivers:                                                             # one warm-up of each
        run(d)
    times, last = {d: [] for d in drivers}, {}
    for _ in range(1 if a.only else a.reps):                                       # alternated repetitions
        for d in drivers:
            dt, last[d] = run(d)
            times[d].append(dt)
    for d in drivers:
        print(f"{d:7s} wall s " + " / ".join(f"{v:.3f}" for v in times[d]) + f"   counters {last[d].counters}   reasons "
              f"{np.bincount(last[d].reason, minlength=5).tolist()}", flush=True)
    if not a.only:
        n, p = last["native"], last["python"]
        print(f"native / python: median wall {np.median(times['native']) / np.median(times['python']):.3f}   max |cost_n - cost_p| / cost_p "
              f"{float(np.max(np.abs(n.cost - p.cost) / p.cost)):.2e}   same counters {n.counters == p.counters}", flush=True)
    eng.free_loss(loss)


if __name__ == "__main__":
    main()
