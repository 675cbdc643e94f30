"""Timing of the objective-gradient launch on HBM slabs against the LDS route (recorded, not gated; not a test).

Workload: ``netlarge_m0`` (N = 100, S = 552), B = 256 candidates log-normal 0.2 around the fixture's two, K = 16 columns (two per
parameter kind), rtol = 1e-7 / atol = 1e-9, outputs ``F`` and ``dF`` only.
  (a) the LDS scoring launch: KC = 3, six chunks per candidate;
  (b) the slab route (``kernel="hbm"``) at chunk widths W = 4, 8, 16 (the dev knob PK_NET_SENS_KC lowers the default 16).
One warm-up per shape, then three alternating repetitions; a host clock around work that ends in a device synchronise.  Also one launch
of the union of 2 copies (N = 200, S = 1 104: the slab route by default) on the full output grid.

    python tools/gpu_net_sens_hbm_time.py [--B 256] [--reps 3]"""
import argparse
import os
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
from phoskintime_amd.global_model import NetworkEngine, synthetic      # noqa: E402

KINDS = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
OPT = dict(rtol=1e-7, atol=1e-9)


def _row(g, k):
    return np.concatenate([np.ravel(g[n][k]) for n in KINDS[:-1]] + [[float(g["tf_scale"][k])]])


def _timed(eng, loss, X, t, cols, y0, kernel, kc):
    if kc is None:
        os.environ.pop("PK_NET_SENS_KC", None)
    else:
        os.environ["PK_NET_SENS_KC"] = str(kc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.simulate_objective_grad_batch(loss, X, t, cols, y0=y0, lambdas=og.LAM, want_sums=False, kernel=kernel, **OPT)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    os.environ.pop("PK_NET_SENS_KC", None)
    assert out is not None
    return dt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    g = np.load(ref.GOLDEN / "netlarge_m0.npz")
    net = nm.Network.from_npz(g)
    eng = NetworkEngine.from_npz(g)
    t = g["t_eval"]
    rng = np.random.default_rng(0)
    X = np.stack([_row(g, k % 2) for k in range(a.B)]) * np.exp(0.2 * rng.standard_normal((a.B, eng.n_var)))
    sl = ref.slices(net)
    cols = np.array([sl[k][0] + j for k in KINDS[:-1] for j in (0, min(1, sl[k][1] - sl[k][0] - 1))] + [sl["tf_scale"][0]], dtype=np.int32)
    cols = np.concatenate([cols, [sl["A_i"][0] + 50]]).astype(np.int32)[:16]
    assert np.unique(cols).size == 16
    loss = eng.make_loss(og.loss_data(net, t), t.size)
    assert eng.objective_grad_columns_per_launch() == 3
    shapes = [("lds  KC=3 (6 chunks)", "auto", None, 0)] + [(f"slab W={w}", "hbm", w, w) for w in (4, 8, 16)]
    for name, kernel, kc, _ in shapes:                                             # one warm-up per shape
        _timed(eng, loss, X, t, cols, g["y0"], kernel, kc)
    times = {name: [] for name, *_ in shapes}
    steps, ref_dF = {}, None
    for _ in range(a.reps):                                                        # alternating repetitions
        for name, kernel, kc, _ in shapes:
            dt, out = _timed(eng, loss, X, t, cols, g["y0"], kernel, kc)
            times[name].append(dt)
            steps[name] = float(out["n_steps"][:, 0].double().mean())
            assert not out["status"].any()
            dF = out["dF"].cpu().numpy()
            if ref_dF is None:
                ref_dF = dF
            steps[name + " dF"] = float(np.abs(dF - ref_dF).max() / np.abs(ref_dF).max())
    for name, kernel, kc, w in shapes:
        os.environ["PK_NET_SENS_KC"] = str(w) if w else "3"
        byt = eng.sens_workspace_bytes(a.B, 16, True) if w else 0
        os.environ.pop("PK_NET_SENS_KC", None)
        print(f"{name:22s} wall s " + " / ".join(f"{v:.3f}" for v in times[name]) + f"   accepted steps (chunk 0, mean) {steps[name]:.0f}"
              f"   slab bytes {byt}   max |dF - dF(lds)| / max|dF| {steps[name + ' dF']:.2e}", flush=True)
    eng.free_loss(loss)
    # the 2-copy union on its full grid: beyond the LDS kernels, the slab route by default
    d = dict(g)
    eu = NetworkEngine.from_npz(synthetic.tile_network(d, 2))
    Xu = synthetic.tile_candidate(X[:min(a.B, 256)], 2, d)
    ld1 = og.loss_data(net, t)
    ldu = {k: (np.concatenate([v, v + net.N]) if k in ("p_prot", "p_rna", "p_pho") else np.concatenate([v, v]) if isinstance(v, np.ndarray) else v)
           for k, v in ld1.items()}
    lossu = eu.make_loss(ldu, t.size)
    slu = ref.slices(type("U", (), dict(n_K=2 * net.n_K, N=2 * net.N, total_sites=2 * net.total_sites)))
    cu = np.array([slu[k][0] + j for k in KINDS[:-1] for j in (0, 1)] + [slu["tf_scale"][0], slu["A_i"][0] + 150], dtype=np.int32)
    y0u = np.tile(g["y0"], 2)
    assert eu.objective_grad_columns_per_launch() == 0
    _timed(eu, lossu, Xu, t, cu, y0u, "auto", None)
    dt, out = _timed(eu, lossu, Xu, t, cu, y0u, "auto", None)
    print(f"union x2 (N={eu.N}, S={eu.S}), B={Xu.shape[0]}, K=16, default route: wall s {dt:.3f}   accepted steps (mean) "
          f"{float(out['n_steps'][:, 0].double().mean()):.0f}   flagged {int((out['status'] != 0).sum())}   slab bytes {eu.sens_workspace_bytes(Xu.shape[0], 16, True)}",
          flush=True)


if __name__ == "__main__":
    main()
