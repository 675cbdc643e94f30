#!/usr/bin/env python3
"""Golden vectors for NetworkEngine.desc_from_system, made by RUNNING THE REFERENCE (needs a checkout of it; the tests only read the result).

    python tools/make_golden_from_system.py distributive|combinatorial
or  python tools/make_golden_from_system.py all     (spawns both: the reference fixes MODEL at import time)

Builds the seeded 8-protein network of tools/make_golden_pins.py main_network through the reference's own Index / KinaseInput /
build_W_parallel / build_tf_matrix / System, and writes every attribute desc_from_system reads from that System -- the protein
count, the index maps (kinase order, protein -> row, kinase -> column, orphan -> proxy), the offsets and the CSR / kinase arrays --
with the dtypes the reference holds them in, to tests/golden/from_system_m<MODEL>.npz.  Only numbers and names are written."""
import subprocess, sys, pathlib
import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"


def _map(d):
    keys = list(d.keys())
    return np.array(keys, dtype=str) if keys else np.zeros(0, dtype="<U1"), np.array([d[k] for k in keys])


def main(model_name):
    import pandas as pd
    sys.path.insert(0, str(REPO / "tools"))
    import make_golden_network as mg
    mods, tmp = mg.import_reference(model_name)
    cfg, net, bm = mods["config"], mods["network"], mods["buildmat"]
    rng = np.random.default_rng(31 + 100 * cfg.MODEL)                      # the network of tools/make_golden_pins.py main_network
    prots, kinases, inter, tf_net = mg.synth_frames(rng, 8, 3, 2, 2, 10)
    idx = net.Index(inter, tf_interactions=tf_net, kin_beta_map={k: float(rng.uniform(0.5, 1.5)) for k in kinases}, tf_beta_map={})
    grid = np.asarray(cfg.TIME_POINTS_PROTEIN, float)
    rows = []
    for k in idx.kinases:
        base = 1.0 + 0.5 * np.sin(rng.uniform(0, 6) + np.arange(grid.size) * rng.uniform(0.2, 0.8))
        for t, v in zip(grid, base):
            rows.append(dict(protein=k, time=float(t), fc=float(max(v, 1e-6))))
    kin_in = net.KinaseInput(idx.kinases, pd.DataFrame(rows))
    W = bm.build_W_parallel(inter, idx, n_cores=1)
    tf_mat = bm.build_tf_matrix(tf_net, idx, tf_beta_map={}, kin_beta_map={})
    tf_deg = np.asarray(np.abs(tf_mat).sum(axis=1)).ravel().astype(np.float64); tf_deg[tf_deg < 1e-12] = 1.0
    d = dict(c_k=np.ones(len(idx.kinases)), A_i=np.ones(idx.N), B_i=np.full(idx.N, 0.2), C_i=np.full(idx.N, 0.5), D_i=np.full(idx.N, 0.05),
             Dp_i=np.full(idx.total_sites, 0.05), E_i=np.ones(idx.N), tf_scale=0.1)
    sysm = net.System(idx, W, tf_mat, kin_in, d, tf_deg)
    p2i_k, p2i_v = _map(idx.p2i)
    k2i_k, k2i_v = _map(idx.k2i)
    px_k, px_v = _map(getattr(idx, "proxy_map", {}))
    out = dict(model=cfg.MODEL, N=idx.N, kinases=np.array(list(idx.kinases), dtype=str), p2i_keys=p2i_k, p2i_values=p2i_v, k2i_keys=k2i_k,
               k2i_values=k2i_v, has_proxy_map=hasattr(idx, "proxy_map"), proxy_keys=px_k, proxy_values=np.array(px_v, dtype=str),
               offset_y=np.asarray(idx.offset_y), offset_s=np.asarray(idx.offset_s), n_sites=np.asarray(idx.n_sites))
    for k in ("W_indptr", "W_indices", "W_data", "TF_indptr", "TF_indices", "TF_data", "tf_deg", "kin_grid", "kin_Kmat"):
        out[k] = np.asarray(getattr(sysm, k))
    np.savez_compressed(OUT / f"from_system_m{cfg.MODEL}.npz", **out)
    print("wrote from_system for", model_name, flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which == "all":
        procs = [subprocess.Popen([sys.executable, __file__, m]) for m in ("distributive", "combinatorial")]
        sys.exit(max(p.wait() for p in procs))
    main(which)
