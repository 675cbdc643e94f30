"""Seeded synthetic networks of the shape SURVEY.md section 8d prescribes for BASELINE configs 4 / 5 (the reference ships no data):
N proteins, 1-6 sites each, n_K kinases of which half are also proteins (driven), ~1.5 kinases per site with alpha ~ U(0.2, 1),
a signed sparse TF net, K(t) = 1 + 0.3 * smooth noise clipped at 1e-6, defaults as global_model/runner.py:515-524."""
from __future__ import annotations

import numpy as np


def make_network(N: int = 100, total_sites: int = 300, n_K: int = 40, n_tf_edges: int = 250, model: int = 0, seed: int = 20260519, max_sites: int | None = None):
    rng = np.random.default_rng(seed)
    # sites per protein: >= 0, sum = total_sites, <= 6 (model 2: <= 3)
    cap = max_sites if max_sites is not None else (3 if model == 2 else 6)
    n_sites = np.zeros(N, dtype=np.int32)
    while n_sites.sum() < total_sites:
        i = int(rng.integers(0, N))
        if n_sites[i] < cap:
            n_sites[i] += 1
    offset_s = np.concatenate([[0], np.cumsum(n_sites)[:-1]]).astype(np.int32)
    blk = (1 + (1 << n_sites.astype(np.int64))) if model == 2 else (2 + n_sites)
    offset_y = np.concatenate([[0], np.cumsum(blk)[:-1]]).astype(np.int32)
    # W: each site is hit by 1-2 kinases
    indptr = [0]; indices = []; data = []
    for _ in range(int(n_sites.sum())):
        ks = rng.choice(n_K, size=int(rng.integers(1, 3)), replace=False)
        for k in sorted(ks):
            indices.append(int(k)); data.append(float(rng.uniform(0.2, 1.0)))
        indptr.append(len(indices))
    # TF net (rows = targets), no self loops
    rows = [[] for _ in range(N)]
    edges = set()
    while len(edges) < n_tf_edges:
        a, b = (int(v) for v in rng.choice(N, size=2, replace=False))
        if (a, b) not in edges:
            edges.add((a, b)); rows[b].append((a, float(rng.uniform(-1, 1))))
    tptr = [0]; tind = []; tdat = []
    for r in rows:
        for a, w in sorted(r):
            tind.append(a); tdat.append(w)
        tptr.append(len(tind))
    tf_deg = np.array([sum(abs(w) for _, w in r) for r in rows]); tf_deg[tf_deg < 1e-12] = 1.0
    driver = np.full(N, -1, dtype=np.int32)
    kin_prot = rng.choice(N, size=n_K // 2, replace=False)
    driver[kin_prot] = np.arange(n_K // 2, dtype=np.int32)
    grid = np.array([0.0, 0.5, 0.75, 1.0, 2.0, 4.0, 8.0, 16.0, 30.0, 60.0, 120.0, 240.0, 480.0, 960.0])
    smooth = np.cumsum(rng.standard_normal((n_K, grid.size)), axis=1) / np.sqrt(np.arange(1, grid.size + 1))
    Kmat = np.maximum(1.0 + 0.3 * smooth, 1e-6)
    return dict(model=model, offset_y=offset_y, offset_s=offset_s, n_sites=n_sites,
                W_indptr=np.array(indptr, np.int32), W_indices=np.array(indices, np.int32), W_data=np.array(data),
                TF_indptr=np.array(tptr, np.int32), TF_indices=np.array(tind, np.int32), TF_data=np.array(tdat),
                tf_deg=tf_deg, driver_map=driver, kin_grid=grid, kin_Kmat=Kmat)


def default_candidate(net: dict) -> np.ndarray:
    """Physical defaults of runner.py:515-524 as one candidate row."""
    N = net["offset_y"].size; nK = net["kin_Kmat"].shape[0]; sites = int(net["n_sites"].sum())
    return np.concatenate([np.ones(nK), np.ones(N), np.full(N, 0.2), np.full(N, 0.5), np.full(N, 0.05), np.full(sites, 0.05), np.ones(N), [0.1]])


def random_candidates(net: dict, B: int, seed: int = 0, spread: float = 0.5) -> np.ndarray:
    """B physical candidates: defaults times log-normal factors (sigma = spread)."""
    rng = np.random.default_rng(seed)
    base = default_candidate(net)
    return base[None, :] * np.exp(spread * rng.standard_normal((B, base.size)))


_SCALARS = ("N", "n_K", "total_sites", "S", "n_W_rows")


def tile_network(desc: dict, K: int) -> dict:
    """The disjoint union of K copies of a network description (``make_network`` output or a golden file's topology): copy c's states,
    sites, proteins and kinases follow those of copies 0 .. c-1.  Kinase indices (``W_indices``, ``driver_map`` where >= 0) move by
    c n_K, TF indices by c N, ``kin_Kmat`` is stacked and ``kin_grid`` shared, so copy c integrates exactly like the single network.
    Scalar sizes present in ``desc`` (N, n_K, total_sites, S, n_W_rows) are scaled; ``n_states`` (combinatorial fixtures) is tiled."""
    K = int(K)
    if K < 1:
        raise ValueError("K must be >= 1")
    oy, os_, ns = (np.asarray(desc[k]) for k in ("offset_y", "offset_s", "n_sites"))
    N = oy.size
    n_K = np.asarray(desc["kin_Kmat"]).shape[0]
    model = int(desc["model"])
    blk = (1 + (1 << ns.astype(np.int64))) if model == 2 else (2 + ns.astype(np.int64))
    S, sites = int(blk.sum()), int(ns.sum())
    wp, tp = np.asarray(desc["W_indptr"]), np.asarray(desc["TF_indptr"])
    nnzW, nnzT = int(wp[-1]), int(tp[-1])
    drv = np.asarray(desc["driver_map"])
    cs = range(K)
    out = {k: v for k, v in desc.items() if k in _SCALARS or k in ("model", "kin_grid")}
    out.update(
        offset_y=np.concatenate([oy + c * S for c in cs]).astype(np.int32),
        offset_s=np.concatenate([os_ + c * sites for c in cs]).astype(np.int32),
        n_sites=np.tile(ns, K).astype(np.int32),
        W_indptr=np.concatenate([wp[:1]] + [wp[1:] + c * nnzW for c in cs]).astype(np.int32),
        W_indices=np.concatenate([np.asarray(desc["W_indices"])[:nnzW] + c * n_K for c in cs]).astype(np.int32),
        W_data=np.tile(np.asarray(desc["W_data"], dtype=np.float64)[:nnzW], K),
        TF_indptr=np.concatenate([tp[:1]] + [tp[1:] + c * nnzT for c in cs]).astype(np.int32),
        TF_indices=np.concatenate([np.asarray(desc["TF_indices"])[:nnzT] + c * N for c in cs]).astype(np.int32),
        TF_data=np.tile(np.asarray(desc["TF_data"], dtype=np.float64)[:nnzT], K),
        tf_deg=np.tile(np.asarray(desc["tf_deg"], dtype=np.float64), K),
        driver_map=np.concatenate([np.where(drv >= 0, drv + c * n_K, drv) for c in cs]).astype(np.int32),
        kin_grid=np.asarray(desc["kin_grid"], dtype=np.float64),
        kin_Kmat=np.concatenate([np.asarray(desc["kin_Kmat"], dtype=np.float64)] * K, axis=0),
    )
    for k in _SCALARS:
        if k in desc:
            out[k] = np.asarray(int(np.asarray(desc[k])) * K)
    if "n_states" in desc:
        out["n_states"] = np.tile(np.asarray(desc["n_states"]), K)
    return out


def _blocks(x: np.ndarray, n_K: int, N: int, sites: int):
    """[c_k | A | B | C | D | Dp | E] blocks and tf_scale of candidate rows x [..., n_var]."""
    cuts = np.cumsum([n_K, N, N, N, N, sites, N])
    return np.split(x[..., :-1], cuts[:-1], axis=-1), x[..., -1]


def _dims(desc: dict):
    return np.asarray(desc["kin_Kmat"]).shape[0], np.asarray(desc["offset_y"]).size, int(np.asarray(desc["n_sites"]).sum())


def union_candidate(rows, desc: dict) -> np.ndarray:
    """One candidate of the K-copy union of network ``desc`` from K candidates of the single network (rows [K, n_var], or
    [B, K, n_var] -> [B, n_var of the union]): each parameter block is concatenated copy by copy; the union has ONE tf_scale, so every
    row must carry the same one."""
    n_K, N, sites = _dims(desc)
    rows = np.asarray(rows, dtype=np.float64)
    if rows.shape[-1] != n_K + 5 * N + sites + 1:
        raise ValueError("rows must be [..., K, n_var] of the single network")
    parts, ts = _blocks(rows, n_K, N, sites)
    if not np.all(ts == ts[..., :1]):
        raise ValueError("the copies of a union share one tf_scale")
    flat = lambda a: a.reshape(a.shape[:-2] + (-1,))
    return np.concatenate([flat(p) for p in parts] + [ts[..., :1]], axis=-1)


def tile_candidate(x, K: int, desc: dict) -> np.ndarray:
    """Candidate(s) x ([n_var] or [B, n_var]) of network ``desc`` -> the same candidate(s) on ``tile_network(desc, K)``: every copy
    gets x's parameters, the one global tf_scale is kept."""
    x = np.asarray(x, dtype=np.float64)
    return union_candidate(np.repeat(x[..., None, :], int(K), axis=-2), desc)
