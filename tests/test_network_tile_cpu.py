"""CPU: ``synthetic.tile_network`` / ``tile_candidate`` build the disjoint union of K copies of a network.  The union is a valid
description, and the oracle's right-hand side on it equals, copy by copy and bit for bit, the rhs the reference produced for the single
network (golden ``netlarge_m*``) -- so every copy of a union has reference-run truth at sizes beyond one workgroup's LDS."""
from pathlib import Path

import numpy as np
import pytest

from oracle import network_models as nm
from phoskintime_amd.global_model import synthetic

GOLDEN = Path(__file__).resolve().parent / "golden"
LARGE = sorted(GOLDEN.glob("netlarge_m[0-9].npz"))


def _row(g, k):
    return np.concatenate([np.ravel(g[n][k]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][k])]])


def _params(net, x):
    cuts = np.cumsum([net.n_K, net.N, net.N, net.N, net.N, net.total_sites, net.N])
    return nm.Params(*np.split(x[:-1], cuts[:-1]), float(x[-1]))


@pytest.mark.parametrize("model", [0, 1, 2, 4])
def test_tiled_description_is_valid(model):
    net = synthetic.make_network(N=40, total_sites=90, n_K=12, n_tf_edges=80, model=model, seed=5)
    K = 3
    u = synthetic.tile_network(net, K)
    N, nK = net["offset_y"].size, net["kin_Kmat"].shape[0]
    ns = u["n_sites"]
    blk = (1 + (1 << ns.astype(np.int64))) if model == 2 else 2 + ns
    assert ns.size == K * N and u["kin_Kmat"].shape == (K * nK, net["kin_grid"].size)
    np.testing.assert_array_equal(u["offset_y"], np.concatenate([[0], np.cumsum(blk)[:-1]]))
    np.testing.assert_array_equal(u["offset_s"], np.concatenate([[0], np.cumsum(ns)[:-1]]))
    for p, idx, n_rows, hi in (("W_indptr", "W_indices", int(ns.sum()), K * nK), ("TF_indptr", "TF_indices", K * N, K * N)):
        ptr = u[p]
        assert ptr.size == n_rows + 1 and ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] == u[idx].size
        assert u[idx].min() >= 0 and u[idx].max() < hi
    d = u["driver_map"]
    assert ((d == -1) | ((d >= 0) & (d < K * nK))).all() and (d >= 0).sum() == K * (net["driver_map"] >= 0).sum()
    # copy c's kinase / TF indices are copy 0's moved by c n_K / c N
    nnzT = int(net["TF_indptr"][-1])
    np.testing.assert_array_equal(u["TF_indices"][2 * nnzT:3 * nnzT], net["TF_indices"] + 2 * N)
    x = synthetic.default_candidate(net)
    xu = synthetic.tile_candidate(x, K, net)
    assert xu.size == K * (x.size - 1) + 1 and xu[-1] == x[-1]
    np.testing.assert_array_equal(synthetic.tile_candidate(np.stack([x, 2 * x]), K, net)[1], 2 * xu)
    with pytest.raises(ValueError):
        synthetic.union_candidate(np.stack([x, 2 * x]), net)          # one global tf_scale
    with pytest.raises(ValueError):
        synthetic.tile_network(net, 0)


@pytest.mark.parametrize("f", LARGE, ids=lambda f: f.stem)
def test_union_rhs_equals_the_reference_rhs_per_copy(f):
    g = np.load(f)
    K = 6
    u = synthetic.tile_network(dict(g), K)
    net = nm.Network.from_npz(u)
    assert net.N == K * int(g["N"]) and net.S == K * int(g["S"]) and net.S > 1024
    for k in range(g["y_rand"].shape[0]):
        p = _params(net, synthetic.tile_candidate(_row(g, k), K, dict(g)))
        y = np.tile(g["y_rand"][k], K)
        for ti, t in enumerate(g["t_probe"]):
            np.testing.assert_array_equal(nm.rhs(net, p, y, float(t)), np.tile(g["rhs_rand"][k, ti], K))
