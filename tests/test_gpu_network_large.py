"""GPU: networks beyond one workgroup's LDS (S > 1024, N > 512) on the HBM-workspace ROS34PW2-W kernel (net_solve_ws_kernel, csrc/pk_network_solve.hpp).
Truth comes from the reference: the union of 6 copies of a ``netlarge_m*`` fixture (``synthetic.tile_network``) integrates copy by
copy like the fixture's network, whose LSODA run at 1e-12 (``Y_tight``) the reference produced."""
from pathlib import Path

import numpy as np
import pytest

from oracle import network_models as nm

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
K = 6
LARGE = {m: GOLDEN / f"netlarge_m{m}.npz" for m in (0, 1, 2, 4)}


def band(a, b):
    return float(np.max(np.abs(a - b) / (1e-8 + 1e-6 * np.abs(b))))


def _row(g, k):
    return np.concatenate([np.ravel(g[n][k]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][k])]])


def _union(m):
    from phoskintime_amd.global_model import NetworkEngine, synthetic
    g = np.load(LARGE[m])
    d = dict(g)
    u = synthetic.tile_network(d, K)
    return g, d, u, NetworkEngine.from_npz(g), NetworkEngine.from_npz(u)


def _copies(Y, S):
    """[..., K S] -> [K, ..., S]"""
    return np.moveaxis(Y.reshape(Y.shape[:-1] + (K, S)), -2, 0)


@pytest.mark.parametrize("m", [0, 1, 2, 4])
def test_union_rhs_and_block_diagonal_jacobian(m):
    from phoskintime_amd.global_model import synthetic
    g, d, u, e1, eu = _union(m)
    S = e1.S
    assert eu.S == K * S and eu.N == K * e1.N and eu.S > 1024
    X1 = np.stack([_row(g, k) for k in range(2)])
    Xu = synthetic.tile_candidate(X1, K, d)
    yu = np.tile(g["y_rand"], (1, K))
    for ti, t in enumerate(g["t_probe"]):
        du = _copies(eu.rhs_batch(Xu, yu, float(t)).cpu().numpy(), S)
        scale = 1.0 + np.abs(g["rhs_rand"][:, ti]).max()
        for c in range(K):
            np.testing.assert_allclose(du[c], g["rhs_rand"][:, ti], rtol=1e-12, atol=1e-13 * scale)
    J1 = e1.jacobian_batch(X1[:1], g["y_rand"][0], 3.0).cpu().numpy()[0]
    Ju = eu.jacobian_batch(Xu[:1], yu[0], 3.0).cpu().numpy()[0]
    tol = 1e-14 * (1.0 + np.abs(J1).max())
    for a in range(K):
        for b in range(K):
            blk = Ju[a * S:(a + 1) * S, b * S:(b + 1) * S]
            if a == b:
                np.testing.assert_allclose(blk, J1, rtol=1e-14, atol=tol)
            else:
                assert not blk.any()
    e1.close(); eu.close()


@pytest.mark.parametrize("m", [0, 1, 2, 4])
def test_union_simulate_against_the_reference_run(m):
    from phoskintime_amd.global_model import synthetic
    g, d, u, e1, eu = _union(m)
    S = e1.S
    x1 = _row(g, 0)[None, :]
    xu = synthetic.tile_candidate(x1, K, d)
    assert eu.resolved_method() == "rosw"
    for norm in ("max", "rms"):
        opt = dict(rtol=1e-8, atol=1e-8, err_norm=norm)
        Yu, su, nu = eu.simulate_batch(xu, g["t_eval"], y0=np.tile(g["y0"], K), **opt)
        Y1, s1, n1 = e1.simulate_batch(x1, g["t_eval"], method="rosw", kernel="lds", **opt)
        assert not su.cpu().numpy().any() and not s1.cpu().numpy().any()
        Yc = _copies(Yu.cpu().numpy()[0], S)
        nu, n1 = nu.cpu().numpy()[0], n1.cpu().numpy()[0]
        assert abs(int(nu[0]) - int(n1[0])) <= 1 and abs(int(nu[1]) - int(n1[1])) <= 1, (nu, n1)
        for c in range(K):
            if norm == "max":
                assert band(Yc[c], g["Y_tight"][0]) <= 0.1
            assert band(Yc[c], Y1.cpu().numpy()[0]) <= 0.01
    e1.close(); eu.close()


@pytest.mark.parametrize("m", [0, 1, 2, 4])
def test_union_of_distinct_copies(m):
    """Different parameters per copy break the symmetry a wrong offset would hide: copy c must integrate like the single network with
    copy c's parameters (one shared tf_scale)."""
    from phoskintime_amd.global_model import synthetic
    g, d, u, e1, eu = _union(m)
    rng = np.random.default_rng(100 + m)
    base = _row(g, 0)
    rows = base[None, :] * np.exp(0.2 * rng.standard_normal((K, base.size)))
    rows[:, -1] = base[-1]
    xu = synthetic.union_candidate(rows, d)[None, :]
    opt = dict(rtol=1e-10, atol=1e-10, method="rosw")
    Yu, su, _ = eu.simulate_batch(xu, g["t_eval"], **opt)
    Y1, s1, _ = e1.simulate_batch(rows, g["t_eval"], kernel="lds", **opt)
    assert not su.cpu().numpy().any() and not s1.cpu().numpy().any()
    Yc = _copies(Yu.cpu().numpy()[0], e1.S)
    Y1 = Y1.cpu().numpy()
    for c in range(K):
        assert band(Yc[c], Y1[c]) <= 0.05, (c, band(Yc[c], Y1[c]))
    e1.close(); eu.close()


def _agree(eng, X, t, raw=False, y0=None, **kw):
    Yw, sw, nw = eng.simulate_batch(X, t, raw=raw, y0=y0, kernel="workspace", **kw)
    Yl, sl, nl = eng.simulate_batch(X, t, raw=raw, y0=y0, kernel="lds", method="rosw", **kw)
    Yw, Yl = Yw.cpu().numpy(), Yl.cpu().numpy()
    np.testing.assert_array_equal(sw.cpu().numpy(), sl.cpu().numpy())
    assert (np.abs(nw.cpu().numpy().astype(int) - nl.cpu().numpy().astype(int)) <= 1).all()
    np.testing.assert_array_equal(np.isnan(Yw), np.isnan(Yl))
    ok = np.isfinite(Yl)
    if ok.any():
        assert band(Yw[ok], Yl[ok]) <= 0.01
    return Yw, sw.cpu().numpy(), nw.cpu().numpy()


@pytest.mark.parametrize("f", sorted(GOLDEN.glob("network_m*.npz")) + sorted(GOLDEN.glob("netlarge_m[0-9].npz")), ids=lambda f: f.stem)
def test_workspace_kernel_agrees_with_the_lds_kernel(f):
    from phoskintime_amd.global_model import NetworkEngine
    g = np.load(f)
    eng = NetworkEngine.from_npz(g)
    nc = g["c_k"].shape[0]
    X = np.stack([_row(g, k % nc) for k in range(3)])
    X[2] *= 1.1
    assert eng.resolved_method(kernel="workspace") == "rosw"
    Y, st, _ = _agree(eng, X, g["t_eval"])
    assert not st.any()
    # raw decision vectors, batched y0
    Xr = np.log(np.expm1(X))
    y0 = np.abs(np.stack([g["y0"]] * 3)) * np.linspace(0.9, 1.1, 3)[:, None]
    _agree(eng, Xr, g["t_eval"], raw=True, y0=y0)
    eng.close()


def test_workspace_kernel_edge_shapes_and_failures():
    from phoskintime_amd.global_model import NetworkEngine, synthetic
    from phoskintime_amd._capi import PhoskinError
    net = synthetic.make_network(N=300, total_sites=400, n_K=60, n_tf_edges=700, model=0, seed=77)
    eng = NetworkEngine(**net)
    assert eng.S == 1000
    X = synthetic.random_candidates(net, 8, seed=2)
    t = np.unique(np.concatenate([net["kin_grid"], [15.0]]))
    Y, st, ns = _agree(eng, X, t)
    assert not st.any()
    # T = 1: the initial state, no step
    Y1, s1, n1 = _agree(eng, X[:2], np.array([0.0]))
    np.testing.assert_array_equal(Y1[:, 0], np.broadcast_to(eng.default_y0(), (2, eng.S)))
    assert not n1.any()
    # B = 0 and B = 1
    Y0, s0, _ = eng.simulate_batch(X[:0], t, kernel="workspace")
    assert tuple(Y0.shape) == (0, t.size, eng.S)
    Yb, _, _ = _agree(eng, X[3:4], t)
    np.testing.assert_array_equal(Yb[0], Y[3])                       # independent of the batch around it
    # more than 64 landing points: the buffered stop list
    dense = np.unique(np.concatenate([np.logspace(-3, np.log10(960.0), 100), t]))
    dense = np.concatenate([[0.0], dense[dense > 0]])
    Yd, sd, _ = _agree(eng, X[:2], dense)
    idx = [int(np.where(dense == v)[0][0]) for v in t]
    assert band(Yd[:, idx], Y[:2]) <= 0.3
    # a candidate that exhausts max_steps: flagged, NaN rows from there on, neighbours untouched
    tot = ns.sum(axis=1)
    lim = int((tot.min() + tot.max()) // 2)
    assert tot.min() < lim < tot.max()
    Ym, sm, _ = _agree(eng, X, t, max_steps=lim)
    hit = tot > lim
    assert ((sm != 0) == hit).all() and hit.any()
    np.testing.assert_array_equal(Ym[~hit], Y[~hit])
    for b in np.where(hit)[0]:
        assert np.isnan(Ym[b, -1]).all() and np.isfinite(Ym[b, 0]).all()
    with pytest.raises(PhoskinError):
        eng.simulate_batch(X[:1], t, kernel="workspace", method="ark")
    with pytest.raises(PhoskinError):
        eng.simulate_batch(X[:1], t, kernel="workspace", method="dp5")
    eng.close()


@pytest.mark.parametrize("model", [0, 1])
def test_ten_thousand_state_network(model):
    import torch
    from phoskintime_amd.global_model import NetworkEngine, synthetic
    net = synthetic.make_network(N=2000, total_sites=6000, n_K=200, n_tf_edges=5000, model=model, seed=11)
    eng = NetworkEngine(**net)
    assert eng.S == 10000
    on = nm.Network.from_npz({k: np.asarray(v) for k, v in dict(net, N=eng.N, n_K=eng.n_K, total_sites=eng.total_sites, S=eng.S).items()})
    X = synthetic.random_candidates(net, 2, seed=4, spread=0.3)
    rng = np.random.default_rng(1)
    y = np.abs(eng.default_y0() * np.exp(0.3 * rng.standard_normal(eng.S)))
    cuts = np.cumsum([eng.n_K, eng.N, eng.N, eng.N, eng.N, eng.total_sites, eng.N])
    for t in (0.3, 16.0):
        d = eng.rhs_batch(X, y, t).cpu().numpy()
        for k in range(2):
            want = nm.rhs(on, nm.Params(*np.split(X[k, :-1], cuts[:-1]), float(X[k, -1])), y, t)
            np.testing.assert_allclose(d[k], want, rtol=1e-12, atol=1e-13 * (1.0 + np.abs(want).max()))
    J = eng.jacobian_batch(X[:1], y, 3.0)
    cols = np.linspace(0, eng.S - 1, 32).astype(int)
    Jc = J[0][:, torch.as_tensor(cols, device=J.device)].cpu().numpy()
    del J
    h = 1e-5
    Yp = np.repeat(y[None, :], 64, axis=0)
    Yp[np.arange(32), cols] += h
    Yp[32 + np.arange(32), cols] -= h
    f = eng.rhs_batch(np.repeat(X[:1], 64, axis=0), Yp, 3.0).cpu().numpy()
    cd = ((f[:32] - f[32:]) / (2 * h)).T
    np.testing.assert_allclose(Jc, cd, rtol=2e-7, atol=2e-8)
    P = synthetic.random_candidates(net, 64, seed=5, spread=0.3)
    t = np.unique(np.concatenate([net["kin_grid"], [15.0]]))
    Ya, sa, _ = eng.simulate_batch(P, t, rtol=1e-8, atol=1e-8)
    Yt, stt, _ = eng.simulate_batch(P, t, rtol=1e-11, atol=1e-11)
    assert not sa.cpu().numpy().any() and not stt.cpu().numpy().any()
    assert band(Ya.cpu().numpy(), Yt.cpu().numpy()) <= 0.2
    eng.close()


def _system(u, x, y0):
    """A stand-in with the attribute surface of the reference's System / Index for a union description (every driven protein is its
    kinase's own protein or a proxied orphan, as network.py:454-469 builds them)."""
    from types import SimpleNamespace
    N, nK = u["offset_y"].size, u["kin_Kmat"].shape[0]
    prots = [f"P{i:04d}" for i in range(N)]
    drv = u["driver_map"]
    used = {}
    for i in range(N):
        if drv[i] >= 0 and int(drv[i]) not in used:
            used[int(drv[i])] = prots[i]
    kinases = [used.get(j, f"K{j:03d}") for j in range(nK)]
    proxy = {prots[i]: used[int(drv[i])] for i in range(N) if drv[i] >= 0 and used[int(drv[i])] != prots[i]}
    idx = SimpleNamespace(N=N, proteins=prots, kinases=kinases, p2i={p: i for i, p in enumerate(prots)}, k2i={k: j for j, k in enumerate(kinases)},
                          proxy_map=proxy, sites=[[f"S{j}" for j in range(int(n))] for n in u["n_sites"]], offset_y=u["offset_y"],
                          offset_s=u["offset_s"], n_sites=u["n_sites"])
    sites = int(u["n_sites"].sum())
    c_k, A, B, Cc, D, Dp, E = np.split(x[:-1], np.cumsum([nK, N, N, N, N, sites, N])[:-1])
    sysm = SimpleNamespace(idx=idx, W_indptr=u["W_indptr"], W_indices=u["W_indices"], W_data=u["W_data"], TF_indptr=u["TF_indptr"],
                           TF_indices=u["TF_indices"], TF_data=u["TF_data"], tf_deg=u["tf_deg"], kin_grid=u["kin_grid"], kin_Kmat=u["kin_Kmat"],
                           c_k=c_k, A_i=A, B_i=B, C_i=Cc, D_i=D, Dp_i=Dp, E_i=E, tf_scale=float(x[-1]), y0=lambda: y0.copy())
    return sysm, idx


def test_objectives_and_dropins_on_the_union_network():
    import torch
    from phoskintime_amd.global_model import synthetic
    from phoskintime_amd.global_model import simulate as gsim
    from phoskintime_amd.global_model import config as gcfg
    m = 0
    g, d, u, e1, eu = _union(m)
    X = synthetic.tile_candidate(np.stack([_row(g, k) for k in range(2)]), K, d)
    t = g["t_eval"]
    Y, st, _ = eu.simulate_batch(X, t, rtol=1e-8, atol=1e-8)
    assert not st.cpu().numpy().any()
    lists, ld = eu.make_index_lists(t, [0.0, 1.0, 960.0], [4.0, 60.0], [0.0, 30.0])
    assert eu.simulate_objective_batch(lists, X, t) is None          # no fused path beyond one workgroup: simulate + objective_batch
    defaults = X[0] * 1.2
    lam = dict(protein=1.0, rna=0.5, phospho=2.0, prior=0.3)
    sums, F = eu.objective_batch(lists, Y, x=X, defaults=defaults, lambdas=(1.0, 0.5, 2.0, 0.3))
    F = F.cpu().numpy()
    on = nm.Network.from_npz(u)
    ns = u["n_sites"]
    ldo = dict(ld, prot_map=np.stack([u["offset_y"], (1 << ns) if m == 2 else ns], axis=1))
    Yn = Y.cpu().numpy()
    for k in range(2):
        np.testing.assert_allclose(F[k], nm.objectives(on, X[k], defaults, Yn[k], ldo, 0, lam), rtol=1e-12)
    eu.free_loss(lists)
    # the drop-in simulate_odeint on a System-like object of the union
    gcfg.MODEL = m
    y0 = np.tile(g["y0"], K)
    sysm, _ = _system(u, X[1], y0)
    Yd = gsim.simulate_odeint(sysm, t, 1e-8, 1e-8, 200000)
    np.testing.assert_array_equal(gsim.engine_for(sysm)._keep[10], u["driver_map"])
    Ye, _, _ = eu.simulate_batch(X[1:2], t, y0=y0, rtol=1e-8, atol=1e-8, max_steps=200000 * t.size)
    np.testing.assert_array_equal(Yd, Ye.cpu().numpy()[0])
    e1.close(); eu.close()


_WS_SCRIPT = r"""
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1])
from phoskintime_amd.global_model import NetworkEngine, synthetic
g = np.load(sys.argv[1] + "/tests/golden/netlarge_m0.npz")
d = dict(g)
eng = NetworkEngine.from_npz(synthetic.tile_network(d, 6))
x = np.concatenate([np.ravel(g[n][0]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][0])]])
t = g["t_eval"]
out = {"ws": [eng.workspace_bytes(B) for B in (1, 4096, 16384)], "S": eng.S}
for B in (4096, 16384):
    X = synthetic.tile_candidate(x[None, :] * np.exp(0.1 * np.random.default_rng(B).standard_normal((B, x.size))), 6, d)
    X[:, -1] = x[-1]
    Y, st, _ = eng.simulate_batch(X, t, rtol=1e-5, atol=1e-7)
    out[f"ok{B}"] = bool(np.isfinite(Y[:, -1].cpu().numpy()).all() and not st.cpu().numpy().any())
    out[f"stats{B}"] = eng.ctx.workspace_stats()
print(json.dumps(out))
"""


def test_workspace_is_bounded_in_the_batch():
    """A persistent grid of min(B, resident workgroups): the scratch arena after 4 096 candidates is the one after 16 384 (a fresh process,
    so the context's arena holds nothing else), and it is the grid x slab of pk_network_workspace_bytes plus the arena's growth slack."""
    import json, subprocess, sys
    root = str(Path(__file__).resolve().parents[1])
    r = subprocess.run([sys.executable, "-c", _WS_SCRIPT, root], check=True, capture_output=True, text=True, timeout=900)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    ws1, ws4, ws16 = out["ws"]
    assert ws1 % 128 == 0 and ws4 == ws16 and ws4 % ws1 == 0 and ws4 // ws1 < 4096       # grid = resident workgroups, below both batches
    assert out["ok4096"] and out["ok16384"]
    s4, s16 = out["stats4096"], out["stats16384"]
    assert s4["scratch_bytes"] == s16["scratch_bytes"] and s4["scratch_allocs"] == s16["scratch_allocs"] == 1
    assert s4["scratch_bytes"] == ws4 + ws4 // 2 + (64 << 10)
