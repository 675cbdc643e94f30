"""GPU: the network sensitivity launches on HBM slabs (``kernel="hbm"`` and, by itself, every network on which the LDS kernels carry no
column): ``net_solve_sens_ws_kernel`` / ``net_solve_sens_score_ws_kernel`` (csrc/pk_network_sens.hpp), a persistent grid over
(candidate, column chunk) work items.

Bands.  ``C_BAND = 269`` is tests/test_gpu_network_sens.py's: ten times the worst |dY - ref| / (atol + rtol max|ref column|) measured
there against the stored exact reference (26.89, a transient behind a TF sign change), ``self_err`` the reference's own
self-consistency.  The slab kernels run the LDS kernels' body statement for statement, so they are held to the same band against the same
reference; the trajectory is held to it against ``simulate_batch(kernel="workspace")``.  The scoring flavour's outputs are reproduced
from the launch's own ``Y`` / ``dY`` by tests/net_objgrad_reference.py within its rounding bound.

Agreement with the LDS launch at the same chunk width (one chunk of 8 on the small fixtures): the two differ in rounding only (FMA
contraction differs with the layout's addressing), which a step that straddles a TF sign change can amplify.  Measured on an MI355X
(gfx950), worst |dY_hbm - dY_lds| / (atol + rtol max|column|): 4.93e-06 (figures per candidate at AGREE below); the assertion is ten
times that.

Beyond LDS (test_union_*): the union of 2 copies of ``netlarge_m0`` (N = 200, S = 1 104; ``netlarge_m2``: S = 1 108) takes the slab
route by default -- only there do threads stride past the LDS layout's 4 states each (t <= 8: 489 / 358 accepted steps); truth is the
single network's LDS launch (KC = 3) at the same tolerances, band ``C_BAND (atol + rtol max|column|)`` -- the union's steps differ because
its error norm runs over both copies."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import net_objgrad_reference as og
import net_sens_reference as ref
from oracle import network_models as nm

pytestmark = pytest.mark.gpu
RTOL, ATOL = ref.RTOL_GPU, ref.ATOL_GPU
OPT = dict(rtol=RTOL, atol=ATOL)
C_BAND = 269.0          # tests/test_gpu_network_sens.py
# worst |dY_hbm - dY_lds| / (atol + rtol max|column|), one chunk of 8 columns, B = 3, measured on an MI355X (gfx950), per candidate:
#   network_m0_small  3.1e-07  4.9e-06  3.3e-07      network_m1_small  7.5e-07  3.5e-07  1.5e-06
#   network_m2_small  3.8e-07  3.1e-07  2.4e-07      network_m4_small  2.1e-07  2.7e-07  3.2e-07
# (not bit-equal; accepted and rejected step counts equal on every candidate).  worst 4.93e-06 -> AGREE = 10 x 4.93e-06
AGREE = 4.93e-5
LAM, LAMD = og.LAM, og.LAMD
KEYS = ("pred", "dpred", "loss_sums", "dsums", "F", "dF")
_CACHE = {}


def _np(a):
    return {k: v.cpu().numpy() for k, v in a.items()} if isinstance(a, dict) else a.cpu().numpy()


def _band(mx, rtol=RTOL, atol=ATOL):
    return atol + rtol * mx


def _setup(name):
    """Engine, fixture, stored reference, loss handle and the main slab launches (B = 3, the 8 stored columns) of a fixture, made once."""
    if name not in _CACHE:
        from phoskintime_amd.global_model import NetworkEngine
        s = dict(og.fixture_data(name))
        s["eng"] = eng = NetworkEngine.from_npz(s["g"])
        s["cols"] = s["gold"]["cols"].astype(np.int32)
        s["t"], s["y0"] = s["g"]["t_eval"], s["g"]["y0"]
        s["loss"] = eng.make_loss(s["ld"], s["t"].size)
        s["sens"] = tuple(_np(a) for a in eng.simulate_sens_batch(s["X"], s["t"], s["cols"], y0=s["y0"], kernel="hbm", **OPT))
        _CACHE[name] = s
    return _CACHE[name]


def _grad(s, mode=0, X=None, cols=None, kernel="hbm", everything=True, **kw):
    out = s["eng"].simulate_objective_grad_batch(
        s["loss"], s["X"] if X is None else X, s["t"], s["cols"] if cols is None else cols, y0=s["y0"], loss_mode=mode, defaults=s["defaults"],
        lambdas=LAM, want_pred=everything, want_Y=everything, want_dY=everything, kernel=kernel, **dict(OPT, **kw))
    assert out is not None
    return _np(out)


def _close(got, want, bnd, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    bad = np.abs(got[ok] - want[ok]) > np.broadcast_to(bnd, want.shape)[ok]
    assert not bad.any(), (what, np.abs(got[ok] - want[ok])[bad][:4], np.broadcast_to(bnd, want.shape)[ok][bad][:4])


def _ratio(dY, gold):
    R = gold["dY"]
    cmax = np.abs(R).max(axis=(1, 2))
    err = np.abs(dY - R).max(axis=(1, 2))
    return ((err - gold["self_err"]) / _band(cmax)).max(), (err / _band(cmax)).max()


def _slab_bytes(eng, g, kc, scoring):
    """net_sens_ws_slab_doubles restated: the plain work area (NetLds + 7 S + 3 N), the sensitivity area of the LDS kernels ([sA | sT],
    per column 7 S + sites + N + 2; scoring: N + 4, per column N + 3), whole 128-B lines."""
    N, S, nK, sites = eng.N, eng.S, eng.n_K, int(g["total_sites"])
    plain = eng.n_var + S + nK + sites + 3 * N + 7 * S + 3 * N
    area = 2 * N + kc * (7 * S + sites + N + 2) + ((N + 4 + kc * (N + 3)) if scoring else 0)
    return (plain + area + 15) // 16 * 16 * 8


def test_host_arithmetic(monkeypatch):
    s = _setup("network_m1_small")
    eng, g = s["eng"], s["g"]
    assert eng.n_var > 16
    for sc in (False, True):
        assert [eng.sens_hbm_columns(K, sc) for K in (0, 1, 5, 16, 17, eng.n_var, 10 ** 6)] == [0, 1, 5, 16, 16, 16, 16]
        for K in (1, 2, 8, 16):
            assert eng.sens_workspace_bytes(1, K, sc) == _slab_bytes(eng, g, K, sc), (K, sc)
        # the plain slab of pk_network_workspace_bytes plus the area: the slab grows by whole columns
        assert eng.sens_workspace_bytes(1, 1, sc) > eng.workspace_bytes(1)
    monkeypatch.setenv("PK_NET_SENS_KC", "3")
    assert eng.sens_hbm_columns(8) == 3 and eng.sens_hbm_columns(2, True) == 2
    assert eng.sens_workspace_bytes(1, 8) == 3 * _slab_bytes(eng, g, 3, False)     # one candidate, three chunks: three work items
    monkeypatch.setenv("PK_NET_SENS_KC", "40")                                     # the knob only lowers
    assert eng.sens_hbm_columns(40) == 16
    monkeypatch.delenv("PK_NET_SENS_KC")
    with pytest.raises(ValueError):
        eng.sens_hbm_columns(-1)


@pytest.mark.parametrize("name", ref.NAMES)
def test_small_fixtures_against_the_exact_reference_and_the_lds_launch(name, monkeypatch):
    s = _setup(name)
    eng, gold = s["eng"], s["gold"]
    dY, Y, st, ns = s["sens"]
    assert not st.any() and dY.shape == gold["dY"].shape and np.array_equal(dY[:, 0], np.zeros_like(dY[:, 0]))
    net_ratio, raw_ratio = _ratio(dY, gold)
    print(f"{name}: slab route, steps {ns[:, 0]}; worst |dY - ref| / band (self_err not subtracted) {raw_ratio:.3f}")
    assert net_ratio <= C_BAND
    Yw, stw, _ = (_np(a) for a in eng.simulate_batch(s["X"], s["t"], y0=s["y0"], kernel="workspace", **OPT))
    r = (np.abs(Y - Yw) / _band(np.abs(Yw).max(axis=1, keepdims=True))).max()
    print(f"{name}: |Y(slab sens) - Y(simulate_batch workspace)| / band: {r:.3f}")
    assert r <= C_BAND and np.array_equal(Y[:, 0], Yw[:, 0]) and not stw.any()
    # the LDS launch at the same chunk width
    monkeypatch.setenv("PK_NET_SENS_KC", "8")
    assert eng.sens_columns_per_launch() == 8 and eng.sens_hbm_columns(8) == 8
    dL, YL, stL, nsL = (_np(a) for a in eng.simulate_sens_batch(s["X"], s["t"], s["cols"], y0=s["y0"], **OPT))
    dH, YH, stH, nsH = (_np(a) for a in eng.simulate_sens_batch(s["X"], s["t"], s["cols"], y0=s["y0"], kernel="hbm", **OPT))
    monkeypatch.delenv("PK_NET_SENS_KC")
    assert np.array_equal(dH, dY)                                                  # W = 16 or 8: one chunk of 8 either way
    agree = (np.abs(dH - dL).max(axis=(1, 2)) / _band(np.abs(dL).max(axis=(1, 2)))).max()
    print(f"{name}: worst |dY_hbm - dY_lds| / (atol + rtol max|column|) = {agree:.3e}; n_steps hbm {nsH.tolist()} lds {nsL.tolist()}")
    assert agree <= AGREE
    assert np.abs(nsH.astype(int) - nsL.astype(int)).max() <= 1 and np.array_equal(stH, stL)


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("name", ref.NAMES)
def test_small_fixtures_scoring_flavour_reproduced_from_its_own_trajectory(name, mode):
    s = _setup(name)
    out = _grad(s, mode=mode)
    assert not out["status"].any()
    for k in range(ref.N_CAND):
        r = og.chain(s["net"], out["Y"][k], out["dY"][k], s["ld"], mode, s["X"][k], s["defaults"], LAM, s["cols"])
        for key in KEYS:
            rk = "sums" if key == "loss_sums" else key
            _close(out[key][k], r[rk], og.bound(r, rk), (key, k, mode))
    if mode == 0:
        # the store flavour's dY is the scoring flavour's (the same steps: scoring adds nothing to the error norm)
        assert np.array_equal(out["dY"], s["sens"][0]) and np.array_equal(out["Y"], s["sens"][1])


@pytest.mark.parametrize("name", ["network_m0_small", "network_m2_small"])
def test_exact_claims_K0_and_permutation(name):
    s = _setup(name)
    eng, cols = s["eng"], s["cols"]
    dY, Y, st, ns = s["sens"]
    # K = 0 is simulate_batch / simulate_objective_batch on the workspace kernel, bit for bit
    Yw, stw, nsw = (_np(a) for a in eng.simulate_batch(s["X"], s["t"], y0=s["y0"], kernel="workspace", **OPT))
    d0, Y0, st0, ns0 = eng.simulate_sens_batch(s["X"], s["t"], [], y0=s["y0"], kernel="hbm", **OPT)
    assert d0.shape == (3, s["t"].size, eng.S, 0)
    assert np.array_equal(_np(Y0), Yw) and np.array_equal(_np(st0), stw) and np.array_equal(_np(ns0), nsw)
    z = _np(eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], [], y0=s["y0"], defaults=s["defaults"], lambdas=LAM, want_Y=True, kernel="hbm", **OPT))
    s1, F1, st1, ns1, Y1 = (_np(v) for v in eng.simulate_objective_batch(s["loss"], s["X"], s["t"], y0=s["y0"], defaults=s["defaults"], lambdas=LAM,
                                                                         want_Y=True, kernel="workspace", **OPT))
    for got, want in ((z["loss_sums"], s1), (z["F"], F1), (z["status"], st1), (z["n_steps"], ns1), (z["Y"], Y1)):
        assert np.array_equal(got, want)
    # permuting cols permutes dY / dF exactly within one chunk
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    dYp = _np(eng.simulate_sens_batch(s["X"], s["t"], cols[perm], y0=s["y0"], want_Y=False, kernel="hbm", **OPT)[0])
    assert np.array_equal(dYp, dY[..., perm])
    m, p = _grad(s), _grad(s, cols=cols[perm])
    for k in ("dF", "dpred", "dsums", "dY"):
        assert np.array_equal(p[k], m[k][..., perm]), k
    assert np.array_equal(p["F"], m["F"]) and np.array_equal(p["pred"], m["pred"])


@pytest.mark.parametrize("name", ["network_m0_small", "network_m2_small"])
def test_exact_claims_chunks(name, monkeypatch):
    """three chunks of <= 3 columns: chunk 0 is the launch of its three columns alone, every chunk stays in band"""
    s = _setup(name)
    eng, cols, gold = s["eng"], s["cols"], s["gold"]
    monkeypatch.setenv("PK_NET_SENS_KC", "3")
    assert eng.sens_hbm_columns(8) == 3
    dYc, Yc, stc, nsc = (_np(a) for a in eng.simulate_sens_batch(s["X"], s["t"], cols, y0=s["y0"], kernel="hbm", **OPT))
    ch = _grad(s)
    monkeypatch.delenv("PK_NET_SENS_KC")
    d3, Y3, st3, ns3 = (_np(a) for a in eng.simulate_sens_batch(s["X"], s["t"], cols[:3], y0=s["y0"], kernel="hbm", **OPT))
    assert not stc.any() and np.array_equal(dYc[..., :3], d3) and np.array_equal(Yc, Y3) and np.array_equal(nsc, ns3)
    assert _ratio(dYc, gold)[0] <= C_BAND
    alone = _grad(s, cols=cols[:3])
    for k in ("dF", "dpred", "dsums"):
        assert np.array_equal(ch[k][..., :3], alone[k]), k
    for k in ("F", "loss_sums", "pred", "Y", "n_steps"):
        assert np.array_equal(ch[k], alone[k]), k
    assert not ch["status"].any() and np.isfinite(ch["dF"]).all()


@pytest.mark.parametrize("name", ["network_m0_small", "network_m2_small"])
def test_exact_claims_raw(name):
    """raw = True: d / d raw = d / d physical x softplus'(raw); one raw entry above 20, where softplus is the identity"""
    s = _setup(name)
    eng, cols = s["eng"], s["cols"]
    x_raw = np.stack([nm.inv_softplus(r) for r in s["X"]])
    x_raw[2, cols[5]] = 25.0
    x_phys = eng.unpack_batch(x_raw)
    dr = _np(eng.simulate_sens_batch(x_raw, s["t"], cols, y0=s["y0"], raw=True, want_Y=False, kernel="hbm", **OPT)[0])
    dp = _np(eng.simulate_sens_batch(x_phys, s["t"], cols, y0=s["y0"], want_Y=False, kernel="hbm", **OPT)[0])
    fac = og.softplus_prime(x_raw[:, cols])
    assert fac[2, 5] == 1.0 and np.array_equal(dr[2, ..., 5], dp[2, ..., 5])
    want = dp * fac[:, None, None, :]
    assert (np.abs(dr - want).max(axis=(1, 2)) <= 1e-12 * np.abs(want).max(axis=(1, 2))).all()


def test_slab_reuse_over_more_candidates_than_the_grid():
    import torch
    s = _setup("network_m1_small")
    eng = s["eng"]
    cols = s["cols"][[1, 5]]                                                       # A_i, Dp_i
    slab = eng.sens_workspace_bytes(1, 2, True)
    grid = eng.sens_workspace_bytes(10 ** 6, 2, True) // slab
    cus = torch.cuda.get_device_properties(eng.ctx.device).multi_processor_count
    assert grid >= cus and grid % cus == 0, (grid, cus)                            # whole workgroups per compute unit
    B = grid + 37
    assert eng.sens_workspace_bytes(B, 2, True) == eng.sens_workspace_bytes(grid, 2, True) == grid * slab
    rng = np.random.default_rng(5)
    X = s["X"][0][None, :] * np.exp(0.2 * rng.standard_normal((B, eng.n_var)))
    run = lambda X_: _np(eng.simulate_objective_grad_batch(s["loss"], X_, s["t"], cols, y0=s["y0"], loss_mode=0, defaults=s["defaults"], lambdas=LAM,
                                                                want_pred=True, want_dY=True, kernel="hbm", rtol=1e-5, atol=1e-7))
    m = run(X)
    assert not m["status"].any() and ld_has_rna(s)
    keys = ("F", "dF", "pred", "dpred", "dY", "loss_sums", "dsums", "n_steps")
    for row in (0, grid - 1, grid, B - 1):
        one = run(X[row])
        for k in keys:
            assert np.array_equal(one[k][0], m[k][row]), (k, row)
    # workgroup 0 takes items 0 and `grid` on one slab: a NaN parameter in candidate 0 flags that row alone, and the row that reuses the
    # slab is untouched
    Xn = X.copy()
    Xn[0, cols[0]] = np.nan
    n = run(Xn)
    assert n["status"][0] & 1 and not n["status"][1:].any()                        # PK_ST_NONFINITE
    assert (n["F"][0] == 1e12).all()
    for k in ("dF", "dsums", "dpred", "pred", "dY"):
        assert np.isnan(n[k][0]).all(), k
    for k in keys:
        assert np.array_equal(n[k][1:], m[k][1:]), k


def ld_has_rna(s):
    return s["ld"]["rna_base_idx"] > 0 and s["ld"]["p_rna"].size > 0


def _row(g, k):
    return np.concatenate([np.ravel(g[n][k]) for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")] + [[float(g["tf_scale"][k])]])


def _union(m):
    """netlarge_m<m> and the union of 2 copies of it: engines, candidate 0 on both, the first 7 output times (t <= 8: a few hundred steps,
    the rna baseline t = 4 and one rna row behind it)."""
    from phoskintime_amd.global_model import NetworkEngine, synthetic
    g = np.load(ref.GOLDEN / f"netlarge_m{m}.npz")
    d = dict(g)
    e1, eu = NetworkEngine.from_npz(g), NetworkEngine.from_npz(synthetic.tile_network(d, 2))
    x1 = _row(g, 0)
    xu = synthetic.tile_candidate(x1, 2, d)
    return g, nm.Network.from_npz(g), e1, eu, x1, xu, g["t_eval"][:7], np.tile(g["y0"], 2)


def _union_cols(g, net, kinds):
    """One entry per kind -> (indices on the single network, indices of copy 1's entries on the 2-copy union); the kinase is the one
    that phosphorylates the most sites."""
    nK, N, sites = net.n_K, net.N, net.total_sites
    sl1 = ref.slices(net)
    slu = ref.slices(SimpleNamespace(n_K=2 * nK, N=2 * N, total_sites=2 * sites))
    pick = {"c_k": int(np.bincount(g["W_indices"][:int(g["W_indptr"][-1])], minlength=nK).argmax()), "B_i": 7, "Dp_i": sites - 1, "tf_scale": 0}
    size = {"c_k": nK, "B_i": N, "Dp_i": sites, "tf_scale": 0}
    c1 = [sl1[k][0] + pick[k] for k in kinds]
    cu = [slu[k][0] + size[k] + pick[k] for k in kinds]
    return np.asarray(c1, np.int32), np.asarray(cu, np.int32), slu


UOPT = dict(rtol=1e-6, atol=1e-8)


def _tangent_blocks(m, kinds):
    g, net, e1, eu, x1, xu, t, y0u = _union(m)
    S = e1.S
    assert eu.N == 200 and eu.S == 2 * S > 1024 and eu.sens_columns_per_launch() == 0 and eu.objective_grad_columns_per_launch() == 0
    assert e1.sens_columns_per_launch() == 3
    c1, cu, slu = _union_cols(g, net, kinds)
    d1, Y1, st1, ns1 = (_np(a) for a in e1.simulate_sens_batch(x1, t, c1, y0=g["y0"], **UOPT))
    du, Yu, stu, nsu = (_np(a) for a in eu.simulate_sens_batch(xu, t, cu, y0=y0u, **UOPT))              # default options: the slab route by itself
    assert not st1.any() and not stu.any()
    print(f"netlarge_m{m} x 2: steps union {nsu[0].tolist()} single {ns1[0].tolist()}")
    assert nsu[0, 0] < 1000
    for q, kind in enumerate(kinds):
        want = d1[0, ..., q]
        band = C_BAND * _band(np.abs(want).max(), **UOPT)
        assert np.abs(want).max() > 0
        r1 = np.abs(du[0, :, S:, q] - want).max() / band
        print(f"netlarge_m{m} x 2: column {kind} of copy 1: |block 1 - single| / band {r1:.4f}")
        assert r1 <= 1.0
        if kind == "tf_scale":
            assert np.abs(du[0, :, :S, q] - want).max() <= band
        else:
            assert np.array_equal(du[0, :, :S, q], np.zeros_like(want))            # copy 0 does not know copy 1's parameter: exactly 0.0
    return g, net, e1, eu, x1, xu, t, y0u, c1, cu, slu, d1, Y1


def test_union_beyond_lds_tangents_objective_gradient_and_the_problem_class():
    from phoskintime_amd.global_model import sensitivity as gs
    from phoskintime_amd.global_model.optproblem import GlobalODEBatch
    kinds = ("B_i", "Dp_i", "c_k", "tf_scale")
    g, net, e1, eu, x1, xu, t, y0u, c1, cu, slu, d1, Y1 = _tangent_blocks(0, kinds)
    N = e1.N
    assert (eu.N, eu.S) == (200, 1104)
    # loss lists built for copy 1 only: the single network's lists with the protein indices moved by N
    ld1 = og.loss_data(net, t)
    assert ld_has_rna(dict(ld=ld1))
    ldu = {k: (v + N if k in ("p_prot", "p_rna", "p_pho") else v) for k, v in ld1.items()}
    loss = eu.make_loss(ldu, t.size)
    out = eu.simulate_objective_grad_batch(loss, xu, t, cu, y0=y0u, lambdas=LAM, **UOPT)
    assert out is not None
    out = _np(out)
    assert not out["status"].any()
    # band of tests/test_gpu_network_objgrad.py::_bands, restated: the bands of Y and dY pushed through p = a / c, dp = da / c - a dc / c^2
    # and the squared-error point loss; reference: the chain on the single network's launch
    Yr, dYr = Y1[0], d1[0]
    r = og.chain(net, Yr, dYr, ld1, 0, x1, None, LAM, c1)
    W = gs.observable_weights(e1, ld1)
    tY = C_BAND * _band(np.abs(Yr).max(axis=0), **UOPT)
    tD = C_BAND * _band(np.abs(dYr).max(axis=(0, 1)), **UOPT)
    t_idx = np.concatenate([ld1["t_prot"], ld1["t_rna"], ld1["t_pho"]]).astype(int)
    b_idx = np.concatenate([np.full(ld1["p_prot"].size, ld1["prot_base_idx"]), np.full(ld1["p_rna"].size, ld1["rna_base_idx"]),
                            np.full(ld1["p_pho"].size, ld1["pho_base_idx"])]).astype(int)
    mod = np.concatenate([np.full(ld1["p_prot"].size, 0), np.full(ld1["p_rna"].size, 1), np.full(ld1["p_pho"].size, 2)])
    a, c = np.einsum("os,os->o", W, Yr[t_idx]), np.einsum("os,os->o", W, Yr[b_idx])
    da, dc = np.einsum("os,osk->ok", W, dYr[t_idx]), np.einsum("os,osk->ok", W, dYr[b_idx])
    assert a.min() > 1e-9 and c.min() > 1e-9
    ta = W @ tY; tc = np.where(b_idx == 0, 0.0, ta)
    tda = W.sum(axis=1)[:, None] * tD[None, :]; tdc = np.where((b_idx == 0)[:, None], 0.0, tda)
    tdp = (tda / c[:, None] + (a / c ** 2)[:, None] * tdc + (np.abs(da) / c[:, None] ** 2 + 2 * (a / c ** 3)[:, None] * np.abs(dc)) * tc[:, None]
           + np.abs(dc) / c[:, None] ** 2 * ta[:, None])
    tp = ta / c + a * tc / c ** 2
    obs = np.concatenate([ld1["obs_prot"], ld1["obs_rna"], ld1["obs_pho"]]); w = np.concatenate([ld1["w_prot"], ld1["w_rna"], ld1["w_pho"]])
    gq = -2.0 * (obs - r["pred"])
    per = w[:, None] * (2.0 * tp[:, None] * np.abs(r["dpred"]) + np.abs(gq)[:, None] * tdp)
    bnd = np.stack([per[mod == m_].sum(axis=0) for m_ in range(3)])
    ratio = np.abs(out["dsums"][0] - r["dsums"]) / bnd
    print(f"netlarge_m0 x 2: worst |dsums - single-network chain| / band {ratio.max():.4f}")
    assert ratio.max() <= 1.0 and (np.abs(out["dsums"][0]).max(axis=1) > 0).all()
    eu.free_loss(loss)
    # the optimiser's problem class gets an answer on this network
    keys = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
    dflt = xu * 1.1
    defaults = {k: (dflt[slu[k][0]:slu[k][1]] if k != "tf_scale" else float(dflt[slu[k][0]])) for k in keys}
    prob = GlobalODEBatch(eu, None, ldu, defaults, LAMD, t, y0=y0u, **UOPT)
    res = prob.evaluate_with_grad(nm.inv_softplus(xu)[None, :], cu)
    assert res is not None
    F, dF = (v.cpu().numpy() for v in res)
    assert F.shape == (1, 3) and dF.shape == (1, 3, 4) and np.isfinite(F).all() and np.isfinite(dF).all() and (np.abs(dF).max(axis=2) > 0).all()
    prob.close(); e1.close(); eu.close()


def test_union_beyond_lds_combinatorial_topology():
    out = _tangent_blocks(2, ("Dp_i",))
    out[2].close(); out[3].close()


def test_refusals_that_remain():
    import torch
    from phoskintime_amd import _capi
    s = _setup("network_m0_small")
    eng, cols, lib = s["eng"], s["cols"], s["eng"].ctx.lib
    for kw in (dict(method="ark", kernel="hbm"), dict(method="dp5", kernel="hbm"), dict(kernel="workspace")):
        assert eng.simulate_sens_batch(s["X"], s["t"], cols, y0=s["y0"], **kw) is None
        assert eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], cols, y0=s["y0"], lambdas=LAM, **kw) is None
    for bad in ([0, eng.n_var], [-1], [3, 5, 3]):
        with pytest.raises(_capi.PhoskinError):
            eng.simulate_sens_batch(s["X"], s["t"], bad, y0=s["y0"], kernel="hbm")
        with pytest.raises(_capi.PhoskinError):
            eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], bad, y0=s["y0"], lambdas=LAM, kernel="hbm")
    # B = 0 is PK_OK, straight at the C ABI
    dev = torch.device("cuda", eng.ctx.device)
    xd = torch.as_tensor(s["X"], device=dev); yd = torch.as_tensor(s["y0"], device=dev)
    Y = torch.empty((3, s["t"].size, eng.S), dtype=torch.float64, device=dev)
    one = np.array([0], dtype=np.int32)
    opts = _capi.default_opts(rtol=RTOL, atol=ATOL, kernel="hbm")
    vp = lambda a: C.c_void_p(a.data_ptr())
    assert lib.pk_network_simulate_sens_batch(eng.ctx.handle, eng._h, 0, vp(xd), 0, vp(yd), 0, s["t"].ctypes.data, s["t"].size, C.byref(opts),
                                              one.ctypes.data, 1, vp(Y), vp(Y), None, None) == _capi.PK_OK
    # every other network entry point refuses the value
    assert lib.pk_network_resolve_method(eng._h, C.byref(opts)) == _capi.PK_ERR_UNSUPPORTED
    st = torch.zeros((3,), dtype=torch.int32, device=dev)
    assert lib.pk_network_simulate_batch(eng.ctx.handle, eng._h, 3, vp(xd), 0, vp(yd), 0, s["t"].ctypes.data, s["t"].size, C.byref(opts), vp(Y),
                                         vp(st), None) == _capi.PK_ERR_UNSUPPORTED
    assert b"PK_KERNEL_HBM" in lib.pk_last_error(eng.ctx.handle)
