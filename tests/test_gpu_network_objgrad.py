"""GPU: the three objectives and their gradient from one launch of the sensitivity integrator's scoring flavour
(``NetworkEngine.simulate_objective_grad_batch``, csrc/pk_network_sens.hpp, csrc/pk_network_loss_grad.hpp) on the four
``network_m*_small`` fixtures (S = 20 .. 32), B = 3 candidates, the 8 stored columns, rtol = 1e-8 / atol = 1e-10, and one launch at
``netlarge_m0`` (N = 100, S = 552; B = 2, K = 4: two chunks, strided loops beyond 256 states).  Loss data as in
tests/net_objgrad_reference.py::fixture_data (every protein / site at every time, rna from t = 4 on).

The chain itself (test_chain_*): one launch returns everything; the plain-loop reference chain applied to that launch's own ``Y`` and
``dY`` must reproduce ``pred``, ``dpred``, ``loss_sums``, ``dsums``, ``F``, ``dF`` within (n_terms + OPS) 2^-53 sum|elementary products|
(the operation counts stand in the reference module's docstring), NaN positions equal (mode 2).  ``F`` also agrees with
``nm.objectives`` on the returned ``Y`` at the 1e-11 of the fused-objective test.

Against the exact reference (test_dsums_against_the_exact_reference): ``dsums`` in mode 0 against the chain on the stored exact ``Y`` /
``dY``.  Band per entry, to first order: with g_k = rho'(pred_k) = -2 (obs_k - pred_k) and rho'' = 2,

    |dsums[m, c] - ref| <= sum_k w_k (2 tp_k |dpred_kc| + |g_k| tdp_kc)

where tp_k and tdp_kc are the bands of pred and dpred of ``test_gpu_network_sens.py::test_local_sensitivity_batch``: the bands of Y
(C_BAND (atol + rtol max|Y_s|)) and dY (C_BAND (atol + rtol max|dY_c|) + self_err) pushed through p = a / c, dp = da / c - a dc / c^2.
Pass is ratio <= 1.  Measured on an MI355X (gfx950): worst ratio over candidates, objectives and columns per fixture, then band / |g| at
each objective's largest column, worst over candidates (protein, rna, phospho):

    network_m0_small  ratio 0.0029      band / |g|  7.2e-05  4.4e-04  5.2e-04
    network_m1_small  ratio 0.0011      band / |g|  1.2e-04  5.7e-03  2.7e-04
    network_m2_small  ratio < 0.00005   band / |g|  9.4e-05  1.8e-03  1.6e-04
    network_m4_small  ratio < 0.00005   band / |g|  9.8e-05  2.9e-04  1.9e-04

The per-entry band is at most 0.6 % of an objective's largest gradient entry (rna on the sequential fixture) and the measured error is
at most 0.3 % of the band: C_BAND is ten times a transient outlier of the tangents (see tests/test_gpu_network_sens.py), and a sum over
all rows and observables is not ruled by it.

On a launch with more than one chunk the chain check takes each chunk with the trajectory that chunk integrated: every chunk integrates
the state itself, so chunk j > 0 forms pred, rho' and dpred from ITS y, which lies within rtol / atol of the ``Y`` chunk 0 writes, not on
it (measured at netlarge_m0: |dpred - chain on chunk 0's Y| up to 1e-10 against a rounding bound of 1e-15).  The chunk equals the launch
of its columns alone bit for bit, and that launch returns its ``Y``.

Exact (bit-for-bit) claims: optional outputs change nothing; K = 0 equals ``simulate_objective_batch(method="rosw", kernel="lds")``;
permuting ``cols`` permutes the outputs (K <= KC); a candidate alone equals its row in a batch; chunk 0 of a chunked launch equals the
launch of its columns alone."""
import ctypes as C

import numpy as np
import pytest

import net_objgrad_reference as og
import net_sens_reference as ref
from oracle import network_models as nm

pytestmark = pytest.mark.gpu
RTOL, ATOL = ref.RTOL_GPU, ref.ATOL_GPU
OPT = dict(rtol=RTOL, atol=ATOL)
C_BAND = 269.0          # tests/test_gpu_network_sens.py
LAM, LAMD = og.LAM, og.LAMD
KEYS = ("pred", "dpred", "loss_sums", "dsums", "F", "dF")
_CACHE = {}


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _setup(name):
    """Engine, fixture data, loss handle and the main launch (mode 0, defaults, everything asked for) of a fixture, made once."""
    if name not in _CACHE:
        from phoskintime_amd.global_model import NetworkEngine
        s = dict(og.fixture_data(name))
        s["eng"] = eng = NetworkEngine.from_npz(s["g"])
        s["cols"] = s["gold"]["cols"].astype(np.int32)
        s["t"], s["y0"] = s["g"]["t_eval"], s["g"]["y0"]
        s["loss"] = eng.make_loss(s["ld"], s["t"].size)
        _CACHE[name] = s
        s["main"] = _launch(s)
    return _CACHE[name]


def _launch(s, mode=0, defaults=True, X=None, cols=None, loss=None, everything=True, **kw):
    out = s["eng"].simulate_objective_grad_batch(
        s["loss"] if loss is None else loss, s["X"] if X is None else X, s["t"], s["cols"] if cols is None else cols, y0=kw.pop("y0", s["y0"]),
        loss_mode=mode, defaults=s["defaults"] if defaults else None, lambdas=LAM, want_pred=everything, want_Y=everything, want_dY=everything,
        **OPT, **kw)
    assert out is not None
    return _np(out)


def _close(got, want, bnd, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    bad = np.abs(got[ok] - want[ok]) > np.broadcast_to(bnd, want.shape)[ok]
    assert not bad.any(), (what, np.abs(got[ok] - want[ok])[bad][:4], np.broadcast_to(bnd, want.shape)[ok][bad][:4])


def _check_chain(s, out, Xphys, mode, defaults, scl=None, ld=None, ldo=None, cols=None, net=None):
    """The reference chain on the launch's own Y and dY reproduces its six outputs; F agrees with the oracle on Y."""
    net = s["net"] if net is None else net
    ld = s["ld"] if ld is None else ld
    cols = s["cols"] if cols is None else cols
    assert not out["status"].any()
    for k in range(Xphys.shape[0]):
        r = og.chain(net, out["Y"][k], out["dY"][k], ld, mode, Xphys[k], defaults, LAM, cols, None if scl is None else scl[k])
        for key in KEYS:
            _close(out[key][k], r["sums" if key == "loss_sums" else key], og.bound(r, "sums" if key == "loss_sums" else key), (key, k, mode))
        if ldo is not None or ld is s["ld"]:
            want = nm.objectives(net, Xphys[k], defaults if defaults is not None else Xphys[k], out["Y"][k], s["ldo"] if ldo is None else ldo, mode,
                                 LAMD if defaults is not None else dict(LAMD, prior=0.0))
            np.testing.assert_allclose(out["F"][k], want, rtol=1e-11, equal_nan=True)


@pytest.mark.parametrize("mode", range(8))
@pytest.mark.parametrize("name", ref.NAMES)
def test_chain_all_modes(name, mode):
    s = _setup(name)
    out = s["main"] if mode == 0 else _launch(s, mode=mode)
    _check_chain(s, out, s["X"], mode, s["defaults"])
    if mode == 2:
        assert np.isnan(out["dsums"]).any()                    # negative residuals under the logarithm: NaN in value and gradient alike
    if mode in (0, 5):
        _check_chain(s, _launch(s, mode=mode, defaults=False), s["X"], mode, None)


@pytest.mark.parametrize("name", ref.NAMES)
def test_chain_raw_candidates(name):
    s = _setup(name)
    eng, cols = s["eng"], s["cols"]
    x_raw = np.stack([nm.inv_softplus(r) for r in s["X"]])
    x_raw[2, cols[5]] = 25.0                                   # above 20 softplus is the identity and its derivative exactly 1
    Xp = eng.unpack_batch(x_raw).cpu().numpy()
    scl = og.softplus_prime(x_raw[:, cols])
    assert scl[2, 5] == 1.0 and (scl[:2] < 1.0).all()
    for mode in (0, 3):
        out = _launch(s, mode=mode, X=x_raw, raw=True)
        _check_chain(s, out, Xp, mode, s["defaults"], scl=scl)
    # ... and the raw gradient is the physical one times softplus' (the same steps; one more multiplication per value)
    phys = _launch(s, X=Xp)
    assert np.array_equal(out["n_steps"], _launch(s, mode=3, X=Xp)["n_steps"])
    raw0 = _launch(s, X=x_raw, raw=True)
    want = phys["dsums"] * scl[:, None, :]
    assert (np.abs(raw0["dsums"] - want) <= 4 * og.U * np.abs(want)).all() and np.array_equal(raw0["n_steps"], phys["n_steps"])
    np.testing.assert_allclose(raw0["F"], phys["F"], rtol=1e-12)


@pytest.mark.parametrize("name", ref.NAMES)
def test_optional_outputs_change_nothing_and_K0(name):
    s = _setup(name)
    eng, m = s["eng"], s["main"]
    a = _np(eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], s["cols"], y0=s["y0"], defaults=s["defaults"], lambdas=LAM, want_sums=False, **OPT))
    assert set(a) == {"status", "n_steps", "F", "dF"}
    for k in ("F", "dF", "status", "n_steps"):
        assert np.array_equal(a[k], m[k]), k
    b = _np(eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], s["cols"], y0=s["y0"], defaults=s["defaults"], lambdas=LAM, want_sums=False,
                                              want_F=False, want_pred=True, **OPT))
    assert set(b) == {"status", "n_steps", "pred", "dpred"}
    for k in ("pred", "dpred", "status", "n_steps"):
        assert np.array_equal(b[k], m[k]), k
    for mode in (0, 6):
        z = _np(eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], [], y0=s["y0"], loss_mode=mode, defaults=s["defaults"], lambdas=LAM, want_Y=True, **OPT))
        s1, F1, st1, ns1, Y1 = (v.cpu().numpy() for v in eng.simulate_objective_batch(s["loss"], s["X"], s["t"], y0=s["y0"], loss_mode=mode, defaults=s["defaults"],
                                                                                    lambdas=LAM, want_Y=True, method="rosw", kernel="lds", **OPT))
        assert z["dF"].shape == (3, 3, 0)
        for got, want in ((z["loss_sums"], s1), (z["F"], F1), (z["status"], st1), (z["n_steps"], ns1), (z["Y"], Y1)):
            assert np.array_equal(got, want)


def _bands(s, k, cols_idx=slice(None)):
    """(reference chain on the stored exact Y / dY of candidate k, band of dsums [3, K]) in mode 0: see the module docstring."""
    from phoskintime_amd.global_model import sensitivity as gs
    gold, ld, net = s["gold"], s["ld"], s["net"]
    Yr, dYr = gold["Y"][k], gold["dY"][k][:, :, cols_idx]
    r = og.chain(net, Yr, dYr, ld, 0, s["X"][k], s["defaults"], LAM, s["cols"][cols_idx])
    W = gs.observable_weights(s["eng"], ld)
    band = lambda mx: ATOL + RTOL * mx
    tY = C_BAND * band(np.abs(Yr).max(axis=0))                                               # [S]
    tD = C_BAND * band(np.abs(dYr).max(axis=(0, 1))) + gold["self_err"][k][cols_idx]         # [K]
    t_idx = np.concatenate([ld["t_prot"], ld["t_rna"], ld["t_pho"]]).astype(int)
    b_idx = np.concatenate([np.full(ld["p_prot"].size, ld["prot_base_idx"]), np.full(ld["p_rna"].size, ld["rna_base_idx"]),
                            np.full(ld["p_pho"].size, ld["pho_base_idx"])]).astype(int)
    mod = np.concatenate([np.full(ld["p_prot"].size, 0), np.full(ld["p_rna"].size, 1), np.full(ld["p_pho"].size, 2)])
    a, c = np.einsum("os,os->o", W, Yr[t_idx]), np.einsum("os,os->o", W, Yr[b_idx])
    da, dc = np.einsum("os,osk->ok", W, dYr[t_idx]), np.einsum("os,osk->ok", W, dYr[b_idx])
    assert a.min() > 1e-9 and c.min() > 1e-9
    ta = W @ tY; tc = np.where(b_idx == 0, 0.0, ta)                                          # the baseline row 0 is y0 itself: exact
    tda = W.sum(axis=1)[:, None] * tD[None, :]; tdc = np.where((b_idx == 0)[:, None], 0.0, tda)
    tdp = (tda / c[:, None] + (a / c ** 2)[:, None] * tdc + (np.abs(da) / c[:, None] ** 2 + 2 * (a / c ** 3)[:, None] * np.abs(dc)) * tc[:, None]
           + np.abs(dc) / c[:, None] ** 2 * ta[:, None])
    tp = ta / c + a * tc / c ** 2
    obs = np.concatenate([ld["obs_prot"], ld["obs_rna"], ld["obs_pho"]]); w = np.concatenate([ld["w_prot"], ld["w_rna"], ld["w_pho"]])
    g = -2.0 * (obs - r["pred"])
    per = w[:, None] * (2.0 * tp[:, None] * np.abs(r["dpred"]) + np.abs(g)[:, None] * tdp)
    return r, np.stack([per[mod == m].sum(axis=0) for m in range(3)])


@pytest.mark.parametrize("name", ref.NAMES)
def test_dsums_against_the_exact_reference(name):
    s = _setup(name)
    worst, rel = 0.0, np.zeros(3)
    for k in range(ref.N_CAND):
        r, bnd = _bands(s, k)
        ratio = np.abs(s["main"]["dsums"][k] - r["dsums"]) / bnd
        worst = max(worst, float(ratio.max()))
        big = np.abs(r["dsums"]).argmax(axis=1)
        rel = np.maximum(rel, bnd[np.arange(3), big] / np.abs(r["dsums"][np.arange(3), big]))
        assert ratio.max() <= 1.0, (k, ratio)
    print(f"{name}: worst |dsums - ref| / band {worst:.4f}; band / |g| at the largest column (protein, rna, phospho): "
          + ", ".join(f"{v:.3g}" for v in rel))


@pytest.mark.parametrize("name", ref.NAMES)
def test_columns_order_chunks_and_batch_independence(name, monkeypatch):
    s = _setup(name)
    eng, cols, m = s["eng"], s["cols"], s["main"]
    assert eng.objective_grad_columns_per_launch() >= cols.size                          # one chunk on the small fixtures
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    p = _launch(s, cols=cols[perm])
    for k in ("dF", "dpred", "dsums", "dY"):
        assert np.array_equal(p[k], m[k][..., perm]), k
    assert np.array_equal(p["F"], m["F"]) and np.array_equal(p["pred"], m["pred"])
    # a row of the B = 3 launch equals its B = 1 launch, also with batched y0
    one = _launch(s, X=s["X"][2])
    for k in KEYS + ("status", "n_steps", "Y", "dY"):
        assert np.array_equal(one[k][0], m[k][2]), k
    y0b = s["y0"][None, :] * np.array([1.0, 0.7, 1.3])[:, None]
    bat = _launch(s, y0=y0b, everything=False)
    one = _launch(s, X=s["X"][1], y0=y0b[1], everything=False)
    for k in ("F", "dF", "loss_sums", "dsums", "n_steps"):
        assert np.array_equal(one[k][0], bat[k][1]), k
        assert np.array_equal(bat[k][0], m[k][0]), k
    # K > KC: three chunks; chunk 0 is the launch of its three columns alone, F is chunk 0's, every column stays in the band
    monkeypatch.setenv("PK_NET_SENS_KC", "3")
    assert eng.objective_grad_columns_per_launch() == 3
    ch = _launch(s)
    monkeypatch.delenv("PK_NET_SENS_KC")
    alone = _launch(s, cols=cols[:3])
    assert not ch["status"].any()
    for k in ("dF", "dpred", "dsums"):
        assert np.array_equal(ch[k][..., :3], alone[k]), k
    for k in ("F", "loss_sums", "pred", "Y", "n_steps"):
        assert np.array_equal(ch[k], alone[k]), k
    for k in range(ref.N_CAND):
        r, bnd = _bands(s, k)
        assert (np.abs(ch["dsums"][k] - r["dsums"]) <= bnd).all()


def test_one_state_and_time_observed_twice_counts_twice():
    s = _setup("network_m0_small")
    eng, ld = s["eng"], s["ld"]
    dup = {k: (np.concatenate([v, v[3:4]]) if k.endswith("_prot") and isinstance(v, np.ndarray) else v) for k, v in ld.items()}
    dup["obs_prot"][-1] *= 1.3
    loss = eng.make_loss(dup, s["t"].size)
    out = _launch(s, loss=loss)
    _check_chain(s, out, s["X"], 0, s["defaults"], ld=dup, ldo=og.oracle_ld(dup, s["net"]))
    n_prot = ld["p_prot"].size                                                           # the repeated entry ends the protein list
    assert out["pred"].shape[1] == s["main"]["pred"].shape[1] + 1 and np.array_equal(out["pred"][:, n_prot], out["pred"][:, 3])
    assert np.array_equal(out["dpred"][:, n_prot], out["dpred"][:, 3])
    assert (out["loss_sums"][:, 0] > s["main"]["loss_sums"][:, 0]).all() and np.array_equal(out["loss_sums"][:, 1:], s["main"]["loss_sums"][:, 1:])
    eng.free_loss(loss)


def test_netlarge_two_chunks_and_the_column_query():
    from phoskintime_amd.global_model import NetworkEngine
    g = np.load(ref.GOLDEN / "netlarge_m0.npz")
    eng = NetworkEngine.from_npz(g)
    net = nm.Network.from_npz(g)
    assert (eng.N, eng.S) == (100, 552)
    # net_sens_score_lds_bytes restated: the plain request, [sA | sT], per column 7 S + sites + N + 2; scoring: N + 4, per column N + 3
    N, S, nK, sites, nnz = eng.N, eng.S, eng.n_K, int(g["total_sites"]), int(g["TF_indptr"][-1])
    plain = (eng.n_var + S + nK + sites + 3 * N + 7 * S + 3 * N + 24 + nnz + N) * 8 + ((N + 1 + nnz) * 4 + 7) // 8 * 8
    fixed, per = plain + (2 * N + N + 4) * 8, (7 * S + sites + N + 2 + N + 3) * 8
    assert eng.objective_grad_columns_per_launch() == (160 * 1024 - fixed) // per == 3 and eng.sens_columns_per_launch() == 3
    X = np.stack([eng.pack_params(*(g[k][b] for k in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale"))) for b in range(2)])
    t = g["t_eval"]
    ld0 = og.loss_data(net, t)
    sl = ref.slices(net)
    cols = np.array([sl["c_k"][0] + 1, sl["A_i"][0] + 99, sl["Dp_i"][0] + 351, sl["tf_scale"][0]], dtype=np.int32)      # two chunks: 3 + 1
    loss = eng.make_loss(ld0, t.size)
    s = dict(eng=eng, loss=loss, X=X, t=t, cols=cols, y0=g["y0"], defaults=X[0] * 1.1, ld=ld0, ldo=og.oracle_ld(ld0, net), net=net)
    out = _launch(s)
    # Every chunk integrates the state itself, so a chunk's pred, rho' and tangents belong to ITS trajectory; Y is chunk 0's.  The chain
    # check therefore takes each chunk with the trajectory that chunk integrated: chunk 0 (columns 0..2) with the launch's own Y, chunk 1
    # (column 3) with the Y of the launch of that column alone, which the chunk equals bit for bit
    per_col = ("dpred", "dsums", "dF", "dY")
    head = {k: (v[..., :3] if k in per_col else v) for k, v in out.items()}
    _check_chain(dict(s, cols=cols[:3]), head, X, 0, s["defaults"])
    alone = _launch(dict(s, cols=cols[3:]))
    for k in per_col:
        assert np.array_equal(out[k][..., 3:], alone[k]), k
    _check_chain(dict(s, cols=cols[3:]), alone, X, 0, s["defaults"])
    assert (np.abs(out["dsums"]).max(axis=2) > 0).all()
    eng.free_loss(loss); eng.close()


def test_nan_parameter_fails_its_candidate_and_leaves_the_neighbours():
    s = _setup("network_m1_small")
    m = s["main"]
    X = s["X"].copy()
    X[1, s["cols"][1]] = np.nan
    out = _launch(s, X=X)
    assert out["status"][1] & 1 and out["status"][0] == 0 and out["status"][2] == 0                # PK_ST_NONFINITE
    assert (out["F"][1] == 1e12).all()
    for k in ("dF", "dsums", "dpred", "pred"):
        assert np.isnan(out[k][1]).all(), k
    for k in KEYS + ("Y", "dY", "n_steps"):
        assert np.array_equal(out[k][[0, 2]], m[k][[0, 2]]), k


def test_refusals_and_argument_errors():
    import torch
    from phoskintime_amd import _capi
    s = _setup("network_m0_small")
    eng, cols, lib = s["eng"], s["cols"], s["eng"].ctx.lib
    err = lambda: lib.pk_last_error(eng.ctx.handle)
    for kw in (dict(method="ark"), dict(method="dp5"), dict(kernel="workspace")):
        assert eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], cols, y0=s["y0"], lambdas=LAM, **kw) is None
        assert b"PK_METHOD_ROS34PW2" in err() or b"PK_KERNEL_AUTO" in err()
    # an rna observation before its baseline
    early = dict(s["ld"]); early["t_rna"] = s["ld"]["t_rna"].copy(); early["t_rna"][0] = 0
    loss = eng.make_loss(early, s["t"].size)
    assert eng.simulate_objective_grad_batch(loss, s["X"], s["t"], cols, y0=s["y0"], lambdas=LAM) is None and b"rna baseline" in err()
    eng.free_loss(loss)
    for bad in ([0, eng.n_var], [-1], [3, 5, 3]):
        with pytest.raises(_capi.PhoskinError):
            eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], bad, y0=s["y0"], lambdas=LAM)
    with pytest.raises(_capi.PhoskinError):
        eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"], cols, y0=s["y0"], lambdas=LAM, loss_mode=8)
    with pytest.raises(_capi.PhoskinError):
        eng.simulate_objective_grad_batch(s["loss"], s["X"], s["t"][:-1], cols, y0=s["y0"], lambdas=LAM)
    # straight at the C ABI: all outputs NULL; K > 0 without a derivative output; dF without lambdas
    dev = torch.device("cuda", eng.ctx.device)
    xd = torch.as_tensor(s["X"], device=dev); yd = torch.as_tensor(s["y0"], device=dev)
    F = torch.empty((3, 3), dtype=torch.float64, device=dev); dF = torch.empty((3, 3, 1), dtype=torch.float64, device=dev)
    one = np.array([0], dtype=np.int32)
    lam = (C.c_double * 4)(*LAM)
    opts = _capi.default_opts(rtol=RTOL, atol=ATOL)
    vp = lambda tns: C.c_void_p(tns.data_ptr()) if tns is not None else None
    call = lambda F_, dF_, lam_: lib.pk_network_simulate_objective_grad_batch(
        eng.ctx.handle, eng._h, s["loss"], 3, vp(xd), 0, vp(yd), 0, s["t"].ctypes.data, s["t"].size, C.byref(opts), one.ctypes.data, 1, 0, None,
        C.cast(lam_, C.c_void_p) if lam_ is not None else None, 1e12, None, None, None, None, None, None, vp(F_), vp(dF_), None, None)
    assert call(None, None, lam) == _capi.PK_ERR_ARG and b"NULL" in err()
    assert call(F, None, lam) == _capi.PK_ERR_ARG and b"K > 0" in err()
    assert call(F, dF, None) == _capi.PK_ERR_ARG and b"lambdas" in err()
    assert call(F, dF, lam) == _capi.PK_OK
    torch.cuda.synchronize()
    assert np.isfinite(dF.cpu().numpy()).all()


def test_evaluate_with_grad_equals_the_engine_call():
    from phoskintime_amd.global_model.optproblem import GlobalODEBatch
    s = _setup("network_m0_small")
    eng, g = s["eng"], s["g"]
    keys = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
    sl = ref.slices(s["net"])
    defaults = {k: (s["defaults"][sl[k][0]:sl[k][1]] if k != "tf_scale" else float(s["defaults"][sl[k][0]])) for k in keys}
    prob = GlobalODEBatch(eng, None, s["ld"], defaults, LAMD, s["t"], loss_mode=4, y0=s["y0"], rtol=RTOL, atol=ATOL)
    x_raw = np.stack([nm.inv_softplus(r) for r in s["X"]])
    F, dF = prob.evaluate_with_grad(x_raw, s["cols"])
    want = eng.simulate_objective_grad_batch(prob.loss, x_raw, s["t"], s["cols"], y0=s["y0"], raw=True, rtol=RTOL, atol=ATOL,
                                             max_steps=prob.max_steps * s["t"].size, loss_mode=4, defaults=prob.defaults, lambdas=LAM,
                                             fail_value=prob.fail_value)
    assert F.is_cuda and dF.shape == (3, 3, 8)
    assert np.array_equal(F.cpu().numpy(), want["F"].cpu().numpy()) and np.array_equal(dF.cpu().numpy(), want["dF"].cpu().numpy())
    assert np.isfinite(dF.cpu().numpy()).all() and (np.abs(dF.cpu().numpy()).max(axis=2) > 0).all()
    prob.close()
