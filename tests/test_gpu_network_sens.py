"""GPU: forward parameter sensitivities of the network integrator (``NetworkEngine.simulate_sens_batch``, csrc/pk_network_sens.hpp) and
``global_model.sensitivity.local_sensitivity_batch`` on top of them, on the four ``network_m*_small`` fixtures (S = 20 .. 32), B = 3
candidates, one column per parameter kind (c_k, A_i, B_i, C_i, D_i, Dp_i, E_i, tf_scale), rtol = 1e-8 / atol = 1e-10.

Truth is the stored exact reference of tests/net_sens_reference.py (the oracle's tangent ODE under LSODA at 1e-12).  The band of
column c of a candidate is

    |dY - ref| <= C_BAND (atol + rtol max|ref column|) + self_err[candidate, c]

with self_err the reference's own tolerance-halving self-consistency (stored with it; <= 4.9e-10 of the column maximum).  C_BAND is ten
times the worst ratio measured on an MI355X against this reference: see the figures at C_BAND below.  The project's parity band for states is 1 in
these units; the trajectory Y of a sensitivity launch is held to the same C_BAND against ``simulate_batch(method="rosw", kernel="lds")``
(both are within the integrator's error of the exact solution; their steps differ because the tangents enter the error norm).

Exact (bit-for-bit) claims: K = 0 equals ``simulate_batch`` on the order-3 LDS kernel; permuting ``cols`` permutes dY (K <= KC, maximum
norm); a candidate's results do not depend on the batch around it; raw = True equals the physical dY times softplus' to 1e-12 of the
column maximum (the same steps, one multiplication per stored value)."""
import ctypes as C

import numpy as np
import pytest

import net_sens_reference as ref
from oracle import network_models as nm

pytestmark = pytest.mark.gpu
RTOL, ATOL = ref.RTOL_GPU, ref.ATOL_GPU
# Measured on an MI355X (gfx950) against the stored reference: worst |dY - ref| / (atol + rtol max|ref column|) over all rows and states,
# self_err not subtracted, per fixture and candidate (0, 1, 2):
#   network_m0_small  1.41  26.89  0.32      network_m1_small  22.42  0.64  5.15
#   network_m2_small  0.45   0.44  0.46      network_m4_small   0.63  0.67  0.56
# Away from the outliers the tangents sit where the states do (the parity band is 1).  The three outliers are transients: 26.89 at
# t = 15 (0.5 before, ~1 from t = 30 on), 22.42 at t = 120 (0.3 before, 0.55 at t = 480), 5.15 growing from t = 30.  They follow a
# sign change of a TF input on that candidate's trajectory, where the right-hand side is only C^1 (|v|, the u >= 0 branch), so the
# tangent's right-hand side has a kink: the order-3 step that straddles it loses its order and its embedded estimate under-reads the
# error.  (A fixed-width difference stencil across the same point had put an error of 8e-3 into an earlier version of the reference.)
# worst 26.89 -> C_BAND = 10 x 26.89
C_BAND = 269.0
OPT = dict(rtol=RTOL, atol=ATOL)


def _np(a):
    return a.cpu().numpy()


_CACHE = {}


def _setup(name):
    """Engine, fixture, stored reference and the main launch (B = 3, the 8 reference columns) of a fixture, made once."""
    if name not in _CACHE:
        from phoskintime_amd.global_model import NetworkEngine
        g, net, X = ref.fixture(name)
        gold = ref.load_golden(name)
        assert np.array_equal(gold["X"], X) and np.array_equal(gold["t"], g["t_eval"])
        eng = NetworkEngine.from_npz(g)
        cols = gold["cols"].astype(np.int32)
        dY, Y, st, ns = eng.simulate_sens_batch(X, g["t_eval"], cols, y0=g["y0"], **OPT)
        _CACHE[name] = dict(g=g, net=net, X=X, gold=gold, eng=eng, cols=cols, t=g["t_eval"], y0=g["y0"],
                            main=(_np(dY), _np(Y), _np(st), _np(ns)))
    return _CACHE[name]


def _band(refcol_max):
    return ATOL + RTOL * refcol_max


def _ratio(dY, gold):
    """worst (|dY - ref| - self_err) / (atol + rtol max|ref column|) over candidates, rows, states, per column -> [K]"""
    R = gold["dY"]
    cmax = np.abs(R).max(axis=(1, 2))                                  # [B, K]
    err = np.abs(dY - R).max(axis=(1, 2))
    return ((err - gold["self_err"]) / _band(cmax)).max(axis=0), (err / _band(cmax)).max(axis=0)


@pytest.mark.parametrize("name", ref.NAMES)
def test_dY_against_exact_reference(name):
    s = _setup(name)
    dY, Y, st, ns = s["main"]
    assert not st.any() and dY.shape == s["gold"]["dY"].shape
    assert np.array_equal(dY[:, 0], np.zeros_like(dY[:, 0]))                         # y0 is data
    net_ratio, raw_ratio = _ratio(dY, s["gold"])
    print(f"{name}: steps {ns[:, 0]}; |dY - ref| / band per column (raw, self_err not subtracted): "
          + ", ".join(f"{n}={v:.3f}" for n, v in zip(s["gold"]["names"], raw_ratio)) + f"; worst {raw_ratio.max():.3f}")
    assert net_ratio.max() <= C_BAND


@pytest.mark.parametrize("name", ref.NAMES)
def test_Y_in_band_and_K0_bit_equal(name):
    s = _setup(name)
    eng = s["eng"]
    Ys, sts, nss = (_np(a) for a in eng.simulate_batch(s["X"], s["t"], y0=s["y0"], method="rosw", kernel="lds", **OPT))
    _, Y, st, _ = s["main"]
    r = (np.abs(Y - Ys) / _band(np.abs(Ys).max(axis=1, keepdims=True))).max()
    print(f"{name}: |Y(sens) - Y(simulate_batch)| / band: {r:.3f}")
    assert r <= C_BAND and np.array_equal(Y[:, 0], Ys[:, 0])
    dY0, Y0, st0, ns0 = eng.simulate_sens_batch(s["X"], s["t"], [], y0=s["y0"], **OPT)
    assert dY0.shape == (3, s["t"].size, eng.S, 0)
    assert np.array_equal(_np(Y0), Ys) and np.array_equal(_np(st0), sts) and np.array_equal(_np(ns0), nss)


@pytest.mark.parametrize("name", ref.NAMES)
def test_columns_order_and_chunks(name, monkeypatch):
    s = _setup(name)
    eng, cols, gold = s["eng"], s["cols"], s["gold"]
    dY = s["main"][0]
    KC = eng.sens_columns_per_launch()
    assert KC >= cols.size                                                          # one chunk on the small fixtures
    # permuting cols permutes dY exactly (K <= KC)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    dYp = _np(eng.simulate_sens_batch(s["X"], s["t"], cols[perm], y0=s["y0"], want_Y=False, **OPT)[0])
    assert np.array_equal(dYp, dY[..., perm])
    # a column alone and as first of several: other steps, same band
    cmax = np.abs(gold["dY"]).max(axis=(1, 2))
    for c in (0, 3):
        alone = _np(eng.simulate_sens_batch(s["X"], s["t"], cols[[c]], y0=s["y0"], want_Y=False, **OPT)[0])[..., 0]
        first = _np(eng.simulate_sens_batch(s["X"], s["t"], np.roll(cols, -c), y0=s["y0"], want_Y=False, **OPT)[0])[..., 0]
        r = (np.abs(alone - first).max(axis=(1, 2)) / _band(cmax[:, c])).max()
        print(f"{name}: column {gold['names'][c]} alone vs first of {cols.size}: {r:.3f} bands")
        assert r <= C_BAND
    # K > KC: three chunks of <= 3 columns, each integrating the state itself; every column stays in its band, status ORs, Y is chunk 0's
    monkeypatch.setenv("PK_NET_SENS_KC", "3")
    assert eng.sens_columns_per_launch() == 3
    dYc, Yc, stc, nsc = eng.simulate_sens_batch(s["X"], s["t"], cols, y0=s["y0"], **OPT)
    monkeypatch.delenv("PK_NET_SENS_KC")
    dY3 = _np(eng.simulate_sens_batch(s["X"], s["t"], cols[:3], y0=s["y0"], **OPT)[0])
    assert not _np(stc).any() and np.array_equal(_np(dYc)[..., :3], dY3)           # chunk 0 = the launch of its three columns alone
    net_ratio, raw_ratio = _ratio(_np(dYc), gold)
    print(f"{name}: three chunks: worst {raw_ratio.max():.3f} bands")
    assert net_ratio.max() <= C_BAND


@pytest.mark.parametrize("name", ["network_m0_small", "network_m2_small"])
def test_raw_batched_y0_and_batch_independence(name):
    s = _setup(name)
    eng, cols = s["eng"], s["cols"]
    dY, Y, st, ns = s["main"]
    # row k of the B = 3 launch equals the B = 1 launch bit for bit
    for k in (0, 2):
        d1, y1, s1, n1 = eng.simulate_sens_batch(s["X"][k], s["t"], cols, y0=s["y0"], **OPT)
        assert np.array_equal(_np(d1)[0], dY[k]) and np.array_equal(_np(y1)[0], Y[k]) and np.array_equal(_np(n1)[0], ns[k]) and not _np(s1).any()
    # batched y0: every row starts from its own initial state
    y0b = s["y0"][None, :] * np.array([1.0, 0.7, 1.3])[:, None]
    db, yb, sb, nb = eng.simulate_sens_batch(s["X"], s["t"], cols, y0=y0b, **OPT)
    assert not _np(sb).any() and np.array_equal(_np(yb)[:, 0], y0b) and np.array_equal(_np(db)[0], dY[0])
    d1 = eng.simulate_sens_batch(s["X"][2], s["t"], cols, y0=y0b[2], want_Y=False, **OPT)[0]
    assert np.array_equal(_np(d1)[0], _np(db)[2])
    # raw = True: d / d raw = d / d physical x softplus'(raw); one raw entry above 20, where softplus is the identity
    x_raw = np.stack([nm.inv_softplus(r) for r in s["X"]])
    x_raw[2, cols[5]] = 25.0
    x_phys = eng.unpack_batch(x_raw)
    dr = _np(eng.simulate_sens_batch(x_raw, s["t"], cols, y0=s["y0"], raw=True, want_Y=False, **OPT)[0])
    dp = _np(eng.simulate_sens_batch(x_phys, s["t"], cols, y0=s["y0"], want_Y=False, **OPT)[0])
    fac = np.where(x_raw[:, cols] > 20.0, 1.0, 1.0 / (1.0 + np.exp(-x_raw[:, cols])))          # [B, K]
    assert fac[2, 5] == 1.0 and np.array_equal(dr[2, ..., 5], dp[2, ..., 5])
    want = dp * fac[:, None, None, :]
    assert (np.abs(dr - want).max(axis=(1, 2)) <= 1e-12 * np.abs(want).max(axis=(1, 2))).all()


def test_nan_parameter_is_flagged_and_neighbours_untouched():
    s = _setup("network_m1_small")
    eng, cols = s["eng"], s["cols"]
    dY, Y, st, ns = s["main"]
    X = s["X"].copy()
    X[1, cols[1]] = np.nan
    d, y, stn, _ = (_np(a) for a in eng.simulate_sens_batch(X, s["t"], cols, y0=s["y0"], **OPT))
    assert stn[1] & 1 and stn[0] == 0 and stn[2] == 0                                 # PK_ST_NONFINITE
    assert np.isnan(d[1]).all() and np.isnan(y[1, 1:]).all() and np.array_equal(y[1, 0], s["y0"])
    for k in (0, 2):
        assert np.array_equal(d[k], dY[k]) and np.array_equal(y[k], Y[k])


def test_refusals_and_argument_errors():
    from phoskintime_amd import _capi
    from phoskintime_amd.global_model import NetworkEngine
    s = _setup("network_m0_small")
    eng, cols = s["eng"], s["cols"]
    for kw in (dict(method="ark"), dict(method="dp5"), dict(kernel="workspace")):
        assert eng.simulate_sens_batch(s["X"], s["t"], cols, y0=s["y0"], **kw) is None
        assert b"PK_METHOD_ROS34PW2" in eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"PK_KERNEL_AUTO" in eng.ctx.lib.pk_last_error(eng.ctx.handle)
    for bad in ([0, eng.n_var], [-1], [3, 5, 3]):
        with pytest.raises(_capi.PhoskinError):
            eng.simulate_sens_batch(s["X"], s["t"], bad, y0=s["y0"])
    # NULL dY with K > 0, straight at the C ABI; B = 0 is PK_OK
    import torch
    dev = torch.device("cuda", eng.ctx.device)
    xd = torch.as_tensor(s["X"], device=dev); yd = torch.as_tensor(s["y0"], device=dev)
    Y = torch.empty((3, s["t"].size, eng.S), dtype=torch.float64, device=dev)
    one = np.array([0], dtype=np.int32)
    opts = _capi.default_opts(rtol=RTOL, atol=ATOL)
    call = lambda B, dY: eng.ctx.lib.pk_network_simulate_sens_batch(eng.ctx.handle, eng._h, B, C.c_void_p(xd.data_ptr()), 0, C.c_void_p(yd.data_ptr()), 0,
                                                                     s["t"].ctypes.data, s["t"].size, C.byref(opts), one.ctypes.data, 1,
                                                                     C.c_void_p(Y.data_ptr()), dY, None, None)
    assert call(3, None) == _capi.PK_ERR_ARG and call(0, C.c_void_p(Y.data_ptr())) == _capi.PK_OK
    # KC >= 1 on every fixture and at BASELINE config 5's size (N = 100, S = 552; host arithmetic, nothing is launched)
    for name in ref.NAMES:
        assert _setup(name)["eng"].sens_columns_per_launch() >= 1
    big = NetworkEngine.from_npz(np.load(ref.GOLDEN / "netlarge_m0.npz"))
    assert (big.N, big.S) == (100, 552) and big.sens_columns_per_launch() == 3
    big.close()


@pytest.mark.parametrize("name", ref.NAMES)
def test_local_sensitivity_batch(name):
    from phoskintime_amd.global_model import sensitivity as gs
    s = _setup(name)
    eng, g, gold, net = s["eng"], s["g"], s["gold"], s["net"]
    t = s["t"]
    params = {k: (g[k][0] if k != "tf_scale" else float(g[k][0])) for k in ref.KINDS}
    vary = [str(n) for n in gold["names"]]
    out = gs.local_sensitivity_batch(eng, params, t, t[t >= 4.0], t, vary=vary, perturbation=0.05, y0=s["y0"], rtol=RTOL, atol=ATOL)
    assert out["names"] == vary and not out["status"].any()
    ld = out["layout"]
    # the host chain against the plain-loop restatement, both on the kernel's own dY (the same launch: bit-equal by batch independence)
    dY, Y = s["main"][0][0], s["main"][1][0]
    pred, dpred = ref.np_dpred(net, ld, Y, dY)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert rel(out["pred"], pred) <= 1e-12
    assert (np.abs(out["dpred"] - dpred).max(axis=0) <= 1e-12 * np.abs(dpred).max(axis=0)).all()
    mets = ref.np_metric_grads(pred, dpred)
    for m, (val, grad) in mets.items():
        assert abs(out["metrics"][m][0] - val) <= 1e-12 * abs(val) and rel(out["metrics"][m][1], grad) <= 1e-12, m
    assert out["Y"] == out["metrics"]["total_signal"][0] and np.array_equal(out["dY"], out["metrics"]["total_signal"][1])
    x = s["X"][0][s["cols"]]
    assert np.allclose(out["elasticity"], x * out["dY"] / out["Y"], rtol=1e-14) and np.allclose(out["scaled"], out["dY"] * 0.1 * x, rtol=1e-12)
    # ... and against the exact reference pushed through the same restatement.  Band: the bands of Y and dY propagated through
    # p = a / c, dp = da / c - a dc / c^2 to first order (a, c = W y at the entry's time and at the baseline; no floor is active here)
    Yr, dYr = gold["Y"][0], gold["dY"][0]
    pred_r, dpred_r = ref.np_dpred(net, ld, Yr, dYr)
    W = gs.observable_weights(eng, ld)
    tY = C_BAND * _band(np.abs(Yr).max(axis=0))                                        # [S]
    tD = C_BAND * _band(np.abs(dYr).max(axis=(0, 1))) + gold["self_err"][0]           # [K]
    t_idx = np.concatenate([ld["t_prot"], ld["t_rna"], ld["t_pho"]]).astype(int)
    b_idx = np.concatenate([np.full(ld["p_prot"].size, ld["prot_base_idx"]), np.full(ld["p_rna"].size, ld["rna_base_idx"]),
                            np.full(ld["p_pho"].size, ld["pho_base_idx"])]).astype(int)
    a, c = np.einsum("os,os->o", W, Yr[t_idx]), np.einsum("os,os->o", W, Yr[b_idx])
    da, dc = np.einsum("os,osk->ok", W, dYr[t_idx]), np.einsum("os,osk->ok", W, dYr[b_idx])
    assert a.min() > 1e-9 and c.min() > 1e-9
    ta = W @ tY; tc = np.where(b_idx == 0, 0.0, ta)                                    # the baseline row 0 is y0 itself: exact
    tda = W.sum(axis=1)[:, None] * tD[None, :]; tdc = np.where((b_idx == 0)[:, None], 0.0, tda)
    tol = (tda / c[:, None] + (a / c ** 2)[:, None] * tdc + (np.abs(da) / c[:, None] ** 2 + 2 * (a / c ** 3)[:, None] * np.abs(dc)) * tc[:, None]
           + np.abs(dc) / c[:, None] ** 2 * ta[:, None])
    r = (np.abs(out["dpred"] - dpred_r) / tol).max()
    print(f"{name}: |dpred - reference| / propagated band: worst {r:.3f}")
    assert r <= 1.0
    for m, (val, grad) in ref.np_metric_grads(pred_r, dpred_r).items():
        # every metric gradient is a weighted sum of dpred rows (weights 1, 1 / n, 2 (p - mean) / n, p / |p|): same weights on the bands,
        # plus the weights' own change with pred (variance, l2_norm) bounded by the band of pred = ta / c + a tc / c^2
        n = pred_r.size
        tp = ta / c + a * tc / c ** 2
        w = {"total_signal": np.ones(n), "mean": np.ones(n) / n, "variance": 2 * np.abs(pred_r - pred_r.mean()) / n,
             "l2_norm": pred_r / np.linalg.norm(pred_r)}[m]
        dw = {"total_signal": 0.0, "mean": 0.0, "variance": 4 * tp.max() / n, "l2_norm": 2 * tp.max() / np.linalg.norm(pred_r)}[m]
        mtol = w @ tol + dw * np.abs(dpred_r).sum(axis=0)
        assert (np.abs(out["metrics"][m][1] - grad) <= mtol).all(), m
