"""GPU: the Sobol' path -- ``pk_sobol_build_batch`` / ``pk_sobol_indices_batch`` (csrc/pk_sobol.hip) under ``sensitivity.sobol``'s device
wrappers, the network driver ``temporal_gsa_batch`` and the per-protein twin ``temporal_sobol_batch``.

Truth for the kernels is ``sobol.analyze`` run in ``np.longdouble`` on the same inputs.  The limit on every index and spread is
max(1e-12, 100 E_ROUND), with E_ROUND the error of the float64 host restatement against the same truth, computed here (3.7e-15 on these
inputs, tests/test_sobol_cpu.py); the floor leaves room for another summation order.  That limit supposes well-conditioned columns, so
every comparison first asserts |mean| / std <= 2e3 on the columns it compares.

Truth for the two drivers is the oracle's own chain (LSODA at 1e-12 for the network, the closed form for the per-protein model) on the
same design rows, pushed through ``sobol.analyze``; the device integrates at rtol 1e-9 / atol 1e-11.  A column that the varied entries
do not reach (a protein without sites or TF input; an observable at the baseline time) holds no signal: where it is not exactly constant
its spread is the integrator's step-size noise (<= 2e-11 in the truth here) and an index is a ratio of two such noises, in the
reference as much as here.  Those columns are told apart by a condition on the TRUTH alone -- std >= 1e-3 is compared, std <= 1e-8 is
not, nothing may lie between -- and the signal columns must include every protein the varied entries reach.

Measured (MI355X): 1.567e-9 (network, ``FIG_NET``) and 4.690e-12 (per-protein, ``FIG_PROT``); each assertion is 10 x its figure and at
most 1e-4, the margin covering the step-size differences between the two integrators."""
from pathlib import Path

import numpy as np
import pytest

import sobol_reference as ref
from oracle import network_models as nm
from oracle import protein_models as pm
from phoskintime_amd.sensitivity import sobol

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
RT_PRED = 1e-13                       # the figure of tests/test_gpu_network_measure.py
CAP = 1e-4
FIG_NET = 1.567e-9                    # worst |ST - ST_ref| of test_network_against_the_reference_chain, measured on the MI355X
FIG_PROT = 4.690e-12                  # worst |index - index_ref| of test_per_protein_twin_against_the_closed_form
KEYS = ("S1", "ST", "S1_conf", "ST_conf", "var")


def _np(a):
    return a.cpu().numpy()


def _handle(N, D):
    """A design handle for ``indices_device`` without building a design."""
    from phoskintime_amd import batch
    return dict(ctx=batch.get_context(None), N=N, D=D)


def _indices(Y, D, counts):
    import torch
    out = sobol.indices_device(_handle(Y.shape[0] // (D + 2), D), torch.as_tensor(Y, device="cuda"), counts)
    return {k: _np(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def limit():
    e = ref.e_round((Y, D, counts) for Y, D, counts, *_ in ref.index_cases())
    print(f"E_ROUND = {e:.2e}")
    return max(1e-12, 100.0 * e)


@pytest.mark.parametrize("N,D", [(5, 3), (8, 1), (4, 70)])
def test_build_is_bit_equal_to_the_host_builder(N, D):
    rng = np.random.default_rng(D)
    lb = rng.uniform(-2.0, 1.0, D)
    problem = {"num_vars": D, "bounds": np.stack([lb, lb + rng.uniform(0.1, 3.0, D)], axis=1).tolist()}
    X, h = sobol.sample_device(problem, N, seed=11)
    assert X.shape == (N * (D + 2), D) and h["N"] == N and h["D"] == D
    np.testing.assert_array_equal(_np(X), sobol.sample(problem, N, seed=11))


@pytest.mark.parametrize("N,D,M", ref.SHAPES)
def test_indices_against_the_longdouble_restatement(N, D, M, limit):
    Y, const = ref.random_outputs(N, D, M)
    assert ref.input_condition(Y, const) <= 2e3
    for R in ref.RESAMPLES:
        counts = sobol.resample_counts(N, R, seed=R) if R else None
        want = sobol.analyze(Y.astype(np.longdouble), D, counts)
        got = _indices(Y, D, counts)
        for k in KEYS if R else ("S1", "ST", "var"):
            w, g = np.asarray(want[k], np.float64), got[k]
            assert g.shape == w.shape, (k, R)
            err = ref.worst(g, want[k])
            print(f"N={N} D={D} M={M} R={R} {k}: worst |device - longdouble| = {err:.2e} (limit {limit:.1e})")
            nan = np.zeros(M, bool)
            if const is not None:
                nan[const] = True
            assert np.array_equal(np.isnan(g), np.broadcast_to(nan, g.shape)), (k, R)        # the constant column, and only it
            assert np.array_equal(np.isnan(w), np.isnan(g)), (k, R)
            assert err <= limit, (k, R, err)


def test_an_entry_does_not_depend_on_the_launch_around_it():
    N, D, M = 8, 5, 257
    Y, _ = ref.random_outputs(N, D, M)
    c17 = sobol.resample_counts(N, 17, seed=17)
    full = _indices(Y, D, c17)
    sub = _indices(np.ascontiguousarray(Y[:, 3:40]), D, c17)
    for k in KEYS:
        np.testing.assert_array_equal(sub[k], full[k][..., 3:40])                              # a column subset
    plain = _indices(Y, D, None)
    for k in ("S1", "ST", "var"):
        np.testing.assert_array_equal(plain[k], full[k])                                       # R = 0 against R = 17
    five, again, five_sub = _indices(Y, D, c17[:5]), _indices(Y, D, c17[:5]), _indices(np.ascontiguousarray(Y[:, 3:40]), D, c17[:5])
    for k in ("S1_conf", "ST_conf"):
        np.testing.assert_array_equal(five[k], again[k])                                       # the first 5 resamples alone, twice
        np.testing.assert_array_equal(five_sub[k], five[k][:, 3:40])
    # ... and those 5 are the same numbers as in the 17: their spread follows from the per-resample values of the host restatement
    want = sobol.analyze(Y.astype(np.longdouble), D, c17[:5])
    assert ref.worst(five["S1_conf"], want["S1_conf"]) <= 1e-12


def test_refusals():
    import torch
    from phoskintime_amd import _capi, batch
    ctx = batch.get_context(None)
    lib, h = ctx.lib, ctx.handle
    N, D, M = 4, 2, 3
    Y = torch.zeros((N * (D + 2), M), dtype=torch.float64, device="cuda")
    c = torch.ones((2, N), dtype=torch.int32, device="cuda")
    o = [torch.zeros((D, M), dtype=torch.float64, device="cuda") for _ in range(4)]
    v = torch.zeros(M, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()
    call = lambda N_, D_, M_, R_, s1, sd1: lib.pk_sobol_indices_batch(h, N_, D_, M_, p(Y), p(c), R_, s1, p(o[1]), sd1, p(o[3]), p(v))
    assert call(N, D, M, 1, p(o[0]), p(o[2])) == _capi.PK_ERR_ARG                               # R = 1
    assert call(N, 0, M, 2, p(o[0]), p(o[2])) == _capi.PK_ERR_ARG                               # D = 0
    assert call(N, D, M, 2, None, p(o[2])) == _capi.PK_ERR_ARG                                  # no S1
    assert call(N, D, M, 2, p(o[0]), None) == _capi.PK_ERR_ARG                                  # R = 2 without S1_sd
    assert b"S1_sd" in lib.pk_last_error(h)
    assert call(N, D, 0, 2, p(o[0]), p(o[2])) == _capi.PK_OK                                    # M = 0
    Y1 = torch.rand((D + 2, M), dtype=torch.float64, device="cuda")
    assert lib.pk_sobol_indices_batch(h, 1, D, M, p(Y1), None, 0, p(o[0]), p(o[1]), None, None, None) == _capi.PK_OK      # N = 1
    assert lib.pk_sobol_build_batch(h, 0, D, p(v), p(v), p(v), p(v), p(v)) == _capi.PK_ERR_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        sobol.indices_device(_handle(N, D), Y, np.ones((1, N), np.int32))


def test_ishigami_end_to_end_on_the_device():
    import torch
    X, h = sobol.sample_device(ref.ISHIGAMI_PROBLEM, 4096, seed=0)
    Yd = torch.sin(X[:, 0]) + 7.0 * torch.sin(X[:, 1]) ** 2 + 0.1 * X[:, 2] ** 4 * torch.sin(X[:, 0])
    r = sobol.indices_device(h, Yd, sobol.resample_counts(4096, 10, seed=0))
    S1, ST = _np(r["S1"]), _np(r["ST"])
    print("ishigami on the device: S1", S1, "ST", ST, "S1_conf", _np(r["S1_conf"]))
    assert S1.shape == (3,) and np.max(np.abs(S1 - ref.ISHIGAMI_S1)) <= 0.01 and np.max(np.abs(ST - ref.ISHIGAMI_ST)) <= 0.01
    assert np.all(_np(r["S1_conf"]) > 0) and np.all(_np(r["S1_conf"]) < 0.1)


# ------------------------------------------------------------------------------------------------ network driver
def _net(name):
    from phoskintime_amd.global_model import NetworkEngine
    g = np.load(GOLDEN / f"{name}.npz")
    params = {k: g[k][1] for k in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")}
    params["tf_scale"] = float(g["tf_scale"][1])
    return g, NetworkEngine.from_npz(g), params


def _conditioned(pred):
    """Columns of pred on which the index limit applies: not constant and |mean| / std <= 2e3."""
    sd = pred.std(axis=0)
    return (pred.max(axis=0) != pred.min(axis=0)) & (np.abs(pred.mean(axis=0)) <= 2e3 * sd)


@pytest.mark.parametrize("name", ["network_m0_small", "network_m2_small"])
def test_network_driver_against_its_own_pred(name, limit):
    from phoskintime_amd.global_model.sensitivity import temporal_gsa_batch
    g, eng, params = _net(name)
    out = temporal_gsa_batch(eng, params, n_samples=16, seed=1, num_resamples=8, return_pred=True)
    T, N, D = 7, eng.N, len(out["names"])
    # (d) the reference's problem: every c_k, then E_i of the proteins that occur as a TF column
    assert out["names"] == [f"c_k_{k}" for k in range(eng.n_K)] + [f"E_i_{i}" for i in np.unique(g["TF_indices"])]
    assert out["param_values"].shape == (16 * (D + 2), D) and not out["status"].any()
    pred = _np(out["pred"])
    assert pred.shape == (16 * (D + 2), N * T)
    # (a) the four outputs are sobol.analyze of the returned pred with the same counts; [T, N_prot, D] <- pred[:, p T + k]
    want = sobol.analyze(pred.astype(np.longdouble), D, sobol.resample_counts(16, 8, 1))
    ok = _conditioned(pred)
    assert ok.sum() >= 2 * (T - 1)
    for k in ("ST", "S1", "ST_conf", "S1_conf"):
        assert out[k].shape == (T, N, D)
        w = np.asarray(want[k], np.float64).reshape(D, N, T).transpose(2, 1, 0)
        mask = ok.reshape(N, T).T
        assert not np.isnan(out[k][mask]).any() and np.isnan(out[k][0]).all(), k
        err = ref.worst(out[k][mask], w[mask])
        print(f"{name} {k}: worst |driver - analyze(pred)| on {int(ok.sum())} conditioned columns = {err:.2e} (limit {limit:.1e})")
        assert err <= limit, k
    for p_, k_ in ((0, 1), (3, 6)):                                       # the layout once more, from single columns
        assert ok[p_ * T + k_]
        np.testing.assert_allclose(out["ST"][k_, p_], np.asarray(sobol.analyze(pred[:, p_ * T + k_], D)["ST"], np.float64), rtol=0, atol=limit)
    # (b) the fold change at t = 0 is exactly 1: NaN there, 0 in the heatmap, which holds no NaN anywhere
    assert np.all(pred[:, 0::T] == 1.0)
    assert np.isnan(out["ST"][0]).all() and np.all(out["heatmap"][0] == 0.0) and not np.isnan(out["heatmap"]).any()
    assert np.all(out["heatmap"] >= 0.0)
    # proteins=: only those rows
    two = temporal_gsa_batch(eng, params, n_samples=16, seed=1, num_resamples=8, proteins=[3, 0])
    np.testing.assert_array_equal(two["ST"], out["ST"][:, [3, 0]])
    # (c) fused and unfused at the same method / kernel
    kw = dict(n_samples=16, seed=1, num_resamples=0, return_pred=True, method="rosw", kernel="lds")
    a, b = temporal_gsa_batch(eng, params, fused=True, **kw), temporal_gsa_batch(eng, params, fused=False, **kw)
    np.testing.assert_array_equal(a["status"], b["status"])
    np.testing.assert_allclose(_np(a["pred"]), _np(b["pred"]), rtol=RT_PRED, atol=0)
    assert np.isnan(a["ST_conf"]).all()
    eng.close()


def _signal_columns(truth):
    sd = truth.std(axis=0)
    sig = sd >= 1e-3
    assert np.all(sig | (sd <= 1e-8)), "a truth column between noise and signal: the partition is not clear-cut"
    return sig


def test_network_against_the_reference_chain():
    """ST of three entries (one c_k, two E_i) on network_m0_small, n_samples = 4 (20 rows), against the oracle's simulate_and_measure at
    1e-12 on the same rows.  Measured worst |ST - ST_ref| over the 18 signal columns at t > 0: 1.567e-9 (FIG_NET); asserted: 10 x that."""
    from phoskintime_amd.global_model.sensitivity import temporal_gsa_batch
    g, eng, params = _net("network_m0_small")
    vary = ["c_k_1", "E_i_0", "E_i_3"]
    out = temporal_gsa_batch(eng, params, vary=vary, n_samples=4, seed=1, num_resamples=0, y0=g["y0"], rtol=1e-9, atol=1e-11)
    assert out["names"] == vary and out["param_values"].shape == (20, 3)
    assert not out["status"].any()                                        # a failed row would replace data by zeros
    net = nm.Network.from_npz(g)
    center = eng.pack_params(*(params[k] for k in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")))
    vidx = [1, eng.n_K + 4 * eng.N + eng.total_sites + 0, eng.n_K + 4 * eng.N + eng.total_sites + 3]
    cuts = np.cumsum([eng.n_K, eng.N, eng.N, eng.N, eng.N, eng.total_sites])
    times = out["times"]
    truth = []
    for row in out["param_values"]:
        x = center.copy(); x[vidx] = row
        fr = nm.simulate_and_measure(net, nm.Params(*np.split(x[:-1], cuts), float(x[-1])), times, [], [], y0=g["y0"], rtol=1e-12, atol=1e-12,
                                     mxstep=500000)
        truth.append(fr["p_fc"])                                          # protein-major, then time: column p T + k
    truth = np.asarray(truth)
    T, N = times.size, eng.N
    sig = _signal_columns(truth).reshape(N, T)
    assert not sig[:, 0].any() and sig[[0, 1, 3], 1:].all()               # the proteins the three entries reach, at every t > 0
    want = np.asarray(sobol.analyze(truth, 3)["ST"]).reshape(3, N, T).transpose(2, 1, 0)
    err = float(np.max(np.abs(out["ST"] - want)[sig.T]))
    print(f"network ST against the reference chain: worst |ST - ST_ref| over {int(sig.sum())} signal columns = {err:.3e}")
    assert np.isnan(out["ST"][0]).all()
    assert err <= min(CAP, 10.0 * FIG_NET)
    eng.close()


def test_per_protein_twin_against_the_closed_form():
    """temporal_sobol_batch("distmod", num_psites = 2, n_samples = 8): 80 rows, flat from the oracle's closed form on the same rows.
    Measured worst |index - index_ref| over S1 and ST on the 48 signal columns: 4.690e-12 (FIG_PROT; the flat itself is 5.7e-6 band widths
    from the closed form); asserted: 10 x that."""
    from phoskintime_amd.sensitivity.analysis import temporal_sobol_batch
    n, t = 2, pm.TIME_POINTS
    popt = np.array([1.2, 0.4, 0.9, 0.3, 0.8, 1.5, 0.25, 0.6])
    y0 = np.ones(pm.n_states(pm.DIST, n))
    out = temporal_sobol_batch("distmod", popt, y0, n, t, perturbation=0.2, n_samples=8, seed=2, num_resamples=6, return_flat=True,
                               rtol=1e-9, atol=1e-11)
    P = popt.size
    X = out["param_values"]
    assert X.shape == (8 * (P + 2), P) and not out["status"].any() and len(out["names"]) == P
    np.testing.assert_array_equal(X, sobol.sample(out["problem"], 8, seed=2))
    assert np.all(X >= popt * 0.8 - 1e-15) and np.all(X <= popt * 1.2 + 1e-15)
    flat = _np(out["flat"])
    truth = np.stack([pm.flatten_observables(pm.DIST, np.clip(pm.solve_exact_lti(pm.DIST, x, y0, n, t), 0, None), n) for x in X])
    assert flat.shape == truth.shape
    band = max(pm.band_error(flat[b], truth[b]) for b in range(X.shape[0]))
    print(f"per-protein flat: band error vs the closed form = {band:.3e}")
    assert band < 0.1
    sig = _signal_columns(truth)
    assert sig.sum() == truth.shape[1] - (1 + n)                          # all but P(t0) and the sites at t0, which are y0
    want = sobol.analyze(truth, P)
    err = 0.0
    for k in ("S1", "ST"):
        assert out[k].shape == (truth.shape[1], P)
        assert np.isnan(out[k][~sig]).all() and np.isnan(out[k + "_conf"][~sig]).all() and np.isfinite(out[k + "_conf"][sig]).all()
        err = max(err, float(np.max(np.abs(out[k] - np.asarray(want[k]).T)[sig])))
    print(f"per-protein indices against the closed form: worst |index - index_ref| = {err:.3e}")
    assert err <= min(CAP, 10.0 * FIG_PROT)
