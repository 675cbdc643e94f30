"""GPU: the order-3 Rosenbrock-W network kernels measure the fold-change observables and reduce them to the scalar Morris metric as they
integrate (net_rosw_solve<MODEL, SCORE_MEASURE>, csrc/pk_network_solve.hpp): ``simulate_measure_batch`` on the general LDS kernel and on
the HBM-workspace kernel, all four topologies, any size, and ``run_sensitivity_batch(fused=True)`` on top of it.

Truth in every case is the trajectory ``simulate_batch`` returns for the same method / kernel / tolerances, pushed through two
independent routes: ``observables_batch`` (net_observables_kernel) and ``_np_pred`` below, a numpy restatement of the fold-change formulas
of the oracle's ``simulate_and_measure``, followed by ``nm.compute_scalar_metric``.

Tolerances.  ``pred``: rtol 1e-13 -- each entry is at most 17 additions and one division of the same operands (17 x 2^-53 ~ 2e-15).
``metric``: rtol 1e-11, the project's figure for a few hundred terms summed in another order (RT of test_gpu_network_fused_rosw.py).  For
the variance that bound holds only while the data are well conditioned, so ``_check`` first asserts sqrt(1 + mean^2 / var) <= 100 on the
numpy ``pred`` of each compared row (a condition on the inputs; 1.04-1.28 on the fixtures' own reference trajectories).  status,
n_steps and the optional trajectory are the same arithmetic as ``simulate_batch`` and must be bit-equal."""
from pathlib import Path

import numpy as np
import pytest

from oracle import network_models as nm

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
RT_PRED = 1e-13
RT = 1e-11
METRICS = ("total_signal", "mean", "variance", "l2_norm")
NAMES = ["network_m0_small", "network_m1_small", "network_m2_small", "network_m4_small"]


def _x(eng, g, k):
    return eng.pack_params(g["c_k"][k], g["A_i"][k], g["B_i"][k], g["C_i"][k], g["D_i"][k], g["Dp_i"][k], g["E_i"][k], g["tf_scale"][k])


def _np(a):
    return a.cpu().numpy()


def _setup(name):
    from phoskintime_amd.global_model import NetworkEngine
    g = np.load(GOLDEN / f"{name}.npz")
    return g, NetworkEngine.from_npz(g)


def _lists(eng, t, t_rna=None):
    """Every protein / site at every time of its modality, rna from t = 4 on (the reference's production shape)."""
    h, ld = eng.make_index_lists(t, t, t[t >= 4.0] if t_rna is None else t_rna, t)
    eng.free_loss(h)
    return ld


def _shuffled(ld, rng):
    """The same entries, each modality in a random order."""
    out = dict(ld)
    for m, keys in (("prot", ("p_prot", "t_prot", "obs_prot", "w_prot")), ("rna", ("p_rna", "t_rna", "obs_rna", "w_rna")),
                    ("pho", ("p_pho", "s_pho", "t_pho", "obs_pho", "w_pho"))):
        perm = rng.permutation(ld["p_" + m].size)
        for k in keys:
            out[k] = np.asarray(ld[k])[perm]
    return out


def _np_pred(eng, Y, ld, eps=1e-12):
    """pred [n_prot + n_rna + n_pho] of one trajectory Y [T, S] in the order of the lists: the formulas of the oracle's
    simulate_and_measure (total = P0 + sites / all 2^ns states; a site of the combinatorial topology = all masks with its bit; floors
    max(., eps) on numerator and baseline; baselines at ld's indices)."""
    oy, ns, comb = eng._keep[0], eng._keep[2], eng.model == 2
    fc = lambda a, c: np.maximum(a, eps) / np.maximum(c, eps)
    out = []
    for i, t in zip(ld["p_prot"], ld["t_prot"]):
        cnt = (1 << int(ns[i])) if comb else 1 + int(ns[i])
        tot = Y[:, oy[i] + 1: oy[i] + 1 + cnt].sum(axis=1)
        out.append(fc(tot[t], tot[ld["prot_base_idx"]]))
    for i, t in zip(ld["p_rna"], ld["t_rna"]):
        out.append(fc(Y[t, oy[i]], Y[ld["rna_base_idx"], oy[i]]))
    for i, j, t in zip(ld["p_pho"], ld["s_pho"], ld["t_pho"]):
        if comb:
            m = np.arange(1 << int(ns[i]))
            sig = Y[:, oy[i] + 1 + m[(m >> j) & 1 == 1]].sum(axis=1)
        else:
            sig = Y[:, oy[i] + 2 + j]
        out.append(fc(sig[t], sig[ld["pho_base_idx"]]))
    return np.asarray(out, dtype=np.float64)


def _np_metric(ld, pred, metric):
    a, b = ld["p_prot"].size, ld["p_prot"].size + ld["p_rna"].size
    return nm.compute_scalar_metric(pred[:a], pred[a:b], pred[b:], metric)


def _check(eng, h, ld, X, t, opt, ok_rows, flagged=(), raw=False, y0=None, metrics=METRICS, want_Y_for="variance"):
    """simulate_measure_batch against simulate_batch -> observables_batch and -> numpy, for the rows ``ok_rows``."""
    n_obs = ld["p_prot"].size + ld["p_rna"].size + ld["p_pho"].size
    Y, st, ns = eng.simulate_batch(X, t, y0=y0, raw=raw, **opt)
    Yn, stn = _np(Y), _np(st)
    assert not stn[list(ok_rows)].any() and all(stn[k] != 0 for k in flagged)
    obs = _np(eng.observables_batch(h, Y, n_obs)) if n_obs else np.zeros((X.shape[0], 0))
    ref = {k: _np_pred(eng, Yn[k], ld) for k in ok_rows}
    for metric in metrics:
        out = eng.simulate_measure_batch(h, X, t, y0=y0, raw=raw, metric=metric, want_pred=True, want_Y=(metric == want_Y_for), **opt)
        assert out is not None
        val, pred, st1, ns1, Y1 = out
        val = _np(val)
        np.testing.assert_array_equal(_np(st1), stn); np.testing.assert_array_equal(_np(ns1), _np(ns))
        if metric == want_Y_for:
            np.testing.assert_array_equal(_np(Y1), Yn)                    # the NaN rows of a flagged candidate included
        else:
            assert Y1 is None
        pred = _np(pred) if n_obs else np.zeros((X.shape[0], 0))
        assert pred.shape == (X.shape[0], n_obs)
        for k in ok_rows:
            np.testing.assert_allclose(pred[k], obs[k], rtol=RT_PRED)
            np.testing.assert_allclose(pred[k], ref[k], rtol=RT_PRED)
            if metric == "variance" and n_obs:
                mu, var = ref[k].mean(), ref[k].var()
                assert var == 0.0 or np.sqrt(1.0 + mu * mu / var) <= 100.0      # well conditioned: the 1e-11 below applies
            np.testing.assert_allclose(val[k], _np_metric(ld, ref[k], metric), rtol=RT)
        for k in flagged:
            assert np.isnan(val[k]) and np.isnan(pred[k]).all()
    return Yn


@pytest.mark.parametrize("kernel", ["lds", "workspace"])
@pytest.mark.parametrize("name", NAMES)
def test_all_topologies_on_both_kernels_against_both_routes(name, kernel):
    g, eng = _setup(name)
    t = g["t_eval"]
    K = g["c_k"].shape[0]
    rng = np.random.default_rng(3)
    X = np.stack([_x(eng, g, k % K) for k in range(6)]) * np.exp(0.3 * rng.standard_normal((6, eng.n_var)))
    X[5, eng.n_K + eng.N: eng.n_K + 2 * eng.N] = np.nan                 # B_i = NaN: this candidate is flagged
    ld = _lists(eng, t)
    assert ld["rna_base_idx"] > 0 and ld["prot_base_idx"] == 0 and ld["pho_base_idx"] == 0
    h = eng.make_loss(ld, t.size)
    opt = dict(rtol=1e-8, atol=1e-8, method="rosw", kernel=kernel)
    _check(eng, h, ld, X, t, opt, ok_rows=range(5), flagged=(5,))
    # raw candidates + batched initial states
    Xraw = np.log(np.expm1(np.maximum(X[:5], 1e-12)))
    y0b = np.tile(g["y0"], (5, 1)) * rng.uniform(0.8, 1.2, size=(5, eng.S))
    _check(eng, h, ld, Xraw, t, opt, ok_rows=range(5), raw=True, y0=y0b)
    # only the metric: neither pred nor Y is allocated or written
    val, pred, _, _, Y = eng.simulate_measure_batch(h, X, t, metric="l2_norm", **opt)
    full = eng.simulate_measure_batch(h, X, t, metric="l2_norm", want_pred=True, want_Y=True, **opt)
    assert pred is None and Y is None
    np.testing.assert_array_equal(_np(val), _np(full[0]))
    eng.free_loss(h); eng.close()


@pytest.mark.parametrize("kernel", ["lds", "workspace"])
def test_edge_shapes(kernel):
    """T = 1 (only the initial row: every fold change is exactly 1), T = 2, an empty batch, a grid with more than 64 landing points (the
    staged stop list), lists with all three modalities empty, and caller lists in a shuffled order (pred comes back in that order)."""
    g, eng = _setup("network_m0_small")
    X = np.stack([_x(eng, g, 0), _x(eng, g, 1)])
    opt = dict(rtol=1e-8, atol=1e-8, method="rosw", kernel=kernel)
    dense = np.concatenate([[0.0], np.unique(np.concatenate([np.logspace(-3, np.log10(960.0), 100), g["t_eval"][1:]]))])
    assert dense.size > 65
    for t in (np.array([0.0]), np.array([0.0, 7.5]), dense):
        ld = _lists(eng, t, t_rna=(t[-1:] if t.size <= 2 else None))
        h = eng.make_loss(ld, t.size)
        n_obs = ld["p_prot"].size + ld["p_rna"].size + ld["p_pho"].size
        _check(eng, h, ld, X, t, opt, ok_rows=range(2))
        if t.size == 1:
            want = dict(total_signal=float(n_obs), mean=1.0, variance=0.0, l2_norm=np.sqrt(n_obs))
            for metric in METRICS:
                val, pred, _, ns, _ = eng.simulate_measure_batch(h, X, t, metric=metric, want_pred=True, **opt)
                assert (_np(pred) == 1.0).all() and not _np(ns).any()
                if metric == "variance":
                    assert (_np(val) == 0.0).all()                      # exactly: Welford on equal values, merged pairwise
                else:
                    np.testing.assert_allclose(_np(val), want[metric], rtol=1e-15)
        empty = eng.simulate_measure_batch(h, np.zeros((0, eng.n_var)), t, want_pred=True, want_Y=True, **opt)
        assert empty is not None and empty[0].shape == (0,) and empty[1].shape == (0, n_obs) and empty[4].shape == (0, t.size, eng.S)
        eng.free_loss(h)
    t = g["t_eval"]
    ld = _lists(eng, t)
    none = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in ld.items()}
    h0 = eng.make_loss(none, t.size)
    for metric in METRICS:
        val, pred, st, _, _ = eng.simulate_measure_batch(h0, X, t, metric=metric, want_pred=True, **opt)
        assert (_np(val) == 0.0).all() and pred.shape == (2, 0) and not _np(st).any()
    eng.free_loss(h0)
    mixed = _shuffled(ld, np.random.default_rng(4))
    assert not np.array_equal(mixed["t_prot"], ld["t_prot"]) and (np.diff(mixed["t_pho"]) < 0).any()
    hs = eng.make_loss(mixed, t.size)
    _check(eng, hs, mixed, X, t, opt, ok_rows=range(2))
    eng.free_loss(hs); eng.close()


def test_persistent_grid_resets_per_candidate():
    """More candidates than workgroups of the persistent workspace grid: a workgroup's second candidate must start from a clean Welford
    triple / partial sum and its own rna baseline.  Rows grid .. grid + 4 repeat rows 0 .. 4 -- row 4 a failing one -- and must come
    back bit-equal, for the variance too."""
    g, eng = _setup("network_m0_small")
    t = g["t_eval"]
    grid = eng.workspace_bytes(10 ** 6) // eng.workspace_bytes(1)
    assert grid >= 5
    B = grid + 5
    rng = np.random.default_rng(9)
    X = _x(eng, g, 0)[None, :] * np.exp(0.2 * rng.standard_normal((B, eng.n_var)))
    X[4, eng.n_K + eng.N: eng.n_K + 2 * eng.N] = np.nan
    X[grid:] = X[:5]
    ld = _lists(eng, t)
    h = eng.make_loss(ld, t.size)
    opt = dict(rtol=1e-5, atol=1e-7, method="rosw", kernel="workspace")
    for metric in ("variance", "total_signal"):
        val, pred, st, ns, _ = eng.simulate_measure_batch(h, X, t, metric=metric, want_pred=True, **opt)
        val, pred, st, ns = _np(val), _np(pred), _np(st), _np(ns)
        assert st[4] != 0 and np.isnan(val[4]) and np.isnan(pred[4]).all() and not st[:4].any() and np.isfinite(val[:4]).all()
        np.testing.assert_array_equal(val[grid:], val[:5]); np.testing.assert_array_equal(pred[grid:], pred[:5])
        np.testing.assert_array_equal(st[grid:], st[:5]); np.testing.assert_array_equal(ns[grid:], ns[:5])
    # ... and a candidate's value does not depend on the batch around it: the first rows alone, bit for bit
    alone = eng.simulate_measure_batch(h, X[:4], t, metric="total_signal", **opt)
    np.testing.assert_array_equal(_np(alone[0]), val[:4])
    eng.free_loss(h); eng.close()


@pytest.mark.parametrize("m", [0, 2])
def test_default_plan_on_a_network_beyond_lds(m):
    """S = 1 050 (distributive) / 1 509 (combinatorial): beyond one workgroup the default plan is the order-3 method on the workspace
    kernel, so the default call measures."""
    from phoskintime_amd.global_model import NetworkEngine, synthetic
    desc = synthetic.make_network(N=300, total_sites=450, n_K=30, n_tf_edges=700, model=m, seed=11, max_sites=4)
    eng = NetworkEngine(**desc)
    assert eng.S > 1024 and eng.resolved_method() == "rosw"
    X = synthetic.random_candidates(desc, 3, seed=2, spread=0.3)
    t = np.array([0.0, 1.0, 4.0, 15.0, 60.0])
    ld = _lists(eng, t)
    h = eng.make_loss(ld, t.size)
    _check(eng, h, ld, X, t, dict(rtol=1e-6, atol=1e-8), ok_rows=range(3), want_Y_for="mean")
    eng.free_loss(h); eng.close()


def test_refusals():
    """The register-resident kernels do not measure: network_m0_small (N = 6, <= 3 sites) plans the thread-per-protein register kernel
    when asked for the order-3 method with kernel "auto", network_m2_small the combinatorial register kernel; the additive and the
    explicit integrator never measure; an rna observation before its baseline cannot be measured in one pass."""
    for name in ("network_m0_small", "network_m2_small"):
        g, eng = _setup(name)
        t = g["t_eval"]
        X = _x(eng, g, 0)[None, :]
        ld = _lists(eng, t)
        h = eng.make_loss(ld, t.size)
        assert eng.resolved_method("rosw") == "rosw"
        assert eng.simulate_measure_batch(h, X, t, method="rosw") is None
        assert "lds" in (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode()
        assert eng.simulate_measure_batch(h, X, t, method="rosw", kernel="lds") is not None
        assert eng.simulate_measure_batch(h, X, t, method="ark") is None
        assert eng.simulate_measure_batch(h, X, t, method="dp5", rtol=1e-5, atol=1e-7) is None
        assert eng.simulate_measure_batch(h, X, t, method="dp5") is None
        with pytest.raises(ValueError):
            eng.simulate_measure_batch(h, X, t, method="rosw", kernel="lds", metric="dynamics")
        eng.free_loss(h)
        early = dict(ld); early["t_rna"] = ld["t_rna"].copy(); early["t_rna"][0] = 0
        h2 = eng.make_loss(early, t.size)
        for kernel in ("lds", "workspace"):
            assert eng.simulate_measure_batch(h2, X, t, method="rosw", kernel=kernel) is None
        eng.free_loss(h2); eng.close()


def test_c_abi_argument_errors():
    """metric_id outside 0..3 and three NULL outputs are argument errors; a grid of another length than the lists' too."""
    import ctypes as C
    from phoskintime_amd import _capi
    from phoskintime_amd.batch import _ptr
    import torch
    g, eng = _setup("network_m0_small")
    t = np.ascontiguousarray(g["t_eval"], dtype=np.float64)
    ld = _lists(eng, t)
    h = eng.make_loss(ld, t.size)
    dev = torch.device("cuda", eng.ctx.device)
    x = torch.as_tensor(_x(eng, g, 0)[None, :], device=dev); y0 = torch.as_tensor(g["y0"], device=dev)
    val = torch.empty(1, dtype=torch.float64, device=dev); st = torch.zeros(1, dtype=torch.int32, device=dev)
    opts = eng._opts("rosw", "lds", rtol=1e-6, atol=1e-8)
    call = lambda T, mid, out: eng.ctx.lib.pk_network_simulate_measure_batch(eng.ctx.handle, eng._h, h, 1, _ptr(x), 0, _ptr(y0), 0, t.ctypes.data, T,
                                                                             C.byref(opts), 1e-12, mid, None, None, out, _ptr(st), None)
    assert call(t.size, 4, _ptr(val)) == _capi.PK_ERR_ARG and call(t.size, -1, _ptr(val)) == _capi.PK_ERR_ARG
    assert call(t.size, 0, None) == _capi.PK_ERR_ARG
    assert call(t.size - 1, 0, _ptr(val)) == _capi.PK_ERR_ARG
    assert call(t.size, 0, _ptr(val)) == _capi.PK_OK
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and np.isfinite(float(val[0]))
    eng.free_loss(h); eng.close()


def test_run_sensitivity_batch_fused_equals_the_three_step_route():
    from phoskintime_amd import _capi
    from phoskintime_amd.global_model.sensitivity import run_sensitivity_batch
    g, eng = _setup("network_m0_small")
    t = g["t_eval"]
    fitted = dict(c_k=g["c_k"][1], A_i=g["A_i"][1], B_i=g["B_i"][1], C_i=g["C_i"][1], D_i=g["D_i"][1], Dp_i=g["Dp_i"][1], E_i=g["E_i"][1],
                  tf_scale=float(g["tf_scale"][1]))
    vary = ["c_k_0", "A_i_1", "D_i_2", "E_i_3", "tf_scale"]
    kw = dict(trajectories=4, num_levels=8, seed=3, vary=vary, return_pred=True, method="rosw", kernel="lds")
    for metric in METRICS:
        a = run_sensitivity_batch(eng, fitted, t, t[t >= 4.0], t, metric=metric, fused=False, **kw)
        b = run_sensitivity_batch(eng, fitted, t, t[t >= 4.0], t, metric=metric, fused=True, **kw)
        assert a["Y"].shape == (4 * 6,) and not a["status"].any()
        np.testing.assert_array_equal(a["status"], b["status"]); np.testing.assert_array_equal(a["param_values"], b["param_values"])
        np.testing.assert_allclose(b["Y"], a["Y"], rtol=RT)
        np.testing.assert_allclose(_np(b["pred"]), _np(a["pred"]), rtol=RT_PRED)
        assert a["mean_steps"] == b["mean_steps"]
        assert set(a["Si"].keys()) == set(b["Si"].keys())
        for k in a["Si"]:
            assert np.shape(a["Si"][k]) == np.shape(b["Si"][k])
    # kernel "auto" at the default method is a plan this launch does not run on: refused with the library's reason, not answered otherwise
    with pytest.raises(_capi.PhoskinError, match="fused"):
        run_sensitivity_batch(eng, fitted, t, t[t >= 4.0], t, fused=True, trajectories=2, vary=vary, seed=3, method="ark")
    eng.close()
