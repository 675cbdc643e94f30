"""GPU: the order-3 Rosenbrock-W network kernels score the three-objective loss as they integrate (net_rosw_solve<MODEL, FUSED = true>,
csrc/pk_network_solve.hpp): ``simulate_objective_batch(..., method="rosw")`` / ``kernel="workspace"`` on the general LDS kernel and on
the HBM-workspace kernel, all four topologies, any size.  Truth: the oracle's ``nm.objectives`` (restated from the reference, pinned by
``pins_network_m*.npz``) on the trajectory ``simulate_batch`` returns for the same method and kernel; the two-launch path
(``simulate_batch`` + ``objective_batch``) is checked against it in the same tests.

Tolerance: rtol = 1e-11 on the sums and objectives, as in test_fused_simulate_objective_equals_the_two_launch_path -- the same
non-negative terms summed in another order (a few hundred terms: relative rounding <= n * 2^-53 ~ 1e-13).  status, n_steps and the
optional trajectory are the same arithmetic and must be bit-equal."""
from pathlib import Path

import numpy as np
import pytest

from oracle import network_models as nm

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
RT = 1e-11
LAM = (1.0, 0.5, 2.0, 0.7)
LAMD = dict(protein=1.0, rna=0.5, phospho=2.0, prior=0.7)


def _x(eng, g, k):
    return eng.pack_params(g["c_k"][k], g["A_i"][k], g["B_i"][k], g["C_i"][k], g["D_i"][k], g["Dp_i"][k], g["E_i"][k], g["tf_scale"][k])


def _np(a):
    return a.cpu().numpy()


def _loss_data(eng, t, rng, t_rna=None):
    """Every protein / site at every time of its modality (rna from t = 4 on: the reference's production shape), random observations
    and weights."""
    lists, ld = eng.make_index_lists(t, t, t[t >= 4.0] if t_rna is None else t_rna, t)
    eng.free_loss(lists)
    for k in ("obs_prot", "obs_rna", "obs_pho"):
        ld[k] = np.abs(1.0 + 0.2 * rng.standard_normal(ld[k].size))
    for k in ("w_prot", "w_rna", "w_pho"):
        ld[k] = rng.uniform(0.5, 2.0, ld[k].size)
    return ld


def _oracle_ld(ld, offset_y, n_sites, model):
    ns = np.asarray(n_sites)
    return dict(ld, prot_map=np.stack([np.asarray(offset_y), (1 << ns) if model == 2 else ns], axis=1))


def _setup(name):
    from phoskintime_amd.global_model import NetworkEngine
    g = np.load(GOLDEN / f"{name}.npz")
    return g, NetworkEngine.from_npz(g)


@pytest.mark.parametrize("kernel", ["lds", "workspace"])
@pytest.mark.parametrize("name", ["network_m0_small", "network_m1_small", "network_m2_small", "network_m4_small"])
def test_all_topologies_on_both_kernels_against_the_oracle_and_the_two_launch_path(name, kernel):
    g, eng = _setup(name)
    model = int(g["model"])
    net = nm.Network.from_npz(g)
    t = g["t_eval"]
    K = g["c_k"].shape[0]
    rng = np.random.default_rng(3)
    X = np.stack([_x(eng, g, k % K) for k in range(6)]) * np.exp(0.3 * rng.standard_normal((6, eng.n_var)))
    X[5, eng.n_K + eng.N: eng.n_K + 2 * eng.N] = np.nan                 # B_i = NaN: this candidate must come back as fail_value
    ld = _loss_data(eng, t, rng)
    assert ld["rna_base_idx"] > 0 and ld["prot_base_idx"] == 0
    ldo = _oracle_ld(ld, g["offset_y"], g["n_sites"], model)
    loss = eng.make_loss(ld, t.size)
    defaults = X[0] * 1.1
    opt = dict(rtol=1e-8, atol=1e-8, method="rosw", kernel=kernel)
    Y, st, ns = eng.simulate_batch(X, t, **opt)
    Yn = _np(Y)
    assert int(st[5]) != 0 and not _np(st)[:5].any()
    for mode in range(8):
        s2, F2 = eng.objective_batch(loss, Y, loss_mode=mode, x=X, defaults=defaults, lambdas=LAM, status=st)
        out = eng.simulate_objective_batch(loss, X, t, loss_mode=mode, defaults=defaults, lambdas=LAM, want_Y=(mode == 0), **opt)
        assert out is not None
        s1, F1, st1, ns1, Y1 = out
        np.testing.assert_array_equal(_np(st1), _np(st)); np.testing.assert_array_equal(_np(ns1), _np(ns))
        np.testing.assert_allclose(_np(s1)[:5], _np(s2)[:5], rtol=RT, equal_nan=True)
        np.testing.assert_allclose(_np(F1), _np(F2), rtol=RT, equal_nan=True)
        assert (_np(F1)[5] == 1e12).all() and (_np(F2)[5] == 1e12).all()
        for k in range(5):
            want = nm.objectives(net, X[k], defaults, Yn[k], ldo, mode, LAMD)
            np.testing.assert_allclose(_np(F1)[k], want, rtol=RT, equal_nan=True)
            np.testing.assert_allclose(_np(F2)[k], want, rtol=RT, equal_nan=True)
        if mode == 0:
            np.testing.assert_array_equal(_np(Y1), Yn)                  # the NaN rows of the flagged candidate included
        else:
            assert Y1 is None
    # no prior term
    _, Fn2 = eng.objective_batch(loss, Y, lambdas=LAM, status=st)
    _, Fn1, _, _, _ = eng.simulate_objective_batch(loss, X, t, lambdas=LAM, **opt)
    np.testing.assert_allclose(_np(Fn1), _np(Fn2), rtol=RT)
    # raw candidates + batched initial states
    Xraw = np.log(np.expm1(np.maximum(X[:5], 1e-12)))
    y0b = np.tile(g["y0"], (5, 1)) * rng.uniform(0.8, 1.2, size=(5, eng.S))
    Yb, stb, nsb = eng.simulate_batch(Xraw, t, y0=y0b, raw=True, **opt)
    _, Fb2 = eng.objective_batch(loss, Yb, x=Xraw, raw=True, defaults=defaults, lambdas=LAM, status=stb)
    _, Fb1, stf, nsf, none = eng.simulate_objective_batch(loss, Xraw, t, y0=y0b, raw=True, defaults=defaults, lambdas=LAM, **opt)
    assert none is None and not _np(stb).any()
    np.testing.assert_array_equal(_np(stf), _np(stb)); np.testing.assert_array_equal(_np(nsf), _np(nsb))
    np.testing.assert_allclose(_np(Fb1), _np(Fb2), rtol=RT)
    Xp = _np(eng.unpack_batch(Xraw))
    for k in range(5):
        np.testing.assert_allclose(_np(Fb1)[k], nm.objectives(net, Xp[k], defaults, _np(Yb)[k], ldo, 0, LAMD), rtol=RT)
    eng.free_loss(loss); eng.close()


def test_what_the_dense_tables_forbade():
    """One (state, time) observed twice is accepted on this path (the lists are scored as lists); an rna observation before its baseline
    still is not: the baseline would not exist yet when the observation's row is scored."""
    g, eng = _setup("network_m0_small")
    t = g["t_eval"]
    rng = np.random.default_rng(5)
    X = np.stack([_x(eng, g, k) for k in range(3)])
    ld = _loss_data(eng, t, rng)
    dup = {k: (np.concatenate([v, v[:1]]) if k.endswith("_prot") and isinstance(v, np.ndarray) else v) for k, v in ld.items()}
    dup["obs_prot"][-1] *= 1.3
    loss = eng.make_loss(dup, t.size)
    net = nm.Network.from_npz(g)
    ldo = _oracle_ld(dup, g["offset_y"], g["n_sites"], 0)
    assert eng.simulate_objective_batch(loss, X, t, rtol=1e-8, atol=1e-8) is None            # the default path: the dense tables
    for kernel in ("lds", "workspace"):
        opt = dict(rtol=1e-8, atol=1e-8, method="rosw", kernel=kernel)
        Y, st, _ = eng.simulate_batch(X, t, **opt)
        s2, F2 = eng.objective_batch(loss, Y, x=X, defaults=X[0] * 1.1, lambdas=LAM, status=st)
        out = eng.simulate_objective_batch(loss, X, t, defaults=X[0] * 1.1, lambdas=LAM, **opt)
        assert out is not None
        np.testing.assert_allclose(_np(out[0]), _np(s2), rtol=RT)
        np.testing.assert_allclose(_np(out[1]), _np(F2), rtol=RT)
        for k in range(3):
            np.testing.assert_allclose(_np(out[1])[k], nm.objectives(net, X[k], X[0] * 1.1, _np(Y)[k], ldo, 0, LAMD), rtol=RT)
    eng.free_loss(loss)
    early = dict(ld); early["t_rna"] = ld["t_rna"].copy(); early["t_rna"][0] = 0
    l2 = eng.make_loss(early, t.size)
    for kernel in ("lds", "workspace"):
        assert eng.simulate_objective_batch(l2, X, t, method="rosw", kernel=kernel) is None
    eng.free_loss(l2); eng.close()


@pytest.mark.parametrize("m", [0, 2])
def test_default_plan_on_a_network_beyond_lds(m):
    """S = 1 050 (distributive) / 1 509 (combinatorial, blocks of up to 16 states) from the same builder call: beyond one workgroup, the
    default plan is the order-3 method on the workspace kernel.  The default call still answers None; on request the launch is fused, and
    GlobalODEBatch asks for it by itself."""
    from phoskintime_amd.global_model import NetworkEngine, synthetic
    from phoskintime_amd.global_model.optproblem import GlobalODEBatch
    desc = synthetic.make_network(N=300, total_sites=450, n_K=30, n_tf_edges=700, model=m, seed=11, max_sites=4)
    eng = NetworkEngine(**desc)
    assert eng.S > 1024 and eng.resolved_method() == "rosw"
    X = synthetic.random_candidates(desc, 3, seed=2, spread=0.3)
    t = np.array([0.0, 1.0, 4.0, 15.0, 60.0])
    rng = np.random.default_rng(m)
    ld = _loss_data(eng, t, rng)
    loss = eng.make_loss(ld, t.size)
    opt = dict(rtol=1e-6, atol=1e-8)
    assert eng.simulate_objective_batch(loss, X, t, **opt) is None
    dflt = synthetic.default_candidate(desc)
    Y, st, ns = eng.simulate_batch(X, t, **opt)
    assert not _np(st).any()
    s2, F2 = eng.objective_batch(loss, Y, x=X, defaults=dflt, lambdas=LAM, status=st)
    out = eng.simulate_objective_batch(loss, X, t, defaults=dflt, lambdas=LAM, method="rosw", **opt)
    assert out is not None
    np.testing.assert_array_equal(_np(out[2]), _np(st)); np.testing.assert_array_equal(_np(out[3]), _np(ns))
    np.testing.assert_allclose(_np(out[0]), _np(s2), rtol=RT)
    np.testing.assert_allclose(_np(out[1]), _np(F2), rtol=RT)
    assert out[4] is None
    eng.free_loss(loss)
    cuts = np.cumsum([eng.n_K, eng.N, eng.N, eng.N, eng.N, eng.total_sites, eng.N])
    parts = np.split(dflt[:-1], cuts[:-1])
    dd = dict(zip(("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i"), parts)); dd["tf_scale"] = float(dflt[-1])
    prob = GlobalODEBatch(eng, None, ld, dd, LAMD, t, **opt)
    Xraw = np.log(np.expm1(X))
    F = _np(prob.evaluate_device(Xraw))
    assert prob.fused is True
    Yr, sr, _ = eng.simulate_batch(Xraw, t, raw=True, max_steps=prob.max_steps * t.size, **opt)
    _, Fr = eng.objective_batch(prob.loss, Yr, x=Xraw, raw=True, defaults=prob.defaults, lambdas=prob.lam, status=sr)
    np.testing.assert_allclose(F, _np(Fr), rtol=RT)
    np.testing.assert_array_equal(_np(prob.evaluate_device(Xraw)), F)     # the cached answer: the same launch again
    prob.close(); eng.close()


def test_persistent_grid_resets_per_candidate():
    """More candidates than workgroups of the persistent workspace grid: a workgroup's second candidate must start from clean partial
    sums, rna baseline and non-finite flag.  Rows grid .. grid + 4 repeat rows 0 .. 4 -- row 4 a failing one -- and must come back
    bit-equal."""
    g, eng = _setup("network_m0_small")
    t = g["t_eval"]
    grid = eng.workspace_bytes(10 ** 6) // eng.workspace_bytes(1)
    assert grid >= 5
    B = grid + 5
    rng = np.random.default_rng(9)
    base = _x(eng, g, 0)
    X = base[None, :] * np.exp(0.2 * rng.standard_normal((B, eng.n_var)))
    X[4, eng.n_K + eng.N: eng.n_K + 2 * eng.N] = np.nan
    X[grid:] = X[:5]
    ld = _loss_data(eng, t, rng)
    loss = eng.make_loss(ld, t.size)
    opt = dict(rtol=1e-5, atol=1e-7, method="rosw", kernel="workspace")
    s1, F1, st1, ns1, _ = eng.simulate_objective_batch(loss, X, t, defaults=base, lambdas=LAM, **opt)
    s1, F1, st1, ns1 = _np(s1), _np(F1), _np(st1), _np(ns1)
    assert st1[4] != 0 and (F1[4] == 1e12).all() and not st1[:4].any() and np.isfinite(F1[:4]).all()
    np.testing.assert_array_equal(F1[grid:], F1[:5])
    np.testing.assert_array_equal(s1[grid:grid + 4], s1[:4])
    np.testing.assert_array_equal(st1[grid:], st1[:5]); np.testing.assert_array_equal(ns1[grid:], ns1[:5])
    # ... and the whole batch against the two-launch path
    Y, st, ns = eng.simulate_batch(X, t, **opt)
    _, F2 = eng.objective_batch(loss, Y, x=X, defaults=base, lambdas=LAM, status=st)
    np.testing.assert_array_equal(st1, _np(st)); np.testing.assert_array_equal(ns1, _np(ns))
    np.testing.assert_allclose(F1, _np(F2), rtol=RT)
    eng.free_loss(loss); eng.close()


@pytest.mark.parametrize("kernel", ["lds", "workspace"])
def test_edge_shapes(kernel):
    """One candidate on the shortest grids -- T = 1 (only the initial row: every fold change is 1) and T = 2 --, an empty batch, and a
    grid with more than 64 landing points (the staged stop list); no trajectory is asked for anywhere."""
    g, eng = _setup("network_m0_small")
    X = _x(eng, g, 0)[None, :]
    opt = dict(rtol=1e-8, atol=1e-8, method="rosw", kernel=kernel)
    lam = (1.0, 1.0, 1.0, 0.5)
    dense = np.concatenate([[0.0], np.unique(np.concatenate([np.logspace(-3, np.log10(960.0), 100), g["t_eval"][1:]]))])
    assert dense.size > 65
    for t in (np.array([0.0]), np.array([0.0, 7.5]), dense):
        rng = np.random.default_rng(0)
        ld = _loss_data(eng, t, rng, t_rna=(t[-1:] if t.size <= 2 else None))
        loss = eng.make_loss(ld, t.size)
        Y, st, ns = eng.simulate_batch(X, t, **opt)
        s2, F2 = eng.objective_batch(loss, Y, x=X, defaults=X[0], lambdas=lam, status=st)
        out = eng.simulate_objective_batch(loss, X, t, defaults=X[0], lambdas=lam, **opt)
        assert out is not None and out[4] is None
        np.testing.assert_array_equal(_np(out[2]), _np(st)); np.testing.assert_array_equal(_np(out[3]), _np(ns))
        np.testing.assert_allclose(_np(out[0]), _np(s2), rtol=RT)
        np.testing.assert_allclose(_np(out[1]), _np(F2), rtol=RT)
        if t.size == 1:                                                   # pred = 1 everywhere: the sums are the squared distances of the observations from 1
            want = [float(np.sum(ld["w_" + m] * (ld["obs_" + m] - 1.0) ** 2)) for m in ("prot", "rna", "pho")]
            assert ld["rna_base_idx"] == 0 and not _np(ns).any()
            np.testing.assert_allclose(_np(out[0])[0], want, rtol=1e-12)
        empty = eng.simulate_objective_batch(loss, np.zeros((0, eng.n_var)), t, **opt)
        assert empty is not None and empty[1].shape == (0, 3)
        eng.free_loss(loss)
    eng.close()


def test_refusals():
    """The register-resident kernels do not score: network_m0_small (N = 6, <= 3 sites) plans the thread-per-protein register kernel
    when asked for the order-3 method with kernel "auto", network_m2_small (<= 3 sites) the combinatorial register kernel; the explicit
    integrator never scores."""
    for name in ("network_m0_small", "network_m2_small"):
        g, eng = _setup(name)
        t = g["t_eval"]
        X = _x(eng, g, 0)[None, :]
        ld = _loss_data(eng, t, np.random.default_rng(1))
        loss = eng.make_loss(ld, t.size)
        assert eng.resolved_method("rosw") == "rosw"
        assert eng.simulate_objective_batch(loss, X, t, method="rosw") is None
        assert "lds" in (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode()
        assert eng.simulate_objective_batch(loss, X, t, method="rosw", kernel="lds") is not None
        assert eng.simulate_objective_batch(loss, X, t, method="dp5", rtol=1e-5, atol=1e-7) is None
        assert eng.simulate_objective_batch(loss, X, t, method="dp5", kernel="workspace", rtol=1e-5, atol=1e-7) is None
        with pytest.raises(ValueError):
            eng.simulate_objective_batch(loss, X, t, method="bdf")
        eng.free_loss(loss); eng.close()


_ARENA_SCRIPT = r"""
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1])
from phoskintime_amd.global_model import NetworkEngine
g = np.load(sys.argv[1] + "/tests/golden/network_m0_small.npz")
eng = NetworkEngine.from_npz(g)
x = eng.pack_params(*(g[k][0] for k in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")))
X = np.repeat(x[None, :], 8, axis=0)
Y, st, _ = eng.simulate_batch(X, g["t_eval"], rtol=1e-5, atol=1e-7, kernel="workspace")
ok = bool(np.isfinite(Y.cpu().numpy()).all() and not st.cpu().numpy().any())
print(json.dumps({"ws": eng.workspace_bytes(8), "ok": ok, "stats": eng.ctx.workspace_stats()}))
"""


def test_workspace_bytes_is_the_plain_slab_before_and_after_a_fused_launch():
    """The N extra doubles belong to fused launches alone: ``workspace_bytes`` reports the plain slab whatever ran before."""
    g, eng = _setup("network_m0_small")
    t = g["t_eval"]
    X = np.stack([_x(eng, g, k) for k in range(2)])
    before = [eng.workspace_bytes(B) for B in (1, 8, 10 ** 6)]
    ld = _loss_data(eng, t, np.random.default_rng(2))
    loss = eng.make_loss(ld, t.size)
    assert eng.simulate_objective_batch(loss, X, t, method="rosw", kernel="workspace") is not None
    assert [eng.workspace_bytes(B) for B in (1, 8, 10 ** 6)] == before
    slab = 8 * (eng.n_var + 8 * eng.S + eng.n_K + eng.total_sites + 6 * eng.N)
    assert before[0] == (slab + 127) // 128 * 128
    eng.free_loss(loss); eng.close()


def test_plain_workspace_simulate_takes_the_arena_it_took():
    """A plain workspace simulate in a fresh process (so the context's arena holds nothing else) takes grid x slab plus the arena's growth
    slack, as test_workspace_is_bounded_in_the_batch states it.  (Passes with and without the fused kernels: that is its point.)"""
    import json, subprocess, sys
    root = str(Path(__file__).resolve().parents[1])
    r = subprocess.run([sys.executable, "-c", _ARENA_SCRIPT, root], check=True, capture_output=True, text=True, timeout=300)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["ws"] > 0 and out["ws"] % 128 == 0
    assert out["stats"]["scratch_allocs"] == 1 and out["stats"]["scratch_bytes"] == out["ws"] + out["ws"] // 2 + (64 << 10)
