"""GPU: the network entry points of the C ABI answer what the plan table of tests/test_net_plan_cpu.py predicts for the facts of three
networks -- i.e. pk_network.hip tells net_plan (csrc/pk_net_plan.hpp) the right numbers about a network and launches what it is told.

  m0    tests/golden/network_m0_small: arrow topology, 6 proteins, <= 3 sites -- every one-workgroup kernel fits, the dense lanes too
  m2    tests/golden/network_m2_small: combinatorial topology, 6 proteins, <= 3 sites -- the register kernel of that topology
  big   synthetic, 260 proteins, S = 1 040: beyond the one-workgroup kernels (S > 1024, N > 256) -- workspace kernel and slab tangents

Each flavour is called with B = 2, T = 3 and two tangent columns.  Asserted: the return code, the text of pk_last_error, what
pk_network_resolve_method says for the same options, and for accepted launches finite outputs and status == 0."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import net_objgrad_reference as og
import net_sens_reference as ref
import test_net_plan_cpu as tbl

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED = 0, -2
T_EVAL = np.array([0.0, 4.0, 8.0])
B, K = 2, 2
_CACHE = {}


def _setup(name):
    if name not in _CACHE:
        import torch
        from phoskintime_amd.global_model import NetworkEngine, synthetic
        if name == "big":
            net = synthetic.make_network(N=260, total_sites=520, n_K=20, n_tf_edges=300, model=0)
            eng = NetworkEngine(**net)
        else:
            net = np.load(ref.GOLDEN / f"network_{name}_small.npz")
            eng = NetworkEngine.from_npz(net)
        dev = torch.device("cuda", eng.ctx.device)
        ld = og.loss_data(SimpleNamespace(N=eng.N, n_sites=np.asarray(net["n_sites"])), T_EVAL)
        s = SimpleNamespace(eng=eng, dev=dev, loss=eng.make_loss(ld, T_EVAL.size),
                            x=torch.as_tensor(synthetic.random_candidates(net, B, seed=1, spread=0.1), device=dev),
                            y0=torch.as_tensor(eng.default_y0(), device=dev), cols=np.array([0, eng.n_var - 1], np.int32))
        s.n_obs = eng._n_obs[s.loss]
        _CACHE[name] = s
    return _CACHE[name]


def _call(s, flavour, method=None, kernel="auto"):
    """One call of the flavour's entry point -> (rc, pk_last_error text, the outputs that must be finite, status)."""
    import torch
    from phoskintime_amd import _capi
    eng, lib, h = s.eng, s.eng.ctx.lib, s.eng.ctx.handle
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=s.dev)
    opts = eng._opts(method or "auto", kernel, rtol=1e-6, atol=1e-8)
    status = torch.full((B,), -1, dtype=torch.int32, device=s.dev)
    nsteps = torch.zeros((B, 2), dtype=torch.int32, device=s.dev)
    lam = (C.c_double * 4)(1.0, 1.0, 1.0, 0.0)
    head = (B, p(s.x), 0, p(s.y0), 0, T_EVAL.ctypes.data, T_EVAL.size, C.byref(opts))
    Y, F, sums = new(B, T_EVAL.size, eng.S), new(B, 3), new(B, 3)
    eng.ctx.set_stream(torch.cuda.current_stream(s.dev).cuda_stream)
    if flavour == "plain":
        out = [Y]
        rc = lib.pk_network_simulate_batch(h, eng._h, *head, p(Y), p(status), p(nsteps))
    elif flavour == "objective":
        out = [F, sums]
        rc = lib.pk_network_simulate_objective_batch(h, eng._h, s.loss, *head, 0, None, C.cast(lam, C.c_void_p), 1e12, None, p(status), p(nsteps), p(sums), p(F))
    elif flavour == "measure":
        out = [new(B, s.n_obs), new(B)]
        rc = lib.pk_network_simulate_measure_batch(h, eng._h, s.loss, *head, 1e-12, 0, None, p(out[0]), p(out[1]), p(status), p(nsteps))
    elif flavour == "sens":
        out = [Y, new(B, T_EVAL.size, eng.S, K)]
        rc = lib.pk_network_simulate_sens_batch(h, eng._h, *head, s.cols.ctypes.data, K, p(Y), p(out[1]), p(status), p(nsteps))
    else:
        out = [F, sums, new(B, 3, K), new(B, 3, K)]
        rc = lib.pk_network_simulate_objective_grad_batch(h, eng._h, s.loss, *head, s.cols.ctypes.data, K, 0, None, C.cast(lam, C.c_void_p), 1e12, None, None,
                                                          None, None, p(sums), p(out[3]), p(F), p(out[2]), p(status), p(nsteps))
    msg = (lib.pk_last_error(h) or b"").decode() if rc else ""
    torch.cuda.synchronize(s.dev)
    return rc, msg, [o.cpu().numpy() for o in out], status.cpu().numpy()


LDS = dict(method="rosw", kernel="lds")
WS = dict(kernel="workspace")
# (flavour, options) -> the refusal text, or None for an accepted launch.  Read off the table for: m0 -- ArkPair by default (the scoring
# dense-lane kernel), Reg for "rosw", Lds on request; m2 -- Ark by default, CombReg for "rosw"; big -- Workspace whatever is asked, DP5
# and ARK436 refused by size, no tangent column in LDS
COMMON = [("plain", dict(kernel="hbm"), tbl.HBM_ELSEWHERE), ("objective", dict(method="rosw", kernel="hbm"), tbl.HBM_ELSEWHERE),
          ("measure", dict(kernel="hbm"), tbl.HBM_ELSEWHERE),
          ("plain", dict(method="dp5", **WS), tbl.DP5_WORKSPACE), ("plain", dict(method="ark", **WS), tbl.ARK_WORKSPACE),
          ("plain", WS, None), ("objective", WS, None), ("measure", WS, None), ("sens", {}, None), ("sens", dict(kernel="hbm"), None),
          ("grad", {}, None), ("grad", dict(kernel="hbm"), None),
          ("sens", dict(method="ark"), tbl.SENS_METHOD[tbl.SENS]), ("sens", dict(method="dp5"), tbl.SENS_METHOD[tbl.SENS]), ("sens", WS, tbl.SENS_WORKSPACE[tbl.SENS]),
          ("grad", dict(method="ark"), tbl.SENS_METHOD[tbl.SENS_SCORE]), ("grad", dict(method="dp5"), tbl.SENS_METHOD[tbl.SENS_SCORE]),
          ("grad", WS, tbl.SENS_WORKSPACE[tbl.SENS_SCORE])]
SMALL = [("plain", {}, None), ("plain", dict(method="rosw"), None), ("plain", LDS, None), ("plain", dict(method="dp5"), None), ("plain", dict(method="ark"), None),
         ("plain", dict(method="ark", kernel="lds"), tbl.ARK_FITS), ("objective", dict(method="rosw"), tbl.LISTS_REG), ("objective", LDS, None),
         ("measure", {}, tbl.MEASURE_ORDER3), ("measure", dict(method="dp5"), tbl.MEASURE_ORDER3), ("measure", dict(method="rosw"), tbl.MEASURE_REG), ("measure", LDS, None)]
# a loss handle of the combinatorial topology holds no dense tables: the entry point says so before it plans
NO_TABLES = ("fused objective: protein / phospho baselines must be time index 0, rna observations not earlier than "
             "the rna baseline, and no (state, time) observed twice")
CASES = {"m0": COMMON + SMALL + [("objective", {}, None), ("objective", dict(kernel="hbm"), tbl.HBM_ELSEWHERE),("objective", dict(kernel="lds"), tbl.TABLES_DENSE), ("objective", dict(method="dp5"), tbl.TABLES_DENSE)],
         "m2": COMMON + SMALL + [("objective", {}, NO_TABLES), ("objective", dict(method="dp5"), NO_TABLES)],
         "big": COMMON + [("plain", {}, None), ("plain", LDS, None), ("plain", dict(method="ark"), tbl.ARK_WORKSPACE), ("plain", dict(method="dp5"), tbl.DP5_SIZE),
                          ("objective", {}, tbl.TABLES_DENSE), ("objective", LDS, None), ("measure", {}, None), ("measure", LDS, None)]}
ARK, ROSW, DP5 = tbl.ARK436, tbl.ROS34PW2, tbl.DP5
# pk_network_resolve_method for (method, kernel): the plain plan's method; of a refused plan PK_ERR_UNSUPPORTED, except DP5 refused by size
RESOLVE = {"m0": {("auto", "auto"): ARK, ("ark", "auto"): ARK, ("rosw", "auto"): ROSW, ("dp5", "auto"): DP5, ("auto", "lds"): ROSW, ("ark", "lds"): UNSUPPORTED,
                  ("auto", "workspace"): ROSW, ("ark", "workspace"): UNSUPPORTED, ("dp5", "workspace"): UNSUPPORTED, ("auto", "hbm"): UNSUPPORTED}}
RESOLVE["m2"] = RESOLVE["m0"]
RESOLVE["big"] = {**RESOLVE["m0"], ("auto", "auto"): ROSW, ("ark", "auto"): UNSUPPORTED, ("dp5", "auto"): DP5}


@pytest.mark.parametrize("name", ("m0", "m2", "big"))
def test_entry_points_answer_what_the_plan_table_predicts(name):
    s = _setup(name)
    eng = s.eng
    lds_route = name != "big"
    assert (eng.S > 1024) == (name == "big") and (eng.sens_columns_per_launch() >= 1) == lds_route and (eng.objective_grad_columns_per_launch() >= 1) == lds_route
    assert eng.sens_hbm_columns(K) == K and eng.sens_hbm_columns(40, True) == 16
    lib = eng.ctx.lib
    for (method, kernel), want in RESOLVE[name].items():
        assert lib.pk_network_resolve_method(eng._h, C.byref(eng._opts(method, kernel))) == want, (method, kernel)
    assert lib.pk_network_resolve_method(eng._h, None) == RESOLVE[name][("auto", "auto")]
    for flavour, kw, refusal in CASES[name]:
        rc, msg, out, status = _call(s, flavour, **kw)
        what = (name, flavour, kw, rc, msg)
        if refusal is not None:
            assert (rc, msg) == (UNSUPPORTED, refusal), what
            assert all(np.isnan(o).all() for o in out) and (status == -1).all(), what          # a refused call launches nothing
        else:
            assert (rc, msg) == (OK, ""), what
            assert all(np.isfinite(o).all() for o in out) and not status.any(), what
