"""GPU: every network integrator kernel but the explicit DP5 one, held step for step to the numpy restatement of
tests/net_step_reference.py (pinned by tests/test_net_step_reference_cpu.py).

a. Forced grid.  rtol = atol = TOL with h0 = 1e9: the kernel takes exactly one step per stop (n_steps proves it on every candidate: the
   restatement's own error norm is <= 0.5 there, FORCED_WORST), and every stop is an output row.  Each row k >= 1 of a compared candidate is
   held to ONE long-double step of the restatement taken from the kernel's own row k - 1, with the route's operator (the exact block, or
   the approximate factorisation), in units of tau = 2^-53 |majorant|_inf.  A coefficient wrong in its 12th digit, a frozen factor taken at
   the wrong state or the wrong operator moves that ratio by orders of magnitude (the commit that added this file lists them).
b. Free running.  The four reference-run networks at rtol = atol = 1e-8: accepted and rejected steps within 2 of the restatement's loop,
   band error against LSODA at 1e-12 under the 0.5 of tests/test_gpu_network.py.
c. Failure exits of the one-thread-per-protein kernels (routes rosw, pair0, sgs, and default on topology 2), on the same free-running
   grid with the three golden candidates: a NaN parameter flags its candidate alone, and a step budget of half candidate 0's count leaves
   the rows reached before the exit as they were and NaN after it.

Routes (what net_state_plan resolves them to on these networks is held by tests/test_net_plan_cpu.py; here resolved_method is asserted):

    default                          ArkPair on the register diet (topologies 0 / 1 / 4), ark2 exact (topology 2, <= 3 sites),
                                     the general LDS kernel with the order-3 method (topology 2, 4 sites)
    method="rosw"                    Reg <MODEL, 4 | 6 | 8>, CombReg <2 | 3>, Lds (topology 2, 4 sites)
    method="rosw", kernel="lds"      Lds (64 threads; 256 on the 70-protein network)
    kernel="workspace"               Workspace
    child, PK_ARK_PAIR=0             Ark <MODEL, 4 | 6 | 8>: one thread per protein
    child, PK_ARK_PAIR=1             ArkPair out of registers (bit-identical to the register diet)
    child, PK_ARK2_EXACT=0           ark2 <2 | 3> on the approximate factorisation

Worst ratio |y_gpu - y_ref|_inf / tau measured on the MI355X per route and method over every network and compared candidate, and the bound
C = 4 x that, rounded up to a power of two (the margin: net_rcp is a Newton-refined reciprocal, site sums run in another order per
layout).  The condition of the construction is that no ratio lies above 64 x R64 of the restatement (net_step_reference.R64: 0.5, and
0.25 for the order-4 method on the approximate factorisation), i.e. above 32 resp. 16:

    route       method   kernels                                   measured    C
    default     ark      ArkPair (diet), ark2 exact                   0.445    2
    default     rosw     Lds (topology 2, 4 sites)                    0.399    2
    rosw        rosw     Reg, CombReg, Lds                            0.549    4
    rosw_lds    rosw     Lds                                          0.662    4
    workspace   rosw     Workspace                                    0.662    4
    pair0       ark      Ark                                          0.445    2
    pair1       ark      ArkPair (registers)                          0.445    2
    sgs         ark      ark2 on the approximate factorisation        0.129    1

(the restatement in double against itself in long double: 0.40 / 0.43 / 0.30 / 0.14 for rosw exact / ark exact / rosw SGS / ark SGS.)
The 70-protein network compares 2 candidates, the others 3.  The free runs stop at the eighth output time of the reference-run grids
(t = 15: 100-300 steps of the order-4 method, 700-1 300 of the order-3 one), which keeps the restatement's loop to seconds.
"""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import net_step_reference as nr
from oracle import network_models as nm

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ROUTES = {"default": {}, "rosw": dict(method="rosw"), "rosw_lds": dict(method="rosw", kernel="lds"), "workspace": dict(kernel="workspace")}
#: child processes: the switch, and the networks on which it changes the kernel
CHILDREN = {"pair0": ({"PK_ARK_PAIR": "0"}, (0, 1, 4)), "pair1": ({"PK_ARK_PAIR": "1"}, (0, 1, 4)), "sgs": ({"PK_ARK2_EXACT": "0"}, (2,))}
TAGS = nr.GOLDEN_SMALL + tuple(s[0] for s in nr.SYNTHETIC)
FREE_TOL = 1e-8

FREE_ROWS = 8
#: (route, method) -> C of the table above
C = {("default", "ark"): 2, ("default", "rosw"): 2, ("rosw", "rosw"): 4, ("rosw_lds", "rosw"): 4, ("workspace", "rosw"): 4, ("pair0", "ark"): 2,
     ("pair1", "ark"): 2, ("sgs", "ark"): 1}


@functools.lru_cache(maxsize=None)
def _case(tag):
    return nr.case(tag)


def _model(tag):
    return int(tag[9]) if tag.startswith("network_m") else int(tag[1])


def _ark_fits(tag):
    return _model(tag) != 2 or int(_case(tag)[1].n_sites.max()) <= 3


def expected(tag, route):
    """(method, operator) the route runs on this network."""
    comb = _model(tag) == 2
    if route in ("default", "pair0", "pair1", "sgs") and _ark_fits(tag):
        return "ark", "sgs" if route == "sgs" else "exact"
    return "rosw", "sgs" if comb else "exact"


def _golden_x(eng, g, k):
    return eng.pack_params(g["c_k"][k], g["A_i"][k], g["B_i"][k], g["C_i"][k], g["D_i"][k], g["Dp_i"][k], g["E_i"][k], g["tf_scale"][k])


def failure_exits(eng, g, kw):
    """The three golden candidates on the free-running grid, three times: as they are ("clean"), with a NaN in candidate 1's first A_i
    ("nan"), and on a step budget of half the accepted + rejected steps candidate 0 took in the clean run ("max")."""
    X = np.stack([_golden_x(eng, g, k) for k in (0, 1, 2)])
    Xn = X.copy()
    Xn[1, np.size(g["c_k"][1])] = np.nan                                          # pack_params order: c_k, then A_i
    run = lambda x, **o: [v.cpu().numpy() for v in eng.simulate_batch(x, g["t_eval"][:FREE_ROWS], y0=g["y0"], rtol=FREE_TOL, atol=FREE_TOL, **kw, **o)]
    clean = run(X)
    runs = {"clean": clean, "nan": run(Xn), "max": run(X, max_steps=int(clean[2][0].sum()) // 2)}
    return {name + k: v for name, r in runs.items() for k, v in zip(("Y", "st", "ns"), r)}


def run_routes(out_path, routes, models):
    """Every network of `models` through every route of `routes`, forced grid (all) and free running (the reference-run networks), into
    one .npz.  Runs in this process or, for the switches that are read once per process, in a child."""
    from phoskintime_amd.global_model import NetworkEngine
    out = {}
    for tag in TAGS:
        if _model(tag) not in models:
            continue
        desc, net, X, y0, t = _case(tag)
        eng = NetworkEngine(**desc)
        for route in routes:
            kw = ROUTES[route]
            out["%s/%s/method" % (route, tag)] = np.array(eng.resolved_method(kw.get("method", "auto"), kw.get("kernel", "auto")))
            Y, st, ns = eng.simulate_batch(X, t, y0=y0, rtol=nr.TOL, atol=nr.TOL, h0=nr.H0, **kw)
            for k, v in (("Y", Y), ("st", st), ("ns", ns)):
                out["%s/%s/%s" % (route, tag, k)] = v.cpu().numpy()
            if tag in nr.GOLDEN_SMALL:
                g = np.load(nr.GOLDEN / (tag + ".npz"))
                Xg = np.stack([_golden_x(eng, g, k) for k in (0, 1)])
                Y, st, ns = eng.simulate_batch(Xg, g["t_eval"][:FREE_ROWS], y0=g["y0"], rtol=FREE_TOL, atol=FREE_TOL, **kw)
                for k, v in (("freeY", Y), ("freest", st), ("freens", ns)):
                    out["%s/%s/%s" % (route, tag, k)] = v.cpu().numpy()
                for k, v in failure_exits(eng, g, kw).items():
                    out["%s/%s/%s" % (route, tag, k)] = v
        eng.close()
    np.savez(out_path, **out)


_CHILD = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import test_gpu_network_steps as m; m.run_routes(sys.argv[2], ('default',), tuple(int(v) for v in sys.argv[3].split(',')))"


def collect(directory):
    """{route: arrays}: the four routes of this process, then one child per switch, one after another."""
    directory = Path(directory)
    run_routes(directory / "base.npz", tuple(ROUTES), (0, 1, 2, 4))
    data = {}
    base = np.load(directory / "base.npz")
    for route in ROUTES:
        data[route] = {k[len(route) + 1:]: base[k] for k in base.files if k.startswith(route + "/")}
    for name, (env, models) in CHILDREN.items():
        f = directory / (name + ".npz")
        subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), str(f), ",".join(str(m) for m in models)], check=True, env={**os.environ, **env}, timeout=300)
        z = np.load(f)
        data[name] = {k[len("default/"):]: z[k] for k in z.files}
    return data


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return collect(tmp_path_factory.mktemp("net_steps"))


def routes_of(tag):
    return tuple(ROUTES) + tuple(name for name, (_, models) in CHILDREN.items() if _model(tag) in models and _ark_fits(tag))


_worst = {}
_seen = {}


def forced_ratios(data, tag, route, compared):
    """Worst |y_gpu - y_ref|_inf / tau of the route's rows on this network, after the structural assertions.  Routes that wrote the same
    bits (the two pair kernels; often the LDS and the workspace kernel) share one evaluation of the reference."""
    desc, net, X, y0, t = _case(tag)
    d = data[route]
    method, operator = expected(tag, route)
    assert str(d[tag + "/method"]) == method, (tag, route)
    Y, st, ns = d[tag + "/Y"], d[tag + "/st"], d[tag + "/ns"]
    n_stops = len(nr.stops_of(net, t))
    assert n_stops == t.size - 1                                                 # every stop is an output row
    assert not st.any() and (ns == np.array([n_stops, 0])).all(), (tag, route, st, ns)      # one accepted step per row, on all B candidates
    assert Y.shape == (nr.B, t.size, net.S) and np.isfinite(Y).all()
    assert (Y[:, 0].view(np.uint64) == np.ascontiguousarray(y0).view(np.uint64)).all()          # row 0 is y0, bit for bit
    key = (tag, method, operator, compared, Y[list(compared)].tobytes())
    if key not in _seen:
        worst = (0.0, None, None)
        for c in compared:
            p = nr.params_of(net, X[c])
            for k in range(1, t.size):
                yref, tau = nr.step_reference(method, operator, net, p, Y[c], t, k)
                ratio = float(np.max(np.abs(Y[c, k] - np.asarray(yref, float)))) / tau
                if not ratio <= worst[0]:
                    worst = (ratio, c, k)
        _seen[key] = worst
    ratio, c, k = _seen[key]
    if not ratio <= _worst.get((route, method), (0.0,))[0]:
        _worst[route, method] = (ratio, tag, c, k)
    return ratio


@pytest.mark.parametrize("tag", TAGS)
def test_forced_grid_rows_are_one_reference_step_from_the_row_before(gpu, tag):
    compared = nr.COMPARED if _case(tag)[1].N < 50 else nr.COMPARED[:2]          # the 70-protein network: S = 290 dense in long double
    failures = []
    for route in routes_of(tag):
        method, operator = expected(tag, route)
        ratio = forced_ratios(gpu, tag, route, compared)
        print("%-18s %-10s %-5s %-5s ratio %8.3f   worst so far (ratio, network, candidate, row) %s" % (tag, route, method, operator, ratio, _worst.get((route, method))))
        assert C[route, method] <= 64 * nr.R64[method, operator]                  # the condition of the construction
        if not ratio <= C[route, method]:
            failures.append((route, method, operator, ratio))
    assert not failures, failures
    if _model(tag) != 2:                                                         # the two pair kernels: the same arithmetic
        for k in ("Y", "ns", "st"):
            np.testing.assert_array_equal(gpu["default"][tag + "/" + k], gpu["pair1"][tag + "/" + k])


@functools.lru_cache(maxsize=None)
def _free_reference(tag, method, operator, k):
    g = np.load(nr.GOLDEN / (tag + ".npz"))
    f = nr.ARK_TOLFAC if method == "ark" else 1.0
    return nr.integrate(method, nm.Network.from_npz(g), nm.Params.from_npz(g, k), g["y0"], g["t_eval"][:FREE_ROWS], rtol=f * FREE_TOL, atol=f * FREE_TOL, operator=operator)


@pytest.mark.parametrize("method", ("ark", "rosw"))
@pytest.mark.parametrize("tag", nr.GOLDEN_SMALL)
def test_free_running_step_counts_and_band(gpu, tag, method):
    g = np.load(nr.GOLDEN / (tag + ".npz"))
    routes = [r for r in routes_of(tag) if expected(tag, r)[0] == method]
    assert routes
    for route in routes:
        operator = expected(tag, route)[1]
        d = gpu[route]
        assert not d[tag + "/freest"].any(), (tag, route)
        for k in (0, 1):
            _, status, counts = _free_reference(tag, method, operator, k)
            got = tuple(int(v) for v in d[tag + "/freens"][k])
            tight = g["Y_tight"][k][:FREE_ROWS]
            band = float(np.max(np.abs(d[tag + "/freeY"][k] - tight) / (1e-8 + 1e-6 * np.abs(tight))))
            print("%-18s %-10s %-5s %-5s candidate %d steps %s restatement %s band %.4f" % (tag, route, method, operator, k, got, counts, band))
            assert status == 0 and abs(got[0] - counts[0]) <= 2 and abs(got[1] - counts[1]) <= 2, (tag, route, k, got, counts)
            assert band <= 0.5, (tag, route, k, band)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("tag", nr.GOLDEN_SMALL)
def test_failure_exits_flag_one_candidate_and_fill_unreached_rows(gpu, tag):
    """The NONFINITE / MAXSTEPS exits and the NaN fill of the one-thread-per-protein kernels (Reg, CombReg, Ark, ark2): four copies of
    one stop loop, held to one statement of the rule."""
    g = np.load(nr.GOLDEN / (tag + ".npz"))
    routes = [r for r in routes_of(tag) if r in ("rosw", "pair0", "sgs") or (r == "default" and _model(tag) == 2)]
    assert "rosw" in routes and len(routes) >= 2, routes
    for route in routes:
        d = {k: gpu[route]["%s/%s" % (tag, k)] for k in ("cleanY", "cleanst", "cleanns", "nanY", "nanst", "nanns", "maxY", "maxst", "maxns")}
        Y, st, ns = d["cleanY"], d["cleanst"], d["cleanns"]
        assert Y.shape[:2] == (3, FREE_ROWS) and not st.any() and np.isfinite(Y).all(), (tag, route, st)
        y0 = np.ascontiguousarray(np.broadcast_to(g["y0"], Y[:, 0].shape), dtype=np.float64)
        # (a) a NaN in one A_i of candidate 1
        assert d["nanst"][1] & nr.ST_NONFINITE, (tag, route, d["nanst"])
        assert _same_bits(d["nanY"][1, 0], y0[1]) and np.isnan(d["nanY"][1, 1:]).all(), (tag, route)
        for c in (0, 2):
            assert _same_bits(d["nanY"][c], Y[c]) and d["nanst"][c] == st[c] and (d["nanns"][c] == ns[c]).all(), (tag, route, c)
        # (b) max_steps = m, half the clean count of candidate 0
        m = int(ns[0].sum()) // 2
        assert m >= 1 and int(ns[0].sum()) > m
        print("%-18s %-8s clean steps %s budget %d  status %s  steps %s" % (tag, route, ns.tolist(), m, d["maxst"].tolist(), d["maxns"].tolist()))
        for c in range(3):
            if int(ns[c].sum()) <= m:                                            # the budget does not bind: the clean run
                assert _same_bits(d["maxY"][c], Y[c]) and d["maxst"][c] == 0 and (d["maxns"][c] == ns[c]).all(), (tag, route, c)
                continue
            assert d["maxst"][c] & nr.ST_MAXSTEPS and int(d["maxns"][c].sum()) == m, (tag, route, c, d["maxst"], d["maxns"])
            reached = np.isfinite(d["maxY"][c]).all(axis=1)
            k = int(reached.sum())
            assert reached[0] and 1 <= k < FREE_ROWS and reached[:k].all() and not reached[k:].any(), (tag, route, c, reached)
            assert _same_bits(d["maxY"][c, :k], Y[c, :k]) and np.isnan(d["maxY"][c, k:]).all(), (tag, route, c, k)
