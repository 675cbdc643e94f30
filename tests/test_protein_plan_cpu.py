"""CPU: protein_plan of csrc/pk_plan.hpp -- which kernel pk_solve_protein_batch launches for (model, n_sites, B, opts, environment switches)
-- compiled for the host with g++ and held to a table of plans.  The table was written out from pk_solve_protein_batch as it stood before
the plan existed (thresholds, predicates and the order of its tests), not from protein_plan."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "phoskintime_amd" / "csrc"

SHIM = r"""
#include <cstring>
#include "pk_plan.hpp"
// out: kernel, code, G, structured, pinned_family, refusal given; msg: the refusal text
extern "C" void shim_plan(int model, int n_sites, long long B, const int* opts, const int* switches, const int* facts, long long* out, char* msg, int msg_len) {
  pk_solver_opts o;
  std::memset(&o, 0, sizeof o);
  o.method = opts[0]; o.linsolve = opts[1]; o.stage_form = opts[2]; o.kernel = opts[3];
  o.rtol = 1e-6; o.atol = 1e-8; o.rk4_h = 1e-3; o.max_steps = 100000; o.clip_nonneg = 1;
  pk::ProteinSwitches sw;
  const int defaults[5] = {sw.wide_rand_exact, sw.rand_level6, sw.rand_parity56, sw.tpr, sw.dist_sched};
  if (switches) { sw.wide_rand_exact = switches[0]; sw.rand_level6 = switches[1]; sw.rand_parity56 = switches[2]; sw.tpr = switches[3]; sw.dist_sched = switches[4]; }
  pk::ProteinFacts f;
  f.tpr_available = facts[0]; f.rand_dense_available = facts[1]; f.wide_chain_fits = facts[2];
  const pk::ProteinPlan p = pk::protein_plan(model, n_sites, B, o, sw, f);
  out[0] = (long long)p.kernel; out[1] = p.code; out[2] = p.G; out[3] = p.structured; out[4] = p.pinned_family; out[5] = p.refusal != nullptr;
  out[6] = p.launches;
  for (int i = 0; i < 5; ++i) out[7 + i] = defaults[i];
  msg[0] = 0;
  if (p.refusal) { std::strncpy(msg, p.refusal, msg_len - 1); msg[msg_len - 1] = 0; }
}
"""

KERNELS = ("Group", "Tpr", "DistFast", "RandFast", "RandParity", "RandLevel", "RandDense", "WideRand", "WideChain")      # enum ProteinKernel, in order
DIST, SUCC, RAND = 0, 1, 2
RODAS4, BDF2, RK4, LRP8, LRP12 = 0, 1, 2, 3, 5
AUTO, DENSE, STRUCTURED = 0, 1, 2
K_AUTO, K_GROUP, K_TPR, K_WORKSPACE = 0, 1, 2, 3
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
M = 10**6


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_plan")
    (d / "shim.cpp").write_text(SHIM)
    (d / "only.cpp").write_text('#include "pk_plan.hpp"\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{CSRC}", str(d / "only.cpp")], check=True)      # stands alone: no HIP header
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", f"-I{CSRC}", str(d / "shim.cpp"), "-o", str(d / "libshim.so")], check=True)
    lib = C.CDLL(str(d / "libshim.so"))
    lib.shim_plan.restype = None
    lib.shim_plan.argtypes = [C.c_int, C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    return lib


class Plan:
    def __init__(self, out, msg):
        self.kernel = KERNELS[out[0]]
        self.code, self.G, self.structured, self.pinned, self.refused, self.launches = out[1], out[2], bool(out[3]), bool(out[4]), bool(out[5]), out[6]
        self.defaults = tuple(out[7:12])
        self.msg = msg


def plan(lib, model, n, B=100, method=LRP12, linsolve=AUTO, stage_form=0, kernel=K_AUTO, exact=1, level6=0, parity56=-1, tpr=-1, sched=0x100,
         tpr_available=None, dense_available=None, chain_fits=True, default_switches=False):
    # the three predicates as their kernels' translation units define them: thread-per-replica kernels exist for distmod n <= 12,
    # succmod n <= 14 and randmod n <= 3; the dense in-register inverse for randmod n = 7
    if tpr_available is None:
        tpr_available = n <= {DIST: 12, SUCC: 14, RAND: 3}[model]
    if dense_available is None:
        dense_available = n == 7
    opts = (C.c_int * 4)(method, linsolve, stage_form, kernel)
    sw = None if default_switches else (C.c_int * 5)(exact, level6, parity56, tpr, sched)
    facts = (C.c_int * 3)(int(tpr_available), int(dense_available), int(chain_fits))
    out = (C.c_longlong * 12)()
    msg = C.create_string_buffer(512)
    lib.shim_plan(model, n, B, opts, sw, facts, out, msg, 512)
    p = Plan(list(out), msg.value.decode())
    assert p.refused == (p.code != OK) and (p.msg != "") == p.refused              # a refusal carries its text, an accepted plan none
    return p


def test_switch_defaults_are_those_of_an_empty_environment(shim):
    p = plan(shim, DIST, 4, default_switches=True)
    assert p.defaults == (1, 0, -1, -1, 0x100)
    assert (p.kernel, p.code) == ("DistFast", OK)


def test_distmod(shim):
    k = lambda *a, **kw: plan(shim, DIST, *a, **kw).kernel
    assert (k(4, 32767), k(4, 32768)) == ("DistFast", "Tpr")
    assert (k(8, 32767), k(8, 32768)) == ("DistFast", "Tpr")
    assert (k(9, 49151), k(9, 49152)) == ("DistFast", "Tpr")
    assert (k(12, 49151), k(12, 49152)) == ("DistFast", "Tpr")
    assert k(13, M) == "DistFast"
    assert k(4, M, kernel=K_GROUP) == "DistFast" and k(4, 1, kernel=K_TPR) == "Tpr"
    assert k(4, M, tpr=0) == "DistFast" and k(4, 1, tpr=1) == "Tpr"
    assert k(4, M, tpr=1, kernel=K_GROUP) == "DistFast" and k(4, 1, tpr=0, kernel=K_TPR) == "Tpr"          # opts->kernel wins over PK_TPR
    assert k(13, 1, kernel=K_TPR) == "DistFast"                                       # no thread-per-replica kernel at this size: the pin has nothing to select
    for method in (RODAS4, LRP8):                                                    # thread per replica integrates with LRP12 only
        assert k(4, M, method=method) == "DistFast" and k(4, 1, method=method, kernel=K_TPR) == "DistFast"
    for linsolve, structured in ((STRUCTURED, True), (DENSE, False)):
        p = plan(shim, DIST, 4, M, linsolve=linsolve)
        assert (p.kernel, p.code, p.structured, p.G, p.launches) == ("Group", OK, structured, 8, (M + 31) // 32)
    for kw in (dict(method=BDF2), dict(method=RK4), dict(stage_form=1)):
        p = plan(shim, DIST, 4, M, **kw)
        assert (p.kernel, p.code, p.structured) == ("Group", OK, True)
    for n, G in ((6, 8), (7, 16), (14, 16), (15, 32), (30, 32), (31, 64), (62, 64)):   # lane-group width: the power of two that holds n + 2 states
        p = plan(shim, DIST, n, 1000)
        assert (p.kernel, p.G, p.launches) == ("DistFast", G, -(-1000 // (256 // G)))
    p = plan(shim, DIST, 63)
    assert (p.kernel, p.code, p.launches, p.pinned) == ("WideChain", OK, 100, False)
    for kw in (dict(method=RODAS4), dict(method=LRP8), dict(stage_form=1)):
        p = plan(shim, DIST, 63, **kw)
        assert p.code == ERR_UNSUPPORTED and "LRP12" in p.msg
    p = plan(shim, DIST, 2000, chain_fits=False)
    assert p.code == ERR_UNSUPPORTED and "1276" in p.msg


def test_dist_sched_refuses_the_distfast_plan_only(shim):
    p = plan(shim, DIST, 4, 32767, sched=-1)
    assert (p.kernel, p.code) == ("DistFast", ERR_ARG) and p.msg.startswith("PK_DIST_SCHED must be one of")
    assert plan(shim, DIST, 30, 2, sched=-1, method=RODAS4).code == ERR_ARG
    for kw in (dict(B=32768), dict(B=1, kernel=K_TPR), dict(B=M, linsolve=DENSE), dict(B=M, method=BDF2)):      # Tpr, Tpr, Group, Group
        assert plan(shim, DIST, 4, sched=-1, **kw).code == OK
    assert plan(shim, SUCC, 4, sched=-1).code == OK and plan(shim, RAND, 4, sched=-1).code == OK and plan(shim, DIST, 63, sched=-1).code == OK


def test_succmod(shim):
    k = lambda *a, **kw: plan(shim, SUCC, *a, **kw).kernel
    assert (k(8, 16383), k(8, 16384)) == ("Group", "Tpr")
    assert (k(9, 32767), k(9, 32768)) == ("Group", "Tpr")
    assert (k(14, 32767), k(14, 32768)) == ("Group", "Tpr")
    assert k(15, M) == "Group"
    assert k(8, M, kernel=K_GROUP) == "Group" and k(8, 1, kernel=K_TPR) == "Tpr" and k(8, 1, tpr=1) == "Tpr" and k(8, M, tpr=0) == "Group"
    p = plan(shim, SUCC, 8, 100)
    assert (p.kernel, p.structured, p.G, p.launches) == ("Group", True, 16, 7)
    assert plan(shim, SUCC, 8, 100, linsolve=DENSE).structured is False
    assert k(63) == "WideChain" and plan(shim, SUCC, 63, method=LRP8).code == ERR_UNSUPPORTED
    for n in range(1, 80):
        for B in (1, M):
            for method in (RODAS4, BDF2, RK4, LRP8, LRP12):
                assert k(n, B, method=method) != "DistFast"


def test_randmod_up_to_six_sites(shim):
    k = lambda *a, **kw: plan(shim, RAND, *a, **kw).kernel
    assert (k(3, 32767), k(3, 32768)) == ("RandFast", "Tpr")
    assert k(4, M) == "RandFast" and k(4, 1, kernel=K_TPR) == "RandFast"
    assert k(5) == "RandFast" and k(5, parity56=1) == "RandParity" and k(5, parity56=0) == "RandFast"
    p = plan(shim, RAND, 5, linsolve=DENSE)
    assert (p.kernel, p.structured, p.G) == ("Group", False, 64)
    assert plan(shim, RAND, 4, linsolve=STRUCTURED).structured is False                # randmod has no structured solve
    p = plan(shim, RAND, 6, kernel=K_GROUP)
    assert (p.kernel, p.code, p.pinned, p.launches) == ("RandParity", OK, False, 100)
    p = plan(shim, RAND, 6, parity56=0)
    assert (p.kernel, p.G, p.launches) == ("RandFast", 64, 25)
    assert k(6, parity56=1) == "RandParity"
    assert k(6, level6=1) == "RandLevel" and k(6, level6=1, parity56=1) == "RandLevel"   # the level switch is tested first
    assert k(6, level6=1, method=LRP8) == "RandFast"
    assert k(6, method=RODAS4) == "RandFast" and k(6, method=LRP8) == "RandFast"
    assert k(6, linsolve=DENSE) == "RandFast" and k(6, linsolve=STRUCTURED) == "RandFast"
    for kw in (dict(method=BDF2), dict(method=RK4), dict(stage_form=1), dict(stage_form=1, method=RODAS4)):
        p = plan(shim, RAND, 6, **kw)
        assert p.code == ERR_UNSUPPORTED and "S = 65" in p.msg


def test_randmod_from_seven_sites(shim):
    k = lambda *a, **kw: plan(shim, RAND, *a, **kw).kernel
    assert k(7) == "RandParity" and k(7, exact=2) == "RandDense" and k(7, exact=0) == "WideRand"
    assert k(7, dense_available=False) == "WideRand" and k(7, exact=2, dense_available=False) == "WideRand"
    assert k(8) == "RandParity" and k(8, exact=2) == "RandLevel" and k(8, exact=0) == "WideRand"
    assert k(9) == "WideRand" and k(9, exact=2) == "WideRand" and k(12, method=RODAS4) == "WideRand"
    assert k(7, method=LRP8) == "RandParity"                                          # any resolvent method selects the size's kernel
    for n in (7, 8, 9):
        for kw in (dict(method=RK4), dict(method=BDF2), dict(stage_form=1)):
            p = plan(shim, RAND, n, **kw)
            assert p.code == ERR_UNSUPPORTED and "n_sites >= 7" in p.msg
    for n in (7, 8):
        assert [plan(shim, RAND, n, 2, kernel=kern).pinned for kern in (K_AUTO, K_GROUP, K_TPR)] == [False, True, True]
    assert plan(shim, RAND, 9, 2, kernel=K_GROUP).launches == 2


def test_explicit_linsolve_reaches_the_lane_group_kernels_at_every_size_and_switch(shim):
    """What tests/test_gpu_group_matrix.py relies on: with linsolve DENSE or STRUCTURED, every model, method and form runs on the lane-group
    kernel at every size up to 64 states, whatever the environment switches say, at the width that holds the states."""
    sizes = [(DIST, n) for n in (1, 6, 7, 14, 15, 30, 31, 62)] + [(SUCC, n) for n in (1, 6, 7, 14, 15, 30, 31, 62)] + [(RAND, n) for n in (1, 2, 3, 4, 5)]
    switches = (dict(), dict(tpr=1), dict(tpr=0), dict(parity56=1), dict(parity56=0), dict(level6=1), dict(exact=0), dict(exact=2), dict(sched=-1))
    for model, n in sizes:
        S = 2 + (n if model != RAND else 2 ** n - 1)
        G = 8 if S <= 8 else 16 if S <= 16 else 32 if S <= 32 else 64
        for linsolve in (DENSE, STRUCTURED):
            for method, form in ((LRP12, 0), (LRP8, 0), (RODAS4, 0), (RODAS4, 1), (BDF2, 0), (RK4, 0)):
                for sw in switches:
                    for kern in (K_AUTO, K_TPR):
                        p = plan(shim, model, n, 37, method=method, linsolve=linsolve, stage_form=form, kernel=kern, **sw)
                        assert (p.kernel, p.code, p.G, p.launches) == ("Group", OK, G, -(-37 // (256 // G))), (model, n, linsolve, method, form, sw, kern)
                        assert p.structured == (linsolve == STRUCTURED and model != RAND)


def test_kernel_table_of_the_rand_matrix_reaches_the_kernels_it_names(shim):
    """What tests/test_gpu_rand_matrix.py relies on: for every row of group_reference.KERNELS -- its switches, n, B, opts.kernel and each of
    its methods -- protein_plan answers with the ProteinKernel the row claims.  The plan picks the launcher; which instantiation the
    launcher then runs (PK_RAND_ROWS, PK_RAND_PARITY6_TB, PK_RAND_PARITY8_GRID, B >= 1024 at n = 7, the thread count of the wide chain)
    it cannot prove: that part of the table rests on reading launch_rand_fast (csrc/pk_inst_rand_fast.hip) and launch_rand_parity /
    launch_wide_chain (csrc/pk_inst_wide.hip)."""
    import group_reference as gr
    meth = {"lrp12": LRP12, "lrp8": LRP8, "rodas4": RODAS4}
    for k in gr.KERNELS:
        sw = dict(exact=int(k.env.get("PK_WIDE_RAND_EXACT", 1)), level6=int(k.env.get("PK_RAND_LEVEL6", 0)), parity56=int(k.env.get("PK_RAND_PARITY56", -1)))
        assert set(k.env) <= {"PK_WIDE_RAND_EXACT", "PK_RAND_LEVEL6", "PK_RAND_PARITY56", "PK_RAND_ROWS", "PK_RAND_PARITY6_TB", "PK_RAND_PARITY8_GRID"}
        for method in k.methods:
            p = plan(shim, k.model, k.n, k.B, method=meth[method], kernel=K_TPR if k.kernel == "tpr" else K_AUTO, **sw)
            assert (p.kernel, p.code) == (k.plan, OK), (k, method, p.kernel, p.code)
            assert not p.pinned, k                                    # a pinned family would keep n = 7 on the 256-thread grid at every B
        # the cut-out replicas of the independence test stay on the same launcher
        assert plan(shim, k.model, k.n, 1, kernel=K_TPR if k.kernel == "tpr" else K_AUTO, **sw).kernel == k.plan, k
    # n = 7: the launcher changes instantiation at B = 1024 unless the family is pinned -- the plan's part of that is pinned_family
    for B in (1023, 1024):
        assert [plan(shim, RAND, 7, B, kernel=kern).pinned for kern in (K_AUTO, K_GROUP, K_TPR)] == [False, True, True]
        assert plan(shim, RAND, 7, B).kernel == "RandParity"
    # n = 6 with LRP8 / RODAS4 is RandFast under every switch group but the level one's LRP12
    for sw in (dict(), dict(parity56=0), dict(parity56=1), dict(level6=1)):
        for method in (LRP8, RODAS4):
            assert plan(shim, RAND, 6, 37, method=method, **sw).kernel == "RandFast"


def test_unknown_kernel_and_the_launch_limit(shim):
    for model, n in ((DIST, 4), (SUCC, 8), (RAND, 3), (RAND, 6), (RAND, 9), (DIST, 70)):
        for kern in (K_WORKSPACE, -1):
            p = plan(shim, model, n, kernel=kern)
            assert p.code == ERR_ARG and "opts->kernel" in p.msg
    top = 0x7fffffff
    # lane groups: 256 / G replicas per workgroup, and the workgroups are what the limit is tested on
    assert plan(shim, DIST, 4, 32 * top, tpr=0).code == OK and plan(shim, DIST, 4, 32 * top + 1, tpr=0).code == ERR_ARG
    assert plan(shim, SUCC, 20, 8 * top).code == OK and plan(shim, SUCC, 20, 8 * top + 1).code == ERR_ARG
    # one workgroup (or wave) per replica: the batch itself; where a method refusal applies as well, the limit is tested first
    for model, n, kw in ((RAND, 6, {}), (RAND, 6, dict(level6=1)), (RAND, 7, {}), (RAND, 9, {}), (DIST, 63, {}), (RAND, 9, dict(method=RK4)), (DIST, 63, dict(method=LRP8))):
        p = plan(shim, model, n, top + 1, **kw)
        assert p.code == ERR_ARG and "batch too large" in p.msg
    assert plan(shim, RAND, 9, top).code == OK and plan(shim, DIST, 63, top).code == OK
    # ... and a refusal that the lane-group path tests before its geometry wins over the limit
    assert plan(shim, RAND, 6, 64 * top, method=BDF2, parity56=0).code == ERR_UNSUPPORTED
