"""CPU: net_plan of csrc/pk_net_plan.hpp -- which kernel a network launch runs for (network facts, opts, launch flavour, tangent columns,
environment knobs), with which method, threads and column chunking, or the text it is refused with -- compiled for the host with g++ and
held to a table of plans.  The table was written out from pk_network.hip as it stood before the plan covered every flavour (net_plan,
the ladders of net_simulate_impl and the option translation of the two tangent entry points: thresholds, order of the tests, refusal
texts), not from the new function."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "phoskintime_amd" / "csrc"

SHIM = r"""
#include <cstring>
#include "pk_net_plan.hpp"
// facts: model N S n_var max_sites arkp_fits arkp_fuses_loss sens_lds_columns sens_score_lds_columns; bytes: solve fused reg rk45 ark
// out: method kernel code threads KC hbm, refusal given, the two NetSwitches defaults
extern "C" void shim_net_plan(const int* facts, const long long* bytes, const int* opts, int flavour, int K, const int* switches, int* out, char* msg,
                              int msg_len) {
  const pk::NetFacts f{facts[0], facts[1], facts[2], facts[3], facts[4], (size_t)bytes[0], (size_t)bytes[1], (size_t)bytes[2], (size_t)bytes[3],
                       (size_t)bytes[4], facts[5] != 0, facts[6] != 0, facts[7], facts[8]};
  pk_solver_opts o;
  std::memset(&o, 0, sizeof o);
  o.method = opts[0]; o.linsolve = opts[1]; o.kernel = opts[2];
  o.rtol = 1e-6; o.atol = 1e-8;
  pk::NetSwitches sw;
  out[7] = sw.net_threads; out[8] = sw.sens_hbm_width;
  if (switches) { sw.net_threads = switches[0]; sw.sens_hbm_width = switches[1]; }
  const pk::NetPlan p = pk::net_plan(f, o, (pk::NetFlavour)flavour, K, sw);
  out[0] = p.method; out[1] = (int)p.kernel; out[2] = p.code; out[3] = p.threads; out[4] = p.KC; out[5] = p.hbm; out[6] = p.refusal != nullptr;
  msg[0] = 0;
  if (p.refusal) { std::strncpy(msg, p.refusal, msg_len - 1); msg[msg_len - 1] = 0; }
}
"""

KERNELS = ("DP5", "Workspace", "ArkPair", "Ark", "CombReg", "Reg", "Lds")                     # enum NetKernel, in order
PLAIN, TABLES, LISTS, MEASURE, SENS, SENS_SCORE = range(6)                                   # enum NetFlavour, in order
RODAS4, DP5, LRP12, ARK436, ROS34PW2 = 0, 4, 5, 6, 7
AUTO, DENSE, STRUCTURED = 0, 1, 2
K_AUTO, K_WORKSPACE, K_HBM = 0, 3, 4
OK, ERR_UNSUPPORTED = 0, -2
KiB = 1024

# the refusal texts of pk_network.hip, in the order it tests them
HBM_ELSEWHERE = ("PK_KERNEL_HBM is read by pk_network_simulate_sens_batch and pk_network_simulate_objective_grad_batch only; "
                 "ask for PK_KERNEL_WORKSPACE here")
DP5_WORKSPACE = "PK_KERNEL_WORKSPACE integrates with PK_METHOD_ROS34PW2 only"
DP5_SIZE = "PK_METHOD_DP5: S <= 1024 states and N <= 512 proteins per network"
DP5_LDS = "network too large for one workgroup's LDS (160 KiB)"
ARK_WORKSPACE = "PK_METHOD_ARK436: not on the workspace kernel (networks beyond one workgroup's LDS); use PK_METHOD_ROS34PW2"
ARK_FITS = ("PK_METHOD_ARK436: <= 8 sites per protein and N <= 256 (topologies 0 / 1 / 4: <= 512 lanes of the dense layout); "
            "combinatorial topology: <= 3 sites, N <= 256; use PK_METHOD_ROS34PW2")
SENS_MISMATCH = "network sensitivities: the plan for these options is neither the general LDS kernel nor the HBM-workspace kernel"
MEASURE_REG = ("fused measurement: not on the register-resident kernels; ask for the general LDS kernel "
               "(opts->linsolve = PK_LINSOLVE_STRUCTURED, kernel = \"lds\" in Python) or PK_KERNEL_WORKSPACE")
MEASURE_ORDER3 = ("fused measurement: the order-3 integrator only; ask for opts->method = PK_METHOD_ROS34PW2 (method = \"rosw\" in "
                  "Python) on the general LDS kernel or the workspace kernel, or call pk_network_simulate_batch + pk_network_observables_batch")
LISTS_REG = ("fused objective with PK_METHOD_ROS34PW2: not on the register-resident kernels; ask for the general LDS "
             "kernel (opts->linsolve = PK_LINSOLVE_STRUCTURED, kernel = \"lds\" in Python) or PK_KERNEL_WORKSPACE")
LISTS_ORDER3 = "fused objective on request: PK_METHOD_ROS34PW2 on the LDS or the workspace kernel only"
TABLES_DENSE = ("fused objective: topologies 0 / 1 / 4 on the default additive integrator only; "
                "use pk_network_simulate_batch + pk_network_objective_batch")
SENS_METHOD = {SENS: "network sensitivities integrate with PK_METHOD_ROS34PW2 only: leave opts->method at its default or ask for PK_METHOD_ROS34PW2",
               SENS_SCORE: "objective gradients integrate with PK_METHOD_ROS34PW2 only: leave opts->method at its default or ask for PK_METHOD_ROS34PW2"}
SENS_WORKSPACE = {SENS: "network sensitivities: PK_KERNEL_WORKSPACE names the state kernel; leave opts->kernel at PK_KERNEL_AUTO, or "
                        "ask for the tangents on HBM slabs with PK_KERNEL_HBM",
                  SENS_SCORE: "objective gradients: PK_KERNEL_WORKSPACE names the state kernel; leave opts->kernel at PK_KERNEL_AUTO, or "
                              "ask for the tangents on HBM slabs with PK_KERNEL_HBM"}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_net_plan")
    (d / "shim.cpp").write_text(SHIM)
    (d / "only.cpp").write_text('#include "pk_net_plan.hpp"\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{CSRC}", str(d / "only.cpp")], check=True)      # stands alone: no HIP header
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", f"-I{CSRC}", str(d / "shim.cpp"), "-o", str(d / "libshim.so")], check=True)
    lib = C.CDLL(str(d / "libshim.so"))
    lib.shim_net_plan.restype = None
    lib.shim_net_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.c_char_p, C.c_int]
    return lib


class Plan:
    def __init__(self, out, msg):
        self.method, self.kernel, self.code, self.threads, self.KC, self.hbm, self.refused = out[0], KERNELS[out[1]], out[2], out[3], out[4], bool(out[5]), bool(out[6])
        self.defaults = (out[7], out[8])
        self.msg = msg


def plan(lib, flavour=PLAIN, method=LRP12, linsolve=AUTO, kernel=K_AUTO, K=0, model=0, N=100, S=500, n_var=700, max_sites=4, solve_lds=80 * KiB,
         fused_lds=None, reg_lds=40 * KiB, rk45_lds=60 * KiB, ark_lds=90 * KiB, arkp_fits=False, arkp_fuses_loss=True, sens_cols=4, score_cols=3,
         net_threads=0, W=16, default_switches=False):
    """The defaults: an arrow-topology network of 100 proteins with up to 4 sites that fits every one-workgroup kernel but the dense-lane one."""
    facts = (C.c_int * 9)(model, N, S, n_var, max_sites, int(arkp_fits), int(arkp_fuses_loss), sens_cols, score_cols)
    nbytes = (C.c_longlong * 5)(solve_lds, solve_lds + 8 * N if fused_lds is None else fused_lds, reg_lds, rk45_lds, ark_lds)
    opts = (C.c_int * 3)(method, linsolve, kernel)
    sw = None if default_switches else (C.c_int * 2)(net_threads, W)
    out = (C.c_int * 9)()
    msg = C.create_string_buffer(512)
    lib.shim_net_plan(facts, nbytes, opts, flavour, K, sw, out, msg, 512)
    p = Plan(list(out), msg.value.decode())
    assert p.refused == (p.code != OK) and (p.msg != "") == p.refused              # a refusal carries its text, an accepted plan none
    assert p.code in (OK, ERR_UNSUPPORTED)
    return p


ROSW = dict(method=ROS34PW2)
LDS = dict(method=ROS34PW2, linsolve=STRUCTURED)          # the general LDS kernel on request
COMB = dict(model=2, max_sites=3)


def test_switch_defaults_are_those_of_an_empty_environment(shim):
    p = plan(shim, default_switches=True, **LDS)
    assert p.defaults == (0, 16) and (p.kernel, p.threads) == ("Lds", 256)


def test_plain_reaches_each_of_the_seven_kernels(shim):
    mk = lambda **kw: (lambda p: (p.kernel, p.method, p.code))(plan(shim, **kw))
    assert mk(method=DP5) == ("DP5", DP5, OK)
    assert mk(kernel=K_WORKSPACE) == ("Workspace", ROS34PW2, OK) and mk(kernel=K_WORKSPACE, **ROSW) == ("Workspace", ROS34PW2, OK)
    assert mk(arkp_fits=True) == ("ArkPair", ARK436, OK) and mk(arkp_fits=True, method=ARK436) == ("ArkPair", ARK436, OK)
    assert mk() == ("Ark", ARK436, OK) and mk(method=ARK436) == ("Ark", ARK436, OK) and mk(method=RODAS4) == ("Ark", ARK436, OK)
    assert mk(**COMB) == ("Ark", ARK436, OK) and mk(**COMB, **ROSW) == ("CombReg", ROS34PW2, OK)
    assert mk(**ROSW) == ("Reg", ROS34PW2, OK) and mk(arkp_fits=True, **ROSW) == ("Reg", ROS34PW2, OK)
    assert mk(**LDS) == ("Lds", ROS34PW2, OK)
    for kw in (dict(), dict(method=ARK436), ROSW, COMB, dict(N=64), dict(N=65), dict(N=256)):          # ARK and register kernels: one thread per protein, whole waves
        N = kw.get("N", 100)
        assert plan(shim, **kw).threads == -(-N // 64) * 64
    for fl in range(6):
        assert (plan(shim, fl).KC, plan(shim, fl).hbm) == ((0, False) if fl < SENS else ((4, 3)[fl - SENS], False))


def test_size_boundaries_from_both_sides(shim):
    k = lambda **kw: plan(shim, **kw).kernel
    # beyond the one-workgroup kernels: S > 1024, N > 512, more than 160 KiB for the general LDS kernel
    assert (k(S=1024, **LDS), k(S=1025, **LDS)) == ("Lds", "Workspace")
    assert (k(N=512, S=1024, **LDS), k(N=513, S=1024, **LDS)) == ("Lds", "Workspace")
    assert (k(S=1024), k(S=1025), k(N=513)) == ("Ark", "Workspace", "Workspace")
    assert (k(solve_lds=160 * KiB, **LDS), k(solve_lds=160 * KiB + 8, **LDS)) == ("Lds", "Workspace")
    assert (k(solve_lds=160 * KiB + 8), k(solve_lds=160 * KiB + 8, **ROSW)) == ("Workspace", "Workspace")
    assert k(solve_lds=200 * KiB, **COMB, **ROSW) == "CombReg" and k(solve_lds=200 * KiB, **COMB) == "Ark"      # small combinatorial blocks are exempt ...
    assert k(solve_lds=200 * KiB, model=2, max_sites=4) == "Workspace" and k(solve_lds=200 * KiB, N=257, **COMB) == "Workspace"      # ... only they
    # one thread per protein: N <= 256
    assert (k(N=256), k(N=257)) == ("Ark", "Lds") and (k(N=256, **ROSW), k(N=257, **ROSW)) == ("Reg", "Lds")
    assert (k(N=256, **COMB), k(N=257, **COMB)) == ("Ark", "Lds") and (k(N=256, **COMB, **ROSW), k(N=257, **COMB, **ROSW)) == ("CombReg", "Lds")
    assert (k(N=257, arkp_fits=True), k(N=512, arkp_fits=True), k(N=513, arkp_fits=True)) == ("ArkPair", "ArkPair", "Workspace")      # the dense lanes: the caller's predicate
    # sites per protein: 3 (combinatorial), 8 (the other topologies)
    assert (k(model=2, max_sites=3), k(model=2, max_sites=4)) == ("Ark", "Lds")
    assert (k(model=2, max_sites=3, **ROSW), k(model=2, max_sites=4, **ROSW)) == ("CombReg", "Lds")
    assert (k(max_sites=8), k(max_sites=9)) == ("Ark", "Lds") and (k(max_sites=8, **ROSW), k(max_sites=9, **ROSW)) == ("Reg", "Lds")
    for model in (1, 4):
        assert (k(model=model), k(model=model, **ROSW), k(model=model, max_sites=9)) == ("Ark", "Reg", "Lds")
    # the LDS of the additive and the register kernels
    assert (k(ark_lds=160 * KiB), k(ark_lds=160 * KiB + 8), k(ark_lds=160 * KiB + 8, arkp_fits=True)) == ("Ark", "Reg", "ArkPair")
    assert (k(reg_lds=64 * KiB, **ROSW), k(reg_lds=64 * KiB + 8, **ROSW)) == ("Reg", "Lds")
    # PK_LINSOLVE_STRUCTURED forces the general LDS kernel; PK_LINSOLVE_DENSE is as good as auto
    assert (k(), k(linsolve=STRUCTURED), k(linsolve=DENSE)) == ("Ark", "Lds", "Ark")
    assert (k(arkp_fits=True), k(arkp_fits=True, linsolve=STRUCTURED)) == ("ArkPair", "Lds")
    assert (k(**ROSW), k(**LDS), k(**COMB, **ROSW), k(**COMB, **LDS)) == ("Reg", "Lds", "CombReg", "Lds")
    assert k(kernel=K_WORKSPACE, linsolve=STRUCTURED) == "Workspace"


def test_ark436_and_dp5_requests(shim):
    r = lambda **kw: (lambda p: (p.code, p.method, p.msg))(plan(shim, **kw))
    ark = dict(method=ARK436)
    for kw in (dict(kernel=K_WORKSPACE), dict(S=1025), dict(N=513), dict(solve_lds=160 * KiB + 8)):
        assert r(**ark, **kw) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, ARK_WORKSPACE)
    for kw in (dict(linsolve=STRUCTURED), dict(N=257), dict(max_sites=9), dict(model=2, max_sites=4), dict(ark_lds=160 * KiB + 8), dict(arkp_fits=True, linsolve=STRUCTURED)):
        assert r(**ark, **kw) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, ARK_FITS)
    assert r(**ark, N=257, arkp_fits=True)[:2] == (OK, ARK436) and r(**ark, ark_lds=160 * KiB)[:2] == (OK, ARK436)
    dp5 = dict(method=DP5)
    for kw in (dict(), dict(S=1024, N=512), dict(rk45_lds=160 * KiB), dict(linsolve=STRUCTURED), dict(model=2, max_sites=9), dict(solve_lds=200 * KiB)):
        p = plan(shim, **dp5, **kw)
        assert (p.kernel, p.method, p.code) == ("DP5", DP5, OK)
    assert r(**dp5, kernel=K_WORKSPACE) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, DP5_WORKSPACE)
    assert r(**dp5, kernel=K_WORKSPACE, S=1025) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, DP5_WORKSPACE)
    # a DP5 request on a network too large for its kernel still reports PK_METHOD_DP5
    assert r(**dp5, S=1025) == (ERR_UNSUPPORTED, DP5, DP5_SIZE) and r(**dp5, N=513) == (ERR_UNSUPPORTED, DP5, DP5_SIZE)
    assert r(**dp5, S=1025, rk45_lds=200 * KiB) == (ERR_UNSUPPORTED, DP5, DP5_SIZE)
    assert r(**dp5, rk45_lds=160 * KiB + 8) == (ERR_UNSUPPORTED, DP5, DP5_LDS)


def test_hbm_belongs_to_the_tangent_flavours(shim):
    for fl in (PLAIN, TABLES, LISTS, MEASURE):
        for kw in (dict(), ROSW, LDS, dict(method=DP5), dict(method=ARK436), dict(S=1025), dict(arkp_fits=True)):
            p = plan(shim, fl, kernel=K_HBM, **kw)
            assert (p.code, p.method, p.msg) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, HBM_ELSEWHERE)


def test_score_tables(shim):
    p = plan(shim, TABLES, arkp_fits=True)
    assert (p.kernel, p.method, p.code) == ("ArkPair", ARK436, OK)
    assert plan(shim, TABLES, arkp_fits=True, method=ARK436).code == OK
    refused = (dict(arkp_fits=True, arkp_fuses_loss=False), dict(), dict(method=DP5), dict(S=1025), dict(**COMB, **ROSW), ROSW, LDS, dict(arkp_fits=True, **ROSW),
               dict(arkp_fits=True, linsolve=STRUCTURED), dict(kernel=K_WORKSPACE))          # ArkPair without the scoring kernel, then the six other kernels
    for kw in refused:
        p = plan(shim, TABLES, **kw)
        assert (p.code, p.msg) == (ERR_UNSUPPORTED, TABLES_DENSE)
    assert plan(shim, TABLES, method=ARK436, linsolve=STRUCTURED).msg == ARK_FITS          # the state plan's refusal answers first
    assert plan(shim, TABLES, method=DP5, S=1025).msg == DP5_SIZE


def test_score_lists_and_measure(shim):
    for fl, reg_text, order3_text in ((LISTS, LISTS_REG, LISTS_ORDER3), (MEASURE, MEASURE_REG, MEASURE_ORDER3)):
        p = plan(shim, fl, **LDS)
        assert (p.kernel, p.method, p.code, p.threads) == ("Lds", ROS34PW2, OK, 256)
        for kw in (dict(kernel=K_WORKSPACE), dict(S=1025, **ROSW), dict(solve_lds=160 * KiB + 8, **LDS)):
            p = plan(shim, fl, **kw)
            assert (p.kernel, p.method, p.code) == ("Workspace", ROS34PW2, OK)
        for kw in (ROSW, dict(**COMB, **ROSW)):                                            # Reg, CombReg
            p = plan(shim, fl, **kw)
            assert (p.code, p.msg) == (ERR_UNSUPPORTED, reg_text)
        for kw in (dict(), dict(arkp_fits=True), dict(method=DP5), dict(method=ARK436), COMB):      # Ark, ArkPair, DP5, Ark, Ark
            p = plan(shim, fl, **kw)
            assert (p.code, p.msg) == (ERR_UNSUPPORTED, order3_text)
        assert plan(shim, fl, method=ARK436, kernel=K_WORKSPACE).msg == ARK_WORKSPACE        # the state plan's refusal answers first
        assert plan(shim, fl, method=DP5, kernel=K_WORKSPACE).msg == DP5_WORKSPACE
        # the rna baseline comes on top of the LDS of a plain launch: past 160 KiB the workspace kernel takes over
        assert [plan(shim, fl, fused_lds=160 * KiB + d, **LDS).kernel for d in (-8, 0, 8)] == ["Lds", "Lds", "Workspace"]
        assert plan(shim, fl, fused_lds=160 * KiB + 8, **ROSW).msg == reg_text                # ... of the LDS kernel alone
    for fl in (PLAIN, SENS, SENS_SCORE):
        assert plan(shim, fl, K=2, fused_lds=160 * KiB + 8, **LDS).kernel == "Lds"


@pytest.mark.parametrize("fl", (SENS, SENS_SCORE))
def test_tangent_flavours(shim, fl):
    cols = dict(sens_cols=6, score_cols=5)
    kc = 6 if fl == SENS else 5
    for kw in (dict(method=ARK436), dict(method=DP5), dict(method=DP5, kernel=K_WORKSPACE), dict(method=ARK436, kernel=K_HBM), dict(method=DP5, S=1025)):
        p = plan(shim, fl, K=2, **kw)
        assert (p.code, p.method, p.msg) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, SENS_METHOD[fl])
    for kw in (dict(kernel=K_WORKSPACE), dict(kernel=K_WORKSPACE, **ROSW), dict(kernel=K_WORKSPACE, S=1025)):
        p = plan(shim, fl, K=2, **kw)
        assert (p.code, p.method, p.msg) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED, SENS_WORKSPACE[fl])
    # the LDS route: always the order-3 method on the general LDS kernel, whatever method and linsolve say and whichever kernel a plain launch takes
    for kw in (dict(), ROSW, LDS, dict(method=RODAS4, linsolve=DENSE), dict(arkp_fits=True), COMB, dict(**COMB, **ROSW)):
        for K in (0, 1, 40):
            p = plan(shim, fl, K=K, **cols, **kw)
            assert (p.kernel, p.method, p.code, p.KC, p.hbm) == ("Lds", ROS34PW2, OK, kc, False)
    # the slab route: where not one column fits beside the state, and on request
    zero = dict(sens_cols=0) if fl == SENS else dict(score_cols=0)
    for kw in (zero, dict(kernel=K_HBM), dict(kernel=K_HBM, **ROSW), dict(S=1025, N=513, **zero), dict(solve_lds=200 * KiB, **zero), dict(COMB, **zero)):
        p = plan(shim, fl, K=5, **dict(cols, **kw))
        assert (p.kernel, p.method, p.code, p.KC, p.hbm) == ("Workspace", ROS34PW2, OK, 5, True)
    other = dict(score_cols=0) if fl == SENS else dict(sens_cols=0)                         # each flavour reads its own count
    assert plan(shim, fl, K=5, **dict(cols, **other)).hbm is False
    # KC = min(K, n_var, W) on slabs
    kcs = lambda **kw: [plan(shim, fl, K=K, kernel=K_HBM, **kw).KC for K in (1, 15, 16, 17, 40)]
    assert kcs() == [1, 15, 16, 16, 16] and kcs(W=4) == [1, 4, 4, 4, 4] and kcs(n_var=3) == [1, 3, 3, 3, 3] and kcs(n_var=3, W=2) == [1, 2, 2, 2, 2]
    assert plan(shim, fl, K=0, kernel=K_HBM).KC == 0 and plan(shim, fl, K=5, W=4, **cols).KC == kc      # W is the slab route's alone
    # facts that no network has: a column count >= 1 beside a state plan on the workspace kernel
    for kw in (dict(S=1025), dict(N=513), dict(solve_lds=160 * KiB + 8)):
        p = plan(shim, fl, K=2, **kw)
        assert (p.code, p.msg) == (ERR_UNSUPPORTED, SENS_MISMATCH)


def test_threads_of_the_general_lds_kernel(shim):
    t = lambda fl=PLAIN, **kw: (lambda p: (p.kernel, p.threads))(plan(shim, fl, **dict(LDS, **kw)))[1]
    assert plan(shim, S=128, N=64, **LDS).kernel == "Lds"
    assert (t(S=128, N=64), t(S=129, N=64), t(S=128, N=65), t(S=1024, N=512), t(S=3, N=1)) == (64, 256, 256, 256, 64)
    for fl in (LISTS, MEASURE, SENS, SENS_SCORE):
        assert (t(fl, S=128, N=64), t(fl, S=129, N=64)) == (64, 256)
    # PK_NET_THREADS: 64, 128 or 256 where every thread then owns <= 4 states and <= 2 proteins
    assert (t(S=256, N=128, net_threads=64), t(S=257, N=128, net_threads=64), t(S=256, N=129, net_threads=64)) == (64, 256, 256)
    assert (t(S=512, N=256, net_threads=128), t(S=513, N=256, net_threads=128), t(S=512, N=257, net_threads=128)) == (128, 256, 256)
    assert (t(S=100, N=50, net_threads=128), t(S=100, N=50, net_threads=256), t(S=1024, N=512, net_threads=256)) == (128, 256, 256)
    for v in (0, 1, 32, 63, 65, 100, 192, 512, -64):
        assert (t(S=100, N=50, net_threads=v), t(S=500, N=100, net_threads=v)) == (64, 256)
    assert plan(shim, net_threads=64, N=200).threads == 256 and plan(shim, net_threads=64, N=200, **ROSW).threads == 256      # Ark, Reg: whole waves, no override
    # tangents: 256 threads where a workgroup carries min(K, KC) * S > 512 tangent entries, after the override
    small = dict(S=100, N=50)
    for fl, cols in ((SENS, "sens_cols"), (SENS_SCORE, "score_cols")):
        tt = lambda K, KC, **kw: t(fl, K=K, **{cols: KC}, **small, **kw)
        assert (tt(5, 5), tt(6, 6), tt(10, 5), tt(5, 8), tt(6, 8), tt(40, 6)) == (64, 256, 64, 64, 256, 256)
        assert (tt(5, 5, net_threads=128), tt(6, 6, net_threads=64), tt(6, 6, net_threads=128)) == (128, 256, 256)
        assert (t(fl, K=4, S=128, N=64, **{cols: 4}), t(fl, K=5, S=128, N=64, **{cols: 5})) == (64, 256)      # 512 / 640
    assert t(PLAIN, K=40, sens_cols=40, **small) == 64 and t(LISTS, K=40, sens_cols=40, **small) == 64


# The networks of tests/net_step_reference.py, on which tests/test_gpu_network_steps.py holds every integrator kernel to a one-step
# restatement: (topology, N, S, max_sites) and the kernel of each of its routes -- default, method="rosw", method="rosw" + kernel="lds",
# kernel="workspace", and the default with PK_ARK_PAIR=0 (no dense lane layout) -- with the threads of the general LDS kernel
STEP_NETWORKS = {
    "network_m0_small": ((0, 6, 20, 3), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "network_m1_small": ((1, 6, 21, 3), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "network_m2_small": ((2, 6, 32, 3), ("Ark", "CombReg", "Lds", "Workspace", "Ark"), 64),
    "network_m4_small": ((4, 6, 20, 3), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m0_c4": ((0, 5, 21, 4), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m0_c6": ((0, 6, 29, 6), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m0_c8": ((0, 7, 38, 8), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m1_c4": ((1, 5, 21, 4), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m1_c6": ((1, 6, 29, 6), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m1_c8": ((1, 7, 38, 8), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m4_c4": ((4, 5, 21, 4), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m4_c6": ((4, 6, 29, 6), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m4_c8": ((4, 7, 38, 8), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 64),
    "m2_c2": ((2, 6, 23, 2), ("Ark", "CombReg", "Lds", "Workspace", "Ark"), 64),
    "m2_c3": ((2, 6, 33, 3), ("Ark", "CombReg", "Lds", "Workspace", "Ark"), 64),
    "m2_c4": ((2, 5, 34, 4), ("Lds", "Lds", "Lds", "Workspace", "Lds"), 64),
    "m0_wide": ((0, 70, 290, 4), ("ArkPair", "Reg", "Lds", "Workspace", "Ark"), 256),
}


def test_routes_of_the_step_reference_networks(shim):
    import net_step_reference as nr
    assert set(STEP_NETWORKS) == set(nr.GOLDEN_SMALL) | {s[0] for s in nr.SYNTHETIC}
    for tag, (facts, kernels, lds_threads) in STEP_NETWORKS.items():
        desc, net, X, y0, t = nr.case(tag)
        model, N, S, max_sites = facts
        assert (net.model, net.N, net.S, int(net.n_sites.max())) == facts, tag
        # byte counts: an upper bound on each kernel's request (parameters, 8 vectors of S, 7 of N, the TF CSR twice over, the reductions,
        # and the additive kernel's four parked block vectors per thread); every one is a fraction of its threshold
        threads = -(-N // 64) * 64
        lds = 8 * (X.shape[1] + 8 * S + 7 * N + net.n_K + net.total_sites + 2 * int(net.TF_indptr[-1]) + 32) + 8 * 4 * (2 + (1 << max_sites if model == 2 else max_sites)) * threads
        assert lds <= 64 * KiB
        kw = dict(model=model, N=N, S=S, n_var=X.shape[1], max_sites=max_sites, solve_lds=lds, reg_lds=lds, rk45_lds=lds, ark_lds=lds)
        dense = model != 2                               # net_arkp_fits: a lane table (topologies 0 / 1 / 4, <= 8 sites) of <= 512 lanes
        got = [plan(shim, arkp_fits=dense, **kw), plan(shim, arkp_fits=dense, **kw, **ROSW), plan(shim, arkp_fits=dense, **kw, **LDS),
               plan(shim, arkp_fits=dense, kernel=K_WORKSPACE, **kw), plan(shim, arkp_fits=False, **kw)]
        assert tuple(p.kernel for p in got) == kernels and all(p.code == OK for p in got), tag
        additive = model != 2 or max_sites <= 3
        assert [p.method for p in got] == [ARK436 if additive else ROS34PW2, ROS34PW2, ROS34PW2, ROS34PW2, ARK436 if additive else ROS34PW2], tag
        assert got[2].threads == lds_threads and got[4].threads == -(-N // 64) * 64, tag
        if not additive:
            assert plan(shim, method=ARK436, **kw).msg == ARK_FITS
