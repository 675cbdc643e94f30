// pk_plan.hpp -- which kernel pk_solve_protein_batch runs for (model, n_sites, B, opts): one pure host function, protein_plan, as net_plan
// is for the network path.  Plain C++ over include/phoskin.h: no HIP, no getenv, no statics, so it compiles under hipcc (pk_capi.hip, its
// only user in the library) and under g++ (tests/test_protein_plan_cpu.py holds it to a table of plans).  The caller brings in what lives
// elsewhere: the environment switches (ProteinSwitches, read once per process by pk_capi.hip) and the answers of the predicates that
// are defined next to their kernels (ProteinFacts).  The tests of protein_plan run in the order in which pk_solve_protein_batch has always
// made them: where two refusals apply, the earlier one answers.
#pragma once
#include "../../include/phoskin.h"

namespace pk {

// one enumerator per launcher of pk_launch.hpp that the per-protein solve can reach
enum class ProteinKernel {
  Group,        // kSolve[model][G]: lane groups of 8-64 lanes, every method and linsolve (pk_solve_kernel.hpp)
  Tpr,          // launch_tpr: one lane per replica, small systems at large batches (pk_tpr.hpp)
  DistFast,     // launch_dist_fast: distmod throughput layout, 4-16 lanes per replica (pk_dist_fast.hpp)
  RandFast,     // launch_rand_fast: randmod n <= 6, 2^n lanes per replica, in-register inverse (pk_rand_fast.hpp)
  RandParity,   // launch_rand_parity: randmod n = 5-8, parity elimination (pk_rand_parity.hpp)
  RandLevel,    // launch_rand_level: randmod n = 6 / 8, block elimination over the popcount levels (pk_rand_level.hpp)
  RandDense,    // launch_rand_dense: randmod n = 7, the full 128 x 128 inverse in registers (pk_rand_dense.hpp)
  WideRand,     // launch_wide_rand: randmod n >= 7, ROS34PW2-W on the n-cube, one workgroup per replica (pk_wide.hpp)
  WideChain,    // launch_wide_chain: distmod / succmod beyond 64 states, LRP12 with exact structured solves (pk_wide.hpp)
};

// The environment switches of the selection with the values of an empty environment; protein_switches() in pk_capi.hip reads them once
// per process and says what each one was measured for.
struct ProteinSwitches {
  int wide_rand_exact = 1;    // PK_WIDE_RAND_EXACT, randmod n = 7 / 8: 1 parity elimination, 2 dense inverse (n = 7) / level blocks (n = 8), 0 the n-cube kernel
  int rand_level6 = 0;        // PK_RAND_LEVEL6=1: randmod n = 6 on the level-block kernel
  int rand_parity56 = -1;     // PK_RAND_PARITY56: 0 keeps randmod n = 6 off the parity kernel, 1 also sends n = 5 there
  int tpr = -1;               // PK_TPR=0 / 1: never / always thread per replica where such a kernel exists (opts->kernel wins)
  int dist_sched = 0x100;     // PK_DIST_SCHED as dist_sched_env() parses it: negative for a value that names no pacing policy, 0x100 when unset
};

// What the plan needs to know about (model, n_sites) from the kernels' translation units; the caller asks the predicates of pk_launch.hpp.
struct ProteinFacts {
  bool tpr_available = false;          // tpr_available(model, n_sites)
  bool rand_dense_available = false;   // rand_dense_available(n_sites)
  bool wide_chain_fits = false;        // wide_chain_fits(S, n_sites)
};

struct ProteinPlan {
  ProteinKernel kernel = ProteinKernel::Group;   // of a refused plan: the launcher the refusal speaks for, Group where none was chosen yet
  int code = PK_OK;
  const char* refusal = nullptr;       // null when accepted.  The PK_DIST_SCHED refusal (the only one of a DistFast plan) ends where the
                                       // caller appends the accepted names, which live with the parser (kDistSchedNames)
  int G = 0;                           // lane-group width of Group / DistFast / RandFast (Tpr carries it along), 0 elsewhere
  bool structured = false;             // Group: structured instead of dense linear solves
  bool pinned_family = false;          // RandParity at n = 7 / 8: the caller pinned the kernel family, keep the 256-thread grid at every B
  long long launches = 0;              // what the path's launch limit was tested on: B, or the workgroups ceil(B / (256 / G)) of the lane-group
                                       // geometry (Tpr is chosen after that test and keeps its count)
};

constexpr long long kLaunchLimit = 0x7fffffffLL;
constexpr const char* kChainTooWide = "distmod / succmod: n_sites <= 1276 (sixteen LDS vectors of n_sites + 2 doubles per workgroup)";

inline int protein_states(int model, int n_sites) { return 2 + (model == PK_MODEL_RAND ? (1 << n_sites) - 1 : n_sites); }   // pk::n_states
inline bool resolvent_method(int m) { return m == PK_METHOD_RODAS4 || m == PK_METHOD_LRP8 || m == PK_METHOD_LRP12; }
inline int group_width(int S) { return S <= 8 ? 8 : S <= 16 ? 16 : S <= 32 ? 32 : S <= 64 ? 64 : 0; }
// systems beyond one wavefront's lane groups (pk_wide.hpp): distmod / succmod with more than 64 states, randmod with n_sites >= 7
inline bool is_wide(int model, int n_sites) { return model == PK_MODEL_RAND ? n_sites >= 7 : protein_states(model, n_sites) > 64; }

// model in 0..2 and n_sites in 1..20 (randmod) / >= 1 are the caller's to check (check_model); B >= 1.
inline ProteinPlan protein_plan(int model, int n_sites, long long B, const pk_solver_opts& o, const ProteinSwitches& sw, const ProteinFacts& f) {
  using K = ProteinKernel;
  ProteinPlan p;
  p.launches = B;
  const auto refuse = [&p](int code, const char* why) { p.code = code; p.refusal = why; return p; };
  const auto pick = [&p](K k) { p.kernel = k; return p; };
  const auto over = [&p] { return p.launches > kLaunchLimit; };
  const char* const too_large = "batch too large for one launch";

  if (o.kernel < PK_KERNEL_AUTO || o.kernel > PK_KERNEL_TPR) return refuse(PK_ERR_ARG, "unknown opts->kernel");
  const int S = protein_states(model, n_sites);
  const bool lrp12 = o.method == PK_METHOD_LRP12 && !o.stage_form;       // the default method in resolvent form: all that the specialised exact kernels integrate
  if (is_wide(model, n_sites)) {
    // one workgroup per replica (pk_wide.hpp).  distmod / succmod: LRP12 with exact structured solves; randmod: ROS34PW2-W on the n-cube
    // (selected by any of the implicit one-step methods: there is no exact sparse resolvent for the LRP / RODAS family at this size)
    p.kernel = model == PK_MODEL_RAND ? K::WideRand : K::WideChain;
    if (model != PK_MODEL_RAND && !f.wide_chain_fits) return refuse(PK_ERR_UNSUPPORTED, kChainTooWide);     // check_model's answer, which every entry point gives first
    if (over()) return refuse(PK_ERR_ARG, too_large);
    if (model != PK_MODEL_RAND)
      return lrp12 ? p : refuse(PK_ERR_UNSUPPORTED, "distmod / succmod with more than 64 states integrate with method LRP12 (the default) only");
    if (!resolvent_method(o.method) || o.stage_form)
      return refuse(PK_ERR_UNSUPPORTED, "randmod n_sites >= 7: method must be LRP12 / LRP8 / RODAS4 in resolvent form (n = 7: LRP12 with the dense inverse; beyond: additive Runge-Kutta on the n-cube)");
    const int exact = sw.wide_rand_exact;
    const auto parity = [&] { p.pinned_family = o.kernel != PK_KERNEL_AUTO; return pick(K::RandParity); };
    if (n_sites == 7 && exact == 1 && f.rand_dense_available) return parity();
    if (f.rand_dense_available && exact != 0) return pick(K::RandDense);   // n = 7, PK_WIDE_RAND_EXACT=2 (PK_WIDE_RAND_DENSE=0 also selects the n-cube kernel)
    if (n_sites == 8 && exact != 0) return exact == 2 ? pick(K::RandLevel) : parity();
    return p;
  }
  if (model == PK_MODEL_RAND && n_sites == 6 && sw.rand_level6 == 1 && lrp12) { p.kernel = K::RandLevel; return over() ? refuse(PK_ERR_ARG, too_large) : p; }
  if (model == PK_MODEL_RAND && ((n_sites == 6 && sw.rand_parity56 != 0) || (n_sites == 5 && sw.rand_parity56 == 1)) && lrp12 && o.linsolve == PK_LINSOLVE_AUTO) {
    p.kernel = K::RandParity;
    return over() ? refuse(PK_ERR_ARG, too_large) : p;
  }
  const bool rand_fast = model == PK_MODEL_RAND && resolvent_method(o.method) && (o.linsolve == PK_LINSOLVE_AUTO || S > 64) && !o.stage_form;
  if (S > 64 && !rand_fast)       // n = 6: the in-register inverse of pk_rand_fast.hpp is the only solver (every `linsolve` value selects it)
    return refuse(PK_ERR_UNSUPPORTED, "randmod n_sites = 6 (S = 65): only method RODAS4 / LRP8 in resolvent form (the generic kernels hold one state per lane)");
  p.G = S > 64 ? 64 : group_width(S);
  const long long rpb = 256 / p.G;
  p.launches = (B + rpb - 1) / rpb;
  if (over()) return refuse(PK_ERR_ARG, too_large);
  p.structured = o.linsolve != PK_LINSOLVE_DENSE && model != PK_MODEL_RAND;
  // small systems, large batches: one lane per replica (64 replicas per wave: the batch must be large enough to occupy the SIMDs).
  // Thresholds from tools/gpu_bench_dev.py tprB (crossover against the lane-group kernels).  opts->kernel pins the family (sharded runs
  // that must reproduce single-GPU bits); the PK_TPR=0 / 1 environment variable does the same for dev A/B runs.
  const int tpr_pin = o.kernel == PK_KERNEL_GROUP ? 0 : o.kernel == PK_KERNEL_TPR ? 1 : sw.tpr;
  const long long tpr_min = model == PK_MODEL_SUCC ? (n_sites <= 8 ? 16384 : 32768) : model == PK_MODEL_RAND ? 32768 : (n_sites <= 8 ? 32768 : 49152);
  if (lrp12 && o.linsolve == PK_LINSOLVE_AUTO && f.tpr_available && (tpr_pin == 1 || (tpr_pin != 0 && B >= tpr_min))) return pick(K::Tpr);
  if (model == PK_MODEL_DIST && resolvent_method(o.method) && o.linsolve == PK_LINSOLVE_AUTO && !o.stage_form) {
    p.kernel = K::DistFast;                                              // throughput layout: 4-16 lanes per replica, shadowed or resident R / P rows
    return sw.dist_sched < 0 ? refuse(PK_ERR_ARG, "PK_DIST_SCHED must be one of: ") : p;
  }
  return pick(rand_fast ? K::RandFast : K::Group);                       // RandFast: 2^n lanes per replica, shadowed mRNA row
}

}  // namespace pk
