// pk_net_plan.hpp -- which kernel a network launch runs, with which method, threads and tangent chunking, or why it is refused: one pure
// host function, net_plan, for every flavour of launch.  Plain C++ over include/phoskin.h: no HIP, no getenv, no statics, so it compiles
// under hipcc (pk_network.hip, its only user in the library) and under g++ (tests/test_net_plan_cpu.py holds it to a table of plans).  The
// caller brings in what lives elsewhere: byte counts and predicates defined next to the kernels (NetFacts) and the environment knobs
// (NetSwitches); it launches what the plan says and never adjusts it.  The tests run in the order in which the entry points have always
// made them: where two refusals apply, the earlier one answers.
#pragma once
#include <cstddef>
#include "../../include/phoskin.h"

namespace pk {

enum class NetKernel { DP5, Workspace, ArkPair, Ark, CombReg, Reg, Lds };
// Plain: pk_network_simulate_batch.  ScoreTables / ScoreLists: ..._objective_batch on the loss handle's dense tables / time-bucketed lists
// (the entry point picks the lists for PK_METHOD_ROS34PW2 or PK_KERNEL_WORKSPACE).  Measure: ..._measure_batch.  Sens / SensScore:
// ..._sens_batch / ..._objective_grad_batch with K > 0 columns; their K = 0 forms are Plain / ScoreLists with net_tangent_opts
enum class NetFlavour { Plain, ScoreTables, ScoreLists, Measure, Sens, SensScore };

struct NetFacts {
  int model, N, S, n_var, max_sites;
  size_t solve_lds, solve_fused_lds, solve_reg_lds, rk45_lds, ark_lds;   // dynamic LDS in bytes: net_solve_lds_bytes, net_solve_fused_lds_bytes, net_solve_reg_lds_bytes,
                                                                         // net_rk45_lds_bytes, net_ark_lds_bytes at one thread per protein in whole waves
  bool arkp_fits, arkp_fuses_loss;                                       // net_arkp_fits, net_arkp_fuses_loss
  int sens_lds_columns, sens_score_lds_columns;                          // pk_network_sens_columns_per_launch, pk_network_objective_grad_columns_per_launch
};
struct NetSwitches {
  int net_threads = 0;       // PK_NET_THREADS: 64 / 128 / 256 threads for the general LDS kernel where the network fits them, else ignored
  int sens_hbm_width = 16;   // W, the slab route's columns per work item, after PK_NET_SENS_KC lowered it
};
struct NetPlan {
  int method;                // PK_METHOD_DP5 / ARK436 / ROS34PW2; of a refused plan PK_ERR_UNSUPPORTED, except a DP5 request refused for the network's size
  NetKernel kernel;
  int code;
  const char* refusal;       // null when accepted
  int threads;               // Lds: 64 / 256 by size; ARK and register kernels: one thread per protein, in whole waves; else unused
  int KC;                    // Sens / SensScore: columns per workgroup (LDS route) or per work item (slabs); 0 elsewhere
  bool hbm;                  // Sens / SensScore: state and tangents on HBM slabs (kernel == Workspace) instead of in LDS (kernel == Lds)
};

constexpr size_t kNetLdsLimit = 160 * 1024;      // dynamic LDS of one workgroup

inline int net_sens_hbm_columns(int K, int n_var, int W) { return K < n_var ? (K < W ? K : W) : (n_var < W ? n_var : W); }   // min(K, n_var, W)

// What the two tangent entry points integrate with, whatever method and linsolve the caller names: the order-3 method on the general LDS
// kernel, with PK_KERNEL_HBM on the workspace kernel
inline pk_solver_opts net_tangent_opts(pk_solver_opts o) {
  o.kernel = o.kernel == PK_KERNEL_HBM ? PK_KERNEL_WORKSPACE : PK_KERNEL_AUTO;
  o.method = PK_METHOD_ROS34PW2; o.linsolve = PK_LINSOLVE_STRUCTURED;
  return o;
}

// Method and kernel of the state integration.  PK_METHOD_DP5 on request; PK_METHOD_ARK436 where its kernel fits and is the default (or
// was asked for); otherwise PK_METHOD_ROS34PW2, on the workspace kernel for networks beyond the one-workgroup LDS kernels (S > 1024,
// N > 512, or more than 160 KiB of LDS for the general one; small combinatorial blocks run out of registers and are exempt) and on request
inline NetPlan net_state_plan(const NetFacts& f, const pk_solver_opts& o) {
  const bool structured = o.linsolve == PK_LINSOLVE_STRUCTURED, ws_forced = o.kernel == PK_KERNEL_WORKSPACE;
  const int threads = ((f.N + 63) / 64) * 64;
  const auto take = [&](int m, NetKernel k) { return NetPlan{m, k, PK_OK, nullptr, threads, 0, false}; };
  const auto refuse = [&](int m, const char* why) { return NetPlan{m, NetKernel::Lds, PK_ERR_UNSUPPORTED, why, threads, 0, false}; };
  if (o.kernel == PK_KERNEL_HBM)
    return refuse(PK_ERR_UNSUPPORTED, "PK_KERNEL_HBM is read by pk_network_simulate_sens_batch and pk_network_simulate_objective_grad_batch only; "
                                      "ask for PK_KERNEL_WORKSPACE here");
  if (o.method == PK_METHOD_DP5) {
    if (ws_forced) return refuse(PK_ERR_UNSUPPORTED, "PK_KERNEL_WORKSPACE integrates with PK_METHOD_ROS34PW2 only");
    if (f.S > 1024 || f.N > 512) return refuse(PK_METHOD_DP5, "PK_METHOD_DP5: S <= 1024 states and N <= 512 proteins per network");
    if (f.rk45_lds > kNetLdsLimit) return refuse(PK_METHOD_DP5, "network too large for one workgroup's LDS (160 KiB)");
    return take(PK_METHOD_DP5, NetKernel::DP5);
  }
  // combinatorial blocks: <= 3 sites per protein (and N <= 256) run one thread per protein out of registers (pk_network_solve_reg2.hpp);
  // larger blocks run in the general LDS kernel with the same approximate factorisation, swept serially by the protein's thread
  const bool comb_reg = f.model == 2 && f.max_sites <= 3 && f.N <= 256;
  if (ws_forced || f.S > 1024 || f.N > 512 || (!comb_reg && f.solve_lds > kNetLdsLimit)) {
    if (o.method == PK_METHOD_ARK436)
      return refuse(PK_ERR_UNSUPPORTED, "PK_METHOD_ARK436: not on the workspace kernel (networks beyond one workgroup's LDS); use PK_METHOD_ROS34PW2");
    return take(PK_METHOD_ROS34PW2, NetKernel::Workspace);
  }
  // one thread per protein (N <= 256), or [r3] the dense lane layout of topologies 0 / 1 / 4 (<= 512 lanes: up to 512 proteins)
  const bool ark_fits = f.N <= 256 && f.max_sites <= (f.model == 2 ? 3 : 8) && !structured;
  const bool ark_ok = (ark_fits && f.ark_lds <= kNetLdsLimit) || (!structured && f.arkp_fits);
  if (o.method == PK_METHOD_ARK436 && !ark_ok)
    return refuse(PK_ERR_UNSUPPORTED, "PK_METHOD_ARK436: <= 8 sites per protein and N <= 256 (topologies 0 / 1 / 4: <= 512 lanes of the dense layout); "
                                      "combinatorial topology: <= 3 sites, N <= 256; use PK_METHOD_ROS34PW2");
  // [r3] the combinatorial topology takes the additive method by default too: with the EXACT block solve (parity elimination of the
  // bit-pattern block, pk_network_solve_ark.hpp) it needs 4.6x fewer steps than the order-3 method and runs 1.8x faster at equal band error
  if (ark_ok && o.method != PK_METHOD_ROS34PW2) return take(PK_METHOD_ARK436, f.arkp_fits ? NetKernel::ArkPair : NetKernel::Ark);
  // ROS34PW2: the register-resident kernels (one thread per protein) when every block fits their per-thread arrays; PK_LINSOLVE_STRUCTURED
  // forces the LDS kernel (kept as the general fallback and as the A/B reference)
  if (comb_reg && !structured) return take(PK_METHOD_ROS34PW2, NetKernel::CombReg);
  if (f.model != 2 && f.N <= 256 && f.max_sites <= 8 && f.solve_reg_lds <= 64 * 1024 && !structured) return take(PK_METHOD_ROS34PW2, NetKernel::Reg);
  return take(PK_METHOD_ROS34PW2, NetKernel::Lds);
}

// `asked`: the caller's options (pk_default_opts for NULL).  K: the tangent columns of Sens / SensScore, ignored elsewhere
inline NetPlan net_plan(const NetFacts& f, const pk_solver_opts& asked, NetFlavour fl, int K, const NetSwitches& sw) {
  using NK = NetKernel;
  const bool score = fl == NetFlavour::SensScore, tangents = score || fl == NetFlavour::Sens, lists = fl == NetFlavour::ScoreLists || fl == NetFlavour::Measure;
  NetPlan p{PK_ERR_UNSUPPORTED, NK::Lds, PK_OK, nullptr, 0, 0, false};
  const auto refuse = [&p](const char* why) { p.code = PK_ERR_UNSUPPORTED; p.refusal = why; return p; };
  pk_solver_opts o = asked;
  int KC = 0;
  if (tangents) {
    // always the order-3 method: an explicit request for another integrator, or for the state-only workspace kernel, is refused by name
    if (asked.method == PK_METHOD_ARK436 || asked.method == PK_METHOD_DP5)
      return refuse(score ? "objective gradients integrate with PK_METHOD_ROS34PW2 only: leave opts->method at its default or ask for PK_METHOD_ROS34PW2"
                          : "network sensitivities integrate with PK_METHOD_ROS34PW2 only: leave opts->method at its default or ask for PK_METHOD_ROS34PW2");
    if (asked.kernel == PK_KERNEL_WORKSPACE)
      return refuse(score ? "objective gradients: PK_KERNEL_WORKSPACE names the state kernel; leave opts->kernel at PK_KERNEL_AUTO, or "
                            "ask for the tangents on HBM slabs with PK_KERNEL_HBM"
                          : "network sensitivities: PK_KERNEL_WORKSPACE names the state kernel; leave opts->kernel at PK_KERNEL_AUTO, or "
                            "ask for the tangents on HBM slabs with PK_KERNEL_HBM");
    o = net_tangent_opts(asked);
    // the LDS kernel where a column fits beside the state; the slabs on request and wherever it does not
    KC = asked.kernel == PK_KERNEL_HBM ? 0 : score ? f.sens_score_lds_columns : f.sens_lds_columns;
    if (KC < 1) { KC = net_sens_hbm_columns(K, f.n_var, sw.sens_hbm_width); o.kernel = PK_KERNEL_WORKSPACE; }
  }
  p = net_state_plan(f, o);
  if (p.code != PK_OK) return p;
  p.KC = KC; p.hbm = tangents && o.kernel == PK_KERNEL_WORKSPACE;
  const bool reg = p.kernel == NK::Reg || p.kernel == NK::CombReg, rosw = p.kernel == NK::Lds || p.kernel == NK::Workspace;
  if (fl == NetFlavour::ScoreTables && !(p.kernel == NK::ArkPair && f.arkp_fuses_loss))
    return refuse("fused objective: topologies 0 / 1 / 4 on the default additive integrator only; use pk_network_simulate_batch + pk_network_objective_batch");
  if (fl == NetFlavour::Measure && reg)
    return refuse("fused measurement: not on the register-resident kernels; ask for the general LDS kernel "
                  "(opts->linsolve = PK_LINSOLVE_STRUCTURED, kernel = \"lds\" in Python) or PK_KERNEL_WORKSPACE");
  if (fl == NetFlavour::Measure && !rosw)
    return refuse("fused measurement: the order-3 integrator only; ask for opts->method = PK_METHOD_ROS34PW2 (method = \"rosw\" in Python) on the general "
                  "LDS kernel or the workspace kernel, or call pk_network_simulate_batch + pk_network_observables_batch");
  if (fl == NetFlavour::ScoreLists && reg)
    return refuse("fused objective with PK_METHOD_ROS34PW2: not on the register-resident kernels; ask for the general LDS kernel "
                  "(opts->linsolve = PK_LINSOLVE_STRUCTURED, kernel = \"lds\" in Python) or PK_KERNEL_WORKSPACE");
  // unreachable through pk_network_simulate_objective_batch: it picks this flavour only for PK_METHOD_ROS34PW2 or PK_KERNEL_WORKSPACE, and
  // with either net_state_plan answers Workspace, CombReg, Reg, Lds or a refusal of its own
  if (fl == NetFlavour::ScoreLists && !rosw) return refuse("fused objective on request: PK_METHOD_ROS34PW2 on the LDS or the workspace kernel only");
  // unreachable with the facts of a real network: net_tangent_opts leaves net_state_plan Lds or Workspace, a column count >= 1 means
  // S <= 1024, N <= 512 and an LDS request within 160 KiB that contains solve_lds (so Lds), and the slab route forces Workspace
  if (tangents && p.kernel != (p.hbm ? NK::Workspace : NK::Lds))
    return refuse("network sensitivities: the plan for these options is neither the general LDS kernel nor the HBM-workspace kernel");
  // the rna baseline (N doubles) comes on top of the LDS of a plain launch: past 160 KiB the workspace kernel takes over
  if (lists && p.kernel == NK::Lds && f.solve_fused_lds > kNetLdsLimit) p.kernel = NK::Workspace;
  if (p.kernel == NK::Lds) {
    // every thread owns <= 4 states and <= 2 proteins (register-cached contexts in the kernel)
    p.threads = (f.S <= 128 && f.N <= 64) ? 64 : 256;                 // measured at S = 500: 256 threads beat 128 by 1.33x
    const int v = sw.net_threads;
    if ((v == 64 || v == 128 || v == 256) && f.S <= 4 * v && f.N <= 2 * v) p.threads = v;
    if (tangents && (size_t)(K < KC ? K : KC) * f.S > 512) p.threads = 256;
  }
  return p;
}

}  // namespace pk
