// pk_dist_fast.hpp -- throughput kernel for the distributive model (models/distmod.py:7-65), adaptive resolvent-form one-step
// methods (RODAS4, LRP8, LRP12: ResolventTab).
//
// Same integrator, same arithmetic per state as solve_kernel<M_DIST, G, RODAS4, true> (arrow elimination), but laid
// out for the VALU instead of for generality -- measured on MI355X the generic kernel spends its time in the LDS
// crossbar (ds_swizzle broadcasts / reductions: 194 LDS-pipe instructions per step, profiles/r01_a_*):
//
//   * a replica is owned by G lanes (G = 4, 8 or 16), each lane holding RPL site rows in registers
//     (site i = lane + G * j), so S = 32 runs EIGHT replicas per wavefront instead of two;
//   * SHADOWED layout (RES = false: every size of the RODAS4 / LRP8 table, and the LRP12 sizes whose lane layout has no two spare
//     slots): the two coupling rows (mRNA R and unphosphorylated protein P) are "shadowed": every lane of the group carries
//     them and updates them redundantly, so no broadcast is ever needed.  The copies agree to rounding, not to the bit: each lane
//     inverts 1 + q B in a chain with its own site pivots (factor(), below), so the lanes' R and P drift a few ulps apart (4.7e-14
//     relative at most in the CPU model, tools/pivot_chain_sensitivity.py).  Everything that steers a replica -- the error norm, the
//     site sum, the non-finite test -- is reduced over the group and so uniform; lane 0 emits R and P;
//   * RESIDENT layout (RES = true: the LRP12 sizes with G * RPL >= n + 2, the benchmark's n = 30 on 4 x 8 among them): R and P ride in
//     slots 0 and 1 of the lane layout as rows of lanes 0 and 1, the sites follow in state order.  There is ONE copy of each (nothing to
//     agree or drift), no lane pushes a redundant R / P through the stages, and no row is idle at n + 2 = G * RPL.  Described at the
//     kernel, below;
//   * the step loop never evaluates the right-hand side: f(y) = J y + b is affine (b = A in row R, zero elsewhere) and J = (I - M) / q,
//     so the first stage is  M^{-1} h f(y) = (M^{-1} (y + q b) - y) / gamma  -- the same solve() on the state itself with q A added to
//     row R, then one subtraction per row; 1 / gamma is folded into the tableau weights at compile time.  The site sum that closes
//     row P, its only reader the right-hand side, is formed in the prologue (initial step estimate) and in the cold non-finite test.
//     A stage costs exactly ONE group reduction (inside the arrow solve); all of them are DPP moves only;
//   * LRP8 and LRP12 take their error estimate as a repeated difference: two solves, then NS - 2 stages v <- v - M^{-1} v, each cheaper than a
//     solve (one multiply and one FMA per row, the group sum's input from a sum carried from stage to stage); y_new is summed in that basis
//     (ResolventTab::BN) and the estimate is the last v times E_2 / gamma -- no second accumulation.  RODAS4 keeps both weighted sums;
//   * SCALED rows (dist_scaled(), below: the parked LRP12 layouts with registers to spare, the benchmark's 4 x 8 resident among them): a site
//     row goes through the stages in units of its own coupling weight c_j = winv_j s_j (s_j: the row's rate, fixed per replica in the
//     prologue), so that x_P enters every row with the coefficient 1: a solve and a difference stage are ONE FMA per row, the group sum's
//     input is an FMA dot product, and nothing is tracked from stage to stage.  The state is divided into those units once per step
//     (rho_j = y_j ic_j; or enters the first stage as itself, dist_stage1_state()) and y_new and the error row are multiplied back once
//     per step.  Described at factor() and solve() in the kernel;
//   * no LDS-pipe instruction in the solve chain; LDS only as thread-private parking space in the PARK layouts (below).
//
// pk_dist_rows.hpp holds the rows a lane carries (Stg) and what is done for every row of a lane -- the vector updates, both error norms,
// the sign-bit OR and the clip -- once over the lane's row list, whichever layout the rows come from.  Wave pacing and the wave trace are
// two helpers below (DistPace, DistWaveTrace), empty unless their flag is on.
//
// dR/dt = A - B R ; dP/dt = C R - (D + sum S_i) P + sum X_i ; dX_i/dt = S_i P - (1 + D_i) X_i
#pragma once
#include "pk_dist_rows.hpp"
#include "pk_env.hpp"

namespace pk {

// the sum over all sites of a replica: a tree over the lane's rows, then the group reduction
template <int G, int RPL>
__device__ __forceinline__ double site_sum(const double (&s)[RPL], int lane) { return gsum<G>(tree_sum(s), lane); }

// What is uniform over a launch and chosen by run-time fields of SolveArgs, as a compile-time configuration.  DistFixed names one
// combination (the launchers pick it when SolveArgs matches); DistAny reads every choice from SolveArgs at run time and serves the rest.
//   metric class: none / running sum only (total_signal, mean_activity) / second moments and first differences (the other metrics)
enum { PK_DM_NONE = 0, PK_DM_SUM = 1, PK_DM_FULL = 2 };
__host__ __device__ __forceinline__ int dist_metric_class(const SolveArgs& A) {
  return !A.metric ? PK_DM_NONE : (A.metric_id == PK_METRIC_TOTAL_SIGNAL || A.metric_id == PK_METRIC_MEAN_ACTIVITY) ? PK_DM_SUM : PK_DM_FULL;
}
template <bool CLIP, bool NORM, bool FLAT, bool SOL, int MC>
struct DistFixed {
  static constexpr int SLOT_MC = MC;                 // which bookkeeping slots exist (Parked)
  static constexpr bool LITERAL = false;             // the step loop's error norm is err_norm; a landing does not mask its idle rows
  __host__ __device__ static __forceinline__ bool clip(const SolveArgs&) { return CLIP; }
  __host__ __device__ static __forceinline__ bool normalize(const SolveArgs&) { return NORM; }
  __host__ __device__ static __forceinline__ bool flat(const SolveArgs&) { return FLAT; }
  __host__ __device__ static __forceinline__ bool sol(const SolveArgs&) { return SOL; }
  __host__ __device__ static __forceinline__ int mclass(const SolveArgs&) { return MC; }
  static bool matches(const SolveArgs& A) {
    return (A.clip != 0) == CLIP && (A.normalize != 0) == NORM && (A.flat != nullptr) == FLAT && (A.sol != nullptr) == SOL && dist_metric_class(A) == MC;
  }
};
struct DistAny {
  static constexpr int SLOT_MC = PK_DM_FULL;
  // the run-time kernel keeps the literal forms -- the NaN-propagating maximum (group_max) in the step loop, idle rows masked to zero at
  // a landing: slower, and what the specialised kernels are tested against (tests/test_gpu_dist_fast_variants.py on healthy replicas,
  // tests/test_gpu_dist_fast_norm.py on replicas with non-finite parameters)
  static constexpr bool LITERAL = true;
  __host__ __device__ static __forceinline__ bool clip(const SolveArgs& A) { return A.clip != 0; }
  __host__ __device__ static __forceinline__ bool normalize(const SolveArgs& A) { return A.normalize != 0; }
  __host__ __device__ static __forceinline__ bool flat(const SolveArgs& A) { return A.flat != nullptr; }
  __host__ __device__ static __forceinline__ bool sol(const SolveArgs& A) { return A.sol != nullptr; }
  __host__ __device__ static __forceinline__ int mclass(const SolveArgs& A) { return dist_metric_class(A); }
  static bool matches(const SolveArgs&) { return true; }
};
// the combinations the library's own callers produce (batch.solve_ode_batch): trajectories + a running-sum metric (the Morris scan),
// trajectories alone, the flat observable vector alone (the fits); all clipped, none normalised
using DistSolSum = DistFixed<true, false, false, true, PK_DM_SUM>;
using DistSolOnly = DistFixed<true, false, false, true, PK_DM_NONE>;
using DistFlatOnly = DistFixed<true, false, true, false, PK_DM_NONE>;

// number of per-lane slots: site rates S_i and 1 + D_i always; the running sum from PK_DM_SUM on; previous outputs, second moment, first
// differences and shift only in PK_DM_FULL (the resident layout has no previous R / P beside the previous outputs of its slots: two fewer)
template <int RPL, int MC, bool RES = false> constexpr int dist_fast_slots() {
  return MC == PK_DM_FULL ? 3 * RPL + (RES ? 4 : 6) : MC == PK_DM_SUM ? 2 * RPL + 1 : 2 * RPL;
}

// Per-lane values that are touched once per step (site rates) or once per output (metric bookkeeping).  In registers by default;
// PARK = true keeps them in LDS (slot-major: slot * NT + thread, conflict-free), which frees up to 6 * RPL + 12 VGPRs: what lets the
// 4-lane x 8-row layout (30 % fewer instructions per replica than 8 x 4) run two waves per SIMD instead of one.
template <int RPL, bool PARK, int NT> struct Parked;
template <int RPL, int NT> struct Parked<RPL, false, NT> {
  double v[3 * RPL + 6];
  __device__ __forceinline__ explicit Parked(double*) {}
  template <int K> __device__ __forceinline__ double get() const { return v[K]; }
  template <int K> __device__ __forceinline__ void set(double x) { v[K] = x; }
  __device__ __forceinline__ void fence() {}
};
template <int RPL, int NT> struct Parked<RPL, true, NT> {
  typedef __attribute__((address_space(3))) double lds_double;
  lds_double* base;
  __device__ __forceinline__ explicit Parked(double* lds) : base((lds_double*)lds + threadIdx.x) {}
  template <int K> __device__ __forceinline__ double get() const { return base[K * NT]; }
  template <int K> __device__ __forceinline__ void set(double x) { base[K * NT] = x; }
  // no instruction: the compiler forgets what it knows about the slots' contents, so a get() after it is a real LDS read and not a
  // value it kept alive (or copied) in registers since the matching set()
  __device__ __forceinline__ void fence() { asm volatile("" : "+v"(base)); }
};
// the parked layouts keep the site rows of the accepted state in RPL more slots (the step loop reads them at the top of a step, accepting lanes write them)
template <int RPL, bool PARK, int NT = 256, class CFG = DistAny, bool RES = false>
constexpr size_t dist_fast_lds_bytes() { return PARK ? (size_t)(dist_fast_slots<RPL, CFG::SLOT_MC, RES>() + RPL) * NT * sizeof(double) : 0; }

// Wave pacing (SolveArgs::sched; the parked one-wave LRP12 kernels only, every other instantiation ignores the field).  The waves of a SIMD
// share its VALU by priority, then by age, and nothing else in this kernel sets a priority: the policies below only tell the arbiter which
// wave to prefer.  They move no work, wait on nothing and change no value; a wrong guess costs time, never progress.
//   LEAD   when the grid exceeds the resident capacity R1 (SolveArgs::R1: more than one round of waves), one first-round wave per SIMD runs
//          at priority 3 for its whole life, so that it ends early and the SIMD's next wave starts as early as possible.  Two rules name
//          that wave: LEAD_SLOT, hardware wave slot 0 among the workgroups below R1; LEAD_BLOCK, the workgroups below R1 / 3;
//   LEVEL  every other wave takes its priority from its own progress, the output index k of its slowest live replica: 2 before output
//          PK_DSCHED_K2, 1 before PK_DSCHED_K1, 0 from there on (4 + 4 + 5 of the benchmark's 13 intervals), re-evaluated at the top of
//          each step.  Two v_cmp on the lanes' k feed the scalar unit, which does the rest; with the policy off a uniform branch skips them.
// The PK_DSCHED_* bits of the policies live with the parser of the switch that names them (pk_env.hpp).
constexpr int PK_DSCHED_K2 = 5, PK_DSCHED_K1 = 9;
// s_getreg operands: id | offset << 6 | (size - 1) << 11.  HW_ID (register 4): wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]
constexpr int PK_HWREG_HW_ID = 4 | (31 << 11), PK_HWREG_HW_ID_WAVE = 4 | (3 << 11), PK_HWREG_XCC_ID = 20 | (31 << 11);

template <bool PACE> struct DistPace {           // PACE = false: nothing
  __device__ __forceinline__ void enter(const SolveArgs&) {}
  __device__ __forceinline__ void step(int) const {}
};
template <> struct DistPace<true> {
  bool paced = false;
  // everything here is uniform over the wave (kernel arguments, blockIdx, a hardware register) and runs on the scalar unit
  __device__ __forceinline__ void enter(const SolveArgs& A) {
    const int sched = A.sched;
    if (sched != PK_DSCHED_OFF) {
      bool leader = false;
      if ((int)gridDim.x > A.R1) {
        if (sched & PK_DSCHED_LEAD_SLOT) leader = (int)blockIdx.x < A.R1 && __builtin_amdgcn_s_getreg(PK_HWREG_HW_ID_WAVE) == 0;
        if (sched & PK_DSCHED_LEAD_BLOCK) leader = leader || (int)blockIdx.x < A.R1 / 3;
      }
      if (leader) __builtin_amdgcn_s_setprio(3);
      paced = !leader && (sched & PK_DSCHED_LEVEL) != 0;
    }
  }
  // k: this lane's output index.  The slowest live replica of the wave decides: a replica that is done has left the loop and no longer votes
  __device__ __forceinline__ void step(const int k) const {
    if (paced) {
      if (__builtin_amdgcn_ballot_w64(k < PK_DSCHED_K2) != 0) __builtin_amdgcn_s_setprio(2);
      else if (__builtin_amdgcn_ballot_w64(k < PK_DSCHED_K1) != 0) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
  }
};

// Wave timeline of the diagnostic build (TRACE = 1, one instantiation in pk_inst_dist_fast12t.hip; no shipped kernel holds any of it):
// lane 0 of each wave writes one record, at entry and again before finish(), to a buffer of its own that nothing else reads.
struct DistTraceRec {
  unsigned long long t_entry, t_exit;      // s_memrealtime (100 MHz)
  unsigned block, hw_id, xcc_id, iters;    // blockIdx.x, raw HW_ID and XCC_ID, step-loop iterations of the wave
};
struct DistTraceBuf { DistTraceRec* rec; long long capacity; };
template <int TRACE> struct DistTrace;     // get(): the buffer; specialised where the traced kernel is instantiated

template <int TRACE> struct DistWaveTrace {
  int witer = 0;                           // this lane's trips through the step loop
  __device__ __forceinline__ void enter() {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const DistTraceBuf tb = DistTrace<TRACE>::get();
    if (threadIdx.x == 0 && tb.rec && (long long)blockIdx.x < tb.capacity) {
      DistTraceRec* r = tb.rec + blockIdx.x;
      r->t_entry = t0; r->t_exit = 0; r->block = blockIdx.x; r->iters = 0;
      r->hw_id = __builtin_amdgcn_s_getreg(PK_HWREG_HW_ID); r->xcc_id = __builtin_amdgcn_s_getreg(PK_HWREG_XCC_ID);
    }
  }
  __device__ __forceinline__ void step() { ++witer; }
  __device__ __forceinline__ void exit() const {
    int it = witer;
    for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(it, o); it = v > it ? v : it; }
    const DistTraceBuf tb = DistTrace<TRACE>::get();
    if (threadIdx.x == 0 && tb.rec && (long long)blockIdx.x < tb.capacity) {
      DistTraceRec* r = tb.rec + blockIdx.x;
      r->iters = (unsigned)it; r->t_exit = __builtin_amdgcn_s_memrealtime();
    }
  }
};
template <> struct DistWaveTrace<0> {      // the shipped kernels: nothing
  __device__ __forceinline__ void enter() {}
  __device__ __forceinline__ void step() {}
  __device__ __forceinline__ void exit() const {}
};

// Which layouts carry their site rows in units of the rows' coupling weight (the scaled stages of factor() / solve() / diff() in the kernel): a
// trait of the method, the rows per lane and the row placement, shared by the four output classes of a layout as they share its placement.
// Scaling keeps 1 / s_j of every scaled row in registers (the parked slots have no room for it at the occupancy they run at), two VGPRs per
// row that nothing can take back, so it is on exactly where no specialised kernel of the layout loses a wave per SIMD to them
// (tools/kernel_resources.py against the waves the layout's parked slots admit; the table is in DESIGN.md 4.3):
//   resident   6 and 8 rows per lane (n = 21, 22, 29, 30 on four lanes, 41 .. 46 and 57 .. 62 on eight; the benchmark's 4 x 8, its 256-thread
//              variant and the traced build among them);
//   shadowed   5, 6 and 7 rows per lane (n = 19, 20, 23, 24, 27, 28 on four lanes, 39, 40, 47, 48, 55, 56 on eight; and the resident sizes of
//              those row counts under PK_DIST_LAYOUT=shadow).
// Five resident rows run at five waves per SIMD with 96 registers and none to spare (104 scaled); at seven resident rows the sol + sum kernel
// would need 130 against the 128 of four waves; at eight shadowed rows the flat-output kernel of the four-lane layout 171 against the 168
// of three; the unparked layouts (RPL <= 4, LRP12 and the RODAS4 / LRP8 table) were not tried: all of these keep plain units.
// PK_DIST_SCALE_MIN: the smallest rate that serves as a row's scale (the kernel's prologue).
template <int METHOD, int RPL, bool PARK, bool RES> constexpr bool dist_scaled() {
  return PARK && ResolventTab<METHOD>::DIFFERENCE && (RES ? (RPL == 6 || RPL == 8) : (RPL >= 5 && RPL <= 7));
}
constexpr double PK_DIST_SCALE_MIN = 0x1p-600;
// Which scaled layouts form the FIRST stage of a step from the state rows themselves (solve(r, std::true_type) in the kernel): t_j = kappa_j y_j
// with kappa_j = d_j / s_j in the registers that otherwise hold 1 / s_j, instead of rho_j = y_j ic_j with ic_j = piv_j / s_j formed in
// factor().  One operation fewer per scaled row and step, but winv_j of the scaled rows then lives from factor() to the first dot product,
// and two layouts have no registers for that: the flat-output kernels of six resident rows stand at the 128 of four waves per SIMD and
// would need 130 (4 x 6) and 132 (8 x 6); of five shadowed rows, 8 x 5 would need 132 against the same 128 and 4 x 5 stands at 128 exactly.
// So: resident 8 rows, shadowed 6 and 7.  A trait of the layout, shared by its four output classes like dist_scaled(), since it moves bits
// (by roundings: tools/stage1_form_sensitivity.py).
template <int METHOD, int RPL, bool PARK, bool RES> constexpr bool dist_stage1_state() {
  return dist_scaled<METHOD, RPL, PARK, RES>() && (RES ? RPL == 8 : RPL != 5);
}
// Which resident instantiations end factor() with arithmetic on two per-lane constants (selP, notP: two VGPR pairs) where the others keep
// four selects on isP.  Same bits either way (factor(), below), so this is decided kernel by kernel: everywhere but where the four
// registers cost a wave per SIMD -- 96 -> 102 VGPRs at five rows (sol + sum, sol only: five waves), 128 -> 136 in the flat-output kernel at
// six rows (four waves), and two unparked kernels (one row run-time 78 -> 82, two rows flat-only 72 -> 76).  A parked slot instead of the
// registers does not help the first: 16 slots x 512 B is what lets five waves per SIMD share the CU's LDS.
template <int RPL, class CFG> constexpr bool dist_pslot_arith() {
  constexpr bool any = std::is_same<CFG, DistAny>::value, flat = std::is_same<CFG, DistFlatOnly>::value;
  return !(RPL == 1 && any) && !(RPL == 2 && flat) && !(RPL == 5 && !any && !flat) && !(RPL == 6 && flat);
}

// NT threads per workgroup (256, or 64 = one wave: a finished wave's slot is refilled at once instead of when the slowest of four is done)
//
// RES = true is the RESIDENT layout, for sizes whose whole state fits the lane layout (G * RPL >= n + 2): the state vector is laid over
// the G x RPL slots in state order, slot s = lane + G * row holding state s -- R in slot 0 (lane 0, row 0), P in slot 1 (lane 1, row 0),
// site i in slot i + 2, slots >= n + 2 idle (rate 0, diagonal 1, value 0).  Nothing is shadowed: R and P go through the stages, the
// error norm, the parked K_Y slots and a landing as rows of their lanes, and only row 0 ever differs between the lanes of a group:
//   * solve: R is a row with pivot 1 + q B and no coupling; the P slot's "pivot" is q itself, so that its t is r_P / q and the ONE group
//     sum  C x_R + r_P / q + sum t_i  (row 0 enters with the per-lane weight w0 = C, 1, 1, ...) times q sinv is x_P;
//   * first stage: row 0 of the solved vector is fma(q, k3, y_0) with k3 = A | 0 | 0 (lane 0 | lane 1 | the others): y_R + q A in the R
//     slot, the state itself elsewhere;
//   * right-hand side (prologue only, for the initial step estimate): R and P are broadcast from their lanes; row 0 is
//     fma(k1, P, fma(-dg0, X, k3)) with per-lane k1 = 0 | -Dsum | S_i, dg0 = B | -C | 1 + D_i, X = R | R | x_i, k3 = A | sg | 0;
//   * the site sum skips the R and P slots; every reduction that steers a replica is still a group reduction.
template <int G, int RPL, int METHOD, bool PARK = false, int MINB = (PARK ? 2 : 1), int NT = 256, class CFG = DistAny, bool RES = false, int TRACE = 0>
__global__ __launch_bounds__(NT, MINB) void dist_fast_kernel(const SolveArgs A) {
  using Tab = ResolventTab<METHOD>;
  using Vec = Stg<RPL, RES>;
  constexpr bool SCL = dist_scaled<METHOD, RPL, PARK, RES>();     // scaled site rows (factor(), below); J0: the first of them
  constexpr int J0 = RES ? 1 : 0;
  constexpr bool S1 = dist_stage1_state<METHOD, RPL, PARK, RES>();     // the first stage from the state rows (solve(), below)
  constexpr bool PAR = RES && dist_pslot_arith<RPL, CFG>();        // the P slot's fix-ups as arithmetic (factor(), below)
  static_assert(!TRACE || NT == 64, "the trace holds one record per workgroup: one wave each");
  DistWaveTrace<TRACE> trace;
  trace.enter();
  DistPace<PARK && NT == 64 && METHOD == PK_METHOD_LRP12> pace;
  pace.enter(A);
  extern __shared__ __align__(16) double park_lds[];
  Parked<RPL, PARK, NT> pk(park_lds);
  // the parked slots of every wave the launch bounds promise a CU (4 SIMDs x MINB) must fit its 160 KiB; the tightest entry of the launch
  // tables is DistAny at 8 rows: 38 slots x 512 B x 8 waves = 152 KiB, so three more slots per thread would not fit there
  static_assert(dist_fast_lds_bytes<RPL, PARK, 64, CFG, RES>() * 4 * MINB <= 160 * 1024, "parked slots exceed the CU's LDS at this occupancy");
  // slots: [0, RPL) S_i ; [RPL, 2 RPL) 1 + D_i ; then m1 (PK_DM_SUM), or previous site outputs, prevR, prevP, m1, m2, mdyn, shift (PK_DM_FULL);
  // PARK only: [K_Y, K_Y + RPL) the site rows of the last accepted state.  Resident: no prevR / prevP; the rows are the lane's slots
  constexpr int MCS = CFG::SLOT_MC;
  constexpr int NSL = dist_fast_slots<RPL, MCS, RES>(), FB = 3 * RPL + (RES ? 0 : 2);     // FB: first slot after the previous outputs
  constexpr int K_SR = 0, K_DG = RPL, K_PS = 2 * RPL, K_PR = 3 * RPL, K_PP = 3 * RPL + 1, K_M1 = (MCS == PK_DM_FULL ? FB : 2 * RPL),
                K_M2 = FB + 1, K_MD = FB + 2, K_SH = FB + 3, K_Y = NSL;
  constexpr int RPB = NT / G;
  const int lane = lane_id();
  const int l = threadIdx.x & (G - 1);
  const long long rep = (long long)blockIdx.x * RPB + (threadIdx.x / G);
  if (rep >= A.B) return;
  const int n = A.n_sites, S = A.S, T = A.T;
  const int mclass = CFG::mclass(A);
  const double* __restrict__ th = A.theta + rep * A.P;

  // ---- coefficients: uniform (A, B, C, D + sum S) and per site (S_i, 1 + D_i); padding sites are inert (S = 0, d = 1)
  // Resident: the R and P slots have rate 0 (they add nothing to Dsum and Scw); their diagonal slots carry B (pivot 1 + q B) and -C
  // (the P slot has no pivot of this form: factor() puts q in its place), and the three per-lane values of row 0 are kept beside them:
  // w0 (weight of row 0 in the group sum of a solve), k3 (the constant of row 0's right-hand side), both 1 / 0 in a site lane
  const double cA = th[0], cB = th[1], cC = th[2];
  const bool isR = RES && l == 0, isP = RES && l == 1;
  const double w0 = isR ? cC : 1.0, k3 = isR ? cA : 0.0;
  double lsum = 0.0;
  static_for<RPL>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const int i = l + G * j - (RES ? 2 : 0);
    const bool ok = i >= 0 && i < n;
    const double sr = ok ? th[4 + i] : 0.0;
    double dg = ok ? 1.0 + th[4 + n + i] : 1.0;
    if constexpr (RES && j == 0) dg = isR ? cB : isP ? -cC : dg;
    pk.template set<K_SR + j>(sr);
    pk.template set<K_DG + j>(dg);
    lsum += sr;
  });
  const double Dsum = th[3] + gsum<G>(lsum, lane);
  // the sum over the site slots of a resident lane: row 0 of lanes 0 and 1 (R and P) stays out
  auto sites_only = [&](const auto& s) {
    double v[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) v[j] = s[j];
    v[0] = (isR || isP) ? 0.0 : v[0];
    return gsum<G>(tree_sum(v), lane);
  };

  // ---- state
  const double* y0p = A.y0 + (A.y0_batched ? rep * S : 0);
  Vec y;
  if constexpr (!RES) { y.R() = y0p[0]; y.P() = y0p[1]; }
#pragma unroll
  for (int j = 0; j < RPL; ++j) {
    const int i = l + G * j;
    if constexpr (RES) y.s[j] = (i < S) ? y0p[i] : 0.0;
    else y.s[j] = (i < n) ? y0p[2 + i] : 0.0;
  }
  if constexpr (PARK) static_for<RPL>([&](auto jc) { constexpr int j = decltype(jc)::value; pk.template set<K_Y + j>(y.s[j]); });

  // ---- output / fused Morris metric (same semantics as Emitter in pk_solve_kernel.hpp)
  static_for<NSL - 2 * RPL>([&](auto kc) { pk.template set<K_PS + decltype(kc)::value>(0.0); });
  const int T5 = T > 5 ? T - 5 : 0;
  // this lane's first site (resident: first slot) in the trajectory row of the next output time; advanced by one row per landing
  double* srow = CFG::sol(A) ? A.sol + rep * T * S + (RES ? 0 : 2) + l : nullptr;
  // one output row: nf = std::true_type writes the NaN rows of a failed replica (cold), std::false_type the values of v
  auto emit = [&](const int k, const Vec& v, auto nf) {
    constexpr bool nan_fill = decltype(nf)::value;
    double* fl = CFG::flat(A) ? A.flat + rep * A.F : nullptr;
    // The clip `x < 0 ? 0 : x` (a compare and two selects per double) changes a value only where its sign bit is set: x < 0 is false for
    // every x with a clear sign bit, +0 and a positive NaN included.  The specialised kernels therefore OR the high dwords of the row's
    // values (two idle-row zeros of either sign included: a -0 only sends the wave down the literal path) and run the literal clip only
    // when some lane of the wave has a sign bit set -- a branch on the scalar unit, uniform over the wave.  Same bits on both paths.
    bool clip_now = CFG::clip(A);
    if constexpr (!CFG::LITERAL && !nan_fill) if (clip_now) clip_now = __builtin_amdgcn_ballot_w64(sign_or(v) < 0) != 0;
    auto val = [&](double x, int state) {
      if (nan_fill) return __builtin_nan("");
      double r = (CFG::LITERAL && CFG::clip(A)) ? ((x < 0.0) ? 0.0 : x) : x;          // the run-time kernel clips value by value
      if (CFG::normalize(A)) r *= 1.0 / y0p[state];
      return r;
    };
    Vec c = v;                                          // the clipped state
    if constexpr (!CFG::LITERAL && !nan_fill) if (clip_now) {
      asm volatile("" : "+v"(c.s[Vec::tree_row(0)]));   // keeps this a branch: without it the compiler folds the test into each select
      clip_rows(c);
    }
    double vR = 0.0, vP = 0.0;
    if constexpr (!RES) {
      vR = val(c.R(), 0); vP = val(c.P(), 1);
      if (l == 0) {
        if (CFG::sol(A)) { srow[-2] = vR; srow[-1] = vP; }
        if (CFG::flat(A)) { if (k >= 5) fl[k - 5] = vR; fl[T5 + k] = vP; }
      }
    }
    // An idle row (i >= n: rate 0, initial value 0) holds +0 or -0 in every accepted state -- each of its stage values is
    // fma(0, x_P, +-0) with x_P finite; a scaled row has scale 0 there and is fma(0, A_j, +0) -- so its clipped value is a zero already.
    // Adding a zero of either sign instead of +0.0 can change the row sum only from one zero to the other, and the running sum it is added to started from +0.0 and takes either zero
    // to the same bits.  Only normalize (which would read y0 past its end) still needs the mask; the run-time kernel keeps it.
    const bool masked = CFG::LITERAL || CFG::normalize(A);
    double vs[RPL];
    // Resident: every lane stores its slots, no lane-0 branch.  Slot s of the flat vector is at T5 + (s - 1) T + k for every s: the
    // sites from T5 + T on, P (s = 1) at T5 + k, and R (s = 0) at k - 5 when T > 5 (T5 = T - 5) -- stored from k = 5 on, and never
    // when T <= 5 (k < T).  The running sum is the plain sum of the lane's emitted values.
    double loc = (!RES && l == 0) ? vR + vP : 0.0;
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
      const int i = l + G * j;
      if constexpr (RES) {
        vs[j] = (i < S || !masked) ? val(c.s[j], i) : 0.0;
        if (i < S) {
          if (CFG::sol(A)) srow[G * j] = vs[j];
          if (CFG::flat(A)) if (j > 0 || i > 0 || k >= 5) fl[T5 + (i - 1) * T + k] = vs[j];
        }
      } else {
        vs[j] = (i < n || !masked) ? val(c.s[j], 2 + i) : 0.0;
        if (i < n) {
          if (CFG::sol(A)) srow[G * j] = vs[j];
          if (CFG::flat(A)) fl[T5 + T + i * T + k] = vs[j];
        }
      }
      loc += vs[j];
    }
    if (CFG::sol(A)) srow += S;
    if (mclass != PK_DM_NONE) {
      // total_signal / mean_activity need the running sum only; the second-moment and first-difference bookkeeping (and its LDS
      // traffic in the parked layouts) exists only for the metrics that use it
      pk.template set<K_M1>(pk.template get<K_M1>() + loc);
      if constexpr (MCS == PK_DM_FULL) if (mclass == PK_DM_FULL) {
        double m2 = pk.template get<K_M2>(), mdyn = pk.template get<K_MD>(), shift = pk.template get<K_SH>();
        double prevR = 0.0, prevP = 0.0;
        if constexpr (!RES) { prevR = pk.template get<K_PR>(); prevP = pk.template get<K_PP>(); }
        if (k == 0) {
          shift = gsum<G>(loc, lane) / (2 + n);
          pk.template set<K_SH>(shift);
          prevR = vR; prevP = vP;
          static_for<RPL>([&](auto jc) { constexpr int j = decltype(jc)::value; pk.template set<K_PS + j>(vs[j]); });
        }
        static_for<RPL>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          const int i = l + G * j;
          const double xs = (i < (RES ? S : n)) ? vs[j] - shift : 0.0;
          m2 = __builtin_fma(xs, xs, m2);
          const double d = vs[j] - pk.template get<K_PS + j>();
          mdyn = __builtin_fma(d, d, mdyn);
          pk.template set<K_PS + j>(vs[j]);
        });
        if constexpr (!RES) {
          if (l == 0) {
            const double a = vR - shift, b = vP - shift;
            m2 = __builtin_fma(a, a, m2); m2 = __builtin_fma(b, b, m2);
            const double dR = vR - prevR, dP = vP - prevP;
            mdyn = __builtin_fma(dR, dR, mdyn); mdyn = __builtin_fma(dP, dP, mdyn);
          }
          pk.template set<K_PR>(vR); pk.template set<K_PP>(vP);
        }
        pk.template set<K_M2>(m2); pk.template set<K_MD>(mdyn);
      }
    }
  };
  auto finish = [&](const int status, const int acc, const int rej) {
    if (mclass != PK_DM_NONE) {
      const double L = 2.0 * T + (double)T * n;
      const double tot = gsum<G>(pk.template get<K_M1>(), lane);
      double m = tot;
      if (A.metric_id == PK_METRIC_MEAN_ACTIVITY) m = tot / L;
      if constexpr (MCS == PK_DM_FULL) if (mclass == PK_DM_FULL) {
        const double m2 = pk.template get<K_M2>(), mdyn = pk.template get<K_MD>(), shift = pk.template get<K_SH>();
        switch (A.metric_id) {
          case PK_METRIC_VARIANCE: { const double q = gsum<G>(m2, lane); const double ms = tot / L - shift; m = q / L - ms * ms; } break;
          case PK_METRIC_DYNAMICS: m = gsum<G>(mdyn, lane); break;
          default: { const double q = gsum<G>(m2, lane); m = sqrt(fmax(q + 2.0 * shift * tot - L * shift * shift, 0.0)); } break;
        }
      }
      if (l == 0) A.metric[rep] = m;
    }
    if (l == 0) {
      if (A.status) A.status[rep] = status;
      if (A.n_steps) { A.n_steps[2 * rep] = acc; A.n_steps[2 * rep + 1] = rej; }
    }
  };

  emit(0, y, std::false_type{});
  int status = PK_ST_OK, nacc = 0;
  if (T < 2) { trace.exit(); finish(status, 0, 0); return; }

  const double rtol = A.rtol, atol = A.atol;
  const DistNorm<G, RPL, RES> norm{rtol, atol, lane};
  auto rhs_of = [&](const Vec& Y, const double sg) {       // f(Y) with sg the site sum of Y: the prologue's initial step estimate only
    Vec f;
    if constexpr (RES) {
      // R and P leave their lanes here.  Row 0: A - B R in lane 0, C R - Dsum P + sg in lane 1, a site row elsewhere
      const double Rb = bcast<G, 0>(Y.s[0]), Pb = bcast<G, 1>(Y.s[0]);
      static_for<RPL>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const double sr = pk.template get<K_SR + j>(), dg = pk.template get<K_DG + j>();
        if constexpr (j == 0) f.s[0] = __builtin_fma(isP ? -Dsum : sr, Pb, __builtin_fma(-dg, isP ? Rb : Y.s[0], isP ? sg : k3));
        else f.s[j] = __builtin_fma(sr, Pb, -dg * Y.s[j]);
      });
    } else {
      f.R() = __builtin_fma(-cB, Y.R(), cA);
      f.P() = __builtin_fma(cC, Y.R(), __builtin_fma(-Dsum, Y.P(), sg));
      static_for<RPL>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        f.s[j] = __builtin_fma(pk.template get<K_SR + j>(), Y.P(), -pk.template get<K_DG + j>() * Y.s[j]);
      });
    }
    return f;
  };

  double tc = A.t[0];
  int k = 1;
  double te = A.t[1];
  double h;
  {
    double sg0;
    if constexpr (RES) sg0 = sites_only(y.s);
    else {
      double v[RPL];                                      // the site rows alone: y.s ends with the shadow rows
#pragma unroll
      for (int j = 0; j < RPL; ++j) v[j] = y.s[j];
      sg0 = site_sum<G>(v, lane);
    }
    const Vec f0 = rhs_of(y, sg0);
    const double d0 = norm.group_max(y, y, y), d1 = norm.group_max(f0, y, y);      // |y| / sc and |f0| / sc with sc = atol + rtol |y|
    h = step_h0(d0, d1, A.h0);
  }
  // ---- scaled rows: the scale s_j of a row, decided here once per replica and never again (a replica's bits do not depend on its wave
  // mates).  It is the rate S_j itself wherever |S_j| >= 2^-600 (a NaN or inf rate included: it reaches Scw and ends as PK_ST_NONFINITE).
  // An idle row, and a real site with rate 0 that starts at 0, has s_j = 0: rho_j = 0, c_j = 0 and every value of the row is 0 w_j, exactly
  // zero.  Any other rate below the floor is replaced by the floor: the row keeps its decay exactly and receives an inflow 2^-600 P, of
  // order 1e-181, which no output can show.  The scale replaces the rate in the row's K_SR slot -- from here on only factor() reads it;
  // Dsum, the right-hand side above and the emitted values have used S_j itself -- and 1 / s_j (0 where s_j is 0) stays in registers, as
  // kappa_j = d_j / s_j where the first stage is formed from the state rows (S1: dist_stage1_state()).
  double is[RPL];
  if constexpr (SCL) static_for<RPL>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    if constexpr (j >= J0) {
      const double sr = pk.template get<K_SR + j>();
      const double s = !(fabs(sr) < PK_DIST_SCALE_MIN) ? sr : (sr == 0.0 && y.s[j] == 0.0) ? 0.0 : PK_DIST_SCALE_MIN;
      pk.template set<K_SR + j>(s);
      is[j] = s != 0.0 ? 1.0 / s : 0.0;
      if constexpr (S1) is[j] *= pk.template get<K_DG + j>();
    }
  });
  // ---- the P slot's two constants (PAR: dist_pslot_arith()): selP is 1 in lane 1 and 0 elsewhere, notP = 1 - selP.  The P lane's diagonal
  // slot, -C until here for the right-hand side above, becomes 1: fma(q, 1, notP) is then q itself, the slot's "pivot" (factor())
  double selP = isP ? 1.0 : 0.0, notP = isP ? 0.0 : 1.0;
  if constexpr (PAR) {
    if (isP) pk.template set<K_DG + 0>(1.0);
    asm volatile("" : "+v"(selP), "+v"(notP));            // two register pairs, not two selects rebuilt from the lane number in every step
  }

  // Arrow factors of M = I - q J (q = gamma h) for the current step size.
  //   rows: (1 + q B) x_R = r_R ; (1 + q d_i) x_i - q S_i x_P = r_i ; (1 + q Dsum) x_P - q C x_R - q sum x_i = r_P
  // The RPL + 1 pivots 1 + q B and 1 + q d_j of a lane do not depend on each other and are inverted through shared reciprocals
  // (chain_rcp, pk_linsolve.hpp): one chain while there are at most five of them, two chains split as evenly as possible above that
  // ({B, rows 0-3} and {rows 4-7} at 8 rows), which halves the dependent latency and keeps every product at five pivots or fewer.
  // A replica is solved while the product of the pivots of each chain is finite (pivots up to about 1e61 each; the parent asked only
  // that each pivot be finite), and a zero or non-finite pivot spoils its chain at once where it reached the group sum one solve later.
  // sinv depends on all of them and keeps its own reciprocal.
  // Resident: a lane has RPL pivots, its slots' (same split rule: one chain up to five, two even ones above -- 4 + 4 at 8 rows).  The R
  // slot's is 1 + q B; the P slot takes q itself as its factor, so the chain of lane 1 hands back 1 / q (what solve() needs to put r_P
  // into the group sum) and nothing is inverted on its own.  Row 0 enters that sum as r_0 ws0 with ws0 = winv_0 w0 (C / (1 + q B) | 1 / q |
  // winv_0), and qs = q sinv is the sum's one multiplier.  So that a solve needs no select for the P slot, whose result is x_P itself,
  // lane 1 ends factor() with winv_0 = 0 and cw_0 = 1: fma(cw_0, x_P, r_P winv_0) is x_P (after Scw, to which the slot adds nothing).
  // Those fix-ups are selects on isP, or, where the registers allow (PAR: dist_pslot_arith()), arithmetic on selP and notP with the same bits:
  // piv_0 = fma(q, dg_0, notP) with the P lane's dg_0 = 1, cw_0 = fma(winv_0, selP, cw_0), winv_0 = winv_0 notP, omw_0 = fma(omw_0, notP, selP).
  // For the difference stages of LRP8 / LRP12 (below) a row also keeps omw_j = 1 - winv_j, and the lane Cl, the sum of cw over the rows its
  // tracked sum runs over (every site row; resident: rows 1 .. RPL - 1, before the P slot's fixup -- row 0 never enters).  omw is formed as
  // (q winv_j) d_j with d_j the diagonal entry (pivot 1 + q d_j), NOT as 1 - winv_j: on the first steps of a run q d_j is 1e-7 .. 1e-13 and the
  // subtraction would keep nine to three digits of it, where the product is good to two ulps.  It costs the same: q winv_j is shared with
  // cw_j = (q winv_j) S_j, one multiply more per row than cw alone instead of one add.  The R slot's d is B; the P slot takes omw = 1
  // (v' = v - x_P) with its other fixups; shadowed, omwR = (q winvR) B and row P subtracts x_P itself.
  //
  // SCALED rows (SCL: dist_scaled(), the parked LRP12 layouts).  A site row is carried through the stages in units of its own coupling
  // weight: with c_j = winv_j s_j (= cw_j / q, s_j the row's scale: its rate, see the prologue), a stage value is v_j = c_j w_j, and with
  // xq = q x_P every row of a solve and of a difference stage is ONE FMA on w with no coefficient on xq:
  //   solve       u_j = cw_j x_P + winv_j r_j   ->  upsilon_j = winv_j rho_j + xq           (r_j = c_j rho_j; written with omw_j: solve())
  //   difference  v'_j = omw_j v_j - cw_j x_P   ->  w'_j = fma(omw_j, w_j, -xq)
  // and the group sum's input sum winv_j v_j is the FMA dot product sum g_j w_j with g_j = winv_j c_j: no product p_j, no add tree, no
  // tracked sum (lam, Cl and the lam - psum cancellation are gone).  The state enters the first solve as rho_j = y_j ic_j with
  // ic_j = piv_j / s_j (c_j ic_j = 1 to a few ulps; or as itself, without ic_j: S1, at solve()), and leaves the step once:
  // y_new_j = fma(c_j, A_j, y_j) with A_j the weighted sum of the row's w, e_j = c_j w_last,j.  factor() keeps c_j in cw[j]; Scw is q sum c_j, the same number up to rounding, and still what the
  // cold non-finite test reads.  Resident: rows 1 .. RPL - 1 are scaled; row 0 (R slot, P slot, two sites) keeps plain units and its explicit
  // term r_0 ws0 in the group sum, but takes xq like the others: cw[0] is cw_0 / q = winv_0 S_0, and in the P slot lane 1's own 1 / q
  // (its chain's result for the "pivot" q), so that fma(cw_0, xq, 0) is x_P; qs = q^2 sinv is then the sum's one multiplier.  Shadowed:
  // every site row is scaled; the shadow rows keep x_R and x_P = (q (C x_R + St) + r_P) sinv as they are, and xq = q x_P is one multiply.
  double winv[RPL], cw[RPL], omw[RPL], g[RPL], ic[RPL], winvR, omwR, Cl, sinv, Scw, qq, qs, ws0;
  auto factor = [&](const double q) {
    qq = q;
    constexpr int X = RES ? 0 : 1;
    constexpr int NP = RPL + X, M0 = NP <= 5 ? NP : (NP + 1) / 2, M1 = NP - M0;
    double piv[NP];
    if constexpr (!RES) piv[0] = __builtin_fma(q, cB, 1.0);
    static_for<RPL>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if constexpr (PAR && j == 0) piv[0] = __builtin_fma(q, pk.template get<K_DG + 0>(), notP);
      else piv[X + j] = __builtin_fma(q, pk.template get<K_DG + j>(), 1.0);
    });
    if constexpr (RES && !PAR) piv[0] = isP ? q : piv[0];
    {
      double a[M0], inv[M0];
#pragma unroll
      for (int i = 0; i < M0; ++i) a[i] = piv[i];
      chain_rcp<M0>(a, inv);
      if constexpr (!RES) winvR = inv[0];
#pragma unroll
      for (int i = X; i < M0; ++i) winv[i - X] = inv[i];
    }
    if constexpr (M1 > 0) {
      double a[M1], inv[M1];
#pragma unroll
      for (int i = 0; i < M1; ++i) a[i] = piv[M0 + i];
      chain_rcp<M1>(a, inv);
#pragma unroll
      for (int i = 0; i < M1; ++i) winv[M0 - X + i] = inv[i];
    }
    static_for<RPL>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if constexpr (SCL) {
        // cw[j] is c_j = cw_j / q in every row (the K_SR slot of a scaled row holds its scale s_j)
        // a scaled row's winv_j ends here (S1: at the first dot product, which follows directly): its solves are written with
        // omw_j = 1 - winv_j (solve(), below)
        cw[j] = winv[j] * pk.template get<K_SR + j>();
        omw[j] = (q * winv[j]) * pk.template get<K_DG + j>();
        if constexpr (j >= J0) {
          g[j] = winv[j] * cw[j];
          if constexpr (!S1) ic[j] = piv[X + j] * is[j];
        }
      } else if constexpr (Tab::DIFFERENCE) {
        const double qw = q * winv[j];
        cw[j] = qw * pk.template get<K_SR + j>();
        omw[j] = qw * pk.template get<K_DG + j>();
      } else cw[j] = q * pk.template get<K_SR + j>() * winv[j];
    });
    if constexpr (!Tab::DIFFERENCE) Scw = gsum<G>(tree_sum(cw), lane);
    else if constexpr (SCL) {
      // the P slot's cw[0] is (1 / q) 0 here, before its fixup below
      if constexpr (!RES) omwR = q * winvR * cB;
      Scw = q * gsum<G>(tree_sum(cw), lane);
    } else if constexpr (!RES) {
      omwR = q * winvR * cB;
      Cl = tree_sum(cw);
      Scw = gsum<G>(Cl, lane);
    } else if constexpr (RPL > 1) {
      double rest[RPL - 1];
#pragma unroll
      for (int j = 1; j < RPL; ++j) rest[j - 1] = cw[j];
      Cl = tree_sum(rest);
      Scw = gsum<G>(Cl + cw[0], lane);
    } else {
      Cl = 0.0;
      Scw = gsum<G>(cw[0], lane);
    }
    sinv = fast_rcp(__builtin_fma(q, Dsum - Scw, 1.0));
    if constexpr (RES) {
      qs = q * sinv;
      if constexpr (SCL) qs *= q;
      ws0 = winv[0] * w0;
      if constexpr (PAR) {
        // the same 64 bits as the selects below for finite values: the P lane's cw[0] is 0 here (its rate slot is 0) and its winv[0] is
        // the chain's 1 / q > 0, products with 0 and 1 are exact; a non-finite winv[0] or omw[0] turns NaN here instead of one
        // operation later, in a step that is rejected either way
        if constexpr (SCL) cw[0] = __builtin_fma(winv[0], selP, cw[0]); else cw[0] += selP;
        winv[0] *= notP;
        if constexpr (Tab::DIFFERENCE) omw[0] = __builtin_fma(omw[0], notP, selP);
      } else {
        if constexpr (SCL) cw[0] = isP ? winv[0] : cw[0]; else cw[0] = isP ? 1.0 : cw[0];
        winv[0] = isP ? 0.0 : winv[0];
        if constexpr (Tab::DIFFERENCE) omw[0] = isP ? 1.0 : omw[0];
      }
    }
  };
  // u = M^{-1} r: ONE group reduction.  lam (difference stages): the sum of u over the lane's tracked rows, from the sum of t the solve
  // forms anyway: sum_j u_j = x_P Cl + sum_j t_j
  double lam = 0.0;
  // Scaled rows: the lane's input to the group sum, sum c_j w_j over its scaled rows as ONE FMA chain (resident: started from row 0's
  // explicit term), and xq = q x_P from it.  c is g, or winv where the first stage takes the state rows themselves (solve(), below).  The
  // seven row FMAs of the stage before and the eight accumulation FMAs fill the gaps of the chain at three waves per SIMD: two chains joined
  // by an add measured 2.3 % slower on the benchmark.  Shadowed, the shadow rows' x_R and x_P come back through the arguments
  auto gdot = [&](const Vec& v, const double (&c)[RPL]) {
    if constexpr (SCL) {
      double a;
      if constexpr (RES) a = v.s[0] * ws0; else a = c[0] * v.s[0];
#pragma unroll
      for (int j = 1; j < RPL; ++j) a = __builtin_fma(c[j], v.s[j], a);
      return a;
    } else return 0.0;
  };
  auto xq_of = [&](const Vec& v, const double (&c)[RPL], double& xR, double& xP) {
    if constexpr (RES) return gsum<G>(gdot(v, c), lane) * qs;
    else {
      xR = v.R() * winvR;
      xP = __builtin_fma(qq, __builtin_fma(cC, xR, gsum<G>(gdot(v, c), lane)), v.P()) * sinv;
      return qq * xP;
    }
  };
  // first (std::true_type: the first stage of a step, scaled rows only): the scaled rows come back as upsilon_j - rho_j, the stage itself.
  // S1 (dist_stage1_state()): r then holds the STATE rows, not rho.  With c_j ic_j = 1 both products the stage needs are known without
  // ic_j: g_j rho_j = winv_j y_j and omw_j rho_j = q (d_j / s_j) y_j, so with kappa_j = d_j / s_j (is[j], fixed per replica in the prologue)
  //   t_j = kappa_j y_j ;  dot term fma(winv_j, y_j, .) ;  zeta_j = fma(-q, t_j, xq)
  // three operations per row where rho takes four (ic_j, rho_j, the dot term, the stage), and the roundings of piv_j / s_j and y_j ic_j are
  // gone.  A row with s_j = 0 has kappa_j = 0 and zeta_j = xq; its c_j is 0, so every value of the row is still 0 w_j
  auto solve = [&](const Vec& r, auto first) {
    Vec u;
    double xR = 0.0;
    if constexpr (SCL) {
      // r and u: scaled rows in units of c_j (rho, upsilon), row 0 of the resident layout and the shadow rows in plain units.  A scaled
      // row is written with omw_j, upsilon_j = rho_j - omw_j rho_j + xq, so that winv_j need not outlive factor() and the first stage
      // upsilon_j - rho_j = fma(-omw_j, rho_j, xq) is formed without its cancellation (one operation where the plain rows take two; the
      // second solve pays it back with its add)
      double xP = 0.0;
      constexpr bool state = S1 && decltype(first)::value;
      const double xq = state ? xq_of(r, winv, xR, xP) : xq_of(r, g, xR, xP);
      if constexpr (RES) u.s[0] = __builtin_fma(cw[0], xq, r.s[0] * winv[0]);
      else { u.R() = xR; u.P() = xP; }
#pragma unroll
      for (int j = J0; j < RPL; ++j) {
        if constexpr (state) u.s[j] = __builtin_fma(-qq, is[j] * r.s[j], xq);
        else if constexpr (decltype(first)::value) u.s[j] = __builtin_fma(-omw[j], r.s[j], xq);
        else u.s[j] = __builtin_fma(-omw[j], r.s[j], r.s[j] + xq);
      }
      return u;
    }
    if constexpr (!RES) xR = r.R() * winvR;
    double t[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) t[j] = r.s[j] * winv[j];
    if constexpr (RES) {
      // row 0 adds C x_R in lane 0 and r_P / q in lane 1: the group sum is C x_R + r_P / q + sum t_i, and x_P = sinv (r_P + q (C x_R + sum t_i))
      double in, tsum = 0.0;
      if constexpr (RPL > 1) {
        double rest[RPL - 1];
#pragma unroll
        for (int j = 1; j < RPL; ++j) rest[j - 1] = t[j];
        tsum = tree_sum(rest);
        in = __builtin_fma(r.s[0], ws0, tsum);
      } else in = r.s[0] * ws0;
      const double xP = gsum<G>(in, lane) * qs;
      if constexpr (Tab::DIFFERENCE && RPL > 1) lam = __builtin_fma(xP, Cl, tsum);
      // uniform over the lanes: cw is 0 in the R slot (x_R = t), and 1 over t = 0 in the P slot (x_P)
#pragma unroll
      for (int j = 0; j < RPL; ++j) u.s[j] = __builtin_fma(cw[j], xP, t[j]);
    } else {
      const double tsum = tree_sum(t);
      const double St = gsum<G>(tsum, lane);
      const double xP = __builtin_fma(qq, __builtin_fma(cC, xR, St), r.P()) * sinv;
      if constexpr (Tab::DIFFERENCE) lam = __builtin_fma(xP, Cl, tsum);
#pragma unroll
      for (int j = 0; j < RPL; ++j) u.s[j] = __builtin_fma(cw[j], xP, t[j]);
      u.R() = xR; u.P() = xP;
    }
    return u;
  };
  // v <- v - M^{-1} v, one difference stage of LRP8 / LRP12, cheaper than a solve and a subtraction.  Every row of a solve obeys
  // u_j = cw_j x_P + winv_j r_j (resident: the R and P slots too, after factor()'s fixups), so v'_j = omw_j v_j - cw_j x_P, uniformly over
  // the lanes; and the group sum that feeds x_P needs sum winv_j v_j = lam - sum omw_j v_j with lam = sum v_j carried from stage to stage
  // by one FMA, lam' = sum p_j - x_P Cl (p_j = omw_j v_j), instead of a second tree.  Resident: row 0 keeps its explicit term v_0 ws0 as
  // in solve(), and lam, the tree and Cl run over rows 1 .. RPL - 1 (none of them at one row per lane).
  // Scaled rows: w'_j = fma(omw_j, w_j, -xq), one FMA per row after the dot product; row 0 of the resident layout and the shadow rows as above.
  auto diff = [&](Vec& v) {
    if constexpr (SCL) {
      double xR = 0.0, xP = 0.0;
      const double xq = xq_of(v, g, xR, xP);
      if constexpr (RES) v.s[0] = __builtin_fma(-cw[0], xq, omw[0] * v.s[0]);
      else { v.R() *= omwR; v.P() -= xP; }
#pragma unroll
      for (int j = J0; j < RPL; ++j) v.s[j] = __builtin_fma(omw[j], v.s[j], -xq);
      return;
    }
    double p[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) p[j] = omw[j] * v.s[j];
    if constexpr (RES) {
      double in, psum = 0.0;
      if constexpr (RPL > 1) {
        double rest[RPL - 1];
#pragma unroll
        for (int j = 1; j < RPL; ++j) rest[j - 1] = p[j];
        psum = tree_sum(rest);
        in = __builtin_fma(v.s[0], ws0, lam - psum);
      } else in = v.s[0] * ws0;
      const double xP = gsum<G>(in, lane) * qs;
#pragma unroll
      for (int j = 0; j < RPL; ++j) v.s[j] = __builtin_fma(-cw[j], xP, p[j]);
      if constexpr (RPL > 1) lam = __builtin_fma(-xP, Cl, psum);
    } else {
      const double psum = tree_sum(p);
      const double xR = v.R() * winvR;
      const double St = gsum<G>(lam - psum, lane);
      const double xP = __builtin_fma(qq, __builtin_fma(cC, xR, St), v.P()) * sinv;
#pragma unroll
      for (int j = 0; j < RPL; ++j) v.s[j] = __builtin_fma(-cw[j], xP, p[j]);
      lam = __builtin_fma(-xP, Cl, psum);
      v.R() *= omwR; v.P() -= xP;
    }
  };

  // resolvent-form step (the right-hand side is affine, f(y) = J y + b with b = A in row R): z_1 = M^{-1} h f(y), z_{k+1} = M^{-1} z_k,
  //   y_new = y + sum_k B_k z_k ,  err = sum_k E_k z_k     (ResolventTab: RODAS4, LRP8 or LRP12)
  // With J = (I - M) / q the first stage needs no right-hand side: gamma z_1 = M^{-1} (y + q b) - y.  The loop carries w_k = gamma z_k
  // (w_{k+1} = M^{-1} w_k) and the weights B_k / gamma, E_k / gamma, divided at compile time.
  // LRP8 and LRP12 (Tab::DIFFERENCE, pk_solve_kernel.hpp) take the two solves w_1, w_2 and then NS - 2 difference stages v_0 = w_2,
  // v_{m+1} = v_m - M^{-1} v_m (diff(), above): y_new = y + (B_1 w_1 + sum_m BN_m v_m) / gamma, and the error estimate is the last v times
  // E_2 / gamma -- no second accumulation; the factor multiplies the reduced norm once.  RODAS4 keeps both weighted sums.
  bool after_reject = false;
  // the non-finite test's view of the ACCEPTED state: R, P and the site sum, reduced over the group.  The step loop carries no site
  // sum, so this cold path forms it from the accepted rows -- in the parked layouts read back from their slots, since y.s holds the
  // candidate from the accept block on.  Resident: R and P are row 0 of lanes 0 and 1
  auto state_bad = [&]() {
    double rows[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) rows[j] = y.s[j];
    if constexpr (PARK) {
      pk.fence();
      static_for<RPL>([&](auto jc) { constexpr int j = decltype(jc)::value; rows[j] = pk.template get<K_Y + j>(); });
    }
    bool b;
    if constexpr (RES) b = ((isR || isP) && nonfinite(rows[0])) || nonfinite(sites_only(rows));
    else b = (nonfinite(y.R())) || (nonfinite(y.P())) || (nonfinite(site_sum<G>(rows, lane)));
    return gmax<G>(b ? 1.0 : 0.0, lane);
  };
  // A, B, C of the same test.  Resident: they are not kept in registers through the loop (B and C live in the diagonal slots of lanes 0
  // and 1, A in lane 0's k3), so this cold path reads them again
  auto coef_bad = [&]() {
    if constexpr (RES) {
      long long r2 = rep;
      asm volatile("" : "+v"(r2));                        // a fresh address: the prologue's pointer is not kept alive for this
      const double* t2 = A.theta + r2 * A.P;
      return (nonfinite(t2[0])) || (nonfinite(t2[1])) || (nonfinite(t2[2]));
    } else return (nonfinite(cA)) || (nonfinite(cB)) || (nonfinite(cC));
  };
  // nacc counts the accepted steps.  nsec counts the rejected ones in the run-time kernel and ALL steps in the specialised kernels (one
  // increment per step whatever its fate, and the budget test reads it without an add; finish() gets the difference -- integer, exact)
  int nsec = 0;
  // vmcnt(0) alone: every load of the prologue has landed before the loop, so the loop's own wait is the one for tnx at a landing and
  // no step waits for the stores of the landing before it
  __builtin_amdgcn_s_waitcnt(0x0F70);
  // The outer loop runs once on a healthy replica.  In the specialised kernels a step whose error is NaN or inf leaves the step loop on a
  // flag; what the run-time kernel decides inside its loop (PK_ST_NONFINITE, or carry on with a tenth of the step) is decided below the
  // step loop, on values that rejected step did not change, and a replica that carries on re-enters the step loop.  A replica's lanes
  // move together, and no other replica's values are read, so every replica takes the steps it took.
  while (true) {
    bool nonfin = false;
    while (true) {
      trace.step();
      pace.step(k);
      const double tnx = A.t[k + 1 < T ? k + 1 : T - 1];   // the output time after te, fetched a whole step before a landing can need it
      // failure exits (step budget, vanishing step): status is set here and the NaN rows are written after the loop
      const bool over = (CFG::LITERAL ? nacc + nsec : nsec) >= A.max_steps;
      const bool last = (tc + 1.0001 * h >= te);
      const double hs = last ? te - tc : ((tc + 2.0 * h > te) ? 0.5 * (te - tc) : h);
      // max_abs_k, and max_raw / min_raw in the controller below: one v_max_f64 / v_min_f64 each (pk_wave.hpp), same bits as fmax / fmin
      if (over || !(hs > 1e-14 * max_abs_k(tc, 1e-3))) { status |= over ? PK_ST_MAXSTEPS : PK_ST_HMIN; break; }
      if constexpr (PARK) {
        // the site rows of the state live in their slots between steps: read here (next to the rate slots, whose wait they share),
        // written by the lanes that accept -- a rejecting lane has nothing to undo and an accepting one nothing to copy
        pk.fence();
        static_for<RPL>([&](auto jc) { constexpr int j = decltype(jc)::value; y.s[j] = pk.template get<K_Y + j>(); });
      }
      factor(Tab::GAM * hs);

      Vec z;
      {
        // y + q b: q A joins row R (resident: k3 is A in lane 0 and 0 elsewhere, so the FMA is uniform over the lanes)
        Vec r = y;
        if constexpr (RES) r.s[0] = __builtin_fma(qq, k3, y.s[0]); else r.R() = __builtin_fma(qq, cA, y.R());
        if constexpr (SCL) {
          // the scaled rows enter as rho_j = y_j / c_j, and solve() hands back the first stage upsilon_j - rho_j in the same units
          if constexpr (!S1) {
#pragma unroll
            for (int j = J0; j < RPL; ++j) r.s[j] = y.s[j] * ic[j];
          }
          z = solve(r, std::true_type{});
#pragma unroll
          for (int j = 0; j < Vec::NR; ++j) if (j < J0 || j >= RPL) z.s[j] -= y.s[j];
        } else {
          z = solve(r, std::false_type{});
          trk_axpy(z, -1.0, y);
        }
      }
      // scaled rows: yn_j holds A_j, the weighted sum of the row's stage values in units of c_j, until the end of the step
      Vec yn = y;
      if constexpr (SCL) {
#pragma unroll
        for (int j = J0; j < RPL; ++j) yn.s[j] = 0.0;
      }
      trk_axpy(yn, Tab::B[0] / Tab::GAM, z);
      double err;
      if constexpr (Tab::DIFFERENCE) {
        z = solve(z, std::false_type{});
        trk_axpy(yn, Tab::BN[0] / Tab::GAM, z);
        static_for<Tab::NS - 2>([&](auto mc) {
          constexpr int m = 1 + decltype(mc)::value;
          diff(z);
          trk_axpy(yn, Tab::BN[m] / Tab::GAM, z);
        });
        if constexpr (SCL) {
          // back to plain units, once per step: the candidate and the error row.  The scaled rows of the state were last read when rho was
          // formed; the final FMA and the norm take them from their slots again (as state_bad() does) rather than keep them in registers
          // through every stage
          pk.fence();
          static_for<RPL - J0>([&](auto jc) { constexpr int j = J0 + decltype(jc)::value; y.s[j] = pk.template get<K_Y + j>(); });
#pragma unroll
          for (int j = J0; j < RPL; ++j) {
            yn.s[j] = __builtin_fma(cw[j], yn.s[j], y.s[j]);
            z.s[j] *= cw[j];
          }
        }
        constexpr double e1 = (Tab::E[1] < 0.0 ? -Tab::E[1] : Tab::E[1]) / Tab::GAM;
        if constexpr (CFG::LITERAL) err = e1 * norm.group_max(z, y, yn); else err = e1 * norm.err_norm(z, y, yn);
      } else {
        Vec u6;
        static_for<Tab::NS - 1>([&](auto kc) {
          constexpr int kk = 1 + decltype(kc)::value;
          constexpr double bk = Tab::B[kk] / Tab::GAM, ek = Tab::E[kk] / Tab::GAM;
          z = solve(z, std::false_type{});
          trk_axpy(yn, bk, z);
          if constexpr (kk == 1) u6 = trk_scale(ek, z); else trk_axpy(u6, ek, z);
        });
        if constexpr (CFG::LITERAL) err = norm.group_max(u6, y, yn); else err = norm.err_norm(u6, y, yn);
      }
      // accept / reject / landing bookkeeping on per-lane predicates (selects, and LDS writes under the lane mask); a NaN or inf error is
      // a rejection too (acc = false), so the state is settled before the non-finite exit below looks at it
      const bool acc = (err <= 1.0);
      if constexpr (PARK) {
        // accepting lanes record the candidate's site rows in their slots (LDS writes under the lane mask instead of a select per dword
        // of the state); y.s is the candidate from here to the end of the iteration -- only a landing, which is an accept, reads it
        if (acc) {
          static_for<RPL>([&](auto jc) { constexpr int j = decltype(jc)::value; pk.template set<K_Y + j>(yn.s[j]); });
          // the time moves under the same mask: one add where tc = acc ? tc + hs : tc was an add and two selects
          if constexpr (!CFG::LITERAL) tc += hs;
        }
#pragma unroll
        for (int j = 0; j < RPL; ++j) y.s[j] = yn.s[j];
        #pragma unroll
        for (int x = 0; x < Vec::X; ++x) y.s[RPL + x] = acc ? yn.s[RPL + x] : y.s[RPL + x];
      } else {
        if (acc) {
          y = yn;
          if constexpr (!CFG::LITERAL) tc += hs;
        }
      }
      if constexpr (CFG::LITERAL) {
        if (err != err || err > 1e300) {
          ++nsec; after_reject = true; h = 0.1 * hs;
          if (state_bad() != 0.0 || coef_bad() || (nonfinite(Dsum)) || (nonfinite(Scw))) {
            status |= PK_ST_NONFINITE; break;
          }
          continue;
        }
      } else {
        ++nsec;
        if (__builtin_expect(err != err || err > 1e300, 0)) { after_reject = true; h = 0.1 * hs; nonfin = true; break; }
      }
      // The controller as a multiplier: err^(-1/Q) by negating the exponent of root_q (pk_solve_kernel.hpp; its two clamps inlined as
      // single instructions), then step_growth's clamps [1/5, 6] -- hs / step_fac(err^(1/Q)) without the reciprocal of a factor that
      // v_log_f32 / v_exp_f32 leave good to 1e-7 anyway.  h moves by an ulp or two of single precision against the quotient
      const float e32 = (float)min_raw_k(max_raw_k(err, 1e-30), 1e30);
      const double finv = step_growth((double)__builtin_amdgcn_exp2f(__builtin_amdgcn_logf(e32) * (float)(-1.0 / Tab::Q)));
      double hnew = hs * finv;
      const bool land = acc && last;
      if constexpr (CFG::LITERAL) { nacc += acc ? 1 : 0; nsec += acc ? 0 : 1; }
      else nacc += (int)acc;                            // the predicate itself: 0 or 1
      if (acc && after_reject) hnew = min_raw(hnew, hs);
      after_reject = !acc;
      if constexpr (CFG::LITERAL) tc = land ? te : (acc ? tc + hs : tc);
      h = (land && hs < h) ? max_raw(hnew, h) : hnew;
      if (land) {
        // a landing sets the time to the output time itself (tc + hs is te only up to rounding); the accept above has already moved
        // tc, which nothing reads in between
        if constexpr (!CFG::LITERAL) tc = te;
        te = tnx;
        asm volatile("" : "+v"(te));                      // pins this copy ahead of the row's stores: its wait then covers the load of tnx alone
        emit(k, y, std::false_type{});
        ++k;
      }
      if (k >= T) break;
    }
    if (CFG::LITERAL || !nonfin) break;
    // cold: decides exactly as the run-time kernel does in its loop.  y is the accepted state (a NaN or inf error is a rejection), the
    // coefficients never change, and Scw is the one the rejected step's factor() computed -- nothing ran since
    if (state_bad() != 0.0 || coef_bad() || (nonfinite(Dsum)) || (nonfinite(Scw))) {
      status |= PK_ST_NONFINITE; break;
    }
  }
  const int nrej = CFG::LITERAL ? nsec : nsec - nacc;
  if (status != PK_ST_OK)                               // a failed replica: NaN rows from the landing it failed at
    for (; k < T; ++k) emit(k, y, std::true_type{});
  trace.exit();
  finish(status, nacc, nrej);
}

}  // namespace pk
