// pk_dist_fast12.hpp -- the LRP12 launch table of the distributive-model throughput kernel (launch_table12, one template for both row
// layouts) and its launch helpers, shared by the translation units that hold the instantiations: pk_inst_dist_fast12.hip (the shadowed
// half of the table, the choice between the halves), pk_inst_dist_fast12r.hip (the resident half), pk_inst_dist_fast12t.hip (traced build).
#pragma once
#include "pk_dist_fast.hpp"
#include "pk_launch.hpp"

namespace pk {

// One instantiation: NT threads per workgroup, launch-uniform choices CFG, shadowed or resident rows (pk_dist_fast.hpp).
template <int G, int RPL, bool PARK, int NT, class CFG, bool RES, int TRACE = 0>
static void launch_cfg(const SolveArgs& a, hipStream_t st) {
  const long long rpb = NT / G;
  const long long nblk = (a.B + rpb - 1) / rpb;
  constexpr size_t lds = dist_fast_lds_bytes<RPL, PARK, NT, CFG, RES>();
  auto kern = dist_fast_kernel<G, RPL, PK_METHOD_LRP12, PARK, (PARK ? 2 : 1), NT, CFG, RES, TRACE>;
  if constexpr (lds > 48 * 1024) {
    static const bool once = [kern] {
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      return true;
    }();
    (void)once;
  }
  if constexpr (PARK && NT == 64) {
    // the paced kernels: the policy, and the workgroups the device holds at once (occupancy of this kernel x compute units, asked once per
    // kernel; a failed query reads as "everything fits one round", which keeps the leaders off)
    static const int resident = [kern] {
      int dev = 0, cus = 0, per_cu = 0;
      if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kern, NT, lds) != hipSuccess || per_cu < 1 || cus < 1) {
        (void)hipGetLastError();
        return 0x7fffffff;
      }
      return per_cu * cus;
    }();
    SolveArgs b = a;
    // unset: what was measured.  Pacing pays while a SIMD gets at most one wave beyond its resident ones -- a grid of up
    // to 4/3 of the resident capacity, the benchmark's 4 096 workgroups on 3 072 slots among them -- in the four-lane layouts; larger
    // grids and the eight-lane layouts, which it slowed, run unpaced.  A setting of PK_DIST_SCHED applies to every grid (A/B runs); one that
    // names no policy, which the C entry points refuse before a launch (pk_capi.hip), runs unpaced if it gets here all the same
    const int env = pk::env().dist_sched;
    const bool pays = G == 4 && nblk <= (long long)resident + resident / 3;
    b.sched = env == PK_DSCHED_UNSET ? (pays ? PK_DSCHED_LEAD_SLOT | PK_DSCHED_LEVEL : PK_DSCHED_OFF) : env < 0 ? (int)PK_DSCHED_OFF : env;
    b.R1 = resident;
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(NT), lds, st, b);
  } else
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(NT), lds, st, a);
}

// The combinations the library's own callers produce get a kernel with those choices compiled in (no dead output paths, no bookkeeping
// slots they do not use); every other combination runs the kernel that reads them from SolveArgs.  The four output classes of a layout
// always share its row placement (RES), so the specialised kernels stay comparable with DistAny bit for bit.
template <int G, int RPL, bool PARK, int NT, bool RES>
static void launch_nt(const SolveArgs& a, hipStream_t st) {
  if (DistSolSum::matches(a)) launch_cfg<G, RPL, PARK, NT, DistSolSum, RES>(a, st);
  else if (DistSolOnly::matches(a)) launch_cfg<G, RPL, PARK, NT, DistSolOnly, RES>(a, st);
  else if (DistFlatOnly::matches(a)) launch_cfg<G, RPL, PARK, NT, DistFlatOnly, RES>(a, st);
  else launch_cfg<G, RPL, PARK, NT, DistAny, RES>(a, st);
}

// PK_DIST_LAYOUT (dev A/B; DistLayoutEnv of pk_env.hpp):
//   8x4     forces the register-only, shadowed 8 x 4 layout for 17 <= n <= 32;
//   wg256   runs the 4 x 8 parked layout in 256-thread workgroups;
//   shadow  keeps the shadowed layout at every n.
//
// The LRP12 layout table: G lanes per replica x RPL rows per lane for the slots a replica needs -- its n sites, and R and P as well in the
// resident layout -- with as few idle slots as possible.
//   * G = 4 up to 32 slots, 8 above: fewer lanes per replica = fewer DPP reduction levels per solve (and, shadowed, less redundant work on
//     the R and P rows);
//   * RPL >= 5 needs more than 256 VGPRs with everything in registers: those layouts park the once-per-step values (site rates) and the
//     once-per-output values (metric bookkeeping) in LDS (Parked<RPL, true>) and run two waves per SIMD, in workgroups of one wave -- a
//     workgroup keeps its LDS and its place on the CU until its slowest wave is done, and the step counts of the replicas differ (35-46
//     on the benchmark's batch), so wave-sized workgroups let the dispatcher refill each wave slot as it ends;
//   * wg256: the 4 x 8 entry in 256-thread workgroups (PK_DIST_LAYOUT=wg256).
// Measured, B = 65 536, theta ~ U(0, 20) (tools/gpu_bench_dev.py layouts): n = 14: 4x4 0.287 ms vs 8x2 0.410; n = 30: 4x8 parked 0.422 vs
// 8x4 0.528; n = 62: 8x8 parked 0.913 vs 16x4 1.206.
// Each half is instantiated in a translation unit of its own (RES = false: pk_inst_dist_fast12.hip, true: pk_inst_dist_fast12r.hip,
// reached through launch_dist_fast12_resident), so that the two compile side by side.
template <bool RES>
static void launch_table12(const SolveArgs& a, bool wg256, hipStream_t st) {
  const int slots = a.n_sites + (RES ? 2 : 0);
  if (slots <= 4) launch_nt<4, 1, false, 256, RES>(a, st);
  else if (slots <= 8) launch_nt<4, 2, false, 256, RES>(a, st);
  else if (slots <= 12) launch_nt<4, 3, false, 256, RES>(a, st);
  else if (slots <= 16) launch_nt<4, 4, false, 256, RES>(a, st);
  else if (slots <= 20) launch_nt<4, 5, true, 64, RES>(a, st);
  else if (slots <= 24) launch_nt<4, 6, true, 64, RES>(a, st);
  else if (slots <= 28) launch_nt<4, 7, true, 64, RES>(a, st);
  else if (slots <= 32 && wg256) launch_nt<4, 8, true, 256, RES>(a, st);
  else if (slots <= 32) launch_nt<4, 8, true, 64, RES>(a, st);
  else if (slots <= 40) launch_nt<8, 5, true, 64, RES>(a, st);
  else if (slots <= 48) launch_nt<8, 6, true, 64, RES>(a, st);
  else if (slots <= 56) launch_nt<8, 7, true, 64, RES>(a, st);
  else launch_nt<8, 8, true, 64, RES>(a, st);
}
// the resident half (pk_inst_dist_fast12r.hip)
void launch_dist_fast12_resident(const SolveArgs& a, bool wg256, hipStream_t st);

// the diagnostic build of the benchmark's kernel (4 x 8 resident, DistSolSum) with the wave timeline, and its buffer (pk_inst_dist_fast12t.hip)
void launch_dist_fast12_traced(const SolveArgs& a, hipStream_t st);
hipError_t dist_trace_set(void* records, long long capacity);

}  // namespace pk
