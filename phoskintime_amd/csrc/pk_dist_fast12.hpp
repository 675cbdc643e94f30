// pk_dist_fast12.hpp -- launch helpers shared by the two translation units that hold the LRP12 instantiations of the distributive-model
// throughput kernel: pk_inst_dist_fast12.hip (launch table, shadowed layout) and pk_inst_dist_fast12r.hip (resident layout).
#pragma once
#include "pk_dist_fast.hpp"
#include "pk_launch.hpp"

namespace pk {

// One instantiation: NT threads per workgroup, launch-uniform choices CFG, shadowed or resident rows (pk_dist_fast.hpp).
template <int G, int RPL, bool PARK, int NT, class CFG, bool RES>
static void launch_cfg(const SolveArgs& a, hipStream_t st) {
  const long long rpb = NT / G;
  const long long nblk = (a.B + rpb - 1) / rpb;
  constexpr size_t lds = dist_fast_lds_bytes<RPL, PARK, NT, CFG, RES>();
  auto kern = dist_fast_kernel<G, RPL, PK_METHOD_LRP12, PARK, (PARK ? 2 : 1), NT, CFG, RES>;
  if constexpr (lds > 48 * 1024) {
    static const bool once = [kern] {
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      return true;
    }();
    (void)once;
  }
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

// resident layout of the LRP12 table's (G, RPL) for n_sites = n, for the sizes with G * RPL >= n + 2 (pk_inst_dist_fast12r.hip)
void launch_dist_fast12_resident(const SolveArgs& a, bool wg256, hipStream_t st);

}  // namespace pk
