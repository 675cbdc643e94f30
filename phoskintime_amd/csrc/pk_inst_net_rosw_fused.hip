// Instantiations + launchers of the order-3 network integrator that scores the three-objective loss as it integrates
// (net_rosw_solve<MODEL, SCORE_LOSS>, pk_network_solve.hpp): the LDS kernel and the workspace kernel, topologies 0 / 1 / 2 / 4.
#include "pk_network_solve.hpp"

namespace pk {

hipError_t net_persistent_grid(const void* kernel, int threads, long long B, int* grid);      // pk_inst_net_ws.hip

namespace {
constexpr int kWsThreads = 256;

const void* ws_fused_kernel(int model) {
  switch (model) {
    case 0: return (const void*)net_solve_ws_fused_kernel<0>;
    case 1: return (const void*)net_solve_ws_fused_kernel<1>;
    case 2: return (const void*)net_solve_ws_fused_kernel<2>;
    default: return (const void*)net_solve_ws_fused_kernel<4>;
  }
}
}  // namespace

hipError_t net_ws_fused_grid(const NetDev& n, long long B, int* grid) { return net_persistent_grid(ws_fused_kernel(n.model), kWsThreads, B, grid); }

// ws: grid x net_ws_fused_slab_doubles(n) doubles
hipError_t launch_net_ws_fused(const NetDev& n, const NetSolveArgs& a, long long B, int grid, double* ws, hipStream_t st) {
  const size_t slab = net_ws_fused_slab_doubles(n);
  switch (n.model) {
    case 0: hipLaunchKernelGGL((net_solve_ws_fused_kernel<0>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    case 1: hipLaunchKernelGGL((net_solve_ws_fused_kernel<1>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    case 2: hipLaunchKernelGGL((net_solve_ws_fused_kernel<2>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    default: hipLaunchKernelGGL((net_solve_ws_fused_kernel<4>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
  }
  return hipGetLastError();
}

// lds: net_solve_fused_lds_bytes (<= 160 KiB: the caller checks)
hipError_t launch_net_lds_fused(const NetDev& n, const NetSolveArgs& a, long long B, int threads, size_t lds, hipStream_t st) {
#define PK_FUSED_LAUNCH(M)                                                                                                            \
  do {                                                                                                                                \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)net_solve_kernel<M, SCORE_LOSS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((net_solve_kernel<M, SCORE_LOSS>), dim3((unsigned)B), dim3(threads), lds, st, n, a);                                  \
  } while (0)
  switch (n.model) {
    case 0: PK_FUSED_LAUNCH(0); break;
    case 1: PK_FUSED_LAUNCH(1); break;
    case 2: PK_FUSED_LAUNCH(2); break;
    default: PK_FUSED_LAUNCH(4); break;
  }
#undef PK_FUSED_LAUNCH
  return hipGetLastError();
}

}  // namespace pk
