// Instantiations + launchers of the order-3 network integrator that measures the fold-change observables and reduces them to the scalar
// Morris metric as it integrates (net_rosw_solve<MODEL, SCORE_MEASURE>, pk_network_solve.hpp): the LDS kernel and the workspace kernel,
// topologies 0 / 1 / 2 / 4.  LDS request and slab are those of the fused objective (the rna baseline: N more doubles per candidate).
#include "pk_network_solve.hpp"

namespace pk {

hipError_t net_persistent_grid(const void* kernel, int threads, long long B, int* grid);      // pk_inst_net_ws.hip

namespace {
constexpr int kWsThreads = 256;

const void* ws_measure_kernel(int model) {
  switch (model) {
    case 0: return (const void*)net_solve_ws_fused_kernel<0, SCORE_MEASURE>;
    case 1: return (const void*)net_solve_ws_fused_kernel<1, SCORE_MEASURE>;
    case 2: return (const void*)net_solve_ws_fused_kernel<2, SCORE_MEASURE>;
    default: return (const void*)net_solve_ws_fused_kernel<4, SCORE_MEASURE>;
  }
}
}  // namespace

hipError_t net_ws_measure_grid(const NetDev& n, long long B, int* grid) { return net_persistent_grid(ws_measure_kernel(n.model), kWsThreads, B, grid); }

// ws: grid x net_ws_fused_slab_doubles(n) doubles
hipError_t launch_net_ws_measure(const NetDev& n, const NetSolveArgs& a, long long B, int grid, double* ws, hipStream_t st) {
  const size_t slab = net_ws_fused_slab_doubles(n);
  switch (n.model) {
    case 0: hipLaunchKernelGGL((net_solve_ws_fused_kernel<0, SCORE_MEASURE>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    case 1: hipLaunchKernelGGL((net_solve_ws_fused_kernel<1, SCORE_MEASURE>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    case 2: hipLaunchKernelGGL((net_solve_ws_fused_kernel<2, SCORE_MEASURE>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    default: hipLaunchKernelGGL((net_solve_ws_fused_kernel<4, SCORE_MEASURE>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
  }
  return hipGetLastError();
}

// lds: net_solve_fused_lds_bytes (<= 160 KiB: the caller checks)
hipError_t launch_net_lds_measure(const NetDev& n, const NetSolveArgs& a, long long B, int threads, size_t lds, hipStream_t st) {
#define PK_MEASURE_LAUNCH(M)                                                                                                          \
  do {                                                                                                                                \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)net_solve_kernel<M, SCORE_MEASURE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((net_solve_kernel<M, SCORE_MEASURE>), dim3((unsigned)B), dim3(threads), lds, st, n, a);                         \
  } while (0)
  switch (n.model) {
    case 0: PK_MEASURE_LAUNCH(0); break;
    case 1: PK_MEASURE_LAUNCH(1); break;
    case 2: PK_MEASURE_LAUNCH(2); break;
    default: PK_MEASURE_LAUNCH(4); break;
  }
#undef PK_MEASURE_LAUNCH
  return hipGetLastError();
}

}  // namespace pk
