// Instantiations + launchers of the sensitivity integrator on HBM-workspace slabs (net_solve_sens_ws_kernel and
// net_solve_sens_score_ws_kernel, pk_network_sens.hpp): net_rosw_sens_solve<MODEL, SENS_STORE / SENS_SCORE, NetWsLayout> on a persistent
// grid over (candidate, column chunk) work items, topologies 0 / 1 / 2 / 4, networks of any size.
#include "pk_network_sens.hpp"

namespace pk {

hipError_t net_persistent_grid(const void* kernel, int threads, long long B, int* grid);      // pk_inst_net_ws.hip

namespace {
constexpr int kWsThreads = 256;

const void* sens_ws_kernel(int model, bool score) {
  switch (model) {
    case 0: return score ? (const void*)net_solve_sens_score_ws_kernel<0> : (const void*)net_solve_sens_ws_kernel<0>;
    case 1: return score ? (const void*)net_solve_sens_score_ws_kernel<1> : (const void*)net_solve_sens_ws_kernel<1>;
    case 2: return score ? (const void*)net_solve_sens_score_ws_kernel<2> : (const void*)net_solve_sens_ws_kernel<2>;
    default: return score ? (const void*)net_solve_sens_score_ws_kernel<4> : (const void*)net_solve_sens_ws_kernel<4>;
  }
}
}  // namespace

// grid = min(work items, resident workgroups of the flavour's kernel)
hipError_t net_sens_ws_grid(const NetDev& n, bool score, long long items, int* grid) {
  return net_persistent_grid(sens_ws_kernel(n.model, score), kWsThreads, items, grid);
}

// ws: grid x net_sens_ws_slab_doubles(n, min(K, KC), score != null) doubles; B x ceil(K / KC) work items
hipError_t launch_net_ws_sens(const NetDev& n, const NetSolveArgs& a, const NetSensArgs& s, const NetSensScoreArgs* sc, long long B, int grid,
                              double* ws, hipStream_t st) {
  const int n_chunks = (s.K + s.KC - 1) / s.KC;
  const long long items = B * n_chunks;
  const size_t slab = net_sens_ws_slab_doubles(n, s.K < s.KC ? s.K : s.KC, sc != nullptr);
#define PK_SENS_WS_LAUNCH(M)                                                                                                              \
  do {                                                                                                                                    \
    if (sc) hipLaunchKernelGGL((net_solve_sens_score_ws_kernel<M>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, s, *sc, items,   \
                               n_chunks, ws, slab);                                                                                       \
    else    hipLaunchKernelGGL((net_solve_sens_ws_kernel<M>), dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, s, items, n_chunks,    \
                               ws, slab);                                                                                                 \
  } while (0)
  switch (n.model) {
    case 0: PK_SENS_WS_LAUNCH(0); break;
    case 1: PK_SENS_WS_LAUNCH(1); break;
    case 2: PK_SENS_WS_LAUNCH(2); break;
    default: PK_SENS_WS_LAUNCH(4); break;
  }
#undef PK_SENS_WS_LAUNCH
  return hipGetLastError();
}

}  // namespace pk
