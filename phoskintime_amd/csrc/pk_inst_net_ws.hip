// Instantiations + launcher of the workspace network integrator (net_solve_ws_kernel, pk_network_solve.hpp): topologies 0 / 1 / 2 / 4.
#include "pk_network_solve.hpp"
#include <algorithm>

namespace pk {

namespace {
constexpr int kWsThreads = 256;

const void* ws_kernel(int model) {
  switch (model) {
    case 0: return (const void*)net_solve_ws_kernel<0>;
    case 1: return (const void*)net_solve_ws_kernel<1>;
    case 2: return (const void*)net_solve_ws_kernel<2>;
    default: return (const void*)net_solve_ws_kernel<4>;
  }
}
}  // namespace

// persistent grid: min(B, workgroups of `kernel` at `threads` each resident on the current device at once)
hipError_t net_persistent_grid(const void* kernel, int threads, long long B, int* grid) {
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0);
  if (e != hipSuccess) return e;
  const long long resident = (long long)std::max(per_cu, 1) * std::max(cus, 1);
  *grid = (int)std::min(B, resident);
  return hipSuccess;
}

hipError_t net_ws_grid(const NetDev& n, long long B, int* grid) { return net_persistent_grid(ws_kernel(n.model), kWsThreads, B, grid); }

hipError_t launch_net_ws(const NetDev& n, const NetSolveArgs& a, long long B, int grid, double* ws, hipStream_t st) {
  const size_t slab = net_ws_slab_doubles(n);
  switch (n.model) {
    case 0: hipLaunchKernelGGL(net_solve_ws_kernel<0>, dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    case 1: hipLaunchKernelGGL(net_solve_ws_kernel<1>, dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    case 2: hipLaunchKernelGGL(net_solve_ws_kernel<2>, dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
    default: hipLaunchKernelGGL(net_solve_ws_kernel<4>, dim3((unsigned)grid), dim3(kWsThreads), 0, st, n, a, B, ws, slab); break;
  }
  return hipGetLastError();
}

}  // namespace pk
