// Instantiations + launcher of the scoring flavour of the sensitivity integrator (net_rosw_sens_solve<MODEL, SENS_SCORE>,
// pk_network_sens.hpp): the three-objective loss and its gradient with respect to the chunk's columns, formed where state and tangents land
// on an output row.  The general LDS kernel, topologies 0 / 1 / 2 / 4, one workgroup per (candidate, column chunk).
#include "pk_network_sens.hpp"

namespace pk {

// lds: net_sens_score_lds_bytes(n, nnzT, min(K, KC)) (<= 160 KiB: the caller checks); grid B x ceil(K / KC)
hipError_t launch_net_lds_sens_score(const NetDev& n, const NetSolveArgs& a, const NetSensArgs& s, const NetSensScoreArgs& sc, long long B, int threads,
                                     size_t lds, hipStream_t st) {
  const unsigned chunks = (unsigned)((s.K + s.KC - 1) / s.KC);
#define PK_SENS_SCORE_LAUNCH(M)                                                                                                        \
  do {                                                                                                                                 \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)net_solve_sens_score_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((net_solve_sens_score_kernel<M>), dim3((unsigned)B, chunks), dim3(threads), lds, st, n, a, s, sc);              \
  } while (0)
  switch (n.model) {
    case 0: PK_SENS_SCORE_LAUNCH(0); break;
    case 1: PK_SENS_SCORE_LAUNCH(1); break;
    case 2: PK_SENS_SCORE_LAUNCH(2); break;
    default: PK_SENS_SCORE_LAUNCH(4); break;
  }
#undef PK_SENS_SCORE_LAUNCH
  return hipGetLastError();
}

}  // namespace pk
