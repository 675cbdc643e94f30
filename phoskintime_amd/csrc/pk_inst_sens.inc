// Instantiations of the forward-sensitivity kernels (pk_sens.hpp), one translation unit per model so that they compile in parallel.
#include "pk_sens.hpp"
#include "pk_launch.hpp"

namespace pk {

template <class Sys, int GP, class Args>
static hipError_t launch_sens_one(const Args& a, hipStream_t st) {
  constexpr int NG = 64 / GP;
  constexpr bool MET = sens_metric_flavour<Args>();
  const long long nblk = (a.s.B + NG - 1) / NG;
  static_assert(sens_metric_lds_bytes<Sys, GP>(true) <= 64 * 1024, "fits the default dynamic-LDS limit");
  size_t lds = sens_lds_bytes<Sys, GP>();
  if constexpr (MET) lds = sens_metric_lds_bytes<Sys, GP>(a.s.metric_id == PK_METRIC_DYNAMICS);
  hipLaunchKernelGGL((sens_kernel<Sys, GP, Args>), dim3((unsigned)nblk), dim3(64), lds, st, a);
  return hipGetLastError();
}

template <int MODEL, class Args>
static hipError_t launch_sens_chain(const Args& a, hipStream_t st) {
  const int n = a.s.n_sites;                                 // columns: 1 + P = 5 + 2 n
  if (n <= 1) return launch_sens_one<ChainSys<MODEL, 1>, 8>(a, st);
  if (n <= 3) return launch_sens_one<ChainSys<MODEL, 3>, 16>(a, st);
  if (n <= 5) return launch_sens_one<ChainSys<MODEL, 5>, 16>(a, st);
  if (n <= 9) return launch_sens_one<ChainSys<MODEL, 9>, 32>(a, st);
  if (n <= 13) return launch_sens_one<ChainSys<MODEL, 13>, 32>(a, st);
  return launch_sens_one<ChainSys<MODEL, 14>, 64>(a, st);
}
