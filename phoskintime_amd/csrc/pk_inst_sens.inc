// Instantiations of the forward-sensitivity kernels (pk_sens.hpp), one translation unit per (flavour, model) so that they compile in
// parallel, and the one table that sends a (model, n_sites) to its kernel, whichever flavour of the output stage (pk_sens_out.hpp) the
// argument type selects: launch_sens, launch_sens_metric and launch_sens_vjp (pk_launch.hpp) are launch_sens_any.
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

// the per-(model, kernel) entries, overloaded on the flavour; each is defined in the unit that instantiates its kernels:
// pk_inst_sens[_metric|_vjp]_{dist,succ}.hip (pk_sens.hpp), ..._rows_{dist,succ}.hip (pk_sens_rows.hpp) and, for all three flavours of
// randmod n = 6, 7 (pk_rand_sens.hpp), pk_inst_wide.hip
#define PK_SENS_ENTRIES(Args)                                  \
  hipError_t launch_sens_dist(const Args&, hipStream_t);       \
  hipError_t launch_sens_succ(const Args&, hipStream_t);       \
  hipError_t launch_sens_rows_dist(const Args&, hipStream_t);  \
  hipError_t launch_sens_rows_succ(const Args&, hipStream_t);  \
  hipError_t launch_rand_sens(const Args&, hipStream_t);
PK_SENS_ENTRIES(SensArgs) PK_SENS_ENTRIES(SensMetricArgs) PK_SENS_ENTRIES(SensVjpArgs)
#undef PK_SENS_ENTRIES
bool sens_takes_rows(int model, int n_sites);                // pk_inst_sens_rand.hip: the one place that reads the switches

// sizes with a sensitivity kernel: distmod / succmod n <= 14 (S <= 16 rows in one lane, 1 + P = 5 + 2 n <= 64 columns in one wave: the
// default below n = 10 / 6) and up to n = 62 (rows across the lanes of a group, eight columns per lane, the columns of a replica cut into
// chunks: pk_sens_rows.hpp; PK_SENS_ROWS=1 forces it everywhere, =2 forbids it below n = 15),
// randmod n = 6, 7 (parity-eliminated inverse in registers serving eight columns per workgroup: pk_rand_sens.hpp),
// randmod n <= 3 (2^n <= 8 coupled rows inverted in registers; 1 + P <= 16 columns) and n = 4, 5 (the inverse shared by the group in LDS)
template <class Args>
static hipError_t launch_sens_any(const Args& a, int model, hipStream_t st) {
  if (sens_takes_rows(model, a.s.n_sites)) return model == M_DIST ? launch_sens_rows_dist(a, st) : launch_sens_rows_succ(a, st);
  if (model == M_DIST) return launch_sens_dist(a, st);
  if (model == M_SUCC) return launch_sens_succ(a, st);
  const int n = a.s.n_sites;
  if (n >= 6) return launch_rand_sens(a, st);                        // 74 / 139 columns of 65 / 129 rows: chunks of eight columns per workgroup
  if (n == 1) return launch_sens_one<CubeSys<1>, 8>(a, st);          // 1 + P = 7
  if (n == 2) return launch_sens_one<CubeSys<2>, 16>(a, st);         // 10
  if (n == 3) return launch_sens_one<CubeSys<3>, 16>(a, st);         // 15
  if (n == 4) return launch_sens_one<CubeLdsSys<4, 32>, 32>(a, st);  // 1 + P = 24 columns, 17 rows
  return launch_sens_one<CubeLdsSys<5, 64>, 64>(a, st);              // 41 columns, 33 rows
}
