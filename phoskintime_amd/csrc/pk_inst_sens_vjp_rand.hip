// VJP flavour of the column-per-lane forward-sensitivity kernels (pk_sens.hpp, SensVjpArgs) for the random model, n <= 5, and the
// dispatch of the flavour: the same kernel per (model, n_sites) as launch_sens takes.
#include "pk_inst_sens.inc"
hipError_t launch_rand_sens_vjp(const SensVjpArgs&, hipStream_t);           // randmod n = 6, 7 (pk_rand_sens.hpp), instantiated beside launch_rand_sens
hipError_t launch_sens_vjp_dist(const SensVjpArgs&, hipStream_t);
hipError_t launch_sens_vjp_succ(const SensVjpArgs&, hipStream_t);
hipError_t launch_sens_vjp_rows_dist(const SensVjpArgs&, hipStream_t);
hipError_t launch_sens_vjp_rows_succ(const SensVjpArgs&, hipStream_t);
bool sens_takes_rows(int model, int n_sites);

hipError_t launch_sens_vjp(const SensVjpArgs& a, int model, hipStream_t st) {
  if (sens_takes_rows(model, a.s.n_sites)) return model == M_DIST ? launch_sens_vjp_rows_dist(a, st) : launch_sens_vjp_rows_succ(a, st);
  if (model == M_DIST) return launch_sens_vjp_dist(a, st);
  if (model == M_SUCC) return launch_sens_vjp_succ(a, st);
  const int n = a.s.n_sites;
  if (n >= 6) return launch_rand_sens_vjp(a, st);
  if (n == 1) return launch_sens_one<CubeSys<1>, 8>(a, st);
  if (n == 2) return launch_sens_one<CubeSys<2>, 16>(a, st);
  if (n == 3) return launch_sens_one<CubeSys<3>, 16>(a, st);
  if (n == 4) return launch_sens_one<CubeLdsSys<4, 32>, 32>(a, st);
  return launch_sens_one<CubeLdsSys<5, 64>, 64>(a, st);
}

}  // namespace pk
