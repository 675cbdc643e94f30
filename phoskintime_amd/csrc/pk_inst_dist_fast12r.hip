// LRP12 instantiations of the distributive-model throughput kernel in the RESIDENT layout (pk_dist_fast.hpp: R and P in slots 0 and 1 of
// the G x RPL lane layout, nothing shadowed), a translation unit of their own so that the two halves of the table compile side by side.
// Same (G, RPL), parking and workgroup size per n as the table in pk_inst_dist_fast12.hip, which calls this for the sizes that fit.
#include "pk_dist_fast12.hpp"
#include <cstdlib>
#include <cstring>

namespace pk {

void launch_dist_fast12_resident(const SolveArgs& a, bool wg256, hipStream_t st) {
  const int n = a.n_sites;
  // dev: PK_DIST_TRACE=1 (read once per process) runs the benchmark's configuration on the traced build of its kernel
  static const bool traced = getenv("PK_DIST_TRACE") && !strcmp(getenv("PK_DIST_TRACE"), "1");
  if (traced && n > 26 && n <= 30 && !wg256 && DistSolSum::matches(a)) { launch_dist_fast12_traced(a, st); return; }
  if (n <= 2) launch_nt<4, 1, false, 256, true>(a, st);
  else if (n <= 6) launch_nt<4, 2, false, 256, true>(a, st);
  else if (n <= 10) launch_nt<4, 3, false, 256, true>(a, st);
  else if (n <= 14) launch_nt<4, 4, false, 256, true>(a, st);
  else if (n <= 18) launch_nt<4, 5, true, 64, true>(a, st);
  else if (n <= 22) launch_nt<4, 6, true, 64, true>(a, st);
  else if (n <= 26) launch_nt<4, 7, true, 64, true>(a, st);
  else if (n <= 30 && wg256) launch_nt<4, 8, true, 256, true>(a, st);
  else if (n <= 30) launch_nt<4, 8, true, 64, true>(a, st);
  else if (n <= 38) launch_nt<8, 5, true, 64, true>(a, st);
  else if (n <= 46) launch_nt<8, 6, true, 64, true>(a, st);
  else if (n <= 54) launch_nt<8, 7, true, 64, true>(a, st);
  else launch_nt<8, 8, true, 64, true>(a, st);
}

}  // namespace pk
