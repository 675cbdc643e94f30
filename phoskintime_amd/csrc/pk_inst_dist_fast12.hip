// The shadowed half of the LRP12 launch table of the distributive-model throughput kernel (pk_dist_fast12.hpp), and the default
// method's launcher: which half serves a size, and the development overrides (PK_DIST_LAYOUT, PK_DIST_TRACE, PK_DIST_SCHED).
#include "pk_dist_fast12.hpp"

namespace pk {

void launch_dist_fast12(const SolveArgs& a, hipStream_t st) {
  const int n = a.n_sites;
  const DistLayoutEnv layout = env().dist_layout;
  const bool wg256 = layout == PK_DLAYOUT_WG256;
  if (layout == PK_DLAYOUT_8X4 && n > 16 && n <= 32) { launch_nt<8, 4, false, 256, false>(a, st); return; }
  // Resident layout (no shadow copies of R and P: pk_dist_fast.hpp) exactly where the table's G x RPL slots hold the whole state,
  // G * RPL >= n + 2: n = 1, 2 (mod 4) up to 30 and n = 33-38, 41-46, 49-54, 57-62
  const int slots = n <= 32 ? 4 * ((n + 3) / 4) : 8 * ((n + 7) / 8);
  if (layout == PK_DLAYOUT_SHADOW || n < 1 || slots < n + 2) { launch_table12<false>(a, wg256, st); return; }
  // dev: PK_DIST_TRACE=1 runs the benchmark's configuration on the traced build of its kernel
  if (env().dist_trace && n > 26 && n <= 30 && !wg256 && DistSolSum::matches(a)) { launch_dist_fast12_traced(a, st); return; }
  launch_dist_fast12_resident(a, wg256, st);
}

}  // namespace pk
