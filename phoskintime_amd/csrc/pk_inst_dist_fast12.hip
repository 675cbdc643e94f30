// LRP12 instantiations of the distributive-model throughput kernel (pk_dist_fast.hpp) -- the default method gets the fine-grained
// layout table: G lanes per replica x RPL site rows per lane with G * RPL >= n_sites and as few idle rows as possible.
//   * fewer lanes per replica = fewer DPP reduction levels per solve and less redundant work on the shadowed (R, P) rows;
//   * a size whose G x RPL slots hold the whole state (G * RPL >= n + 2) runs the RESIDENT layout of the same (G, RPL): R and P in slots
//     0 and 1, no shadow rows at all (instantiated in pk_inst_dist_fast12r.hip; launch helpers shared through pk_dist_fast12.hpp);
//   * RPL >= 5 needs more than 256 VGPRs with everything in registers: those layouts park the once-per-step values (site rates) and the
//     once-per-output values (metric bookkeeping) in LDS (Parked<RPL, true>) and run two waves per SIMD.
// Measured, B = 65 536, theta ~ U(0, 20) (tools/gpu_bench_dev.py layouts): n = 14: 4x4 0.287 ms vs 8x2 0.410; n = 30: 4x8 parked 0.422 vs
// 8x4 0.528; n = 62: 8x8 parked 0.913 vs 16x4 1.206.
#include "pk_dist_fast12.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pk {

const char* const kDistSchedNames = "off, lead, level, lead+level";

// "lead" is the rule the measured timeline picked, hardware wave slot 0; lead:slot and lead:block name the two rules for A/B runs
int dist_sched_parse(const char* v) {
  if (!v || !*v) return -1;
  if (!strcmp(v, "off")) return PK_DSCHED_OFF;
  int bits = 0;
  for (const char* p = v; *p;) {
    const char* e = strchr(p, '+');
    const size_t len = e ? (size_t)(e - p) : strlen(p);
    auto is = [&](const char* w) { return strlen(w) == len && !strncmp(p, w, len); };
    int b;
    if (is("lead") || is("lead:slot")) b = PK_DSCHED_LEAD_SLOT;
    else if (is("lead:block")) b = PK_DSCHED_LEAD_BLOCK;
    else if (is("level")) b = PK_DSCHED_LEVEL;
    else return -1;
    if (bits & b) return -1;
    bits |= b;
    p += len;
    if (e) { ++p; if (!*p) return -1; }
  }
  return bits;
}

// An unknown value reads as -1 here, and the C entry points refuse to launch (pk_capi.hip); a launch that gets here all the same runs unpaced
int dist_sched_env() {
  static const int v = [] { const char* e = getenv("PK_DIST_SCHED"); return e ? dist_sched_parse(e) : PK_DSCHED_UNSET; }();
  return v;
}

template <int G, int RPL>
static void launch_plain(const SolveArgs& a, hipStream_t st) { launch_nt<G, RPL, false, 256, false>(a, st); }

// parked layouts: one wave per workgroup -- a workgroup keeps its LDS and its place on the CU until its slowest wave is done, and the step
// counts of the replicas differ (35-46 on the benchmark's batch), so wave-sized workgroups let the dispatcher refill each wave slot as it ends
template <int G, int RPL>
static void launch_parked(const SolveArgs& a, hipStream_t st) { launch_nt<G, RPL, true, 64, false>(a, st); }

void launch_dist_fast12(const SolveArgs& a, hipStream_t st) {
  const int n = a.n_sites;
  // dev A/B: PK_DIST_LAYOUT=8x4 forces the register-only 8 x 4 layout for 17 <= n <= 32; PK_DIST_LAYOUT=wg256 runs the 4 x 8 parked
  // layout (29 <= n <= 32) in 256-thread workgroups
  static const bool force84 = getenv("PK_DIST_LAYOUT") && !strcmp(getenv("PK_DIST_LAYOUT"), "8x4");
  static const bool wg256 = getenv("PK_DIST_LAYOUT") && !strcmp(getenv("PK_DIST_LAYOUT"), "wg256");
  // Resident layout (no shadow copies of R and P: pk_dist_fast.hpp) exactly where the table's G x RPL slots hold the whole state,
  // G * RPL >= n + 2: n = 1, 2 (mod 4) up to 30 and n = 33-38, 41-46, 49-54, 57-62.  dev A/B: PK_DIST_LAYOUT=shadow keeps the shadowed
  // layout at every n (as does 8x4, which names a shadowed layout); read once per process
  static const bool shadow = getenv("PK_DIST_LAYOUT") && !strcmp(getenv("PK_DIST_LAYOUT"), "shadow");
  const int slots = n <= 32 ? 4 * ((n + 3) / 4) : 8 * ((n + 7) / 8);
  if (!shadow && !(force84 && n > 16 && n <= 32) && n >= 1 && slots >= n + 2) { launch_dist_fast12_resident(a, wg256, st); return; }
  if (n <= 4) launch_plain<4, 1>(a, st);
  else if (n <= 8) launch_plain<4, 2>(a, st);
  else if (n <= 12) launch_plain<4, 3>(a, st);
  else if (n <= 16) launch_plain<4, 4>(a, st);
  else if (n <= 32 && force84) launch_plain<8, 4>(a, st);
  else if (n <= 20) launch_parked<4, 5>(a, st);
  else if (n <= 24) launch_parked<4, 6>(a, st);
  else if (n <= 28) launch_parked<4, 7>(a, st);
  else if (n <= 32 && wg256) launch_nt<4, 8, true, 256, false>(a, st);
  else if (n <= 32) launch_parked<4, 8>(a, st);
  else if (n <= 40) launch_parked<8, 5>(a, st);
  else if (n <= 48) launch_parked<8, 6>(a, st);
  else if (n <= 56) launch_parked<8, 7>(a, st);
  else launch_parked<8, 8>(a, st);
}

}  // namespace pk
