// The shadowed half of the LRP12 launch table of the distributive-model throughput kernel (pk_dist_fast12.hpp), and the default
// method's launcher: which half serves a size, and the development overrides (PK_DIST_LAYOUT, PK_DIST_TRACE, PK_DIST_SCHED).
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

DistLayoutEnv dist_layout_env() {
  static const DistLayoutEnv v = [] {
    const char* e = getenv("PK_DIST_LAYOUT");
    if (!e) return PK_DLAYOUT_NONE;
    return !strcmp(e, "8x4") ? PK_DLAYOUT_8X4 : !strcmp(e, "wg256") ? PK_DLAYOUT_WG256 : !strcmp(e, "shadow") ? PK_DLAYOUT_SHADOW : PK_DLAYOUT_NONE;
  }();
  return v;
}

void launch_dist_fast12(const SolveArgs& a, hipStream_t st) {
  const int n = a.n_sites;
  const DistLayoutEnv layout = dist_layout_env();
  const bool wg256 = layout == PK_DLAYOUT_WG256;
  if (layout == PK_DLAYOUT_8X4 && n > 16 && n <= 32) { launch_nt<8, 4, false, 256, false>(a, st); return; }
  // Resident layout (no shadow copies of R and P: pk_dist_fast.hpp) exactly where the table's G x RPL slots hold the whole state,
  // G * RPL >= n + 2: n = 1, 2 (mod 4) up to 30 and n = 33-38, 41-46, 49-54, 57-62
  const int slots = n <= 32 ? 4 * ((n + 3) / 4) : 8 * ((n + 7) / 8);
  if (layout == PK_DLAYOUT_SHADOW || n < 1 || slots < n + 2) { launch_table12<false>(a, wg256, st); return; }
  // dev: PK_DIST_TRACE=1 (read once per process) runs the benchmark's configuration on the traced build of its kernel
  static const bool traced = getenv("PK_DIST_TRACE") && !strcmp(getenv("PK_DIST_TRACE"), "1");
  if (traced && n > 26 && n <= 30 && !wg256 && DistSolSum::matches(a)) { launch_dist_fast12_traced(a, st); return; }
  launch_dist_fast12_resident(a, wg256, st);
}

}  // namespace pk
