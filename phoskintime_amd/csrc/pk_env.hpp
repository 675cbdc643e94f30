// pk_env.hpp -- every PK_* environment switch the library reads: one typed field each (Env), one parser (env_parse) over a caller-supplied
// lookup, and the word parsers of the two switches that take words.  Plain C++: no HIP, no getenv, no statics, so it compiles under
// hipcc and under g++ (tests/test_env_cpu.py holds env_parse to a table of strings written out from the reads as they stood when each
// launcher parsed its own).  The only getenv calls of the library are in pk_env.hip.
//
// The snapshot rule.  env() (pk_env.hip) parses the process environment once, at its first call, and every FROZEN switch is read from that
// snapshot: all of them freeze together, at the first library call that consults any switch.  Set them before that call -- in practice
// before the process starts or before the library is loaded; a later change is not seen.  The LIVE switches are read again at every call
// through env_live(), so that a process may change them between two library calls.
//
// Each kind of switch keeps the parsing rule it has always had; the rules disagree on the same string on purpose of history, not of
// design ("10" is on for env_starts_1 and off for env_equals_1), and the helpers below name them so that the table in env_parse says
// which switch follows which.  An empty string is a value, not "unset": atoi and atof read it as 0.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace pk {

// ---- the parsing rules, one helper per rule (v: the variable's value, null when unset)
inline int env_atoi(const char* v, int unset) { return v ? atoi(v) : unset; }                 // leading blanks skipped, trailing text ignored, no digits: 0
inline bool env_unless_0(const char* v) { return !(v && v[0] == '0'); }                       // on unless the first character is 0
inline bool env_starts_1(const char* v) { return v && v[0] == '1'; }                          // on when the first character is 1
inline bool env_equals_1(const char* v) { return v && !strcmp(v, "1"); }                      // on for the string "1" alone
inline bool env_atoi_is_1(const char* v) { return v && atoi(v) == 1; }                        // on when atoi reads 1
inline double env_atof(const char* v) { return v ? atof(v) : 0.0; }
inline double env_atof_within_0_1(const char* v, double otherwise) { const double f = env_atof(v); return (f > 0.0 && f <= 1.0) ? f : otherwise; }
inline size_t env_atol_size(const char* v) { return v ? (size_t)atol(v) : (size_t)0; }

// ---- PK_DIST_SCHED: the wave-pacing policy of the parked one-wave distmod LRP12 kernels as bits (pk_dist_fast.hpp, DistPace)
enum { PK_DSCHED_OFF = 0, PK_DSCHED_LEAD_SLOT = 1, PK_DSCHED_LEVEL = 2, PK_DSCHED_LEAD_BLOCK = 4 };
constexpr int PK_DSCHED_UNSET = 0x100;           // no setting: the launch table's own choice applies (pk_dist_fast12.hpp)
constexpr const char* kDistSchedNames = "off, lead, level, lead+level";

// The policy's bits, -1 for a value that names none (null and the empty string among them).  "lead" is the rule the measured timeline
// picked, hardware wave slot 0; lead:slot and lead:block name the two rules for A/B runs
inline int dist_sched_parse(const char* v) {
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

// ---- PK_DIST_LAYOUT: any other word, or none, is no override
enum DistLayoutEnv { PK_DLAYOUT_NONE = 0, PK_DLAYOUT_8X4, PK_DLAYOUT_WG256, PK_DLAYOUT_SHADOW };
inline DistLayoutEnv dist_layout_parse(const char* v) {
  if (!v) return PK_DLAYOUT_NONE;
  return !strcmp(v, "8x4") ? PK_DLAYOUT_8X4 : !strcmp(v, "wg256") ? PK_DLAYOUT_WG256 : !strcmp(v, "shadow") ? PK_DLAYOUT_SHADOW : PK_DLAYOUT_NONE;
}

// ---- PK_ARK_PAIR has always been read by two rules that are not one predicate ("00" and "abc" separate them): both answers are kept
struct ArkPairEnv {
  bool enabled = true;       // env_unless_0: whether the dense lane layout may take a network at all
  int mode = 3;              // env_atoi, 3 when unset: which build of it runs
};
inline ArkPairEnv ark_pair_parse(const char* v) { return {env_unless_0(v), env_atoi(v, 3)}; }

struct Env {
  // -- per-protein solve: what protein_plan (pk_plan.hpp) is told through ProteinSwitches
  int wide_rand_exact = 1;             // PK_WIDE_RAND_EXACT, integer, frozen.  randmod n = 7 / 8, the tests hold the three to agreement: 1 parity elimination
                                       // (pk_rand_parity.hpp); 2 the full 128 x 128 inverse in registers at n = 7 (pk_rand_dense.hpp), block elimination over the
                                       // popcount levels at n = 8 (pk_rand_level.hpp); 0 the n-cube kernel (approximate factorisation), the path of n >= 9
  int rand_level6 = 0;                 // PK_RAND_LEVEL6, integer, frozen.  1: randmod n = 6 on the level-block kernel instead of the one-wave kernel (A/B switch of the tests)
  int rand_parity56 = -1;              // PK_RAND_PARITY56, integer, frozen.  0: randmod n = 6 stays on the in-register inverse of pk_rand_fast.hpp; 1: n = 5 goes to
                                       // the parity kernel as well (dev); anything else: n = 6 alone on the parity kernel
  int tpr = -1;                        // PK_TPR, integer, frozen.  0 / 1: never / always the thread-per-replica family where such a kernel exists (dev A/B runs;
                                       // opts->kernel does the same for callers and wins)
  int dist_sched = PK_DSCHED_UNSET;    // PK_DIST_SCHED, one of kDistSchedNames (dist_sched_parse), frozen.  -1 for any other value: the C entry points then
                                       // refuse the distmod throughput kernel by name, and a launch that gets there all the same runs unpaced
  // -- per-protein solve: what the launchers consult after the plan
  DistLayoutEnv dist_layout = PK_DLAYOUT_NONE;   // PK_DIST_LAYOUT, 8x4 | wg256 | shadow (dist_layout_parse), frozen.  dev A/B of the distmod LRP12 launch table
                                       // (pk_inst_dist_fast12.hip says what each word forces)
  bool dist_trace = false;             // PK_DIST_TRACE, env_equals_1, frozen.  dev: the benchmark's configuration runs on the traced build of its kernel
  bool rand_one_row = false;           // PK_RAND_ROWS, env_equals_1, frozen.  dev A/B: randmod n = 3, 4 keep the one-row-per-lane kernels
  bool tpr_stage = false;              // PK_TPR_STAGE, env_starts_1, frozen.  trajectories of the smallest thread-per-replica systems go through the line buffer
  int level_debug = 0;                 // PK_LEVEL_DEBUG, integer, frozen.  dev timing switches of the level-block kernel: RESULTS ARE GARBAGE when not 0
  int rand_parity8_grid = 256;         // PK_RAND_PARITY8_GRID, integer, frozen.  dev: 512 runs randmod n = 8 on the 16 x 32 thread grid, anything else on 16 x 16
  int rand_parity7_tb = 0;             // PK_RAND_PARITY7_TB, integer, frozen.  dev: 8 / 16 force one wave per replica / the 256-thread grid at randmod n = 7
  int rand_parity6_tb = 8;             // PK_RAND_PARITY6_TB, integer, frozen.  dev: 16 runs randmod n = 6 on the 256-thread grid, anything else one wave per replica
  int rand_sens6_tb = 8;               // PK_RAND_SENS6_TB, integer, frozen.  dev: 8 runs the randmod n = 6 sensitivities one wave per column chunk, anything else
                                       // on the 256-thread grid
  bool wide_rand_dense = true;         // PK_WIDE_RAND_DENSE, env_unless_0, frozen.  off: randmod n = 7 has no exact kernel and runs on the n-cube kernel (tests run both)
  bool wide_rand_drift = true;         // PK_WIDE_RAND_DRIFT, env_unless_0, frozen.  off: the n-cube kernel without its drift removal (A/B runs, tests of the plain path)
  bool wide_rand_rosw = false;         // PK_WIDE_RAND_ROSW, env_atoi_is_1, frozen.  on: the n-cube kernel integrates with ROS34PW2-W, its first version, not the order-4 additive method
  int sens_rows = 0;                   // PK_SENS_ROWS, integer, frozen.  1 / 2: the rows-per-lane sensitivity kernel at every size / at none below 15 sites (A/B switch of the tests)
  int sens_rows_min = 0;               // PK_SENS_ROWS_MIN, integer, frozen.  dev: above 0, the smallest size the rows-per-lane kernel takes by default
  // -- network path
  size_t ark_lds_pad = 0;              // PK_ARK_LDS_PAD, bytes (env_atol_size), frozen.  dev: unused LDS per workgroup of the order-4 kernel, to measure it at fewer workgroups per CU
  bool ark2_exact = true;              // PK_ARK2_EXACT, env_unless_0, frozen.  off: the approximate factorisation as the combinatorial topology's implicit operator
  ArkPairEnv ark_pair;                 // PK_ARK_PAIR, integer (ark_pair_parse), frozen.  0: one thread per protein; 1: the pair layout out of 256 registers; 3: on the register diet
  double ark_tolfac = 0.25;            // PK_ARK_TOLFAC, real in (0, 1] (env_atof_within_0_1), frozen.  dev: the factor on the tolerances of the order-4 method; outside the range 0.25
  double ark_safety = 0.0;             // PK_ARK_SAFETY, real (env_atof), frozen.  dev: safety factor of the order-4 method's step controller, 0 for its own
  double ark_grow = 0.0;               // PK_ARK_GROW, real (env_atof), frozen.  dev: growth limit of the same controller, 0 for its own
  int net_threads = 0;                 // PK_NET_THREADS, integer, LIVE.  64 / 128 / 256 threads for the general LDS kernel where the network fits them, else ignored
  int net_sens_kc = 0;                 // PK_NET_SENS_KC, integer, LIVE.  dev: tangent columns per workgroup or work item, where at least 1 and below the count in force (net_sens_kc)
};

// the two live switches of `e` from `lookup` (pk_env.hip: at every call)
template <class Lookup>
inline void env_parse_live(Env& e, Lookup&& lookup) {
  e.net_threads = env_atoi(lookup("PK_NET_THREADS"), 0);
  e.net_sens_kc = env_atoi(lookup("PK_NET_SENS_KC"), 0);
}

// lookup: const char* (const char* name), null for a variable that is not set
template <class Lookup>
inline Env env_parse(Lookup&& lookup) {
  Env e;
  e.wide_rand_exact = env_atoi(lookup("PK_WIDE_RAND_EXACT"), 1);
  e.rand_level6 = env_atoi(lookup("PK_RAND_LEVEL6"), 0);
  e.rand_parity56 = env_atoi(lookup("PK_RAND_PARITY56"), -1);
  e.tpr = env_atoi(lookup("PK_TPR"), -1);
  if (const char* v = lookup("PK_DIST_SCHED")) e.dist_sched = dist_sched_parse(v);
  e.dist_layout = dist_layout_parse(lookup("PK_DIST_LAYOUT"));
  e.dist_trace = env_equals_1(lookup("PK_DIST_TRACE"));
  e.rand_one_row = env_equals_1(lookup("PK_RAND_ROWS"));
  e.tpr_stage = env_starts_1(lookup("PK_TPR_STAGE"));
  e.level_debug = env_atoi(lookup("PK_LEVEL_DEBUG"), 0);
  e.rand_parity8_grid = env_atoi(lookup("PK_RAND_PARITY8_GRID"), 256);
  e.rand_parity7_tb = env_atoi(lookup("PK_RAND_PARITY7_TB"), 0);
  e.rand_parity6_tb = env_atoi(lookup("PK_RAND_PARITY6_TB"), 8);
  e.rand_sens6_tb = env_atoi(lookup("PK_RAND_SENS6_TB"), 8);
  e.wide_rand_dense = env_unless_0(lookup("PK_WIDE_RAND_DENSE"));
  e.wide_rand_drift = env_unless_0(lookup("PK_WIDE_RAND_DRIFT"));
  e.wide_rand_rosw = env_atoi_is_1(lookup("PK_WIDE_RAND_ROSW"));
  e.sens_rows = env_atoi(lookup("PK_SENS_ROWS"), 0);
  e.sens_rows_min = env_atoi(lookup("PK_SENS_ROWS_MIN"), 0);
  e.ark_lds_pad = env_atol_size(lookup("PK_ARK_LDS_PAD"));
  e.ark2_exact = env_unless_0(lookup("PK_ARK2_EXACT"));
  e.ark_pair = ark_pair_parse(lookup("PK_ARK_PAIR"));
  e.ark_tolfac = env_atof_within_0_1(lookup("PK_ARK_TOLFAC"), 0.25);
  e.ark_safety = env_atof(lookup("PK_ARK_SAFETY"));
  e.ark_grow = env_atof(lookup("PK_ARK_GROW"));
  env_parse_live(e, lookup);
  return e;
}

// PK_NET_SENS_KC lowers a column count, never raises it: the setting where it is at least 1 and below `cap`, else `cap`
inline int net_sens_kc(const Env& e, int cap) { return (e.net_sens_kc >= 1 && e.net_sens_kc < cap) ? e.net_sens_kc : cap; }

// pk_env.hip
const Env& env();        // the snapshot: env_parse over the process environment, made once, at the first call
Env env_live();          // the snapshot with the live switches read afresh; read net_threads and net_sens_kc from here, never from env()

}  // namespace pk
