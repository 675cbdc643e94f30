// pk_lm.hpp -- the row algebra of the bounded Levenberg-Marquardt fit (paramest/multistart.py::fit_rows_batch) for ONE row, as code the
// kernels of pk_lm.hip and a host build share.  Plain C++ over <math.h>: device code under hipcc, host code under g++
// (tests/test_lm_rows_cpu.py).  No statics, no HIP headers in the host build.
//
// Functions that touch a whole vector or matrix take a Team: the threads that work on the row together.  A Team has tid(), size() and
// sync(); LmSerial (one thread) is the host's, the kernels pass their workgroup.  Every entry of every result is formed by ONE thread with a
// sequential sum in ascending index order, so the bits do not depend on the team's size.
//
// The damped matrix lives in a packed lower triangle stored by COLUMNS: entry (i, j), i >= j, sits at lm_tri(P, i, j) = j P - j (j - 1) / 2 +
// (i - j).  The factorisation and the forward substitution walk down a column with one row per thread: consecutive threads then read
// consecutive doubles (no LDS bank conflict), and the pivot-row entry they share is a broadcast.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define PK_LM_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PK_LM_FN inline
#endif

namespace pk {

constexpr int kLmMaxTries = 12;          // damping values tried per iteration before the row goes inactive
constexpr double kLmMu0 = 1e-3;          // first damping value of every row

struct LmSerial {
  PK_LM_FN int tid() const { return 0; }
  PK_LM_FN int size() const { return 1; }
  PK_LM_FN void sync() const {}
};

PK_LM_FN size_t lm_tri(int P, int i, int j) { return (size_t)j * (size_t)P - (size_t)j * (size_t)(j - 1) / 2 + (size_t)(i - j); }
PK_LM_FN size_t lm_tri_len(int P) { return (size_t)P * (size_t)(P + 1) / 2; }

PK_LM_FN bool lm_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }      // false for NaN and +-inf

// 4^lv, exact
PK_LM_FN double lm_pow4(int lv) { return ldexp(1.0, 2 * lv); }

// A variable on a bound whose gradient component points out of the box is fixed for this iteration.
PK_LM_FN bool lm_fixed(double p, double lb, double ub, double g) { return (p <= lb && g > 0.0) || (p >= ub && g < 0.0); }

// Marquardt scaling from the diagonal of J^T J.
PK_LM_FN double lm_scale(double aii) { return fmax(sqrt(aii), 1e-12); }

// The row is done when nothing is free or the free gradient vanishes against the cost.
PK_LM_FN bool lm_row_done(int n_free, double gfree_norm, double cost) { return n_free == 0 || gfree_norm < 1e-14 * fmax(1.0, cost); }

// Damped system of level lv: A masked to the free set plus mu 4^lv DD_i^2 on the free diagonal; a fixed variable gets an identity row and a
// zero right-hand side.  A is the full, exactly symmetric matrix (leading dimension lda; its upper triangle is read); L receives the packed lower triangle, rhs = -g on the free set.
template <class Team>
PK_LM_FN void lm_damped_system(int P, const double* A, int lda, const unsigned char* is_free, const double* DD, const double* g, double mu, int lv,
                               double* L, double* rhs, const Team& team) {
  const double mul = mu * lm_pow4(lv);
  for (int j = 0; j < P; ++j) {
    const bool fj = is_free[j] != 0;
    for (int i = j + team.tid(); i < P; i += team.size()) {
      double v = (fj && is_free[i] != 0) ? A[(size_t)j * lda + i] : 0.0;      // symmetric: entry (i, j) read from row j
      if (i == j) v = fj ? v + mul * (DD[j] * DD[j]) : 1.0;
      L[lm_tri(P, i, j)] = v;
    }
  }
  for (int i = team.tid(); i < P; i += team.size()) rhs[i] = is_free[i] != 0 ? -g[i] : 0.0;
  team.sync();
}

// In-place Cholesky L L^T of the packed lower triangle, column by column (left-looking).  false when a pivot is not finite or not positive:
// the caller takes a zero step.  Every thread returns the same answer.
template <class Team>
PK_LM_FN bool lm_factor(int P, double* L, const Team& team) {
  for (int j = 0; j < P; ++j) {
    for (int i = j + team.tid(); i < P; i += team.size()) {
      double s = L[lm_tri(P, i, j)];
      for (int k = 0; k < j; ++k) s -= L[lm_tri(P, i, k)] * L[lm_tri(P, j, k)];
      L[lm_tri(P, i, j)] = s;
    }
    team.sync();
    const double d = L[lm_tri(P, j, j)];
    if (!(d > 0.0) || !lm_finite(d)) return false;
    const double ljj = sqrt(d);
    team.sync();                                                      // everyone has read the pivot before its owner overwrites it
    for (int i = j + team.tid(); i < P; i += team.size()) L[lm_tri(P, i, j)] = i == j ? ljj : L[lm_tri(P, i, j)] / ljj;
    team.sync();
  }
  return true;
}

// Solve L L^T x = b with the factor of lm_factor; b is overwritten by x.  Non-finite entries of x become 0.
template <class Team>
PK_LM_FN void lm_solve(int P, const double* L, double* b, const Team& team) {
  for (int j = 0; j < P; ++j) {                                        // L y = b, column-oriented: b_i loses L_ij y_j in ascending j
    const double yj = b[j] / L[lm_tri(P, j, j)];
    team.sync();
    for (int i = j + team.tid(); i < P; i += team.size()) b[i] = i == j ? yj : b[i] - L[lm_tri(P, i, j)] * yj;
    team.sync();
  }
  for (int j = P - 1; j >= 0; --j) {                                   // L^T x = y: x_i loses L_ji x_j in descending j
    const double xj = b[j] / L[lm_tri(P, j, j)];
    team.sync();
    for (int i = team.tid(); i <= j; i += team.size()) b[i] = i == j ? xj : b[i] - L[lm_tri(P, j, i)] * xj;
    team.sync();
  }
  for (int i = team.tid(); i < P; i += team.size()) if (!lm_finite(b[i])) b[i] = 0.0;
  team.sync();
}

// Step of one damping level: build, factor, solve.  step = 0 when the factorisation fails; a fixed variable's entry is exactly 0.
// L holds lm_tri_len(P) doubles of work space.
template <class Team>
PK_LM_FN void lm_damped_step(int P, const double* A, int lda, const unsigned char* is_free, const double* DD, const double* g, double mu, int lv,
                             double* L, double* step, const Team& team) {
  lm_damped_system(P, A, lda, is_free, DD, g, mu, lv, L, step, team);
  const bool ok = lm_factor(P, L, team);
  if (ok) {
    lm_solve(P, L, step, team);
  } else {
    team.sync();
    for (int i = team.tid(); i < P; i += team.size()) step[i] = 0.0;
    team.sync();
  }
  for (int i = team.tid(); i < P; i += team.size()) if (is_free[i] == 0) step[i] = 0.0;
  team.sync();
}

// Trial point clip(p + step, lb, ub) and the move dp = trial - p.
template <class Team>
PK_LM_FN void lm_project(int P, const double* p, const double* lb, const double* ub, const double* step, double* trial, double* dp, const Team& team) {
  for (int i = team.tid(); i < P; i += team.size()) {
    const double x = fmin(fmax(p[i] + step[i], lb[i]), ub[i]);
    trial[i] = x;
    dp[i] = x - p[i];
  }
  team.sync();
}

// Predicted reduction -(g . dp + 1/2 dp^T A dp) with the UNMASKED A (symmetric: column i is read as row i).  work holds P doubles.
// The two sums over i run in ascending order on one thread; every thread returns the value.
template <class Team>
PK_LM_FN double lm_predicted(int P, const double* A, int lda, const double* g, const double* dp, double* work, const Team& team) {
  for (int i = team.tid(); i < P; i += team.size()) {
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += A[(size_t)j * lda + i] * dp[j];
    work[i] = s;
  }
  team.sync();
  double gd = 0.0, q = 0.0;
  for (int i = 0; i < P; ++i) { gd += g[i] * dp[i]; q += dp[i] * work[i]; }
  team.sync();
  return -(gd + 0.5 * q);
}

// Gain ratio of a trial: -1 when the model predicts no reduction.
PK_LM_FN double lm_rho(double cost, double cn, double pred) { return pred > 0.0 ? (cost - cn) / pred : -1.0; }
PK_LM_FN bool lm_acceptable(double cost, double cn, double rho) { return cn < cost && rho > 1e-4; }

// Damping after an accepted level lvl / after a round of K rejected levels.
PK_LM_FN double lm_mu_accept(double mu, int lvl, double rho) { return fmax(mu * lm_pow4(lvl) * (rho > 0.75 ? 1.0 / 3.0 : 1.0), 1e-12); }
PK_LM_FN double lm_mu_reject(double mu, int K) { return mu * lm_pow4(K); }

// Convergence of an accepted step: dc = cost - cn, dx = |dp|, xn = |trial|.
PK_LM_FN bool lm_converged(double dc, double cn, double dx, double xn, double ftol, double xtol) {
  return dc <= ftol * fmax(cn, 1e-300) || dx <= xtol * (xtol + xn);
}

// Levels of the next trial round: the caller's choice, or three while at most 256 rows pend and one beyond; never past the budget.
PK_LM_FN int lm_round_levels(int trial_levels, long long pending, int tries) {
  int K = trial_levels > 0 ? trial_levels : (pending <= 256 ? 3 : 1);
  if (K > kLmMaxTries - tries) K = kLmMaxTries - tries;
  return K;
}

}  // namespace pk
