// pk_sens_out.hpp -- the output stage of the forward-sensitivity kernels (sens_kernel in pk_sens.hpp, sens_rows_kernel in pk_sens_rows.hpp,
// rand_sens_kernel in pk_rand_sens.hpp), stated once: the three flavours of it that the argument type selects, where an observed
// (row, output time) lands in flat, how a state becomes the stored value / derivative, what an entry adds to a column's running sums and
// what the reduced sums become.  A kernel's emit is: index, post-process, the flavour's stores, accumulate; its finish reduces the sums
// its own way (registers, LDS slots) and stores sens_reduce_scalar / sens_reduce_grad of them.  The flavours therefore agree on flat,
// status and n_steps by construction.
#pragma once
#include <type_traits>
#include "pk_solve_kernel.hpp"

namespace pk {

struct SensArgs {
  SolveArgs s;
  double* dflat;        // [B, F, P]
};

// The metric flavour of the output stage (a compile-time flavour selected by the argument type, as NetScore selects the scoring flavours
// of net_rosw_solve): besides flat / dflat -- both optional here, null = not written -- the kernels return the scalar Morris output
// m = _compute_Y of the post-processed observables (s.metric [B], s.metric_id; Emitter::finish in pk_solve_kernel.hpp defines it) and its
// gradient d m / d theta (dmetric [B, P]).  The sums run over ALL observed rows i < 2 + n_sites at ALL output times, the mRNA row at
// k < 5 included, which has no slot in flat.
struct SensMetricArgs {
  SolveArgs s;
  double* dflat;        // [B, F, P] | null
  double* dmetric;      // [B, P]
};
template <class Args> constexpr bool sens_metric_flavour() { return std::is_same<Args, SensMetricArgs>::value; }

// The VJP flavour of the output stage, the third one selected by the argument type: a weighted sum over the FLAT entries and its gradient,
//   linear mode        (target null):  c_f = w_f,                            value = sum_f w_f v_f,      grad_p = sum_f c_f d_fp
//   least-squares mode (target set):   r_f = w_f (v_f - target_f), c_f = w_f r_f,  value = 1/2 sum_f r_f^2,  grad_p = sum_f c_f d_fp
// v_f = the post-processed value flat stores, d_fp = the post-processed derivative dflat would store.  The sum index is the flat index:
// the mRNA row at the first five output times has no slot and contributes nothing (the metric flavour sums it).  dflat never exists;
// s.flat is optional.  Every column forms c_f from the state value it sees (the group's published one / its chunk's own integration) and
// keeps ONE running sum over its entries in emit order; no atomics, nothing depends on the batch around a replica.
struct SensVjpArgs {
  SolveArgs s;
  const double* w;      // [F] | [B, F]
  const double* target; // [F] | [B, F] | null
  double* value;        // [B]
  double* grad;         // [B, P]
  int w_batched, target_batched;
};
template <class Args> constexpr bool sens_vjp_flavour() { return std::is_same<Args, SensVjpArgs>::value; }

// running sums a column keeps per entry: none (plain), c_f d_fp (VJP), sum r and sum w x (metric)
template <class Args> constexpr int sens_sum_count() { return sens_metric_flavour<Args>() ? 2 : sens_vjp_flavour<Args>() ? 1 : 0; }

// where the derivative rows go (the VJP flavour has no such output), and a replica's weights and targets (tg null: linear mode)
__device__ __forceinline__ double* sens_dflat(const SensArgs& a) { return a.dflat; }
__device__ __forceinline__ double* sens_dflat(const SensMetricArgs& a) { return a.dflat; }
__device__ __forceinline__ double* sens_dflat(const SensVjpArgs&) { return nullptr; }
// whether a launch writes flat / dflat at all: required by the plain flavour, optional (null = not written) in the other two
__device__ __forceinline__ bool sens_writes_flat(const SensArgs&) { return true; }
__device__ __forceinline__ bool sens_writes_flat(const SensMetricArgs& a) { return a.s.flat != nullptr; }
__device__ __forceinline__ bool sens_writes_flat(const SensVjpArgs& a) { return a.s.flat != nullptr; }
__device__ __forceinline__ bool sens_writes_dflat(const SensArgs&) { return true; }
__device__ __forceinline__ bool sens_writes_dflat(const SensMetricArgs& a) { return a.dflat != nullptr; }
__device__ __forceinline__ bool sens_writes_dflat(const SensVjpArgs&) { return false; }
// where the reduced scalar [B] and gradient [B, P] go
__device__ __forceinline__ double* sens_scalar(const SensMetricArgs& a) { return a.s.metric; }
__device__ __forceinline__ double* sens_scalar(const SensVjpArgs& a) { return a.value; }
__device__ __forceinline__ double* sens_grad(const SensMetricArgs& a) { return a.dmetric; }
__device__ __forceinline__ double* sens_grad(const SensVjpArgs& a) { return a.grad; }

struct VjpRow { const double* w; const double* tg; };
template <class Args>
__device__ __forceinline__ VjpRow vjp_row(const Args& SA, const long long rep, const int F) {
  if constexpr (sens_vjp_flavour<Args>())
    return VjpRow{SA.w + (SA.w_batched ? rep * F : 0), SA.target ? SA.target + (SA.target_batched ? rep * F : 0) : nullptr};
  else return VjpRow{nullptr, nullptr};
}
// One flat entry: returns c_f, the weight of the entry's derivative row; term = the entry's share of value (of 2 value in least-squares mode)
__device__ __forceinline__ double vjp_entry(const VjpRow& vr, const int fi, const double v, double& term) {
  const double w = vr.w[fi];
  if (!vr.tg) { term = w * v; return w; }
  const double r = w * (v - vr.tg[fi]);
  term = r * r;
  return w * r;
}

// One (row, output time) entry of the metric sums.  v: the post-processed state value, pv: the same at the previous output time, c: the
// mean of v at t0 (the shift of Emitter::emit).  Every column keeps a = sum r and b = sum w x over the entries, r being the column's
// entry (v itself in the state column, the post-processed tangent otherwise) and pr its value at the previous output time:
//   variance   w = v - c,        x = r  (v - c in the state column: b = sum (v - c)^2)
//   dynamics   w = v_k - v_k-1,  x = r_k - r_k-1  (nothing at k = 0)
//   l2_norm    w = v,            x = r
// The weight is the same for every column of a row: formed once per row and output time.
__device__ __forceinline__ double metric_weight(const int metric_id, const int k, const double v, const double pv, const double c) {
  switch (metric_id) {
    case PK_METRIC_VARIANCE: return v - c;
    case PK_METRIC_DYNAMICS: return k == 0 ? 0.0 : v - pv;
    default: return v;
  }
}
__device__ __forceinline__ void metric_acc(const int metric_id, const bool state_col, const int k, const double w, const double r, const double pr,
                                           double& a, double& b) {
  a += r;
  double x = r;
  if (metric_id == PK_METRIC_DYNAMICS) x = k == 0 ? 0.0 : r - pr;
  else if (metric_id == PK_METRIC_VARIANCE && state_col) x = w;
  b = __builtin_fma(w, x, b);
}
// m from the state column's sums (L = T (2 + n_sites) entries), and d m / d theta_p from a tangent column's (a0 = the state column's sum v)
__device__ __forceinline__ double metric_value(const int metric_id, const double a, const double b, const double c, const double L) {
  switch (metric_id) {
    case PK_METRIC_TOTAL_SIGNAL: return a;
    case PK_METRIC_MEAN_ACTIVITY: return a / L;
    case PK_METRIC_VARIANCE: { const double ms = a / L - c; return b / L - ms * ms; }      // E[(v-c)^2] - (E[v-c])^2
    case PK_METRIC_DYNAMICS: return b;
    default: return sqrt(b);
  }
}
__device__ __forceinline__ double metric_grad(const int metric_id, const double a, const double b, const double a0, const double m, const double c,
                                              const double L) {
  switch (metric_id) {
    case PK_METRIC_TOTAL_SIGNAL: return a;
    case PK_METRIC_MEAN_ACTIVITY: return a / L;
    case PK_METRIC_VARIANCE: return (2.0 / L) * __builtin_fma(-(a0 / L - c), a, b);        // (2/L) sum (v - mean) d, from the shifted sums
    case PK_METRIC_DYNAMICS: return 2.0 * b;
    default: return m == 0.0 ? 0.0 : b / m;
  }
}

// ---- index: where observed row `row` (0 = R, 1 = P, 2 + j = site / level / mask j) at output time k sits in flat = [R(t5 ..), P(t0 ..),
// site 0 (t0 ..), ...], T5 = max(T - 5, 0); -1 where there is no slot: the mRNA row is observed from the sixth output time on, its first
// five are empty (the metric flavour still sums them, the VJP flavour does not)
__device__ __forceinline__ int sens_flat_index(const int row, const int k, const int T, const int T5) {
  return (row == 0) ? (k >= 5 ? k - 5 : -1) : (row == 1 ? T5 + k : T5 + T + (row - 2) * T + k);
}

// ---- post-processing: the stored state value from the raw state ys of its row, and the stored entry of a column from ys and the column's
// raw value yc (the state column: yc = ys; a tangent column: d ys / d theta_p).  sc = 1 / y0 of the row when `normalize` is set, else 1;
// after a failure everything is NaN.
// The value is clipped below 0; its derivative is dropped only where the state is negative beyond the absolute tolerance: a state that
// has decayed to +-1e-24 (a rate on the bound 0) is not known to be negative, and its row is what moves the rate off the bound
__device__ __forceinline__ double sens_post_entry(const SolveArgs& A, const double ys, const double yc, const double sc, const bool state_col,
                                                  const bool nan_fill) {
  const bool clipped = A.clip && (ys < (state_col ? 0.0 : -A.atol));
  return nan_fill ? __builtin_nan("") : (clipped ? 0.0 : yc * sc);
}
__device__ __forceinline__ double sens_post_value(const SolveArgs& A, const double ys, const double sc, const bool nan_fill) {
  return sens_post_entry(A, ys, ys, sc, true, nan_fill);
}

// ---- accumulation, in two steps (a lane of the rows kernel carries several columns of one row): what the row of an entry gives every
// column, formed once per row and output time, and the fold of one column's entry into the column's running sums a, b (where they live
// is the kernel's business).  fi = the flat index, k = the output time, v = the post-processed state value of the row, r = the column's
// entry (v in the state column), pv / pr = the same two at the previous output time (read by PK_METRIC_DYNAMICS alone), shift = the
// metric flavour's mean at t0.
//   plain:  nothing
//   VJP:    w = c_f, term = the value term (vjp_entry); a += term (state column) or c_f r (tangent column).  The flat index is the sum
//           index: emit skips the entries without a slot (fi < 0) before it comes here
//   metric: w = metric_weight; a += r, b += w x (metric_acc)
struct SensRowTerm { double w, term; };
template <class Args>
__device__ __forceinline__ SensRowTerm sens_row_term(const Args& SA, const VjpRow& vr, const int fi, const int k, const double v, const double pv,
                                                     const double shift) {
  if constexpr (sens_vjp_flavour<Args>()) {
    double term;
    const double cf = vjp_entry(vr, fi, v, term);
    return SensRowTerm{cf, term};
  } else if constexpr (sens_metric_flavour<Args>()) {
    return SensRowTerm{metric_weight(SA.s.metric_id, k, v, pv, shift), 0.0};
  } else {
    return SensRowTerm{0.0, 0.0};
  }
}
template <class Args>
__device__ __forceinline__ void sens_accumulate(const Args& SA, const SensRowTerm& rt, const int k, const double r, const bool state_col,
                                                const double pr, double& a, double& b) {
  if constexpr (sens_vjp_flavour<Args>()) a = state_col ? a + rt.term : __builtin_fma(rt.w, r, a);
  else if constexpr (sens_metric_flavour<Args>()) metric_acc(SA.s.metric_id, state_col, k, rt.w, r, pr, a, b);
}

// ---- reduction: what finish stores from the reduced sums.  The state column's (a0, b0) give the scalar -- value / metric; a column's
// (a, b), with a0 and the scalar m, its entry of grad / dmetric.  L = T (2 + n_sites), the number of summed entries
template <class Args>
__device__ __forceinline__ double sens_reduce_scalar(const Args& SA, const VjpRow& vr, const double a0, const double b0, const double shift,
                                                     const double L) {
  if constexpr (sens_vjp_flavour<Args>()) return vr.tg ? 0.5 * a0 : a0;      // least-squares mode: 1/2 sum r^2
  else return metric_value(SA.s.metric_id, a0, b0, shift, L);
}
template <class Args>
__device__ __forceinline__ double sens_reduce_grad(const Args& SA, const double a, const double b, const double a0, const double m, const double shift,
                                                   const double L) {
  if constexpr (sens_vjp_flavour<Args>()) return a;
  else return metric_grad(SA.s.metric_id, a, b, a0, m, shift, L);
}

}  // namespace pk
