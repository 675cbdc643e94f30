// pk_dist_rows.hpp -- the rows a lane of the distributive-model throughput kernel carries (pk_dist_fast.hpp), and everything that is
// "for every row of this lane": the vector updates of a step, the two error norms (DistNorm), the sign-bit OR and the clip of a landing.
// Each of them is written once over the lane's row list, whichever layout (shadowed or resident) the rows come from.
#pragma once
#include "pk_solve_kernel.hpp"

namespace pk {

// One vector of the system as seen by a lane: a stage, a candidate, an error estimate.
//   s[0 .. RPL)        this lane's slots, state lane + G * j.  Shadowed: site rows only.  Resident: R and P are rows like any other (slot
//                      0 and slot 1), nothing is shadowed;
//   s[RPL], s[RPL + 1] shadowed only: the shadow rows R and P (identical in every lane of the group up to rounding).
template <int RPL, bool RES = false>
struct Stg {
  static constexpr int X = RES ? 0 : 2;      // shadow rows
  static constexpr int NR = RPL + X;         // every row this lane carries
  // Position in s of the k-th operand of a reduction over the lane's rows: R, P, then the slots.  The reductions are trees (and the
  // NaN-propagating maximum a chain) over the operands in this order, so the order is part of the result.
  static constexpr int tree_row(int k) { return k < X ? RPL + k : k - X; }
  double s[NR];
  __device__ __forceinline__ double& R() { static_assert(!RES, "the resident layout has no shadow rows"); return s[RPL]; }
  __device__ __forceinline__ double& P() { static_assert(!RES, "the resident layout has no shadow rows"); return s[RPL + 1]; }
  __device__ __forceinline__ const double& R() const { static_assert(!RES, "the resident layout has no shadow rows"); return s[RPL]; }
  __device__ __forceinline__ const double& P() const { static_assert(!RES, "the resident layout has no shadow rows"); return s[RPL + 1]; }
};
template <int RPL, bool RES>
__device__ __forceinline__ void trk_axpy(Stg<RPL, RES>& acc, const double a, const Stg<RPL, RES>& u) {
#pragma unroll
  for (int j = 0; j < Stg<RPL, RES>::NR; ++j) acc.s[j] = __builtin_fma(a, u.s[j], acc.s[j]);
}
template <int RPL, bool RES>
__device__ __forceinline__ Stg<RPL, RES> trk_scale(const double a, const Stg<RPL, RES>& u) {
  Stg<RPL, RES> r;
#pragma unroll
  for (int j = 0; j < Stg<RPL, RES>::NR; ++j) r.s[j] = a * u.s[j];
  return r;
}

// The sign bits of a lane's rows, ORed: negative when some row has its sign bit set (a landing clips only then: emit in dist_fast_kernel)
template <int RPL, bool RES>
__device__ __forceinline__ int sign_or(const Stg<RPL, RES>& v) {
  using Vec = Stg<RPL, RES>;
  typedef int dwords __attribute__((ext_vector_type(2)));      // element 1 = the high dword; as a shift of the 64 bits the OR is done on both dwords
  int sgn = 0;
#pragma unroll
  for (int k = 0; k < Vec::NR; ++k) sgn |= __builtin_bit_cast(dwords, v.s[Vec::tree_row(k)]).y;
  return sgn;
}
// the literal clip x < 0 ? 0 : x of every row
template <int RPL, bool RES>
__device__ __forceinline__ void clip_rows(Stg<RPL, RES>& c) {
  using Vec = Stg<RPL, RES>;
#pragma unroll
  for (int k = 0; k < Vec::NR; ++k) { double& x = c.s[Vec::tree_row(k)]; x = (x < 0.0) ? 0.0 : x; }
}

// Max-norm helpers over the whole system: the rows of this lane, then across the group.
template <int G, int RPL, bool RES>
struct DistNorm {
  using Vec = Stg<RPL, RES>;
  const double rtol, atol;
  const int lane;
  __device__ __forceinline__ double ratio(double e, double ya, double yb) const {
    // max_abs: fmax(fabs(ya), fabs(yb)) in one v_max_f64 |ya|, |yb| (same bits, a NaN operand dropped as fmax drops it)
    return fabs(e) * approx_rcp(__builtin_fma(rtol, max_abs(ya, yb), atol));
  }
  // NaN-propagating: the initial step estimate; DistAny
  __device__ __forceinline__ double group_max(const Vec& num, const Vec& a, const Vec& b) const {
    auto mx = [](double p, double r) { return (p > r || p != p) ? p : r; };
    constexpr int i0 = Vec::tree_row(0);
    double m = ratio(num.s[i0], a.s[i0], b.s[i0]);
#pragma unroll
    for (int k = 1; k < Vec::NR; ++k) { const int i = Vec::tree_row(k); m = mx(m, ratio(num.s[i], a.s[i], b.s[i])); }
    return gmax<G>(m, lane);
  }
  // The error norm of the step loop: the ratios of group_max for the error estimate e against the accepted state y and the candidate yn,
  // their maximum with v_max_f64 (one instruction per element and per DPP level; it DROPS a NaN).  A NaN ratio (a NaN in a row's error or
  // scale, inf * 0, 0 * inf) is found by unordered compares on pairs of ratios and turned into +inf, which v_max_f64 carries through the
  // group; an inf ratio is the maximum anyway.  The loop treats +inf and NaN alike (reject, then the PK_ST_NONFINITE test), and for finite
  // ratios the maximum has the bits group_max returns.
  __device__ __forceinline__ double err_norm(const Vec& e, const Vec& y, const Vec& yn) const {
    double r[Vec::NR];
    static_for<Vec::NR>([&](auto kc) {
      constexpr int k = decltype(kc)::value, i = Vec::tree_row(k);
      r[k] = ratio(e.s[i], y.s[i], yn.s[i]);
    });
    double m = tree_max(r);
    if (any_nan(r)) m = __builtin_inf();
    return gmax_num<G>(m, lane);
  }
};

}  // namespace pk
