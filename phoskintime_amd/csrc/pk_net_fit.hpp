// pk_net_fit.hpp -- the least-squares form of the network objective that pk_network_fit_batch (pk_net_fit.hip) minimises, as code the
// kernels and a host build share.  Plain C++ over <math.h>, like pk_lm.hpp whose PK_LM_FN it reuses: device code under hipcc, host code
// under g++ (tests/test_net_fit_rows_cpu.py).
//
//   cost = 1/2 sum_m obj_w[m] F_m,  F_m = sums_m norm_m lambda_m + prior          (pk_network_simulate_objective_batch, loss_mode 0)
//        = 1/2 |r|^2 + 1/2 (sum_m obj_w[m]) prior(unfitted entries)
// with the residual rows
//   observation i of modality m:   sqrt(obj_w[m] norm_m lambda_m w_i) (pred_i - obs_i)
//   fitted column c in A, B, C, D, E:   sqrt((sum_m obj_w[m]) lambda_prior / (5 N)) (p_c - d_c) / (d_c + 1e-6)
// p = softplus(x) when the fit runs on raw entries: the prior row's derivative then carries softplus'(x), exactly 1 where softplus
// returns its argument (x > 20), as the tangent launches have it.
#pragma once
#include "pk_lm.hpp"

namespace pk {

// scale of an observation's residual row; the product runs in the order the objective multiplies (sums norm lambda)
PK_LM_FN double nf_obs_scale(double obj_w, double norm, double lam, double w) { return sqrt(((obj_w * norm) * lam) * w); }

// scale of every prior row
PK_LM_FN double nf_prior_scale(const double* obj_w, double lam_prior, int N) {
  return sqrt((((obj_w[0] + obj_w[1]) + obj_w[2]) * lam_prior) / (double)(5 * N));
}

// does entry `col` of the candidate vector [c_k (n_K) | A | B | C | D (N each) | Dp (sites) | E (N) | tf_scale] carry a prior term
PK_LM_FN bool nf_prior_col(int col, int n_K, int N, int sites) {
  return (col >= n_K && col < n_K + 4 * N) || (col >= n_K + 4 * N + sites && col < n_K + 5 * N + sites);
}

PK_LM_FN double nf_softplus(double x) { return x > 20.0 ? x : log1p(exp(x)); }
PK_LM_FN double nf_softplus_prime(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

// prior row of a fitted column (p physical, d the prior centre) and its derivative with respect to the fitted entry (dsoft: softplus' of
// the raw entry, 1 in physical space)
PK_LM_FN double nf_prior_row(double scale, double p, double d) { return scale * ((p - d) / (d + 1e-6)); }
PK_LM_FN double nf_prior_drow(double scale, double d, double dsoft) { return (scale / (d + 1e-6)) * dsoft; }

// The cost the gain ratio compares: three products and two sums, each rounded once (no contraction into fused multiply-adds), so that a
// host twin forms the same bits from the same F
PK_LM_FN double nf_cost(const double* F, const double* obj_w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a = obj_w[0] * F[0], b = obj_w[1] * F[1], c = obj_w[2] * F[2];
  const double s = (a + b) + c;
  return 0.5 * s;
}

// Layout of the normal-equations kernel: the observation rows of [J | r] are K + 1 wide, and their Gram matrix's packed lower triangle (by
// columns, lm_tri with P = K + 1) holds A = J^T J in its first K rows and g = J^T r in row K; entry (K, K) = |r|^2 is not formed.
// Packed entries e = 0 .. nf_entries(K) - 1 are the ones a workgroup sums; nf_entry maps e to (i, j), i >= j.
PK_LM_FN size_t nf_entries(int K) { return lm_tri_len(K + 1) - 1; }
PK_LM_FN void nf_entry(int K, size_t e, int* i, int* j) {
  // column j starts at s_j = j (K + 1) - j (j - 1) / 2; find the last j with s_j <= e by bisection (s is increasing)
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lm_tri(K + 1, mid, mid) <= e) lo = mid; else hi = mid - 1;
  }
  *j = lo;
  *i = lo + (int)(e - lm_tri(K + 1, lo, lo));
}

}  // namespace pk
