// pk_network_solve.hpp -- batched integration of the network ODE: replaces global_model.simulate.simulate_odeint
// (simulate.py:34-80: odeint(rhs_odeint, y0, t, Dfun = fd_jacobian_odeint, rtol, atol, mxstep)) for B candidates.
//
// One workgroup per candidate; state, stage vectors and per-block factors in LDS (net_solve_kernel) or, for networks of any size, in a
// slab of an HBM workspace (net_solve_ws_kernel).  Both kernels run the same body, net_rosw_solve, on two layouts of the thread's work.
//
// Integrator: ROS34PW2 (Rang & Angermann 2005), a 4-stage, order-3, stiffly accurate, L-stable Rosenbrock-W method --
// its order conditions hold for ANY approximation of the Jacobian (table verified in 50-digit arithmetic,
// tools/check_ros34pw2.py).  That licence is used to keep only the per-protein diagonal blocks of J in the linear
// systems (arrow blocks for the distributive / saturating topologies, tridiagonal blocks for the sequential one): all
// stiffness of this system lives inside those blocks (phosphorylation / de-phosphorylation / decay), while the coupling
// between proteins -- transcription-factor input to the mRNA rows -- is slow and bounded; the numpy model
// (tools/proto_rosw_network.py) shows identical step counts with the full and the block-diagonal Jacobian.  So a "linear
// solve" is N independent tiny block solves (one thread per protein) instead of an S x S factorisation
// (the reference hands LSODA a dense finite-difference Jacobian: S + 1 right-hand sides per refresh).
//
// The kinase forcing is piecewise constant (jacspeedup.py:149-172): a step never straddles a bucket edge (every edge is a
// forced landing point) and uses the bucket of its START time throughout, so each step sees an autonomous system.
#pragma once
#include "pk_network.hpp"
#include "pk_step.hpp"
#include "../../include/phoskin.h"

namespace pk {

namespace rosw {
constexpr double GAM = 0.435866521508459;
constexpr double A21 = 2.0, A31 = 1.41921731745576465, A32 = -0.25923221167296971378;
constexpr double A41 = 4.1847604823191607312, A42 = -0.2851920173554959137, A43 = 2.2942803602790417167;
constexpr double C21 = -4.5885607205580834861, C31 = -4.1847604823191607312, C32 = 0.2851920173554959137;
constexpr double C41 = -6.3681792001283577635, C42 = -6.7956209444668361844, C43 = 2.8700986043310560892;
// y1 = Y4 + U4 (stiffly accurate: m = (A41, A42, A43, 1)); error estimate = sum E_i U_i
constexpr double E1 = 0.27774994764796811038, E2 = -1.4032398951759990242, E3 = 1.7726301276675507452, E4 = 0.5;
__device__ constexpr double TA[4][3] = {{0, 0, 0}, {A21, 0, 0}, {A31, A32, 0}, {A41, A42, A43}};
__device__ constexpr double TC[4][3] = {{0, 0, 0}, {C21, 0, 0}, {C31, C32, 0}, {C41, C42, C43}};
}  // namespace rosw

struct NetSolveArgs {
  const double* x; int x_is_raw;
  const double* y0; int y0_batched;
  // landing times (output times + kinase-bucket edges) and the output row each one fills (-1: none); passed by value when short
  double stops_v[64]; int32_t stop_out_v[64];
  const double* stops_p; const int32_t* stop_out_p; int n_stops;
  double t0; int T;
  double* Y;                       // [B, T, S]
  int32_t* status; int32_t* n_steps;
  double rtol, atol, h0; int max_steps;
  double ctl_safety, ctl_grow;     // step-size controller of the additive kernels: h_new = h * min(ctl_grow, ctl_safety / err^(1/4)) (0: defaults 0.9, 6)
  int err_rms;                     // 1: ODEPACK's weighted root-mean-square error norm (what the reference's LSODA controls); 0: max norm
  // fused objective (pk_network_simulate_objective_batch; the pair kernel on the register diet): dense observation tables [T, S] of the
  // loss handle, read at every output time; the trajectory itself is written only if Y != null.  loss_obs == null: plain simulate
  const double* loss_obs; const double* loss_w; const double* loss_defaults;
  double loss_lam[4], loss_norm[3], loss_fail; int loss_mode, loss_rna_base;
  double* loss_sums; double* loss_F;
  // fused objective of the order-3 kernels (net_rosw_solve<.., SCORE_LOSS>): the loss handle's observation lists bucketed by time index
  // instead of the dense tables.  One set of arrays (protein | rna | phospho, each sorted by time index); modality m's observations of
  // output row t are entries loss_ptr[m (T + 1) + t] .. loss_ptr[m (T + 1) + t + 1].  loss_site: phospho entries only
  const int32_t* loss_ptr; const int32_t* loss_prot; const int32_t* loss_site; const double* loss_lobs; const double* loss_lw;
  // fused measurement of the order-3 kernels (net_rosw_solve<.., SCORE_MEASURE>, pk_network_simulate_measure_batch): the same bucketed lists
  // (loss_ptr / loss_prot / loss_site; loss_rna_base), observations and weights unused.  meas_perm: bucketed entry -> its position in the
  // caller's (protein | rna | phospho) lists; meas_pred [B, meas_n] and meas_metric [B] are optional; meas_id: PK_NET_METRIC_*
  int meas; int meas_id; int meas_n; double meas_eps;
  const int32_t* meas_perm; double* meas_pred; double* meas_metric;
};

// What the order-3 body does with an output row besides storing it: nothing, the three-objective loss, or the scalar Morris metric
enum NetScore : int { SCORE_NONE = 0, SCORE_LOSS = 1, SCORE_MEASURE = 2 };

// block-wide NaN-propagating max; `red` holds >= 17 doubles of LDS
__device__ __forceinline__ double block_max(double v, double* red) {
  auto mx = [](double a, double b) { return (a > b || a != a) ? a : b; };
  for (int off = 32; off > 0; off >>= 1) v = mx(v, __shfl_xor(v, off));
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double r = red[0];
  for (int i = 1; i < nw; ++i) r = mx(r, red[i]);
  return r;
}

// block-wide sum (NaN / inf propagate by themselves); `red` holds >= 17 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double r = red[0];
  for (int i = 1; i < nw; ++i) r += red[i];
  return r;
}
// local error of a step from the per-thread partial value `e`: max over all states, or sqrt(mean of squares) (ODEPACK vnorm)
__device__ __forceinline__ double err_reduce(double e, const bool rms, const int S, double* red) {
  return rms ? sqrt(block_sum(e, red) / S) : block_max(e, red);
}
__device__ __forceinline__ double err_acc(double a, double q, const bool rms) {
  return rms ? __builtin_fma(q, q, a) : ((q > a || q != q) ? q : a);
}

// Chan's pairwise merge of two Welford triples (count, mean, M2): (n, m, q) <- (n, m, q) + (nb, mb, qb).  Two empty sides stay empty
__device__ __forceinline__ void welford_merge(double& n, double& m, double& q, const double nb, const double mb, const double qb) {
  const double nn = n + nb, d = mb - m;
  const double r = nn > 0.0 ? nb / nn : 0.0;
  q = q + qb + d * d * n * r;
  m = m + d * r;
  n = nn;
}
// block-wide merge of per-thread Welford triples in a fixed order: a butterfly within the wave (the lower lane's triple is always the
// left operand, so every lane of a wave ends with the same bits), then the waves in increasing order through `red` (>= 12 doubles)
__device__ __forceinline__ void block_welford(double& n, double& m, double& q, double* red) {
  for (int off = 1; off < 64; off <<= 1) {
    const double nb = __shfl_xor(n, off), mb = __shfl_xor(m, off), qb = __shfl_xor(q, off);
    if (threadIdx.x & off) { double n2 = nb, m2 = mb, q2 = qb; welford_merge(n2, m2, q2, n, m, q); n = n2; m = m2; q = q2; }
    else welford_merge(n, m, q, nb, mb, qb);
  }
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[3 * w] = n; red[3 * w + 1] = m; red[3 * w + 2] = q; }
  __syncthreads();
  n = red[0]; m = red[1]; q = red[2];
  for (int i = 1; i < nw; ++i) welford_merge(n, m, q, red[3 * i], red[3 * i + 1], red[3 * i + 2]);
}

// Per-candidate work area of the integrator: NetLds, then [Ys | U1..U4 | R | winv] (S each) and [sinv | cR | gP] (N each)
__host__ __device__ inline size_t net_rosw_doubles(const NetDev& n) { return NetLds::doubles(n) + 7 * (size_t)n.S + 3 * (size_t)n.N; }

// Where a thread finds the states and proteins it owns, and the TF CSR -- all that differs between the LDS and the workspace kernel.
//   states(f): f(k, i, loc, st, ss, ns) for each state k of this thread (protein, position in its block, block start, site offset, sites)
//   prots(f):  f(i, st, ss, ns, drv) for each protein i of this thread (block start, site offset, sites, driver_map entry)
// Both visit k / i = tid, tid + nt, ... in increasing order.
//
// LDS kernel: up to KS states and KP proteins per thread, their contexts in registers (host guarantees S <= KS*nt, N <= KP*nt); TF CSR
// cached in LDS by the kernel
struct NetRegLayout {
  static constexpr int KS = 4, KP = 2;
  const double *tf_dat, *tf_deg; const int32_t *tf_ptr, *tf_idx;
  int S, N;
  int s_i[KS], s_loc[KS], s_st[KS], s_ss[KS], s_ns[KS];
  int p_st[KP], p_ss[KP], p_ns[KP], p_drv[KP];
  __device__ __forceinline__ NetRegLayout(const NetDev& n, const double* dat, const double* deg, const int32_t* ptr, const int32_t* idx)
      : tf_dat(dat), tf_deg(deg), tf_ptr(ptr), tf_idx(idx), S(n.S), N(n.N) {
    const int tid = threadIdx.x, nt = blockDim.x;
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int k = tid + q * nt;
      if (k < S) { const int i = n.state_prot[k]; s_i[q] = i; s_loc[q] = n.state_local[k]; s_st[q] = n.offset_y[i]; s_ss[q] = n.offset_s[i]; s_ns[q] = n.n_sites[i]; }
      else { s_i[q] = 0; s_loc[q] = 0; s_st[q] = 0; s_ss[q] = 0; s_ns[q] = 0; }
    }
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      const int i = tid + q * nt;
      if (i < N) { p_st[q] = n.offset_y[i]; p_ss[q] = n.offset_s[i]; p_ns[q] = n.n_sites[i]; p_drv[q] = n.driver_map[i]; }
      else { p_st[q] = 0; p_ss[q] = 0; p_ns[q] = 0; p_drv[q] = -1; }
    }
  }
  template <class F> __device__ __forceinline__ void states(F&& f) const {
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      const int k = threadIdx.x + q * blockDim.x;
      if (k >= S) break;
      f(k, s_i[q], s_loc[q], s_st[q], s_ss[q], s_ns[q]);
    }
  }
  template <class F> __device__ __forceinline__ void prots(F&& f) const {
#pragma unroll
    for (int q = 0; q < KP; ++q) {
      const int i = threadIdx.x + q * blockDim.x;
      if (i >= N) break;
      f(i, p_st[q], p_ss[q], p_ns[q], p_drv[q]);
    }
  }
};

// workspace kernel: every thread strides over states and proteins (no register contexts, hence no ceiling); topology read from global
struct NetWsLayout {
  const NetDev& n;
  const double *tf_dat, *tf_deg; const int32_t *tf_ptr, *tf_idx;
  __device__ __forceinline__ explicit NetWsLayout(const NetDev& n_)
      : n(n_), tf_dat(n_.TF_data), tf_deg(n_.tf_deg), tf_ptr(n_.TF_indptr), tf_idx(n_.TF_indices) {}
  template <class F> __device__ __forceinline__ void states(F&& f) const {
    for (int k = threadIdx.x; k < n.S; k += blockDim.x) {
      const int i = n.state_prot[k];
      f(k, i, n.state_local[k], n.offset_y[i], n.offset_s[i], n.n_sites[i]);
    }
  }
  template <class F> __device__ __forceinline__ void prots(F&& f) const {
    for (int i = threadIdx.x; i < n.N; i += blockDim.x) f(i, n.offset_y[i], n.offset_s[i], n.n_sites[i], n.driver_map[i]);
  }
};

// ROS34PW2-W of candidate b, from loading x and y0 to the status / n_steps write.  L: the candidate's NetLds; base: its stage vectors
// (net_rosw_doubles - NetLds::doubles of them); red: >= 24 doubles of LDS for the reductions.
//
// SCORE_LOSS: the candidate is scored as it integrates (pk_network_simulate_objective_batch on request of the order-3 method): at the initial
// row and after every landing that fills an output row, the observations of that time index (A.loss_ptr ...) are scored from y -- what
// net_objective_kernel (pk_network_loss.hip) computes from a stored trajectory, into three per-thread partial sums.  Baselines: y0 for
// protein / phospho (time index 0); the mRNA values at output row A.loss_rna_base, kept in rbase (N doubles) from the landing that
// produces them (no rna observation is earlier: the host checks).  The trajectory is written only if A.Y != null.  The plain
// instantiation has none of this: its A.Y is never null and rbase is unused.
//
// SCORE_MEASURE: the same walk over the same buckets, but each entry's fold change is the measurement itself
// (pk_network_simulate_measure_batch): formed as net_observables_kernel forms it from a stored trajectory -- same sums in the same order,
// floor A.meas_eps --, stored at meas_pred[b, meas_perm[k]] when asked for, and folded into the per-thread partial of metric A.meas_id: a
// sum (total signal, mean), a sum of squares (L2 norm) or a Welford triple (variance; never E[p^2] - E[p]^2: fold changes run from 0.2
// to several thousand).  The partials are merged in a fixed order (block_sum / block_welford), so a candidate's value does not depend
// on the batch it shares a launch with.  A flagged candidate gets metric = NaN and an all-NaN pred row.
template <int MODEL, NetScore SCORE, class Layout>
__device__ __forceinline__ void net_rosw_solve(const NetDev& n, const NetSolveArgs& A, const Layout& lay, const long long b, NetLds L,
                                               double* const base, double* const red, double* const rbase = nullptr) {
  using namespace rosw;
  constexpr int model = MODEL;
  const int S = n.S, N = n.N;
  double* y = L.y;                        // current state
  double* Ys = base;                      // stage point
  double* U1 = Ys + S; double* U2 = U1 + S; double* U3 = U2 + S; double* U4 = U3 + S;
  double* R_ = U4 + S;                    // right-hand side of the stage system
  double* winv = R_ + S;                  // per state: 1 / pivot of its row in the block factorisation
  double* sinv = winv + S;                // per protein: 1 / Schur pivot of the P row (arrow blocks)
  double* cR = sinv + N;                  // per protein: d f_P / d R
  double* gP = cR + N;                    // per protein: saturating-kinetics factor 1 / (1 + P)^2 (1 otherwise)
  const double* __restrict__ tf_dat = lay.tf_dat;
  const double* __restrict__ tf_deg = lay.tf_deg;
  const int32_t* __restrict__ tf_ptr = lay.tf_ptr;
  const int32_t* __restrict__ tf_idx = lay.tf_idx;
  const NetSlices sl(n.n_K, N, n.sites);
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* stops = A.stops_p ? A.stops_p : A.stops_v;
  const int32_t* stop_out = A.stop_out_p ? A.stop_out_p : A.stop_out_v;

  const double* xb = A.x + b * n.n_var;
  for (int k = tid; k < n.n_var; k += nt) L.p[k] = A.x_is_raw ? softplus(xb[k]) : xb[k];
  const double* y0 = A.y0 + (A.y0_batched ? b * S : 0);
  constexpr bool FUSED = SCORE == SCORE_LOSS, MEASURE = SCORE == SCORE_MEASURE;
  const bool wY = SCORE == SCORE_NONE || A.Y != nullptr;
  double* Yout = wY ? A.Y + b * (size_t)A.T * S : nullptr;
  for (int k = tid; k < S; k += nt) { const double v = y0[k]; y[k] = v; if (wY) Yout[k] = v; }
  __syncthreads();

  // ---- fused objective / measurement: score output row `row`, which y holds (a barrier lies behind its last write, and none of y changes
  // before the next one).  Partial sums, the Welford triple and the non-finite flag are per thread and per candidate
  double lacc[3] = {0.0, 0.0, 0.0};
  bool ybad = false;
  double wn = 0.0, wm = 0.0, wq = 0.0;      // MEASURE: (count, mean, M2) of the variance; wm alone is the sum / the sum of squares otherwise
  double* const predb = (MEASURE && A.meas_pred) ? A.meas_pred + b * (size_t)A.meas_n : nullptr;
  // entry k of modality m with numerator a and baseline c: one term of the loss, or one measured fold change
  auto entry = [&](const int m, const int k, const double a, const double c) {
    if constexpr (FUSED) {
      const double obs = A.loss_lobs[k], pred = fold_change(a, c);
      lacc[m] += A.loss_lw[k] * point_loss(A.loss_mode, obs - pred, obs, pred);
    } else if constexpr (MEASURE) {
      const double eps = A.meas_eps;
      const double p = (a > eps ? a : eps) / (c > eps ? c : eps);
      if (predb) predb[A.meas_perm[k]] = p;
      if (A.meas_id == PK_NET_METRIC_VARIANCE) { wn += 1.0; const double d = p - wm; wm += d / wn; wq += d * (p - wm); }
      else if (A.meas_id == PK_NET_METRIC_L2_NORM) wm += p * p;
      else wm += p;
    }
  };
  auto score_row = [&](const int row) {
    if constexpr (SCORE != SCORE_NONE) {
      if constexpr (FUSED) for (int k = tid; k < S; k += nt) if (nonfinite(y[k])) ybad = true;   // np.all(np.isfinite(Y)) of the reference (optproblem.py:130)
      if (row == A.loss_rna_base) {
        for (int i = tid; i < N; i += nt) rbase[i] = y[n.offset_y[i]];
        __syncthreads();
      }
      const int32_t* ptr = A.loss_ptr + row;
      const int T1 = A.T + 1;
      for (int k = ptr[0] + tid; k < ptr[1]; k += nt) {                            // protein: P plus all sites / all 2^ns states
        const int i = A.loss_prot[k], st = n.offset_y[i];
        const int cnt = (model == 2) ? (1 << n.n_sites[i]) : 1 + n.n_sites[i];
        double tt = 0.0, tb = 0.0;
        for (int m = 0; m < cnt; ++m) { tt += y[st + 1 + m]; tb += y0[st + 1 + m]; }
        entry(0, k, tt, tb);
      }
      for (int k = ptr[T1] + tid; k < ptr[T1 + 1]; k += nt) {                      // rna: the mRNA row against the kept baseline
        const int i = A.loss_prot[k];
        entry(1, k, y[n.offset_y[i]], rbase[i]);
      }
      for (int k = ptr[2 * T1] + tid; k < ptr[2 * T1 + 1]; k += nt) {              // phospho: site row / all masks with the site's bit
        const int i = A.loss_prot[k], st = n.offset_y[i], j = A.loss_site[k];
        double a, c;
        if (model == 2) {
          a = 0.0; c = 0.0;
          const int cnt = 1 << n.n_sites[i];
          for (int m = 0; m < cnt; ++m) if (m & (1 << j)) { a += y[st + 1 + m]; c += y0[st + 1 + m]; }
        } else { a = y[st + 2 + j]; c = y0[st + 2 + j]; }
        entry(2, k, a, c);
      }
    }
  };
  score_row(0);

  // ---- block factorisation of  g I - J_blockdiag(y)  and block solve  x <- W^{-1} r  (in place: r -> x), one thread per protein
  auto factor = [&](const double g) {
    lay.prots([&](const int i, const int st, const int ss, const int ns, const int) {
      const double Bi = L.p[sl.B + i], Ci = L.p[sl.C + i], Di = L.p[sl.D + i], Ei = L.p[sl.E + i];
      const double* Dp = L.p + sl.Dp + ss;
      const double* Sr = L.Sall + ss;
      winv[st] = 1.0 / (g + Bi);
      if (model == 2) {
        // combinatorial block of any size (2^ns bit-pattern states): -diag(loss) + F (phosphorylation, strictly lower in mask order) +
        // K (dephosphorylation, strictly upper).  W-method licence once more: g I - J_block ~= (D_g - F) D_g^-1 (D_g - K), so only the
        // pivots 1 / (g + loss_m) are stored; the two sweeps run in block_solve (same scheme as pk_network_solve_reg2.hpp, any ns)
        cR[i] = Ci; gP[i] = 1.0;
        const int nst = 1 << ns;
        for (int m = 0; m < nst; ++m) {
          double loss = (m == 0) ? Di : 0.0;
          for (int j = 0; j < ns; ++j) loss += ((m >> j) & 1) ? (Ei + Dp[j] + Di) : Sr[j];
          winv[st + 1 + m] = 1.0 / (g + loss);
        }
      } else if (model == 1) {
        // tridiagonal over P0, P1..Pns: Thomas pivots
        cR[i] = Ci; gP[i] = 1.0;
        double d = g + Di + (ns ? Sr[0] : 0.0);
        winv[st + 1] = 1.0 / d;
        for (int q = 1; q <= ns; ++q) {
          const int j = q - 1;
          const double diag = g + Ei + Dp[j] + Di + ((j < ns - 1) ? Sr[j + 1] : 0.0);
          d = diag - (Sr[j] * Ei) * winv[st + q];        // lower entry -k_j, upper entry of the row above -E
          winv[st + 1 + q] = 1.0 / d;
        }
      } else {
        const bool sat = model == 4;
        const double Rv = y[st], Pv = y[st + 1];
        const double g_p = sat ? 1.0 / ((1.0 + Pv) * (1.0 + Pv)) : 1.0;
        cR[i] = sat ? Ci / ((1.0 + Rv) * (1.0 + Rv)) : Ci;
        gP[i] = g_p;
        double sumS = 0.0, acc = 0.0;
        for (int j = 0; j < ns; ++j) {
          const double wj = 1.0 / (g + Ei + Dp[j] + Di);
          winv[st + 2 + j] = wj;
          sumS += Sr[j];
          acc += Ei * (Sr[j] * g_p) * wj;
        }
        sinv[i] = 1.0 / (g + Di + sumS * g_p - acc);
      }
    });
    __syncthreads();
  };
  auto block_solve = [&](const double* r, double* x) {
    lay.prots([&](const int i, const int st, const int ss, const int ns, const int) {
      const double Ei = L.p[sl.E + i];
      const double* Sr = L.Sall + ss;
      const double xR = r[st] * winv[st];
      x[st] = xR;
      if (model == 2) {
        const int nst = 1 << ns;
        for (int m = 0; m < nst; ++m) {                              // (D_g - F) u = r : ascending masks
          double a = r[st + 1 + m] + ((m == 0) ? cR[i] * xR : 0.0);
          for (int mm = m; mm; mm &= mm - 1) { const int bit = mm & -mm; a = __builtin_fma(Sr[__builtin_ctz(bit)], x[st + 1 + (m ^ bit)], a); }
          x[st + 1 + m] = a * winv[st + 1 + m];
        }
        for (int m = nst - 2; m >= 0; --m) {                         // (D_g - K) x = D_g u : descending masks
          double hi = 0.0;
          for (int mm = ~m & (nst - 1); mm; mm &= mm - 1) hi += x[st + 1 + (m | (mm & -mm))];
          x[st + 1 + m] = __builtin_fma(Ei * hi, winv[st + 1 + m], x[st + 1 + m]);
        }
      } else if (model == 1) {
        // Thomas: forward sweep (lower entries -k_{q-1}), back substitution (upper entries -E); x doubles as work space
        double prev = r[st + 1] + cR[i] * xR;
        x[st + 1] = prev;
        for (int q = 1; q <= ns; ++q) { prev = r[st + 1 + q] + Sr[q - 1] * prev * winv[st + q]; x[st + 1 + q] = prev; }
        double xn = x[st + 1 + ns] * winv[st + 1 + ns];
        x[st + 1 + ns] = xn;
        for (int q = ns - 1; q >= 0; --q) { xn = (x[st + 1 + q] + Ei * xn) * winv[st + 1 + q]; x[st + 1 + q] = xn; }
      } else {
        const double g_p = gP[i];
        double acc = 0.0;
        for (int j = 0; j < ns; ++j) { const double t = r[st + 2 + j] * winv[st + 2 + j]; x[st + 2 + j] = t; acc += Ei * t; }
        const double xP = (r[st + 1] + cR[i] * xR + acc) * sinv[i];
        x[st + 1] = xP;
        for (int j = 0; j < ns; ++j) x[st + 2 + j] += (Sr[j] * g_p) * winv[st + 2 + j] * xP;
      }
    });
    __syncthreads();
  };
  // P_vec -> TF input -> synthesis rate for the state L.y points at (net_prepare_state with the layout's topology)
  auto prepare_state = [&]() {
    lay.prots([&](const int i, const int st, const int, const int ns, const int drv) {
      double tot;
      if (model != 2 && drv >= 0) tot = L.Kt[drv];                  // the combinatorial RHS ignores driver_map (jacspeedup.py:319-327)
      else { tot = 0.0; const int cnt = (model == 2) ? (1 << ns) : 1 + ns; for (int m_ = 0; m_ < cnt; ++m_) tot += L.y[st + 1 + m_]; }
      L.Pvec[i] = tot;
    });
    __syncthreads();
    const double ts = L.p[sl.tf];
    lay.prots([&](const int i, const int, const int, const int, const int) {
      double acc = 0.0;
      for (int e_ = tf_ptr[i]; e_ < tf_ptr[i + 1]; ++e_) acc += tf_dat[e_] * L.Pvec[tf_idx[e_]];
      double v = acc / tf_deg[i];
      if (model != 4) v = v / (1.0 + fabs(v));
      L.synth[i] = synth_rate(L.p[sl.A + i], ts, v, nullptr);
    });
    __syncthreads();
  };
  int status = PK_ST_OK, nacc = 0, nrej = 0;
  double tc = A.t0;
  int jb = net_bucket(tc, n.kin_grid, n.n_grid);
  net_prepare_bucket(n, L, jb);
  double h;
  {
    // first step from the max-norm of y / sc and f / sc
    L.y = y;
    prepare_state();
    double d0 = 0.0, d1 = 0.0;
    for (int k = tid; k < S; k += nt) {
      const double sc = A.atol + A.rtol * fabs(y[k]);
      d0 = fmax(d0, fabs(y[k]) / sc); d1 = fmax(d1, fabs(net_state_rhs(n, L, k)) / sc);
    }
    d0 = block_max(d0, red); d1 = block_max(d1, red);
    // step_h0 of pk_step.hpp, written out: the call changes register allocation and spill counts in these kernels
    h = (d0 > 1e-5 && d1 > 1e-5) ? 0.01 * d0 / d1 : 1e-6;
    if (A.h0 > 0.0) h = A.h0;
    if (!(h > 0.0) || h != h) h = 1e-6;
  }
  bool after_reject = false;
  for (int si = 0; si < A.n_stops && status == PK_ST_OK; ++si) {
    const double te = stops[si];
    while (true) {
      if (nacc + nrej >= A.max_steps) { status |= PK_ST_MAXSTEPS; break; }
      const bool last = (tc + 1.0001 * h >= te);
      const double hs = last ? te - tc : ((tc + 2.0 * h > te) ? 0.5 * (te - tc) : h);
      if (!(hs > 1e-14 * fmax(fabs(tc), 1e-3))) { status |= PK_ST_HMIN; break; }
      const double hinv = 1.0 / hs;
      factor(hinv * (1.0 / GAM));
      // four stages, one loop body (kept rolled: the body is large and register-hungry when replicated); stage j's vector is U1 + j S
#pragma unroll 1
      for (int sg = 0; sg < 4; ++sg) {
        if (sg > 0) {
          for (int k = tid; k < S; k += nt) {
            double v = y[k];
            for (int j = 0; j < sg; ++j) v = __builtin_fma(TA[sg][j], U1[(size_t)j * S + k], v);
            Ys[k] = v;
          }
          __syncthreads();
        }
        L.y = (sg == 0) ? y : Ys;
        prepare_state();
        lay.states([&](const int k, const int i, const int loc, const int st, const int ss, const int ns) {
          double v = net_state_rhs_ctx<MODEL>(n, L, i, loc, st, ss, ns);
          for (int j = 0; j < sg; ++j) v = __builtin_fma(TC[sg][j] * hinv, U1[(size_t)j * S + k], v);
          R_[k] = v;
        });
        __syncthreads();
        block_solve(R_, U1 + (size_t)sg * S);
      }
      // y1 = Ys + U4 ; err
      double e = 0.0;
      for (int k = tid; k < S; k += nt) {
        const double yn = Ys[k] + U4[k];
        const double ev = E1 * U1[k] + E2 * U2[k] + E3 * U3[k] + E4 * U4[k];
        const double q = fabs(ev) / (A.atol + A.rtol * fmax(fabs(y[k]), fabs(yn)));
        e = err_acc(e, q, A.err_rms);
        R_[k] = yn;
      }
      const double err = err_reduce(e, A.err_rms, S, red);
      if (err != err || err > 1e300) {
        ++nrej; after_reject = true; h = 0.1 * hs;
        double bad = 0.0;
        for (int k = tid; k < S; k += nt) if (nonfinite(y[k])) bad = 1.0;
        for (int k = tid; k < n.n_var; k += nt) if (nonfinite(L.p[k])) bad = 1.0;
        if (block_max(bad, red) != 0.0) { status |= PK_ST_NONFINITE; break; }
        continue;
      }
      const double fac = step_fac(cbrt(err));
      double hnew = hs / fac;
      if (err <= 1.0) {
        ++nacc;
        for (int k = tid; k < S; k += nt) y[k] = R_[k];
        __syncthreads();
        tc += hs;
        if (after_reject) hnew = fmin(hnew, hs);
        after_reject = false;
        if (last) {
          tc = te;
          h = (hs < h) ? fmax(hnew, h) : hnew;
          break;
        }
        h = hnew;
      } else {
        ++nrej; after_reject = true;
        h = hnew;
      }
    }
    if (status != PK_ST_OK) break;
    const int row = stop_out[si];
    if (row >= 0) {
      if (wY) for (int k = tid; k < S; k += nt) Yout[(size_t)row * S + k] = y[k];
      score_row(row);
    }
    const int jn = net_bucket(tc, n.kin_grid, n.n_grid);
    if (jn != jb) { jb = jn; net_prepare_bucket(n, L, jb); }
  }
  if (status != PK_ST_OK && wY) {
    // flagged candidate: every output row that was not reached is NaN (never garbage)
    const double qnan = __builtin_nan("");
    for (int si = 0; si < A.n_stops; ++si) {
      const int row = stop_out[si];
      if (row >= 0 && !(stops[si] <= tc)) for (int k = tid; k < S; k += nt) Yout[(size_t)row * S + k] = qnan;
    }
  }
  if (tid == 0) {
    if (A.status) A.status[b] = status;
    if (A.n_steps) { A.n_steps[2 * b] = nacc; A.n_steps[2 * b + 1] = nrej; }
  }
  if constexpr (FUSED) {
    // objective assembly of GlobalODE_MOO._evaluate (optproblem.py:99-160), as net_objective_kernel does it from a stored trajectory
    const double lp = block_sum(lacc[0], red), lr = block_sum(lacc[1], red), lph = block_sum(lacc[2], red);
    double prior = 0.0;
    if (A.loss_defaults) {
      double acc = 0.0;
      for (int k = tid; k < 5 * N; k += nt) {
        const int grp = k / N, i = k - grp * N;
        const int off = (grp == 0 ? sl.A : grp == 1 ? sl.B : grp == 2 ? sl.C : grp == 3 ? sl.D : sl.E) + i;
        const double d = (L.p[off] - A.loss_defaults[off]) / (A.loss_defaults[off] + 1e-6);
        acc = __builtin_fma(d, d, acc);
      }
      prior = A.loss_lam[3] * (block_sum(acc, red) / (double)(5 * N));
    }
    const bool bad = block_max(ybad ? 1.0 : 0.0, red) != 0.0 || status != PK_ST_OK;
    if (tid == 0) {
      if (A.loss_sums) { A.loss_sums[3 * b] = lp; A.loss_sums[3 * b + 1] = lr; A.loss_sums[3 * b + 2] = lph; }
      if (A.loss_F) {
        A.loss_F[3 * b] = bad ? A.loss_fail : (lp * A.loss_norm[0]) * A.loss_lam[0] + prior;
        A.loss_F[3 * b + 1] = bad ? A.loss_fail : (lr * A.loss_norm[1]) * A.loss_lam[1] + prior;
        A.loss_F[3 * b + 2] = bad ? A.loss_fail : (lph * A.loss_norm[2]) * A.loss_lam[2] + prior;
      }
    }
  }
  if constexpr (MEASURE) {
    // _compute_scalar_metric of the reference (sensitivity.py:117-140) over the candidate's fold changes; empty lists give 0
    const double cnt = (double)A.meas_n, qnan = __builtin_nan("");
    double val;
    if (A.meas_id == PK_NET_METRIC_VARIANCE) { block_welford(wn, wm, wq, red); val = wn > 0.0 ? wq / wn : 0.0; }
    else {
      const double sum = block_sum(wm, red);
      val = A.meas_id == PK_NET_METRIC_L2_NORM ? sqrt(sum) : (A.meas_id == PK_NET_METRIC_MEAN && A.meas_n > 0) ? sum / cnt : sum;
    }
    if (status != PK_ST_OK) {
      val = qnan;                                        // a barrier of the reduction lies between the entries written above and these
      if (predb) for (int k = tid; k < A.meas_n; k += nt) predb[k] = qnan;
    }
    if (tid == 0 && A.meas_metric) A.meas_metric[b] = val;
  }
}

__host__ __device__ inline size_t net_solve_lds_bytes(const NetDev& n, int nnzT);

// One workgroup per candidate, everything in dynamic LDS: the work area, 24 doubles of reductions, then the TF CSR (scoring flavours:
// then the rna baseline, N doubles)
template <int MODEL, NetScore SCORE = SCORE_NONE>
__global__ __launch_bounds__(256, 3) void net_solve_kernel(const NetDev n, const NetSolveArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int N = n.N, nnzT = n.TF_indptr[N];
  double* red = lds + net_rosw_doubles(n);
  double* tf_dat = red + 24;
  double* tf_deg = tf_dat + nnzT;
  int32_t* tf_ptr = reinterpret_cast<int32_t*>(tf_deg + N);
  int32_t* tf_idx = tf_ptr + (N + 1);
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int k = tid; k < nnzT; k += nt) { tf_dat[k] = n.TF_data[k]; tf_idx[k] = n.TF_indices[k]; }
  for (int k = tid; k <= N; k += nt) tf_ptr[k] = n.TF_indptr[k];
  for (int k = tid; k < N; k += nt) tf_deg[k] = n.tf_deg[k];
  const NetRegLayout lay(n, tf_dat, tf_deg, tf_ptr, tf_idx);
  net_rosw_solve<MODEL, SCORE>(n, A, lay, blockIdx.x, NetLds(lds, n), lds + NetLds::doubles(n), red,
                               SCORE != SCORE_NONE ? lds + net_solve_lds_bytes(n, nnzT) / 8 : nullptr);
}

// Networks of any size: every per-candidate vector in a slab of an HBM workspace instead of LDS, so nothing limits S or N but device
// memory.  The grid is persistent -- min(B, resident workgroups) -- and each workgroup loops over candidates, so the workspace is
// grid x slab whatever B is.  A slab is the net_rosw_doubles work area padded to whole 128-B lines so that no two workgroups share a line;
// LDS holds only the reduction buffer.  Visibility inside a workgroup: the __syncthreads() between phases (workgroup-scope release /
// acquire), exactly as in the LDS kernel; no workgroup reads another's slab.
template <int MODEL>
__global__ __launch_bounds__(256) void net_solve_ws_kernel(const NetDev n, const NetSolveArgs A, const long long B, double* __restrict__ ws,
                                                           const size_t slab) {
  __shared__ double red[24];
  double* const base0 = ws + (size_t)blockIdx.x * slab;
  const NetWsLayout lay(n);
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();                                   // the previous candidate of this workgroup is done with the slab
    net_rosw_solve<MODEL, SCORE_NONE>(n, A, lay, b, NetLds(base0, n), base0 + NetLds::doubles(n), red);
  }
}

// The same persistent grid scoring the loss or the Morris metric (net_rosw_solve<MODEL, SCORE_LOSS / SCORE_MEASURE>); the slab is N doubles longer: the rna baseline, behind the work
// area.  A kernel of its own so that the plain one keeps its attributes: scoring costs 15 VGPRs (134-136), one workgroup per CU less than
// the plain kernel's four; held to 128 here (12-20 B of scratch per lane) the resident grid stays 1 024
template <int MODEL, NetScore SCORE = SCORE_LOSS>
__global__ __launch_bounds__(256, 4) void net_solve_ws_fused_kernel(const NetDev n, const NetSolveArgs A, const long long B, double* __restrict__ ws,
                                                                    const size_t slab) {
  __shared__ double red[24];
  double* const base0 = ws + (size_t)blockIdx.x * slab;
  const NetWsLayout lay(n);
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();                                   // the previous candidate of this workgroup is done with the slab (rna baseline included)
    net_rosw_solve<MODEL, SCORE>(n, A, lay, b, NetLds(base0, n), base0 + NetLds::doubles(n), red, base0 + net_rosw_doubles(n));
  }
}

__host__ __device__ inline size_t net_ws_slab_doubles(const NetDev& n) { return (net_rosw_doubles(n) + 15) / 16 * 16; }
__host__ __device__ inline size_t net_ws_fused_slab_doubles(const NetDev& n) { return (net_rosw_doubles(n) + n.N + 15) / 16 * 16; }
__device__ __host__ inline size_t net_solve_lds_doubles(const NetDev& n) { return net_rosw_doubles(n) + 24; }
// + the LDS copy of the TF CSR: nnz doubles + N doubles + (N + 1 + nnz) int32 (rounded up to doubles)
__host__ __device__ inline size_t net_solve_lds_bytes(const NetDev& n, int nnzT) {
  return (net_solve_lds_doubles(n) + (size_t)nnzT + n.N) * 8 + (((size_t)n.N + 1 + nnzT) * 4 + 7) / 8 * 8;
}
__host__ inline size_t net_solve_fused_lds_bytes(const NetDev& n, int nnzT) { return net_solve_lds_bytes(n, nnzT) + (size_t)n.N * 8; }

}  // namespace pk
