// pk_network_sens.hpp -- forward parameter sensitivities of the network ODE: dY/dx_c for a handful of entries c of the candidate vector,
// from the order-3 Rosenbrock-W integrator of pk_network_solve.hpp (pk_network_simulate_sens_batch).
//
// Method.  The augmented system (y, s_1 .. s_kc) with  s_c' = f_y(y) s_c + df/dx_c(y),  s_c(t0) = 0 (y0 is data), is integrated by
// ROS34PW2-W with W = blockdiag(W_y, .., W_y): the W-method's order conditions hold for any Jacobian approximation, so the per-protein
// block factors of the state (net_rosw_solve's factor / block_solve, copied here) also solve every stage of every tangent column.  The
// stage right-hand side of a column is the exact directional derivative of net_prepare_bucket / net_prepare_state / net_state_rhs_ctx
// (pk_network.hpp) at the stage point -- no difference quotient: c_k through Kt -> S_all and through P_vec of driven proteins
// (topologies != 2), A_i and tf_scale through synth_rate, the TF coupling through both squashes, B, C, D, Dp, E in the blocks and the
// saturating factors of topology 4.  At |v| = 0 and at the u >= 0 branch the derivative is that of the branch the value takes.
//
// Error control: tangents enter the step's error norm with the states' rtol / atol (maximum norm over states and columns, or the
// root-mean-square over all S (1 + kc) entries) -- the rule of the per-protein sensitivity kernels.
//
// Column chunks.  A workgroup integrates ONE candidate with the kc <= KC columns of one chunk (grid: B x ceil(K / KC)); every chunk
// integrates the state itself, with its own step-size control, so a column is within rtol / atol of the exact derivative but two
// chunks are not bit-coupled.  Chunk 0 writes Y and n_steps (n_steps is chunk 0's); status is the OR over the chunks (the host zeroes
// it before the launch).  A flagged chunk leaves NaN in its own columns at the output rows it did not reach, and in every row if the
// flag is PK_ST_NONFINITE.  The non-finite bail-out of the state kernel is extended to the tangents: a rejected step whose error is not
// finite ends the chunk as PK_ST_NONFINITE when a state, a parameter or a tangent at the start of the step is not finite or a tangent
// has left |s| <= SENS_DIVERGED -- a diverging tangent would otherwise end as a long run of rejected steps.
//
// With x_is_raw the derivative is with respect to the raw entry: the physical tangent is integrated (so the steps do not depend on the
// parametrisation) and every stored value is multiplied by softplus'(raw) -- exactly 1 where softplus returns its argument.
//
// Output policy (NetSensOut).  SENS_STORE writes dY and nothing else.  SENS_SCORE differentiates the three-objective loss where the state
// and the chunk's tangents land on an output row (pk_network_simulate_objective_grad_batch): the step loop is the same statement for
// statement; only row 0 and a landing with row >= 0 differ.  The loss handle's time-bucketed lists are walked as net_rosw_solve<..,
// SCORE_LOSS>'s score_row walks them.  A row's entries (protein | rna | phospho) are taken in tiles of S through the stage vectors Ys, U1,
// U2, U3, which are dead between an accepted step and the next factorisation: a first pass, one thread per entry, leaves numerator a,
// baseline c, w rho'(pred) and w rho(pred) there (and stores pred); then ONE thread per (modality, column) walks the tile's entries of its
// modality in list order, forms da, dc from the column's tangent, and adds w rho' dpred_c to its accumulator dacc[m][c] (LDS, 3 kc doubles;
// the thread of column 0 also adds w rho to lacc[m]).  No reduction and no atomic: every sum is one thread's sequential sum in list order,
// so a candidate's numbers do not depend on the batch, on B or on the position of its column inside the chunk.  dpred is written by
// threads over (entry, column) pairs.  Baselines: y0 for protein / phospho (data: dc = 0); the rna baseline row and its kc tangent rows are
// kept from the landing that produces them (N (1 + kc) doubles of LDS).  Chunk 0 writes pred, loss_sums and F (fail_value under the rule
// of net_rosw_solve); every chunk writes its own columns of dpred, dsums and dF = dsums norm_m lambda_m + d prior / d x_c, NaN if the chunk
// is flagged.  With x_is_raw every derivative is multiplied by softplus'(raw), as dY is.
#pragma once
#include "pk_network_solve.hpp"
#include "pk_network_loss_grad.hpp"

namespace pk {

struct NetSensArgs {
  const int32_t* cols;     // [K] (device): indices into the candidate vector, NetSlices order; distinct, in range (the host checks)
  int K, KC;               // columns asked for; columns per workgroup
  double* dY;              // [B, T, S, K], K contiguous
};

// what a sensitivity workgroup does with an output row: store the tangents, or score the loss and its gradient (and store on request)
enum NetSensOut : int { SENS_STORE = 0, SENS_SCORE = 1 };
// outputs of the scoring flavour beyond NetSolveArgs' (loss_sums, loss_F, meas_pred with meas_perm / meas_n); each optional
struct NetSensScoreArgs {
  double* dpred;           // [B, n_obs, K], caller's list order
  double* dsums;           // [B, 3, K]
  double* dF;              // [B, 3, K]
};

constexpr double SENS_DIVERGED = 1e100;

// LDS of a sensitivity workgroup behind the plain kernel's request: [sA | sT] (N each), the chunk's column table (kc scale factors and kc
// indices, a double each), then per column [s | Ss | V1..V4 | Rt] (S each), dS_all (sites) and dP_vec (N)
__host__ __device__ inline size_t net_sens_col_doubles(const NetDev& n) { return 7 * (size_t)n.S + n.sites + n.N + 2; }
__host__ __device__ inline size_t net_sens_lds_bytes(const NetDev& n, int nnzT, int kc) {
  return net_solve_lds_bytes(n, nnzT) + (2 * (size_t)n.N + (size_t)kc * net_sens_col_doubles(n)) * 8;
}
// largest kc whose request stays within `budget` bytes (0: not even one column fits)
__host__ inline int net_sens_max_columns(const NetDev& n, int nnzT, size_t budget) {
  const size_t fixed = net_sens_lds_bytes(n, nnzT, 0);
  if (fixed >= budget) return 0;
  return (int)((budget - fixed) / (net_sens_col_doubles(n) * 8));
}

// The scoring flavour adds, behind the store flavour's request: the rna baseline (N) and per column its tangent (N), the accumulators
// dacc [3, kc] and lacc [3] (+ 1 of padding)
__host__ __device__ inline size_t net_sens_score_lds_bytes(const NetDev& n, int nnzT, int kc) {
  return net_sens_lds_bytes(n, nnzT, kc) + ((size_t)n.N + 4 + (size_t)kc * ((size_t)n.N + 3)) * 8;
}
__host__ inline int net_sens_score_max_columns(const NetDev& n, int nnzT, size_t budget) {
  const size_t fixed = net_sens_score_lds_bytes(n, nnzT, 0);
  if (fixed >= budget) return 0;
  return (int)((budget - fixed) / ((net_sens_col_doubles(n) + n.N + 3) * 8));
}

// d/d eps of net_state_rhs_ctx at (p + eps e_col, y + eps s), Sall + eps dSr, synth + eps dsynth: the tangent of state (i, loc)
template <int MODEL>
__device__ __forceinline__ double net_state_rhs_tan(const NetDev& n, const NetLds& L, const double* __restrict__ sv, const double* __restrict__ dSall,
                                                    const double dsynth, const int col, const int i, const int loc, const int st, const int ss,
                                                    const int ns) {
  constexpr int model = MODEL;
  const NetSlices sl(n.n_K, n.N, n.sites);
  const double* y = L.y + st;
  const double* s = sv + st;
  const double Bi = L.p[sl.B + i], Ci = L.p[sl.C + i], Di = L.p[sl.D + i], Ei = L.p[sl.E + i];
  const double dB = col == sl.B + i ? 1.0 : 0.0, dC = col == sl.C + i ? 1.0 : 0.0, dD = col == sl.D + i ? 1.0 : 0.0, dE = col == sl.E + i ? 1.0 : 0.0;
  const double* Dp = L.p + sl.Dp + ss;
  const int cDp = col - (sl.Dp + ss);              // the site whose Dp the column is, if in [0, ns)
  const double* Sr = L.Sall + ss;
  const double* dSr = dSall + ss;
  const double R = y[0], sR = s[0];
  if (loc == 0) return dsynth - Bi * sR - dB * R;
  if (model == 0) {
    const double P = y[1], sP = s[1];
    if (loc == 1) {
      double sumS = 0.0, dsumS = 0.0, dback = 0.0;
      for (int j = 0; j < ns; ++j) { sumS += Sr[j]; dsumS += dSr[j]; dback += dE * y[2 + j] + Ei * s[2 + j]; }
      return dC * R + Ci * sR - (dD + dsumS) * P - (Di + sumS) * sP + dback;
    }
    const int j = loc - 2;
    const double dDp = cDp == j ? 1.0 : 0.0;
    return dSr[j] * P + Sr[j] * sP - (dE + dDp + dD) * y[loc] - (Ei + Dp[j] + Di) * s[loc];
  }
  if (model == 4) {
    const double P = y[1], sP = s[1];
    const double hP = P / (1.0 + P), gP = 1.0 / ((1.0 + P) * (1.0 + P));
    if (loc == 1) {
      double v = dC * (R / (1.0 + R)) + Ci * sR / ((1.0 + R) * (1.0 + R)) - dD * P - Di * sP;
      for (int j = 0; j < ns; ++j) v += -(dSr[j] * hP + Sr[j] * gP * sP) + dE * y[2 + j] + Ei * s[2 + j];
      return v;
    }
    const int j = loc - 2;
    const double dDp = cDp == j ? 1.0 : 0.0;
    return dSr[j] * hP + Sr[j] * gP * sP - (dDp + dD + dE) * y[loc] - (Dp[j] + Di + Ei) * s[loc];
  }
  if (model == 1) {
    if (loc == 1) {
      double v = dC * R + Ci * sR - dD * y[1] - Di * s[1];
      if (ns > 0) v += -dSr[0] * y[1] - Sr[0] * s[1] + dE * y[2] + Ei * s[2];
      return v;
    }
    const int j = loc - 2;
    const double dDp = cDp == j ? 1.0 : 0.0;
    double v = dSr[j] * y[loc - 1] + Sr[j] * s[loc - 1] - (dE + dDp + dD) * y[loc] - (Ei + Dp[j] + Di) * s[loc];
    if (j < ns - 1) v += dE * y[loc + 1] + Ei * s[loc + 1] - dSr[j + 1] * y[loc] - Sr[j + 1] * s[loc];
    return v;
  }
  // model 2: loc - 1 = bit mask m
  const int m = loc - 1;
  const double Pm = y[1 + m], sPm = s[1 + m];
  double dacc = (m == 0) ? dC * R + Ci * sR - dD * Pm - Di * sPm : 0.0;
  double loss = 0.0, dloss = 0.0;
  for (int j = 0; j < ns; ++j) {
    const int bit = 1 << j;
    if (m & bit) {
      loss += Ei + Dp[j] + Di;
      dloss += dE + (cDp == j ? 1.0 : 0.0) + dD;
      dacc += dSr[j] * y[1 + (m ^ bit)] + Sr[j] * s[1 + (m ^ bit)];
    } else {
      loss += Sr[j];
      dloss += dSr[j];
      dacc += dE * y[1 + (m | bit)] + Ei * s[1 + (m | bit)];
    }
  }
  return dacc - dloss * Pm - loss * sPm;
}

// ROS34PW2-W of candidate b with the columns [c0, c0 + kc) of S.cols.  L, base, red, lay: as net_rosw_solve; ext: the extra LDS
// (net_sens_lds_bytes - net_solve_lds_bytes of it; SENS_SCORE: net_sens_score_lds_bytes - ...).  The state part is
// net_rosw_solve<MODEL, SCORE_NONE>'s, statement for statement.  SC: the scoring flavour's outputs (SENS_STORE: unused, null)
template <int MODEL, NetSensOut OUT, class Layout>
__device__ __forceinline__ void net_rosw_sens_solve(const NetDev& n, const NetSolveArgs& A, const NetSensArgs& SA, const NetSensScoreArgs* const SC,
                                                    const Layout& lay, const long long b, const int c0, const int kc, NetLds L, double* const base,
                                                    double* const red, double* const ext) {
  using namespace rosw;
  constexpr int model = MODEL;
  constexpr bool SCORE = OUT == SENS_SCORE;
  const int S = n.S, N = n.N, K = SA.K;
  double* y = L.y;
  double* Ys = base;
  double* U1 = Ys + S; double* U2 = U1 + S; double* U3 = U2 + S; double* U4 = U3 + S;
  double* R_ = U4 + S;
  double* winv = R_ + S;
  double* sinv = winv + S;
  double* cR = sinv + N;
  double* gP = cR + N;
  double* sA = ext;                       // per protein: d synth / d A_i
  double* sT = sA + N;                    // per protein: d synth / d tf_scale
  double* scl = sT + N;                   // per column: softplus'(raw entry), or 1
  int32_t* colv = reinterpret_cast<int32_t*>(scl + kc);      // per column: its index into the candidate vector (kc doubles reserved)
  double* tan0 = scl + 2 * (size_t)kc;
  const size_t cst = net_sens_col_doubles(n) - 2;            // doubles of one column's vectors
  // column c: s (current tangent), Ss (stage point), V1..V4 (stage vectors), Rt (stage right-hand side), dSl (d S_all), dPv (d P_vec)
  auto col_s = [&](const int c) { return tan0 + (size_t)c * cst; };
  const double* __restrict__ tf_dat = lay.tf_dat;
  const double* __restrict__ tf_deg = lay.tf_deg;
  const int32_t* __restrict__ tf_ptr = lay.tf_ptr;
  const int32_t* __restrict__ tf_idx = lay.tf_idx;
  const NetSlices sl(n.n_K, N, n.sites);
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* stops = A.stops_p ? A.stops_p : A.stops_v;
  const int32_t* stop_out = A.stop_out_p ? A.stop_out_p : A.stop_out_v;
  const bool chunk0 = c0 == 0;

  const double* xb = A.x + b * n.n_var;
  for (int k = tid; k < n.n_var; k += nt) L.p[k] = A.x_is_raw ? softplus(xb[k]) : xb[k];
  for (int c = tid; c < kc; c += nt) {
    const int col = SA.cols[c0 + c];
    colv[c] = col;
    const double r = xb[col];
    scl[c] = (A.x_is_raw && !(r > 20.0)) ? 1.0 / (1.0 + exp(-r)) : 1.0;
  }
  const double* y0 = A.y0 + (A.y0_batched ? b * S : 0);
  const bool wY = chunk0 && A.Y != nullptr;
  double* Yout = wY ? A.Y + b * (size_t)A.T * S : nullptr;
  const bool wdY = !SCORE || SA.dY != nullptr;                // the store flavour always has dY
  double* dYout = wdY ? SA.dY + b * (size_t)A.T * S * K + c0 : nullptr;       // entry (row, k, c): dYout[((size_t)row * S + k) * K + c]
  for (int k = tid; k < S; k += nt) { const double v = y0[k]; y[k] = v; if (wY) Yout[k] = v; }
  for (int q = tid; q < kc * S; q += nt) {
    const int c = q / S, k = q - c * S;
    col_s(c)[k] = 0.0;
    if (wdY) dYout[(size_t)k * K + c] = 0.0;
  }
  // ---- scoring flavour: its LDS behind the columns' vectors, and what it does with output row `row`, which y and col_s(c) hold
  double* const rbase = tan0 + (size_t)kc * cst;              // rna baseline row
  double* const drb = rbase + N;                              // its tangent, per column
  double* const dacc = drb + (size_t)kc * N;                  // [3, kc]: sum of w rho' dpred_c per modality and column
  double* const lacc = dacc + 3 * (size_t)kc;                 // [3]: sum of w rho per modality
  bool ybad = false;
  double* const predb = (SCORE && chunk0 && A.meas_pred) ? A.meas_pred + b * (size_t)A.meas_n : nullptr;
  double* const dpredb = (SCORE && SC->dpred) ? SC->dpred + b * (size_t)A.meas_n * K + c0 : nullptr;      // entry (o, c): dpredb[(size_t)o * K + c]
  if constexpr (SCORE) for (int q = tid; q < 3 * kc + 3; q += nt) dacc[q] = 0.0;
  __syncthreads();
  auto score_row = [&](const int row) {
    if constexpr (SCORE) {
      if (chunk0) for (int k = tid; k < S; k += nt) if (nonfinite(y[k])) ybad = true;
      if (row == A.loss_rna_base) {
        for (int q = tid; q < (1 + kc) * N; q += nt) {
          const int c = q / N, i = q - c * N;
          const int st = n.offset_y[i];
          if (c == 0) rbase[i] = y[st]; else drb[(size_t)(c - 1) * N + i] = col_s(c - 1)[st];
        }
        __syncthreads();
      }
      const int T1 = A.T + 1;
      const int32_t* ptr = A.loss_ptr + row;
      const int b0 = ptr[0], n0 = ptr[1] - b0, b1 = ptr[T1], n1 = ptr[T1 + 1] - b1, b2 = ptr[2 * T1], n2 = ptr[2 * T1 + 1] - b2;
      const int ntot = n0 + n1 + n2;
      // position v in the row's (protein | rna | phospho) entries -> modality and list entry
      auto locate = [&](const int v, int& m, int& k) {
        if (v < n0) { m = 0; k = b0 + v; } else if (v < n0 + n1) { m = 1; k = b1 + (v - n0); } else { m = 2; k = b2 + (v - n0 - n1); }
      };
      // numerator and baseline of an entry, summed as net_rosw_solve's score_row sums them
      auto entry_val = [&](const int m, const int k, double& a, double& c) {
        const int i = A.loss_prot[k], st = n.offset_y[i];
        if (m == 0) {
          const int cnt = (model == 2) ? (1 << n.n_sites[i]) : 1 + n.n_sites[i];
          a = 0.0; c = 0.0;
          for (int m_ = 0; m_ < cnt; ++m_) { a += y[st + 1 + m_]; c += y0[st + 1 + m_]; }
        } else if (m == 1) { a = y[st]; c = rbase[i]; }
        else {
          const int j = A.loss_site[k];
          if (model == 2) {
            a = 0.0; c = 0.0;
            const int cnt = 1 << n.n_sites[i];
            for (int m_ = 0; m_ < cnt; ++m_) if (m_ & (1 << j)) { a += y[st + 1 + m_]; c += y0[st + 1 + m_]; }
          } else { a = y[st + 2 + j]; c = y0[st + 2 + j]; }
        }
      };
      // the same sums over column cc's tangent; the protein / phospho baseline is data
      auto entry_tan = [&](const int m, const int k, const int cc, double& da, double& dc) {
        const int i = A.loss_prot[k], st = n.offset_y[i];
        const double* sv = col_s(cc);
        dc = 0.0;
        if (m == 0) {
          const int cnt = (model == 2) ? (1 << n.n_sites[i]) : 1 + n.n_sites[i];
          da = 0.0;
          for (int m_ = 0; m_ < cnt; ++m_) da += sv[st + 1 + m_];
        } else if (m == 1) { da = sv[st]; dc = drb[(size_t)cc * N + i]; }
        else {
          const int j = A.loss_site[k];
          if (model == 2) {
            da = 0.0;
            const int cnt = 1 << n.n_sites[i];
            for (int m_ = 0; m_ < cnt; ++m_) if (m_ & (1 << j)) da += sv[st + 1 + m_];
          } else da = sv[st + 2 + j];
        }
      };
      double* const tA = Ys; double* const tC = U1; double* const tG = U2; double* const tL = U3;      // dead until the next step
      for (int v0 = 0; v0 < ntot; v0 += S) {
        const int nv = min(S, ntot - v0);
        for (int e = tid; e < nv; e += nt) {
          int m, k; locate(v0 + e, m, k);
          double a, c; entry_val(m, k, a, c);
          const double obs = A.loss_lobs[k], w = A.loss_lw[k], pred = fold_change(a, c);
          tA[e] = a; tC[e] = c;
          tG[e] = w * point_loss_dpred(A.loss_mode, obs, pred);
          tL[e] = w * point_loss(A.loss_mode, obs - pred, obs, pred);
          if (predb) predb[A.meas_perm[k]] = pred;
        }
        __syncthreads();
        for (int q = tid; q < 3 * kc; q += nt) {
          const int m = q / kc, cc = q - m * kc;
          const int lo = m == 0 ? 0 : (m == 1 ? n0 : n0 + n1), cntm = m == 0 ? n0 : (m == 1 ? n1 : n2), kb = m == 0 ? b0 : (m == 1 ? b1 : b2);
          const int e0 = max(lo - v0, 0), e1 = min(lo + cntm - v0, nv);
          double acc = dacc[q], ls = lacc[m];
          for (int e = e0; e < e1; ++e) {
            double da, dc; entry_tan(m, kb + (v0 + e - lo), cc, da, dc);
            acc += tG[e] * fold_change_tangent(tA[e], tC[e], da, dc);
            ls += tL[e];
          }
          dacc[q] = acc;
          if (cc == 0) lacc[m] = ls;
        }
        if (dpredb) for (int q = tid; q < nv * kc; q += nt) {
          const int e = q / kc, cc = q - e * kc;
          int m, k; locate(v0 + e, m, k);
          double da, dc; entry_tan(m, k, cc, da, dc);
          dpredb[(size_t)A.meas_perm[k] * K + cc] = fold_change_tangent(tA[e], tC[e], da, dc) * scl[cc];
        }
        __syncthreads();
      }
    }
  };
  score_row(0);

  auto factor = [&](const double g) {
    lay.prots([&](const int i, const int st, const int ss, const int ns, const int) {
      const double Bi = L.p[sl.B + i], Ci = L.p[sl.C + i], Di = L.p[sl.D + i], Ei = L.p[sl.E + i];
      const double* Dp = L.p + sl.Dp + ss;
      const double* Sr = L.Sall + ss;
      winv[st] = 1.0 / (g + Bi);
      if (model == 2) {
        cR[i] = Ci; gP[i] = 1.0;
        const int nst = 1 << ns;
        for (int m = 0; m < nst; ++m) {
          double loss = (m == 0) ? Di : 0.0;
          for (int j = 0; j < ns; ++j) loss += ((m >> j) & 1) ? (Ei + Dp[j] + Di) : Sr[j];
          winv[st + 1 + m] = 1.0 / (g + loss);
        }
      } else if (model == 1) {
        cR[i] = Ci; gP[i] = 1.0;
        double d = g + Di + (ns ? Sr[0] : 0.0);
        winv[st + 1] = 1.0 / d;
        for (int q = 1; q <= ns; ++q) {
          const int j = q - 1;
          const double diag = g + Ei + Dp[j] + Di + ((j < ns - 1) ? Sr[j + 1] : 0.0);
          d = diag - (Sr[j] * Ei) * winv[st + q];
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
  // x <- W^{-1} r for the block of protein i (in place: r -> x); no barrier
  auto block_solve_one = [&](const int i, const int st, const int ss, const int ns, const double* r, double* x) {
    const double Ei = L.p[sl.E + i];
    const double* Sr = L.Sall + ss;
    const double xR = r[st] * winv[st];
    x[st] = xR;
    if (model == 2) {
      const int nst = 1 << ns;
      for (int m = 0; m < nst; ++m) {
        double a = r[st + 1 + m] + ((m == 0) ? cR[i] * xR : 0.0);
        for (int mm = m; mm; mm &= mm - 1) { const int bit = mm & -mm; a = __builtin_fma(Sr[__builtin_ctz(bit)], x[st + 1 + (m ^ bit)], a); }
        x[st + 1 + m] = a * winv[st + 1 + m];
      }
      for (int m = nst - 2; m >= 0; --m) {
        double hi = 0.0;
        for (int mm = ~m & (nst - 1); mm; mm &= mm - 1) hi += x[st + 1 + (m | (mm & -mm))];
        x[st + 1 + m] = __builtin_fma(Ei * hi, winv[st + 1 + m], x[st + 1 + m]);
      }
    } else if (model == 1) {
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
  };
  int jb = 0;
  // d S_all of every column for bucket jb (d Kt_k = kin_Kmat[k, jb] where the column is c_k); ends with a barrier
  auto prepare_bucket_tan = [&]() {
    for (int q = tid; q < kc * n.sites; q += nt) {
      const int c = q / n.sites, r = q - c * n.sites;
      const int kk = colv[c] - sl.ck;
      double acc = 0.0;
      if (kk >= 0 && kk < n.n_K)
        for (int e_ = n.W_indptr[r]; e_ < n.W_indptr[r + 1]; ++e_) if (n.W_indices[e_] == kk) acc += n.W_data[e_] * n.kin_Kmat[(size_t)kk * n.n_grid + jb];
      (col_s(c) + 7 * (size_t)S)[r] = acc;
    }
    __syncthreads();
  };
  // P_vec -> TF input -> synthesis rate for the state L.y points at, with the derivatives the tangents need: L.dsyn = d synth_i /
  // d (TF . P_vec)_i, sA, sT; and d P_vec of every column at its stage tangent (stage 0: s itself, else Ss)
  auto prepare_state = [&](const bool first) {
    lay.prots([&](const int i, const int st, const int, const int ns, const int drv) {
      double tot;
      if (model != 2 && drv >= 0) tot = L.Kt[drv];
      else { tot = 0.0; const int cnt = (model == 2) ? (1 << ns) : 1 + ns; for (int m_ = 0; m_ < cnt; ++m_) tot += L.y[st + 1 + m_]; }
      L.Pvec[i] = tot;
    });
    for (int q = tid; q < kc * N; q += nt) {
      const int c = q / N, i = q - c * N;
      const int drv = n.driver_map[i], st = n.offset_y[i], ns = n.n_sites[i];
      const double* sv = col_s(c) + (first ? 0 : S);
      double tot;
      if (model != 2 && drv >= 0) tot = (colv[c] == sl.ck + drv) ? n.kin_Kmat[(size_t)drv * n.n_grid + jb] : 0.0;
      else { tot = 0.0; const int cnt = (model == 2) ? (1 << ns) : 1 + ns; for (int m_ = 0; m_ < cnt; ++m_) tot += sv[st + 1 + m_]; }
      (col_s(c) + 7 * (size_t)S + n.sites)[i] = tot;
    }
    __syncthreads();
    const double ts = L.p[sl.tf];
    lay.prots([&](const int i, const int, const int, const int, const int) {
      double acc = 0.0;
      for (int e_ = tf_ptr[i]; e_ < tf_ptr[i + 1]; ++e_) acc += tf_dat[e_] * L.Pvec[tf_idx[e_]];
      double v = acc / tf_deg[i];
      double dv = 1.0 / tf_deg[i];
      if (model != 4) { const double den = 1.0 + fabs(v); dv *= 1.0 / (den * den); v = v / den; }
      const double Ai = L.p[sl.A + i];
      double d = 0.0;
      L.synth[i] = synth_rate(Ai, ts, v, &d);
      L.dsyn[i] = d * dv;
      const double u = v / (1.0 + fabs(v));
      if (u >= 0.0) { const double q = 1.0 + u + 1e-6; sA[i] = 1.0 + (ts * u) / q; sT[i] = Ai * u / q; }
      else { const double q = 1.0 + ts * fabs(u); sA[i] = 1.0 / q; sT[i] = -Ai * fabs(u) / (q * q); }
    });
    __syncthreads();
  };
  int status = PK_ST_OK, nacc = 0, nrej = 0;
  double tc = A.t0;
  jb = net_bucket(tc, n.kin_grid, n.n_grid);
  net_prepare_bucket(n, L, jb);
  prepare_bucket_tan();
  double h;
  {
    // first step from the max-norm of y / sc and f / sc, as the state kernel takes it (the tangents start at 0)
    L.y = y;
    prepare_state(true);
    double d0 = 0.0, d1 = 0.0;
    for (int k = tid; k < S; k += nt) {
      const double sc = A.atol + A.rtol * fabs(y[k]);
      d0 = fmax(d0, fabs(y[k]) / sc); d1 = fmax(d1, fabs(net_state_rhs(n, L, k)) / sc);
    }
    d0 = block_max(d0, red); d1 = block_max(d1, red);
    h = (d0 > 1e-5 && d1 > 1e-5) ? 0.01 * d0 / d1 : 1e-6;
    if (A.h0 > 0.0) h = A.h0;
    if (!(h > 0.0) || h != h) h = 1e-6;
  }
  const int nerr = S * (1 + kc);
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
#pragma unroll 1
      for (int sg = 0; sg < 4; ++sg) {
        if (sg > 0) {
          for (int k = tid; k < S; k += nt) {
            double v = y[k];
            for (int j = 0; j < sg; ++j) v = __builtin_fma(TA[sg][j], U1[(size_t)j * S + k], v);
            Ys[k] = v;
          }
          for (int q = tid; q < kc * S; q += nt) {
            const int c = q / S, k = q - c * S;
            double* s = col_s(c);
            double v = s[k];
            for (int j = 0; j < sg; ++j) v = __builtin_fma(TA[sg][j], s[(size_t)(2 + j) * S + k], v);
            s[S + k] = v;
          }
          __syncthreads();
        }
        L.y = (sg == 0) ? y : Ys;
        prepare_state(sg == 0);
        lay.states([&](const int k, const int i, const int loc, const int st, const int ss, const int ns) {
          double v = net_state_rhs_ctx<MODEL>(n, L, i, loc, st, ss, ns);
          for (int j = 0; j < sg; ++j) v = __builtin_fma(TC[sg][j] * hinv, U1[(size_t)j * S + k], v);
          R_[k] = v;
        });
        for (int q = tid; q < kc * S; q += nt) {
          const int c = q / S, k = q - c * S;
          const int i = n.state_prot[k], loc = n.state_local[k];
          double* s = col_s(c);
          const double* sv = s + (sg == 0 ? 0 : S);
          const double* dSl = s + 7 * (size_t)S;
          const double* dPv = dSl + n.sites;
          const int col = colv[c];
          double dsynth = 0.0;
          if (loc == 0) {
            double acc = 0.0;
            for (int e_ = tf_ptr[i]; e_ < tf_ptr[i + 1]; ++e_) acc += tf_dat[e_] * dPv[tf_idx[e_]];
            dsynth = L.dsyn[i] * acc + (col == sl.A + i ? sA[i] : 0.0) + (col == sl.tf ? sT[i] : 0.0);
          }
          double v = net_state_rhs_tan<MODEL>(n, L, sv, dSl, dsynth, col, i, loc, n.offset_y[i], n.offset_s[i], n.n_sites[i]);
          for (int j = 0; j < sg; ++j) v = __builtin_fma(TC[sg][j] * hinv, s[(size_t)(2 + j) * S + k], v);
          s[6 * (size_t)S + k] = v;
        }
        __syncthreads();
        lay.prots([&](const int i, const int st, const int ss, const int ns, const int) { block_solve_one(i, st, ss, ns, R_, U1 + (size_t)sg * S); });
        for (int q = tid; q < kc * N; q += nt) {
          const int c = q / N, i = q - c * N;
          double* s = col_s(c);
          block_solve_one(i, n.offset_y[i], n.offset_s[i], n.n_sites[i], s + 6 * (size_t)S, s + (size_t)(2 + sg) * S);
        }
        __syncthreads();
      }
      // y1 = Ys + U4, s1 = Ss + V4 ; err over states and tangents
      double e = 0.0;
      for (int k = tid; k < S; k += nt) {
        const double yn = Ys[k] + U4[k];
        const double ev = E1 * U1[k] + E2 * U2[k] + E3 * U3[k] + E4 * U4[k];
        const double q = fabs(ev) / (A.atol + A.rtol * fmax(fabs(y[k]), fabs(yn)));
        e = err_acc(e, q, A.err_rms);
        R_[k] = yn;
      }
      for (int q_ = tid; q_ < kc * S; q_ += nt) {
        const int c = q_ / S, k = q_ - c * S;
        double* s = col_s(c);
        const double sn = s[S + k] + s[5 * (size_t)S + k];
        const double ev = E1 * s[2 * (size_t)S + k] + E2 * s[3 * (size_t)S + k] + E3 * s[4 * (size_t)S + k] + E4 * s[5 * (size_t)S + k];
        const double q = fabs(ev) / (A.atol + A.rtol * fmax(fabs(s[k]), fabs(sn)));
        e = err_acc(e, q, A.err_rms);
        s[6 * (size_t)S + k] = sn;
      }
      const double err = err_reduce(e, A.err_rms, nerr, red);
      if (err != err || err > 1e300) {
        ++nrej; after_reject = true; h = 0.1 * hs;
        double bad = 0.0;
        for (int k = tid; k < S; k += nt) if (nonfinite(y[k])) bad = 1.0;
        for (int k = tid; k < n.n_var; k += nt) if (nonfinite(L.p[k])) bad = 1.0;
        for (int q = tid; q < kc * S; q += nt) { const int c = q / S; if (!(fabs(col_s(c)[q - c * S]) <= SENS_DIVERGED)) bad = 1.0; }
        if (block_max(bad, red) != 0.0) { status |= PK_ST_NONFINITE; break; }
        continue;
      }
      const double fac = step_fac(cbrt(err));
      double hnew = hs / fac;
      if (err <= 1.0) {
        ++nacc;
        for (int k = tid; k < S; k += nt) y[k] = R_[k];
        for (int q = tid; q < kc * S; q += nt) { const int c = q / S, k = q - c * S; double* s = col_s(c); s[k] = s[6 * (size_t)S + k]; }
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
      if (wdY) for (int q = tid; q < kc * S; q += nt) {
        const int c = q / S, k = q - c * S;
        dYout[((size_t)row * S + k) * K + c] = col_s(c)[k] * scl[c];
      }
      score_row(row);
    }
    const int jn = net_bucket(tc, n.kin_grid, n.n_grid);
    if (jn != jb) { jb = jn; net_prepare_bucket(n, L, jb); prepare_bucket_tan(); }
  }
  if (status != PK_ST_OK) {
    // flagged chunk: every output row that was not reached is NaN (never garbage); a non-finite chunk has no row to trust
    const double qnan = __builtin_nan("");
    const bool all = (status & PK_ST_NONFINITE) != 0;
    for (int si = 0; si < A.n_stops; ++si) {
      const int row = stop_out[si];
      if (row < 0) continue;
      const bool missed = !(stops[si] <= tc);
      if (missed && wY) for (int k = tid; k < S; k += nt) Yout[(size_t)row * S + k] = qnan;
      if (wdY && (missed || all)) for (int q = tid; q < kc * S; q += nt) { const int c = q / S, k = q - c * S; dYout[((size_t)row * S + k) * K + c] = qnan; }
    }
    if (wdY && all) for (int q = tid; q < kc * S; q += nt) { const int c = q / S, k = q - c * S; dYout[(size_t)k * K + c] = qnan; }
  }
  if (tid == 0) {
    if (A.status && status != PK_ST_OK) atomicOr(A.status + b, status);
    if (A.n_steps && chunk0) { A.n_steps[2 * b] = nacc; A.n_steps[2 * b + 1] = nrej; }
  }
  if constexpr (SCORE) {
    // the chunk's columns of dsums and dF (a barrier of score_row lies behind the last accumulation); a flagged chunk has none to trust
    const double qnan = __builtin_nan("");
    const bool flagged = status != PK_ST_OK;
    for (int q = tid; q < 3 * kc; q += nt) {
      const int m = q / kc, cc = q - m * kc, col = colv[cc];
      double dprior = 0.0;
      if (A.loss_defaults && ((col >= sl.A && col < sl.Dp) || (col >= sl.E && col < sl.tf))) {
        const double d = A.loss_defaults[col], den = d + 1e-6;
        dprior = A.loss_lam[3] * ((2.0 * (L.p[col] - d)) / (den * den) / (double)(5 * N));
      }
      const double ds = flagged ? qnan : dacc[q] * scl[cc];
      const double dFv = flagged ? qnan : ((dacc[q] * A.loss_norm[m]) * A.loss_lam[m] + dprior) * scl[cc];
      const size_t at = ((size_t)b * 3 + m) * K + c0 + cc;
      if (SC->dsums) SC->dsums[at] = ds;
      if (SC->dF) SC->dF[at] = dFv;
    }
    __syncthreads();                                    // the dpred entries written at the rows lie behind this barrier
    if (flagged && dpredb) for (int q = tid; q < A.meas_n * kc; q += nt) { const int o = q / kc, cc = q - o * kc; dpredb[(size_t)o * K + cc] = qnan; }
    if (chunk0) {
      // objective assembly as net_rosw_solve<.., SCORE_LOSS> does it, from the list-order sums
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
      const bool bad = block_max(ybad ? 1.0 : 0.0, red) != 0.0 || flagged;
      if (bad && predb) for (int k = tid; k < A.meas_n; k += nt) predb[k] = qnan;
      if (tid == 0) {
        const double lp = lacc[0], lr = lacc[1], lph = lacc[2];
        if (A.loss_sums) { A.loss_sums[3 * b] = lp; A.loss_sums[3 * b + 1] = lr; A.loss_sums[3 * b + 2] = lph; }
        if (A.loss_F) {
          A.loss_F[3 * b] = bad ? A.loss_fail : (lp * A.loss_norm[0]) * A.loss_lam[0] + prior;
          A.loss_F[3 * b + 1] = bad ? A.loss_fail : (lr * A.loss_norm[1]) * A.loss_lam[1] + prior;
          A.loss_F[3 * b + 2] = bad ? A.loss_fail : (lph * A.loss_norm[2]) * A.loss_lam[2] + prior;
        }
      }
    }
  }
}

// One workgroup per (candidate, column chunk): blockIdx.x = candidate, blockIdx.y = chunk.  Dynamic LDS: the plain kernel's request
// (work area, 24 doubles of reductions, TF CSR), then the sensitivity area (net_sens_lds_bytes)
template <int MODEL>
__global__ __launch_bounds__(256) void net_solve_sens_kernel(const NetDev n, const NetSolveArgs A, const NetSensArgs SA) {
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
  const int c0 = blockIdx.y * SA.KC;
  const int kc = min(SA.KC, SA.K - c0);
  net_rosw_sens_solve<MODEL, SENS_STORE>(n, A, SA, nullptr, lay, blockIdx.x, c0, kc, NetLds(lds, n), lds + NetLds::doubles(n), red,
                                         lds + net_solve_lds_bytes(n, nnzT) / 8);
}

// The scoring flavour (NetSensOut above): the same grid and the same LDS layout, net_sens_score_lds_bytes of it; SA.dY may be null
template <int MODEL>
__global__ __launch_bounds__(256) void net_solve_sens_score_kernel(const NetDev n, const NetSolveArgs A, const NetSensArgs SA, const NetSensScoreArgs SC) {
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
  const int c0 = blockIdx.y * SA.KC;
  const int kc = min(SA.KC, SA.K - c0);
  net_rosw_sens_solve<MODEL, SENS_SCORE>(n, A, SA, &SC, lay, blockIdx.x, c0, kc, NetLds(lds, n), lds + NetLds::doubles(n), red,
                                         lds + net_solve_lds_bytes(n, nnzT) / 8);
}

// ---- Networks of any size: the same body with every per-item vector in a slab of an HBM workspace (as net_solve_ws_kernel runs
// net_rosw_solve).  A slab is the plain work area (net_rosw_doubles) followed by the sensitivity area of kc columns -- exactly the doubles
// the LDS kernels place behind the plain request, so the column arithmetic has one source (the nnzT terms cancel in the difference) --
// rounded up to whole 128-B lines.  The chunk width is not bound by LDS
__host__ __device__ inline size_t net_sens_ws_slab_doubles(const NetDev& n, int kc, bool score) {
  const size_t area = ((score ? net_sens_score_lds_bytes(n, 0, kc) : net_sens_lds_bytes(n, 0, kc)) - net_solve_lds_bytes(n, 0)) / 8;
  return (net_rosw_doubles(n) + area + 15) / 16 * 16;
}

// Persistent grid over work items: item w = b * n_chunks + j is candidate b with the columns [j KC, j KC + kc) of SA.cols; workgroup g takes
// w = g, g + grid, ...  LDS holds only the reduction buffer; the TF CSR is read from global memory (NetWsLayout).  Visibility inside a
// workgroup: the body's __syncthreads() (workgroup-scope release / acquire), as in net_solve_ws_kernel; no workgroup reads another's slab,
// and every accumulator slot of the scoring flavour stays one thread's.  The body re-initialises what an item leaves behind (parameters,
// column table, tangents, accumulators; the rna baseline is written at its row before any entry reads it).  status: the chunks of one
// candidate may run in different workgroups and rounds -- the body's atomicOr on status[b] (device scope) forms the OR whatever the order,
// the host zeroes status before the launch
template <int MODEL>
__global__ __launch_bounds__(256) void net_solve_sens_ws_kernel(const NetDev n, const NetSolveArgs A, const NetSensArgs SA, const long long items,
                                                                const int n_chunks, double* __restrict__ ws, const size_t slab) {
  __shared__ double red[24];
  double* const base0 = ws + (size_t)blockIdx.x * slab;
  const NetWsLayout lay(n);
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    __syncthreads();                                   // the previous item of this workgroup is done with the slab
    const long long b = w / n_chunks;
    const int c0 = (int)(w - b * n_chunks) * SA.KC;
    const int kc = min(SA.KC, SA.K - c0);
    net_rosw_sens_solve<MODEL, SENS_STORE>(n, A, SA, nullptr, lay, b, c0, kc, NetLds(base0, n), base0 + NetLds::doubles(n), red,
                                           base0 + net_rosw_doubles(n));
  }
}

template <int MODEL>
__global__ __launch_bounds__(256) void net_solve_sens_score_ws_kernel(const NetDev n, const NetSolveArgs A, const NetSensArgs SA,
                                                                      const NetSensScoreArgs SC, const long long items, const int n_chunks,
                                                                      double* __restrict__ ws, const size_t slab) {
  __shared__ double red[24];
  double* const base0 = ws + (size_t)blockIdx.x * slab;
  const NetWsLayout lay(n);
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    __syncthreads();                                   // the previous item of this workgroup is done with the slab (rna baseline, accumulators)
    const long long b = w / n_chunks;
    const int c0 = (int)(w - b * n_chunks) * SA.KC;
    const int kc = min(SA.KC, SA.K - c0);
    net_rosw_sens_solve<MODEL, SENS_SCORE>(n, A, SA, &SC, lay, b, c0, kc, NetLds(base0, n), base0 + NetLds::doubles(n), red,
                                           base0 + net_rosw_doubles(n));
  }
}

}  // namespace pk
