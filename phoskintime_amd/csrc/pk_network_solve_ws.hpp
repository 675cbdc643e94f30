// pk_network_solve_ws.hpp -- the network integrator of pk_network_solve.hpp (ROS34PW2-W, per-protein block-diagonal W) for networks of ANY
// size: every per-candidate vector lives in a slab of an HBM workspace instead of LDS, so nothing limits S or N but device memory.
//
// Same method decision for decision as net_solve_kernel: block factorisation / solve of all four topologies, bucket-edge landing points,
// first-step heuristic, max / RMS error norm, h0, max_steps, status flags, NaN rows after a failure, long stop lists.  The per-state and
// per-protein arithmetic is the LDS kernel's, statement for statement, so the two agree to the last bits on a network both can run.
//
// Layout: one workgroup per candidate; every thread strides over states and proteins (no per-thread register contexts, hence no ceiling).
// Topology (CSR, offsets, state_prot) is read from global memory; LDS holds only the reduction buffer.  The grid is persistent --
// min(B, resident workgroups) -- and each workgroup loops over candidates, so the workspace is grid x slab whatever B is.  A slab is
// [p | y | Kt | S_all | P_vec | synth | dsyn] (NetLds) + [Ys | U1..U4 | R | winv] (S each) + [sinv | cR | gP] (N each), padded to whole
// 128-B lines so that no two workgroups share a line.  Visibility inside a workgroup: the __syncthreads() between phases (workgroup-scope
// release / acquire), exactly as in the LDS kernel; no workgroup reads another's slab.
#pragma once
#include "pk_network_solve.hpp"

namespace pk {

__host__ __device__ inline size_t net_ws_slab_doubles(const NetDev& n) {
  const size_t d = ((size_t)n.n_var + n.S + n.n_K + n.sites + 3 * (size_t)n.N) + 7 * (size_t)n.S + 3 * (size_t)n.N;
  return (d + 15) / 16 * 16;
}

template <int MODEL>
__global__ __launch_bounds__(256) void net_solve_ws_kernel(const NetDev n, const NetSolveArgs A, const long long B, double* __restrict__ ws,
                                                           const size_t slab) {
  using namespace rosw;
  constexpr int model = MODEL;
  __shared__ double red[24];                           // reductions
  double* const base0 = ws + (size_t)blockIdx.x * slab;
  const int S = n.S, N = n.N;
  const NetSlices sl(n.n_K, N, n.sites);
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* stops = A.stops_p ? A.stops_p : A.stops_v;
  const int32_t* stop_out = A.stop_out_p ? A.stop_out_p : A.stop_out_v;
  const int32_t* __restrict__ tf_ptr = n.TF_indptr;
  const int32_t* __restrict__ tf_idx = n.TF_indices;
  const double* __restrict__ tf_dat = n.TF_data;
  const double* __restrict__ tf_deg = n.tf_deg;

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();                                   // the previous candidate of this workgroup is done with the slab
    NetLds L(base0, n);
    double* base = base0 + NetLds::doubles(n);
    double* y = L.y;                                   // current state
    double* Ys = base;                                 // stage point
    double* U1 = Ys + S; double* U2 = U1 + S; double* U3 = U2 + S; double* U4 = U3 + S;
    double* R_ = U4 + S;                               // right-hand side of the stage system
    double* winv = R_ + S;                             // per state: 1 / pivot of its row in the block factorisation
    double* sinv = winv + S;                           // per protein: 1 / Schur pivot of the P row (arrow blocks)
    double* cR = sinv + N;                             // per protein: d f_P / d R
    double* gP = cR + N;                               // per protein: saturating-kinetics factor 1 / (1 + P)^2 (1 otherwise)

    const double* xb = A.x + b * n.n_var;
    for (int k = tid; k < n.n_var; k += nt) L.p[k] = A.x_is_raw ? softplus(xb[k]) : xb[k];
    const double* y0 = A.y0 + (A.y0_batched ? b * S : 0);
    double* Yout = A.Y + b * (size_t)A.T * S;
    for (int k = tid; k < S; k += nt) { const double v = y0[k]; y[k] = v; Yout[k] = v; }
    __syncthreads();

    // ---- block factorisation of  g I - J_blockdiag(y)  and block solve  x <- W^{-1} r  (in place: r -> x), one thread per protein
    auto factor = [&](const double g) {
      for (int i = tid; i < N; i += nt) {
        const int st = n.offset_y[i], ss = n.offset_s[i], ns = n.n_sites[i];
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
      }
      __syncthreads();
    };
    auto block_solve = [&](const double* r, double* x) {
      for (int i = tid; i < N; i += nt) {
        const int st = n.offset_y[i], ss = n.offset_s[i], ns = n.n_sites[i];
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
      }
      __syncthreads();
    };
    // P_vec -> TF input -> synthesis rate for the state L.y points at (the LDS kernel's prepare_state on the global topology)
    auto prepare_state = [&]() {
      for (int i = tid; i < N; i += nt) {
        const int ns = n.n_sites[i], drv = n.driver_map[i];
        double tot;
        if (model != 2 && drv >= 0) tot = L.Kt[drv];
        else { tot = 0.0; const int cnt = (model == 2) ? (1 << ns) : 1 + ns; const int st = n.offset_y[i]; for (int m_ = 0; m_ < cnt; ++m_) tot += L.y[st + 1 + m_]; }
        L.Pvec[i] = tot;
      }
      __syncthreads();
      const double ts = L.p[sl.tf];
      for (int i = tid; i < N; i += nt) {
        double acc = 0.0;
        for (int e_ = tf_ptr[i]; e_ < tf_ptr[i + 1]; ++e_) acc += tf_dat[e_] * L.Pvec[tf_idx[e_]];
        double v = acc / tf_deg[i];
        if (model != 4) v = v / (1.0 + fabs(v));
        L.synth[i] = synth_rate(L.p[sl.A + i], ts, v, nullptr);
      }
      __syncthreads();
    };
    int status = PK_ST_OK, nacc = 0, nrej = 0;
    double tc = A.t0;
    int jb = net_bucket(tc, n.kin_grid, n.n_grid);
    net_prepare_bucket(n, L, jb);
    double h;
    {
      L.y = y;
      prepare_state();
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
        double* const Us[4] = {U1, U2, U3, U4};
#pragma unroll 1
        for (int sg = 0; sg < 4; ++sg) {
          if (sg > 0) {
            for (int k = tid; k < S; k += nt) {
              double v = y[k];
              for (int j = 0; j < sg; ++j) v = __builtin_fma(TA[sg][j], Us[j][k], v);
              Ys[k] = v;
            }
            __syncthreads();
          }
          L.y = (sg == 0) ? y : Ys;
          prepare_state();
          for (int k = tid; k < S; k += nt) {
            const int i = n.state_prot[k];
            double v = net_state_rhs_ctx<MODEL>(n, L, i, n.state_local[k], n.offset_y[i], n.offset_s[i], n.n_sites[i]);
            for (int j = 0; j < sg; ++j) v = __builtin_fma(TC[sg][j] * hinv, Us[j][k], v);
            R_[k] = v;
          }
          __syncthreads();
          block_solve(R_, Us[sg]);
        }
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
        double fac = cbrt(err) * (1.0 / 0.9);
        fac = fmax(1.0 / 6.0, fmin(5.0, fac));
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
      if (row >= 0) for (int k = tid; k < S; k += nt) Yout[(size_t)row * S + k] = y[k];
      const int jn = net_bucket(tc, n.kin_grid, n.n_grid);
      if (jn != jb) { jb = jn; net_prepare_bucket(n, L, jb); }
    }
    if (status != PK_ST_OK) {
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
  }
}

}  // namespace pk
