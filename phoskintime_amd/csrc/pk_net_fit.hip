// pk_net_fit.hip -- pk_network_fit_batch: a bounded Levenberg-Marquardt polish of B network candidates over K chosen entries of the
// candidate vector, with its whole state in HBM.  The integrations are the library's own entry point
// (pk_network_simulate_objective_grad_batch: K columns for the Jacobian phase, no columns -- the plain order-3 fused objective -- for every
// cost); the four small kernels here do the algebra between them with the per-row rules of pk_lm.hpp and the residual rows of
// pk_net_fit.hpp.  Every sum of every kernel is taken by one thread in list order: a row's iterates depend on its own data only.
//
// Cost consistency: a launch with tangents controls its steps on state and tangents together, so its trajectory lies within rtol / atol of
// the plain launch's, not on it.  Every cost the gain ratio compares (the row's own and every trial's) therefore comes from plain launches;
// the Jacobian phase contributes A = J^T J and g = J^T r only, with r from its own pred.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "../../include/phoskin.h"
#include "pk_network.hpp"
#include "pk_net_fit.hpp"

struct pk_net;
extern "C" int pk_ctx_device(pk_ctx*);
extern "C" void* pk_ctx_stream(pk_ctx*);
extern "C" int pk_ctx_fail(pk_ctx*, int code, const char* msg);
extern "C" void pk_ctx_lock(pk_ctx*);
extern "C" void pk_ctx_unlock(pk_ctx*);
extern "C" int pk_ctx_fit_reserve(pk_ctx*, size_t dev_bytes, size_t pin_bytes, void** dev, void** pin);
extern "C" const pk::NetDev* pk_net_dev(const pk_net*);
extern "C" int pk_loss_fit_view(const pk_loss* l, int32_t* n, const double** obs, const double** w, double* norms, int* T);

namespace pk {

// What every kernel of one fit sees: the caller's arrays, the per-row state and the shapes.  Passed by value.
struct NfProblem {
  int n_var, S, K, n_obs, N, n_K, sites, x_is_raw, y0_batched, bounds_batched;
  int n_mod[3];
  const double *obs[3], *w[3];
  double obj_w[3], norm[3], lam[4];
  const double *y0, *defaults, *lb, *ub;       // lb == NULL: no box
  const int32_t *cols, *colpos;                // cols [K]; colpos [n_var]: position of an entry among the fitted columns, -1 = held
  double *scl, *obsl;                          // [n_obs] residual scale and observation in the caller's (protein | rna | phospho) order
  double *x, *cost, *F, *A, *mu, *g, *DD;
  unsigned char* is_free;
  int32_t* st;
  double ftol, xtol;
};

constexpr int kNfThreads = 256;          // workgroup of net_fit_normal_kernel
constexpr int kNfOwn = 4;                // packed entries of [J | r]^T [J | r] one thread of it sums per pass, in registers
constexpr int kNfTileMax = 32;           // observation rows it holds in LDS at a time, at most
constexpr size_t kNfLdsSoft = 48 * 1024; // LDS the tile is sized for; a K whose single row passes it asks for more, up to 160 KiB
constexpr size_t kNfLdsHard = 160 * 1024;

struct NfBlock {
  __device__ int tid() const { return (int)threadIdx.x; }
  __device__ int size() const { return (int)blockDim.x; }
  __device__ void sync() const { __syncthreads(); }
};

__device__ inline double nf_lb(const NfProblem& pr, long long row, int k) {
  return pr.lb ? pr.lb[(pr.bounds_batched ? row * pr.K : 0) + k] : -INFINITY;
}
__device__ inline double nf_ub(const NfProblem& pr, long long row, int k) {
  return pr.ub ? pr.ub[(pr.bounds_batched ? row * pr.K : 0) + k] : INFINITY;
}

// x0 != NULL (start of the fit, one item per row): x = x0 with the K fitted entries clipped into the box, mu = mu0, status 0; the first
// workgroups also lay out the residual scales and observations in list order.
// x0 == NULL: the rows of a launch on a subset, contiguous as the integrator takes them: xw[q] = x[rows[q]], y0w[q] = y0[rows[q]].
__global__ void net_fit_gather_kernel(NfProblem pr, long long n, const int32_t* rows, const double* x0, double* xw, double* y0w) {
  const int W = pr.y0_batched && y0w && pr.S > pr.n_var ? pr.S : pr.n_var;
  const long long total = n * W, stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long e = first; e < total; e += stride) {
    const long long q = e / W;
    const int c = (int)(e - q * W);
    const long long row = rows ? rows[q] : q;
    if (c < pr.n_var) {
      if (x0) {
        double v = x0[row * pr.n_var + c];
        const int k = pr.colpos[c];
        if (k >= 0) v = fmin(fmax(v, nf_lb(pr, row, k)), nf_ub(pr, row, k));
        pr.x[row * pr.n_var + c] = v;
        if (c == 0) { pr.mu[row] = kLmMu0; pr.st[row] = 0; }
      } else {
        xw[q * pr.n_var + c] = pr.x[row * pr.n_var + c];
      }
    }
    if (pr.y0_batched && y0w && c < pr.S) y0w[q * pr.S + c] = pr.y0[row * pr.S + c];
  }
  if (x0) {
    for (long long f = first; f < pr.n_obs; f += stride) {
      int m = 0, k = (int)f;
      while (m < 2 && k >= pr.n_mod[m]) { k -= pr.n_mod[m]; ++m; }
      pr.scl[f] = nf_obs_scale(pr.obj_w[m], pr.norm[m], pr.lam[m], pr.w[m][k]);
      pr.obsl[f] = pr.obs[m][k];
    }
  }
}

// One workgroup per active row: A = J^T J and g = J^T r of the scaled residual rows, formed from the tangent launch's pred [k, n_obs] and
// dpred [k, n_obs, K]; then the Marquardt scaling, the free set and the flag (0 go on, 1 done, 2 the launch flagged the candidate: nothing
// of the row is touched but its status).
// The rows of [J | r], K + 1 wide, pass through LDS in tiles (coalesced loads: K contiguous); a thread owns kNfOwn packed entries of the
// Gram matrix per pass and sums each over ALL observation rows in list order, prior rows last, in a register -- so every entry is one
// sequential sum whatever K, the tile height or the batch.  Consecutive threads hold consecutive i of one column j: their reads of a tile
// row are consecutive doubles (one bank row per 32 lanes, no conflict) and the shared operand j is a broadcast.
// LDS: tile [tile_rows, K + 1] | prior derivative [K] | prior residual [K] | gradient [K] | diagonal [K].
__global__ void __launch_bounds__(kNfThreads) net_fit_normal_kernel(NfProblem pr, const int32_t* rows, const double* pred, const double* dpred,
                                                                    const int32_t* status, int tile_rows, int32_t* flags) {
  extern __shared__ double sm[];
  const int K = pr.K, W = K + 1, n_obs = pr.n_obs, tid = (int)threadIdx.x, nt = kNfThreads;
  const long long q = blockIdx.x, row = rows[q];
  if (status[q] != 0) {
    if (tid == 0) { flags[q] = 2; pr.st[row] = status[q]; }
    return;
  }
  double* Jt = sm;
  double* dcol = Jt + (size_t)tile_rows * W;
  double* rcol = dcol + K;
  double* gl = rcol + K;
  double* dg = gl + K;
  const double* xrow = pr.x + row * pr.n_var;
  const double sp = nf_prior_scale(pr.obj_w, pr.lam[3], pr.N);
  for (int k = tid; k < K; k += nt) {
    const int col = pr.cols[k];
    double d = 0.0, r = 0.0;
    if (pr.defaults && nf_prior_col(col, pr.n_K, pr.N, pr.sites)) {
      const double xv = xrow[col], dd = pr.defaults[col];
      r = nf_prior_row(sp, pr.x_is_raw ? nf_softplus(xv) : xv, dd);
      d = nf_prior_drow(sp, dd, pr.x_is_raw ? nf_softplus_prime(xv) : 1.0);
      if (!lm_finite(r)) r = 0.0;
      if (!lm_finite(d)) d = 0.0;
    }
    dcol[k] = d; rcol[k] = r;
  }
  __syncthreads();
  const size_t ne = nf_entries(K);
  const double* prow = pred + q * n_obs;
  const double* drow = dpred + q * (size_t)n_obs * K;
  double* A = pr.A + row * (size_t)K * K;
  for (size_t e0 = 0; e0 < ne; e0 += (size_t)nt * kNfOwn) {
    int ei[kNfOwn], ej[kNfOwn];
    double acc[kNfOwn];
#pragma unroll
    for (int r = 0; r < kNfOwn; ++r) {
      const size_t e = e0 + (size_t)r * nt + tid;
      ei[r] = 0; ej[r] = 0; acc[r] = 0.0;
      if (e < ne) nf_entry(K, e, &ei[r], &ej[r]);
    }
    for (int f0 = 0; f0 < n_obs; f0 += tile_rows) {
      const int nf = n_obs - f0 < tile_rows ? n_obs - f0 : tile_rows;
      __syncthreads();                                                              // the previous tile is spent (first pass: dcol, rcol are written)
      for (int e = tid; e < nf * K; e += nt) {
        const int ff = e / K, i = e - ff * K;
        const double v = pr.scl[f0 + ff] * drow[(size_t)f0 * K + e];
        Jt[ff * W + i] = lm_finite(v) ? v : 0.0;
      }
      for (int ff = tid; ff < nf; ff += nt) {
        const double v = pr.scl[f0 + ff] * (prow[f0 + ff] - pr.obsl[f0 + ff]);
        Jt[ff * W + K] = lm_finite(v) ? v : 0.0;
      }
      __syncthreads();
      for (int ff = 0; ff < nf; ++ff) {
        const double* t = Jt + ff * W;
#pragma unroll
        for (int r = 0; r < kNfOwn; ++r) acc[r] += t[ei[r]] * t[ej[r]];
      }
    }
#pragma unroll
    for (int r = 0; r < kNfOwn; ++r) {
      const size_t e = e0 + (size_t)r * nt + tid;
      if (e >= ne) continue;
      const int i = ei[r], j = ej[r];
      double v = acc[r];
      if (i == j) v += dcol[j] * dcol[j];                                           // prior rows: one entry in column j, after the observations
      else if (i == K) v += rcol[j] * dcol[j];
      if (i == K) { gl[j] = v; pr.g[row * K + j] = v; }
      else {
        A[(size_t)i * K + j] = v;
        A[(size_t)j * K + i] = v;
        if (i == j) dg[j] = v;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < K; i += nt) {
    const bool fixed = lm_fixed(xrow[pr.cols[i]], nf_lb(pr, row, i), nf_ub(pr, row, i), gl[i]);
    pr.DD[row * K + i] = lm_scale(dg[i]);
    pr.is_free[row * K + i] = fixed ? 0 : 1;
    dcol[i] = fixed ? 0.0 : 1.0;
    rcol[i] = fixed ? 0.0 : gl[i];
  }
  __syncthreads();
  if (tid == 0) {
    int n_free = 0;
    double s = 0.0;
    for (int i = 0; i < K; ++i) { n_free += dcol[i] != 0.0; s += rcol[i] * rcol[i]; }
    flags[q] = lm_row_done(n_free, sqrt(s), pr.cost[row]) ? 1 : 0;
    pr.st[row] = 0;
  }
}

// One workgroup per (pending row, damping level): damped system in LDS (packed triangle), factor, solve, project on the box, predicted
// reduction; writes the fitted entries of the trial point, the full trial candidate row for the plain launch (the row's x with K entries
// replaced), its y0 row, and the predicted reduction.
// LDS: triangle | step | dp | work | trial | p | lb | ub | g | DD  [K each] | free mask [K bytes].
__global__ void net_fit_trials_kernel(NfProblem pr, const int32_t* rows, long long m, double* trials, double* predred, double* xw, double* y0w) {
  extern __shared__ double sm[];
  const int K = pr.K, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const long long q = blockIdx.x, row = rows[q];
  const int lv = (int)blockIdx.y;
  const long long slot = lv * m + q;
  double* L = sm;
  double* step = L + lm_tri_len(K);
  double* dp = step + K;
  double* work = dp + K;
  double* trial = work + K;
  double* pl = trial + K;
  double* lbl = pl + K;
  double* ubl = lbl + K;
  double* gl = ubl + K;
  double* DDl = gl + K;
  unsigned char* fr = reinterpret_cast<unsigned char*>(DDl + K);
  const double* xrow = pr.x + row * pr.n_var;
  for (int i = tid; i < K; i += nt) {
    pl[i] = xrow[pr.cols[i]]; lbl[i] = nf_lb(pr, row, i); ubl[i] = nf_ub(pr, row, i);
    gl[i] = pr.g[row * K + i]; DDl[i] = pr.DD[row * K + i]; fr[i] = pr.is_free[row * K + i];
  }
  __syncthreads();
  const double* A = pr.A + row * (size_t)K * K;
  const NfBlock team;
  lm_damped_step(K, A, K, fr, DDl, gl, pr.mu[row], lv, L, step, team);
  lm_project(K, pl, lbl, ubl, step, trial, dp, team);
  const double pd = lm_predicted(K, A, K, gl, dp, work, team);
  double* out = xw + slot * pr.n_var;
  for (int c = tid; c < pr.n_var; c += nt) {
    const int k = pr.colpos[c];
    out[c] = k >= 0 ? trial[k] : xrow[c];
  }
  for (int i = tid; i < K; i += nt) trials[slot * K + i] = trial[i];
  if (pr.y0_batched) for (int s = tid; s < pr.S; s += nt) y0w[slot * pr.S + s] = pr.y0[row * pr.S + s];
  if (tid == 0) predred[slot] = pd;
}

// One workgroup per pending row: the costs 1/2 obj_w . F of its L trial launches (Fw [L m, 3], their status beside them), the first
// acceptable level -- a flagged trial never is --, and the update of x, cost, F, mu and the row's status.  flags[q]: bit 0 accepted,
// bit 1 converged, bit 2 still pending.
// init != 0: L = 1, the launch scored the row's start point, which is taken unconditionally.
__global__ void net_fit_accept_kernel(NfProblem pr, const int32_t* rows, long long m, int L, const double* Fw, const int32_t* stw,
                                      const double* trials, const double* predred, int init, int32_t* flags) {
  __shared__ int sel_s;
  const int K = pr.K, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const long long q = blockIdx.x, row = rows ? rows[q] : q;
  double* xrow = pr.x + row * pr.n_var;
  if (tid == 0) {
    int sel = -1, conv = 0, so = 0;
    double cn = 0.0;
    if (init) {
      sel = 0; so = stw[q]; cn = nf_cost(Fw + 3 * q, pr.obj_w);
    } else {
      const double cost = pr.cost[row];
      double rho = -1.0;
      for (int lv = 0; lv < L && sel < 0; ++lv) {
        const long long slot = lv * m + q;
        so |= stw[slot];
        cn = nf_cost(Fw + 3 * slot, pr.obj_w);
        rho = lm_rho(cost, cn, predred[slot]);
        if (stw[slot] == 0 && lm_acceptable(cost, cn, rho)) sel = lv;
      }
      if (sel >= 0) {
        const double* t = trials + (sel * m + q) * K;
        double dx2 = 0.0, xn2 = 0.0;
        for (int i = 0; i < K; ++i) { const double d = t[i] - xrow[pr.cols[i]]; dx2 += d * d; xn2 += t[i] * t[i]; }
        conv = lm_converged(cost - cn, cn, sqrt(dx2), sqrt(xn2), pr.ftol, pr.xtol) ? 1 : 0;
        pr.mu[row] = lm_mu_accept(pr.mu[row], sel, rho);
      } else {
        pr.mu[row] = lm_mu_reject(pr.mu[row], L);
      }
    }
    if (sel >= 0) {
      const long long slot = sel * m + q;
      pr.cost[row] = cn;
      for (int k = 0; k < 3; ++k) pr.F[3 * row + k] = Fw[3 * slot + k];
    }
    pr.st[row] = init ? so : (pr.st[row] | so);
    if (flags) flags[q] = (sel >= 0 ? 1 : 0) | (conv ? 2 : 0) | (sel < 0 ? 4 : 0);
    sel_s = sel;
  }
  __syncthreads();
  const int sel = sel_s;
  if (sel >= 0 && !init) {
    const double* t = trials + (sel * m + q) * K;
    for (int i = tid; i < K; i += nt) xrow[pr.cols[i]] = t[i];
  }
}

namespace {

int nf_tile_rows(int K) {
  const long long room = (long long)(kNfLdsSoft / sizeof(double)) - 4ll * K;
  const long long r = room / (K + 1);
  return (int)std::max<long long>(1, std::min<long long>(kNfTileMax, r));
}
size_t nf_normal_lds(int K, int tile_rows) { return ((size_t)tile_rows * (K + 1) + 4 * (size_t)K) * sizeof(double); }
size_t nf_trials_lds(int K) { return (lm_tri_len(K) + 9 * (size_t)K) * sizeof(double) + (size_t)K; }
int nf_trials_threads(int K) { const int w = (K + 63) / 64 * 64; return w < 256 ? w : 256; }

// carve 256-byte aligned pieces out of one block
struct Carver {
  char* base; size_t off = 0;
  template <class T> T* take(size_t n) { T* p = base ? reinterpret_cast<T*>(base + off) : nullptr; off += (n * sizeof(T) + 255) / 256 * 256; return p; }
};

struct LockGuard {
  pk_ctx* c;
  explicit LockGuard(pk_ctx* ctx) : c(ctx) { pk_ctx_lock(c); }
  ~LockGuard() { pk_ctx_unlock(c); }
};

}  // namespace
}  // namespace pk

#define PK_NF_HIP(ctx, call)                                                                                    \
  do {                                                                                                          \
    hipError_t e_ = (call);                                                                                     \
    if (e_ != hipSuccess) return pk_ctx_fail(ctx, PK_ERR_HIP, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); \
  } while (0)

extern "C" {

int pk_network_fit_batch(pk_ctx* c, pk_net* n, pk_loss* l, int64_t B, const double* x0, int x_is_raw, const double* y0, int y0_is_batched,
                         const double* t_host, int T, const pk_solver_opts* opts_in, const int32_t* cols_host, int K, const double* defaults,
                         const double* lambdas, const double* obj_w, const double* lb, const double* ub, int bounds_are_batched,
                         const pk_fit_opts* fit_in, double fail_value, double* x, double* cost, double* F, double* JTJ, int32_t* reason,
                         int32_t* status, int64_t counters[6]) {
  using namespace pk;
  if (!c || !n || !l) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (T < 1 || !t_host) return pk_ctx_fail(c, PK_ERR_ARG, "t must hold >= 1 time points (host pointer)");
  const NetDev& nd = *pk_net_dev(n);
  if (K < 1) return pk_ctx_fail(c, PK_ERR_ARG, "K must be >= 1: the fit needs at least one column");
  if (K > nd.n_var) return pk_ctx_fail(c, PK_ERR_ARG, "K must be <= n_var");
  if (!cols_host) return pk_ctx_fail(c, PK_ERR_ARG, "cols is NULL");
  std::vector<int32_t> colpos((size_t)nd.n_var, -1);
  for (int k = 0; k < K; ++k) {
    const int col = cols_host[k];
    if (col < 0 || col >= nd.n_var) return pk_ctx_fail(c, PK_ERR_ARG, "cols: index outside [0, n_var)");
    if (colpos[col] >= 0) return pk_ctx_fail(c, PK_ERR_ARG, "cols: an index is repeated");
    colpos[col] = k;
  }
  pk_fit_opts fo;
  if (fit_in) fo = *fit_in; else pk_default_fit_opts(&fo);
  if (fo.trial_levels < 0 || fo.trial_levels > kLmMaxTries) return pk_ctx_fail(c, PK_ERR_ARG, "trial_levels must be 0 (auto) .. 12");
  if (fo.max_iter < 0) return pk_ctx_fail(c, PK_ERR_ARG, "max_iter must be >= 0");
  if (fo.log_space || fo.use_reg) return pk_ctx_fail(c, PK_ERR_ARG, "the network fit has neither log_space nor use_reg: leave both 0");
  if (!lambdas || !obj_w) return pk_ctx_fail(c, PK_ERR_ARG, "lambdas [4] and obj_w [3] (host pointers) are required");
  for (int m = 0; m < 3; ++m) if (!(obj_w[m] >= 0.0)) return pk_ctx_fail(c, PK_ERR_ARG, "obj_w must be >= 0");
  if ((lb == nullptr) != (ub == nullptr)) return pk_ctx_fail(c, PK_ERR_ARG, "lb and ub: pass both, or NULL for both (no box)");
  if (counters) for (int i = 0; i < 6; ++i) counters[i] = 0;
  if (B == 0) return PK_OK;
  if (!x0 || !y0 || !x || !cost || !F || !counters) return pk_ctx_fail(c, PK_ERR_ARG, "x0, y0, x, cost, F and counters must be non-null");
  if (B > 0x7fffffffLL / kLmMaxTries) return pk_ctx_fail(c, PK_ERR_ARG, "batch too large for one launch");

  NfProblem pr{};
  int Tl = 0;
  if (!pk_loss_fit_view(l, pr.n_mod, pr.obs, pr.w, pr.norm, &Tl)) return pk_ctx_fail(c, PK_ERR_ARG, "bad loss handle");
  if (Tl != T) return pk_ctx_fail(c, PK_ERR_ARG, "T differs from the grid the loss data were created for");
  const int n_obs = pr.n_mod[0] + pr.n_mod[1] + pr.n_mod[2], n_var = nd.n_var, S = nd.S;
  const int tile_rows = nf_tile_rows(K);
  const size_t lds_n = nf_normal_lds(K, tile_rows), lds_t = nf_trials_lds(K);
  if (lds_n > kNfLdsHard || lds_t > kNfLdsHard)
    return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "fit: K is beyond what one workgroup of the trial kernel holds in LDS (K (K + 1) / 2 + 9 K doubles within 160 KiB)");

  // rows of one Jacobian launch: dpred of a chunk stays within 1 GiB
  const int64_t per_row = (int64_t)std::max(n_obs, 1) * K * 8;
  const int64_t kc_max = std::max<int64_t>(1, std::min<int64_t>(B, (1ll << 30) / per_row));
  const int64_t KM = fo.trial_levels > 0 ? (int64_t)fo.trial_levels * B : std::max<int64_t>(B, 3 * std::min<int64_t>(B, 256));
  const int64_t NW = std::max(B, KM);

  LockGuard guard(c);                       // the fit arena and its page-locked buffer are this call's until it returns
  char* dev_base = nullptr;
  char* pin_base = nullptr;
  double *xw = nullptr, *y0w = nullptr, *Fw = nullptr, *pred_w = nullptr, *dpred_w = nullptr, *trials_w = nullptr, *predred_w = nullptr;
  int32_t *status_w = nullptr, *rows_d = nullptr, *flags_d = nullptr, *cols_d = nullptr, *colpos_d = nullptr;
  int rc = PK_OK;
  for (int pass = 0; pass < 2; ++pass) {    // first pass measures, second carves
    Carver cv{dev_base};
    pr.mu = cv.take<double>(B); pr.g = cv.take<double>(B * K); pr.DD = cv.take<double>(B * K); pr.is_free = cv.take<unsigned char>(B * K);
    pr.st = status ? status : cv.take<int32_t>(B);
    pr.A = JTJ ? JTJ : cv.take<double>((size_t)B * K * K);
    pr.scl = cv.take<double>(n_obs); pr.obsl = cv.take<double>(n_obs);
    cols_d = cv.take<int32_t>(K); colpos_d = cv.take<int32_t>(n_var);
    rows_d = cv.take<int32_t>(B); flags_d = cv.take<int32_t>(B); status_w = cv.take<int32_t>(NW);
    xw = cv.take<double>((size_t)NW * n_var);
    y0w = y0_is_batched ? cv.take<double>((size_t)NW * S) : nullptr;
    Fw = cv.take<double>((size_t)NW * 3);
    pred_w = cv.take<double>((size_t)kc_max * n_obs); dpred_w = cv.take<double>((size_t)kc_max * n_obs * K);
    trials_w = cv.take<double>((size_t)KM * K); predred_w = cv.take<double>(KM);
    if (pass == 0) {
      void *d = nullptr, *h = nullptr;
      if ((rc = pk_ctx_fit_reserve(c, cv.off, (2 * (size_t)B + K + n_var) * sizeof(int32_t), &d, &h))) return rc;
      dev_base = static_cast<char*>(d); pin_base = static_cast<char*>(h);
    }
  }
  int32_t* rows_h = reinterpret_cast<int32_t*>(pin_base);
  int32_t* flags_h = rows_h + B;
  int32_t* cols_h = flags_h + B;
  pr.n_var = n_var; pr.S = S; pr.K = K; pr.n_obs = n_obs; pr.N = nd.N; pr.n_K = nd.n_K; pr.sites = nd.sites;
  pr.x_is_raw = x_is_raw ? 1 : 0; pr.y0_batched = y0_is_batched ? 1 : 0; pr.bounds_batched = bounds_are_batched ? 1 : 0;
  for (int m = 0; m < 3; ++m) pr.obj_w[m] = obj_w[m];
  for (int m = 0; m < 4; ++m) pr.lam[m] = lambdas[m];
  pr.y0 = y0; pr.defaults = defaults; pr.lb = lb; pr.ub = ub; pr.cols = cols_d; pr.colpos = colpos_d;
  pr.x = x; pr.cost = cost; pr.F = F; pr.ftol = fo.ftol; pr.xtol = fo.xtol;

  PK_NF_HIP(c, hipSetDevice(pk_ctx_device(c)));
  hipStream_t stream = (hipStream_t)pk_ctx_stream(c);
  if (lds_n > 48 * 1024) PK_NF_HIP(c, hipFuncSetAttribute((const void*)net_fit_normal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_n));
  if (lds_t > 48 * 1024) PK_NF_HIP(c, hipFuncSetAttribute((const void*)net_fit_trials_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_t));
  std::memcpy(cols_h, cols_host, (size_t)K * sizeof(int32_t));
  std::memcpy(cols_h + K, colpos.data(), (size_t)n_var * sizeof(int32_t));
  PK_NF_HIP(c, hipMemcpyAsync(cols_d, cols_h, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  PK_NF_HIP(c, hipMemcpyAsync(colpos_d, cols_h + K, (size_t)n_var * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  const double* y0_solve = y0_is_batched ? y0w : y0;
  const auto gather_grid = [&](int64_t rows_n) { return dim3((unsigned)std::min<int64_t>((rows_n * std::max(n_var, S) + 255) / 256, 65535)); };
  // the plain launch: the order-3 fused objective on the route the tangent launch takes for these options (no columns)
  const auto plain = [&](int64_t M, const double* xs, const double* ys) {
    return pk_network_simulate_objective_grad_batch(c, n, l, M, xs, x_is_raw, ys, y0_is_batched, t_host, T, opts_in, nullptr, 0, 0, defaults, lambdas,
                                                    fail_value, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, Fw, nullptr, status_w, nullptr);
  };

  // start values: x = x0 with the fitted entries clipped, mu = mu0; one plain launch scores every row
  hipLaunchKernelGGL(net_fit_gather_kernel, gather_grid(B), dim3(256), 0, stream, pr, (long long)B, (const int32_t*)nullptr, x0, (double*)nullptr, (double*)nullptr);
  if ((rc = plain(B, x, y0))) return rc;
  hipLaunchKernelGGL(net_fit_accept_kernel, dim3((unsigned)B), dim3(64), 0, stream, pr, (const int32_t*)nullptr, (long long)B, 1, (const double*)Fw,
                     (const int32_t*)status_w, (const double*)nullptr, (const double*)nullptr, 1, (int32_t*)nullptr);
  PK_NF_HIP(c, hipGetLastError());
  counters[1] += B; counters[2] += 3;

  std::vector<unsigned char> active((size_t)B, 1);
  std::vector<int32_t> why((size_t)B, 3), idx, pend, next;
  for (int64_t it = 1; it <= fo.max_iter; ++it) {
    idx.clear();
    for (int64_t k = 0; k < B; ++k) if (active[k]) idx.push_back((int32_t)k);
    if (idx.empty()) break;
    counters[0] = it;
    // Jacobian phase: gather, tangent launch, normal equations -- per chunk of rows; ONE wait for the flags
    const int64_t k = (int64_t)idx.size();
    std::memcpy(rows_h, idx.data(), k * sizeof(int32_t));
    PK_NF_HIP(c, hipMemcpyAsync(rows_d, rows_h, k * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    for (int64_t c0 = 0; c0 < k; c0 += kc_max) {
      const int64_t kc = std::min(kc_max, k - c0);
      hipLaunchKernelGGL(net_fit_gather_kernel, gather_grid(kc), dim3(256), 0, stream, pr, (long long)kc, (const int32_t*)(rows_d + c0), (const double*)nullptr, xw, y0w);
      if ((rc = pk_network_simulate_objective_grad_batch(c, n, l, kc, xw, x_is_raw, y0_solve, y0_is_batched, t_host, T, opts_in, cols_host, K, 0, defaults,
                                                         lambdas, fail_value, nullptr, nullptr, pred_w, dpred_w, nullptr, nullptr, nullptr, nullptr,
                                                         status_w, nullptr)))
        return rc;
      hipLaunchKernelGGL(net_fit_normal_kernel, dim3((unsigned)kc), dim3(kNfThreads), lds_n, stream, pr, (const int32_t*)(rows_d + c0), (const double*)pred_w,
                         (const double*)dpred_w, (const int32_t*)status_w, tile_rows, flags_d + c0);
      PK_NF_HIP(c, hipGetLastError());
      counters[2] += 3;
    }
    PK_NF_HIP(c, hipMemcpyAsync(flags_h, flags_d, k * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    PK_NF_HIP(c, hipStreamSynchronize(stream));
    counters[1] += k; counters[3] += 1; counters[4] += 1;
    pend.clear();
    for (int64_t j = 0; j < k; ++j) {
      if (flags_h[j]) { active[idx[j]] = 0; why[idx[j]] = flags_h[j] == 2 ? 4 : 1; }
      else pend.push_back(idx[j]);
    }
    // trial rounds: damped steps of L levels, one plain launch on levels x pending rows, the accept rule; ONE wait for the flags
    int tries = 0;
    while (tries < kLmMaxTries && !pend.empty()) {
      const int64_t m = (int64_t)pend.size();
      const int L = lm_round_levels(fo.trial_levels, m, tries);
      tries += L;
      std::memcpy(rows_h, pend.data(), m * sizeof(int32_t));
      PK_NF_HIP(c, hipMemcpyAsync(rows_d, rows_h, m * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(net_fit_trials_kernel, dim3((unsigned)m, (unsigned)L), dim3(nf_trials_threads(K)), lds_t, stream, pr, (const int32_t*)rows_d, (long long)m,
                         trials_w, predred_w, xw, y0w);
      if ((rc = plain(L * m, xw, y0_solve))) return rc;
      hipLaunchKernelGGL(net_fit_accept_kernel, dim3((unsigned)m), dim3(64), 0, stream, pr, (const int32_t*)rows_d, (long long)m, L, (const double*)Fw,
                         (const int32_t*)status_w, (const double*)trials_w, (const double*)predred_w, 0, flags_d);
      PK_NF_HIP(c, hipGetLastError());
      PK_NF_HIP(c, hipMemcpyAsync(flags_h, flags_d, m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      PK_NF_HIP(c, hipStreamSynchronize(stream));
      counters[1] += L * m; counters[2] += 3; counters[3] += 1; counters[5] += 1;
      next.clear();
      for (int64_t j = 0; j < m; ++j) {
        if (flags_h[j] & 2) { active[pend[j]] = 0; why[pend[j]] = 0; }
        if (flags_h[j] & 4) next.push_back(pend[j]);
      }
      pend.swap(next);
    }
    for (int32_t k2 : pend) { active[k2] = 0; why[k2] = 2; }      // no acceptable step within the damping budget: stalled
  }
  if (reason) {
    // the reasons go up through the page-locked buffer; the copy is waited for because `why` dies with this call
    std::memcpy(rows_h, why.data(), B * sizeof(int32_t));
    PK_NF_HIP(c, hipMemcpyAsync(reason, rows_h, B * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  PK_NF_HIP(c, hipStreamSynchronize(stream));      // the column lists of the last launches live in this call's buffers
  return PK_OK;
}

}  // extern "C"
