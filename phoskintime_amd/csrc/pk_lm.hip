// pk_lm.hip -- pk_fit_protein_rows_batch: the bounded Levenberg-Marquardt fit of paramest/multistart.py::fit_rows_batch (jacobian="sens")
// with its whole state in HBM.  The solves are the library's own entry points (pk_solve_protein_batch, pk_solve_protein_sens_batch); the four
// small kernels here do the algebra between them with the per-row rules of pk_lm.hpp.  Every sum of every kernel is taken by one thread in
// ascending index order (or as fixed partial sums of a fixed workgroup size): a row's iterates depend on its own data only.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/phoskin.h"
#include "pk_lm.hpp"

extern "C" int pk_ctx_device(pk_ctx*);
extern "C" void* pk_ctx_stream(pk_ctx*);
extern "C" int pk_ctx_fail(pk_ctx*, int code, const char* msg);
extern "C" void pk_ctx_lock(pk_ctx*);
extern "C" void pk_ctx_unlock(pk_ctx*);
extern "C" int pk_ctx_fit_reserve(pk_ctx*, size_t dev_bytes, size_t pin_bytes, void** dev, void** pin);

namespace pk {

// What every kernel of one fit sees: the caller's arrays, the per-row state and the shapes.  Passed by value.
struct LmProblem {
  int P, S, F, Nr, log_space, use_reg, y0_batched, target_batched, sigma_batched, bounds_batched;
  const double *y0, *target, *sigma, *lam, *lb, *ub;
  double *p, *cost, *r, *A, *mu, *g, *DD;
  unsigned char* is_free;
  double ftol, xtol;
};

constexpr int kLmThreads = 256;          // workgroup of lm_normal_kernel and lm_accept_kernel: their partial sums are cut by it
constexpr int kLmTile = 32;              // rows of the weighted Jacobian lm_normal_kernel holds in LDS at a time
constexpr int kLmMaxP = kLmThreads;      // one thread per gradient entry in lm_normal_kernel

struct LmBlock {
  __device__ int tid() const { return (int)threadIdx.x; }
  __device__ int size() const { return (int)blockDim.x; }
  __device__ void sync() const { __syncthreads(); }
};

__device__ inline double lm_isig(const LmProblem& pr, long long row, int f) {
  return pr.sigma ? 1.0 / pr.sigma[(pr.sigma_batched ? row * pr.Nr : 0) + f] : 1.0;
}

// Entry f of the weighted residual of `row` at the point x (fitted space) whose solve wrote flat: data rows, then the ridge rows
// (lam / P) x^2 against 0.  A non-finite residual is very bad, not fatal.
__device__ inline double lm_residual(const LmProblem& pr, long long row, const double* flat, const double* x, int f) {
  double rr;
  if (f < pr.F) {
    rr = (flat[f] - pr.target[(pr.target_batched ? row * pr.F : 0) + f]) * lm_isig(pr, row, f);
  } else {
    const double xv = x[f - pr.F];
    rr = ((pr.lam ? pr.lam[row] / pr.P : 0.0) * xv * xv) * lm_isig(pr, row, f);
  }
  return lm_finite(rr) ? rr : 1e6;
}

// theta (exp of the fitted point under log_space) and the y0 rows of n = levels * m solves, contiguous as the solve entry points take them:
// solve q belongs to problem rows[q % m] (rows == NULL: problem q % m).  src_by_row: the point is src[problem], else src[q].
// With p_out the point is first clipped into the box and stored as the problem's start value, with the first damping value beside it.
__global__ void lm_gather_kernel(LmProblem pr, long long n, long long m, const int32_t* rows, const double* src, int src_by_row,
                                 double* p_out, double* theta, double* y0_out) {
  const int W = pr.y0_batched && pr.S > pr.P ? pr.S : pr.P;
  const long long total = n * W;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long q = e / W;
    const int c = (int)(e - q * W);
    const long long row = rows ? rows[q % m] : q % m;
    if (c < pr.P) {
      double x = src[(src_by_row ? row : q) * pr.P + c];
      if (p_out) {
        const long long b = (pr.bounds_batched ? row * pr.P : 0) + c;
        x = fmin(fmax(x, pr.lb[b]), pr.ub[b]);
        p_out[row * pr.P + c] = x;
        if (c == 0) pr.mu[row] = kLmMu0;
      }
      theta[q * pr.P + c] = pr.log_space ? exp(x) : x;
    }
    if (pr.y0_batched && c < pr.S) y0_out[q * pr.S + c] = pr.y0[row * pr.S + c];
  }
}

// One workgroup per active row: J^T J and J^T r of the weighted Jacobian, formed in flight from the sensitivity launch's dflat [k, F, P]
// (tiles of kLmTile rows pass through LDS once), the Marquardt scaling, the free set and the done flag.
// LDS: packed triangle of accumulators | tile [kLmTile, P] | r tile [kLmTile] | column weights [P] | gradient [P].
__global__ void __launch_bounds__(kLmThreads) lm_normal_kernel(LmProblem pr, const int32_t* rows, const double* dflat, int32_t* done) {
  extern __shared__ double sm[];
  const int P = pr.P, F = pr.F, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const long long q = blockIdx.x, row = rows[q];
  const int ntri = (int)lm_tri_len(P);
  double* acc = sm;
  double* Jt = acc + ntri;
  double* rt = Jt + kLmTile * P;
  double* w = rt + kLmTile;
  double* gl = w + P;
  const double* prow = pr.p + row * P;
  const double* rrow = pr.r + row * pr.Nr;
  for (int e = tid; e < ntri; e += nt) acc[e] = 0.0;
  for (int i = tid; i < P; i += nt) w[i] = pr.log_space ? exp(prow[i]) : 1.0;       // chain rule of theta = exp(p)
  double g_acc = 0.0;
  __syncthreads();
  for (int f0 = 0; f0 < F; f0 += kLmTile) {
    const int nf = F - f0 < kLmTile ? F - f0 : kLmTile;
    for (int e = tid; e < nf * P; e += nt) {
      const int ff = e / P, i = e - ff * P;
      double v = dflat[(q * F + f0 + ff) * P + i];
      if (pr.log_space) v *= w[i];
      v *= lm_isig(pr, row, f0 + ff);
      Jt[e] = lm_finite(v) ? v : 0.0;                                               // a failed solve contributes no direction
    }
    for (int ff = tid; ff < nf; ff += nt) rt[ff] = rrow[f0 + ff];
    __syncthreads();
    for (int j = 0, o = tid; j < P; o += nt) {                                      // packed entries tid, tid + nt, ...: (i, j) = (j + o, j)
      while (j < P && o >= P - j) { o -= P - j; ++j; }
      if (j >= P) break;
      const int i = j + o;
      double s = acc[lm_tri(P, i, j)];
      for (int ff = 0; ff < nf; ++ff) s += Jt[ff * P + i] * Jt[ff * P + j];
      acc[lm_tri(P, i, j)] = s;
    }
    if (tid < P) for (int ff = 0; ff < nf; ++ff) g_acc += Jt[ff * P + tid] * rt[ff];
    __syncthreads();
  }
  if (pr.use_reg && tid < P) {                                                      // ridge rows diag(2 (lam / P) p / sigma): after the data rows
    double d = 2.0 * (pr.lam ? pr.lam[row] / P : 0.0) * prow[tid] * lm_isig(pr, row, F + tid);
    if (!lm_finite(d)) d = 0.0;
    acc[lm_tri(P, tid, tid)] += d * d;
    g_acc += d * rrow[F + tid];
  }
  __syncthreads();
  double* A = pr.A + row * P * P;
  for (int j = 0, o = tid; j < P; o += nt) {
    while (j < P && o >= P - j) { o -= P - j; ++j; }
    if (j >= P) break;
    const int i = j + o;
    const double v = acc[lm_tri(P, i, j)];
    A[(size_t)i * P + j] = v;
    A[(size_t)j * P + i] = v;
  }
  if (tid < P) {
    const long long b = (pr.bounds_batched ? row * P : 0) + tid;
    const bool fixed = lm_fixed(prow[tid], pr.lb[b], pr.ub[b], g_acc);
    pr.g[row * P + tid] = g_acc;
    pr.DD[row * P + tid] = lm_scale(acc[lm_tri(P, tid, tid)]);
    pr.is_free[row * P + tid] = fixed ? 0 : 1;
    gl[tid] = fixed ? 0.0 : g_acc;
    w[tid] = fixed ? 0.0 : 1.0;
  }
  __syncthreads();
  if (tid == 0) {
    int n_free = 0;
    double s = 0.0;
    for (int i = 0; i < P; ++i) { n_free += w[i] != 0.0; s += gl[i] * gl[i]; }
    done[q] = lm_row_done(n_free, sqrt(s), pr.cost[row]) ? 1 : 0;
  }
}

// One workgroup per (pending row, damping level): damped system in LDS (packed triangle), factor, solve, project on the box, predicted
// reduction; writes the trial point, its theta and y0 row for the trial solve, and the predicted reduction.
// LDS: triangle | step | dp | work | trial | p | lb | ub | g | DD  [P each] | free mask [P bytes].
__global__ void lm_trials_kernel(LmProblem pr, const int32_t* rows, long long m, double* trials, double* pred, double* theta, double* y0_out) {
  extern __shared__ double sm[];
  const int P = pr.P, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const long long q = blockIdx.x, row = rows[q];
  const int lv = (int)blockIdx.y;
  const long long slot = lv * m + q;
  double* L = sm;
  double* step = L + lm_tri_len(P);
  double* dp = step + P;
  double* work = dp + P;
  double* trial = work + P;
  double* pl = trial + P;
  double* lbl = pl + P;
  double* ubl = lbl + P;
  double* gl = ubl + P;
  double* DDl = gl + P;
  unsigned char* fr = reinterpret_cast<unsigned char*>(DDl + P);
  for (int i = tid; i < P; i += nt) {
    const long long b = (pr.bounds_batched ? row * P : 0) + i;
    pl[i] = pr.p[row * P + i]; lbl[i] = pr.lb[b]; ubl[i] = pr.ub[b];
    gl[i] = pr.g[row * P + i]; DDl[i] = pr.DD[row * P + i]; fr[i] = pr.is_free[row * P + i];
  }
  __syncthreads();
  const double* A = pr.A + row * P * P;
  const LmBlock team;
  lm_damped_step(P, A, P, fr, DDl, gl, pr.mu[row], lv, L, step, team);
  lm_project(P, pl, lbl, ubl, step, trial, dp, team);
  const double pd = lm_predicted(P, A, P, gl, dp, work, team);
  for (int i = tid; i < P; i += nt) {
    trials[slot * P + i] = trial[i];
    theta[slot * P + i] = pr.log_space ? exp(trial[i]) : trial[i];
  }
  if (pr.y0_batched) for (int s = tid; s < pr.S; s += nt) y0_out[slot * pr.S + s] = pr.y0[row * pr.S + s];
  if (tid == 0) pred[slot] = pd;
}

// One workgroup per pending row: residuals and costs of its K trial solves (flat [K m, F]), the first acceptable level, and the update
// of p, cost, r and mu.  flags[q]: bit 0 accepted, bit 1 converged, bit 2 still pending.
// init != 0: K = 1, the point is the row's start value and is taken unconditionally (the initial residuals).
__global__ void __launch_bounds__(kLmThreads) lm_accept_kernel(LmProblem pr, const int32_t* rows, long long m, int K, const double* flat,
                                                                 const double* trials, const double* pred, int init, int32_t* flags) {
  __shared__ double part[kLmThreads];
  __shared__ double cn[kLmMaxTries];
  __shared__ int sel_s, conv_s;
  const int P = pr.P, Nr = pr.Nr, tid = (int)threadIdx.x;
  const long long q = blockIdx.x, row = rows ? rows[q] : q;
  double* prow = pr.p + row * P;
  for (int lv = 0; lv < K; ++lv) {
    const long long slot = lv * m + q;
    const double* x = init ? prow : trials + slot * P;
    double s = 0.0;
    for (int f = tid; f < Nr; f += kLmThreads) { const double rr = lm_residual(pr, row, flat + slot * pr.F, x, f); s += rr * rr; }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int i = 0; i < kLmThreads; ++i) t += part[i];
      cn[lv] = 0.5 * t;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int sel = -1, conv = 0;
    if (init) {
      sel = 0;
    } else {
      const double cost = pr.cost[row];
      double rho = -1.0;
      for (int lv = 0; lv < K && sel < 0; ++lv) {
        rho = lm_rho(cost, cn[lv], pred[lv * m + q]);
        if (lm_acceptable(cost, cn[lv], rho)) sel = lv;
      }
      if (sel >= 0) {
        const double* x = trials + (sel * m + q) * P;
        double dx2 = 0.0, xn2 = 0.0;
        for (int i = 0; i < P; ++i) { const double d = x[i] - prow[i]; dx2 += d * d; xn2 += x[i] * x[i]; }
        conv = lm_converged(cost - cn[sel], cn[sel], sqrt(dx2), sqrt(xn2), pr.ftol, pr.xtol) ? 1 : 0;
        pr.mu[row] = lm_mu_accept(pr.mu[row], sel, rho);
      } else {
        pr.mu[row] = lm_mu_reject(pr.mu[row], K);
      }
    }
    if (sel >= 0) pr.cost[row] = cn[sel];
    sel_s = sel; conv_s = conv;
  }
  __syncthreads();
  const int sel = sel_s;
  if (sel >= 0) {
    const long long slot = sel * m + q;
    const double* x = init ? prow : trials + slot * P;
    for (int f = tid; f < Nr; f += kLmThreads) pr.r[row * Nr + f] = lm_residual(pr, row, flat + slot * pr.F, x, f);
    __syncthreads();                                                                // the ridge residuals above read the point
    if (!init) for (int i = tid; i < P; i += kLmThreads) prow[i] = x[i];
  }
  if (tid == 0 && flags) flags[q] = (sel >= 0 ? 1 : 0) | (conv_s ? 2 : 0) | (sel < 0 ? 4 : 0);
}

namespace {

size_t lm_normal_lds(int P) { return (lm_tri_len(P) + (size_t)kLmTile * P + kLmTile + 2 * (size_t)P) * sizeof(double); }
size_t lm_trials_lds(int P) { return (lm_tri_len(P) + 9 * (size_t)P) * sizeof(double) + (size_t)P; }
int lm_trials_threads(int P) { const int w = (P + 63) / 64 * 64; return w < kLmThreads ? w : kLmThreads; }

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

#define PK_LM_HIP(ctx, call)                                                                                    \
  do {                                                                                                          \
    hipError_t e_ = (call);                                                                                     \
    if (e_ != hipSuccess) return pk_ctx_fail(ctx, PK_ERR_HIP, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); \
  } while (0)

extern "C" {

void pk_default_fit_opts(pk_fit_opts* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_iter = 100;
  o->trial_levels = 0;
  o->log_space = 0;
  o->use_reg = 0;
  o->ftol = 1e-10;
  o->xtol = 1e-10;
}

int pk_fit_protein_rows_batch(pk_ctx* c, int model, int n_sites, int64_t R, const double* P0, const double* y0, int y0_is_batched,
                              const double* t, int T, const double* target, int target_is_batched, const double* sigma, int sigma_is_batched,
                              const double* lam, const double* lb, const double* ub, int bounds_are_batched, const pk_solver_opts* opts_in,
                              const pk_fit_opts* fit_in, double* p, double* cost, double* r, double* JTJ, int32_t* reason, int64_t counters[6]) {
  using namespace pk;
  if (!c) return PK_ERR_ARG;
  if (R < 0) return pk_ctx_fail(c, PK_ERR_ARG, "R must be >= 0");
  if (T < 1) return pk_ctx_fail(c, PK_ERR_ARG, "T must be >= 1");
  // model, size and the sizes without a sensitivity kernel: the sensitivity entry point's own answers (an empty batch launches nothing)
  int rc = pk_solve_protein_sens_batch(c, model, n_sites, 0, nullptr, nullptr, 0, nullptr, T, opts_in, nullptr, nullptr, nullptr, nullptr);
  if (rc) return rc;
  pk_fit_opts fo;
  if (fit_in) fo = *fit_in; else pk_default_fit_opts(&fo);
  if (fo.trial_levels < 0 || fo.trial_levels > kLmMaxTries) return pk_ctx_fail(c, PK_ERR_ARG, "trial_levels must be 0 (auto) .. 12");
  if (fo.max_iter < 0) return pk_ctx_fail(c, PK_ERR_ARG, "max_iter must be >= 0");
  pk_solver_opts so;
  if (opts_in) so = *opts_in; else pk_default_opts(&so);
  if (so.method != PK_METHOD_LRP12 || so.stage_form)
    return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "forward sensitivities integrate with method LRP12 (the default) only");
  if (counters) for (int i = 0; i < 6; ++i) counters[i] = 0;
  if (R == 0) return PK_OK;
  if (!P0 || !y0 || !t || !target || !lb || !ub || !p || !cost || !counters)
    return pk_ctx_fail(c, PK_ERR_ARG, "P0, y0, t, target, lb, ub, p, cost and counters must be non-null");
  if (fo.use_reg && !lam) return pk_ctx_fail(c, PK_ERR_ARG, "use_reg needs lam");
  if (R > 0x7fffffffLL / kLmMaxTries) return pk_ctx_fail(c, PK_ERR_ARG, "batch too large for one launch");

  const int P = pk_protein_n_params(model, n_sites), S = pk_protein_n_states(model, n_sites), F = pk_protein_flat_len(model, n_sites, T);
  if (P < 1 || P > kLmMaxP) return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "fit: more parameters than one workgroup of the normal-equations kernel holds");
  const int Nr = F + (fo.use_reg ? P : 0);
  // rows of one Jacobian launch: dflat of a chunk stays within 1 GiB
  const int64_t per_row = (int64_t)F * P * 8;
  const int64_t kc_max = std::max<int64_t>(1, std::min<int64_t>(R, (1ll << 30) / std::max<int64_t>(per_row, 1)));
  const int64_t KM = fo.trial_levels > 0 ? (int64_t)fo.trial_levels * R : std::max<int64_t>(R, 3 * std::min<int64_t>(R, 256));
  const int64_t NW = std::max(R, KM);

  LockGuard guard(c);                       // the fit arena and its page-locked buffer are this call's until it returns
  char* dev_base = nullptr;
  char* pin_base = nullptr;
  LmProblem pr{};
  double *theta_w = nullptr, *y0_w = nullptr, *flat_w = nullptr, *dflat_w = nullptr, *trials_w = nullptr, *pred_w = nullptr;
  int32_t *status_w = nullptr, *rows_d = nullptr, *flags_d = nullptr;
  size_t dev_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {    // first pass measures, second carves
    Carver cv{dev_base};
    pr.mu = cv.take<double>(R); pr.g = cv.take<double>(R * P); pr.DD = cv.take<double>(R * P); pr.is_free = cv.take<unsigned char>(R * P);
    pr.r = r ? r : cv.take<double>(R * Nr);
    pr.A = JTJ ? JTJ : cv.take<double>(R * P * P);
    rows_d = cv.take<int32_t>(R); flags_d = cv.take<int32_t>(R); status_w = cv.take<int32_t>(NW);
    theta_w = cv.take<double>(NW * P);
    y0_w = y0_is_batched ? cv.take<double>(NW * S) : nullptr;
    flat_w = cv.take<double>(NW * F);
    dflat_w = cv.take<double>(kc_max * F * P);
    trials_w = cv.take<double>(KM * P); pred_w = cv.take<double>(KM);
    dev_bytes = cv.off;
    if (pass == 0) {
      void *d = nullptr, *h = nullptr;
      if ((rc = pk_ctx_fit_reserve(c, dev_bytes, 2 * (size_t)R * sizeof(int32_t), &d, &h))) return rc;
      dev_base = static_cast<char*>(d); pin_base = static_cast<char*>(h);
    }
  }
  int32_t* rows_h = reinterpret_cast<int32_t*>(pin_base);
  int32_t* flags_h = rows_h + R;
  pr.P = P; pr.S = S; pr.F = F; pr.Nr = Nr; pr.log_space = fo.log_space ? 1 : 0; pr.use_reg = fo.use_reg ? 1 : 0;
  pr.y0_batched = y0_is_batched ? 1 : 0; pr.target_batched = target_is_batched ? 1 : 0; pr.sigma_batched = sigma_is_batched ? 1 : 0;
  pr.bounds_batched = bounds_are_batched ? 1 : 0;
  pr.y0 = y0; pr.target = target; pr.sigma = sigma; pr.lam = lam; pr.lb = lb; pr.ub = ub; pr.p = p; pr.cost = cost;
  pr.ftol = fo.ftol; pr.xtol = fo.xtol;

  PK_LM_HIP(c, hipSetDevice(pk_ctx_device(c)));
  hipStream_t stream = (hipStream_t)pk_ctx_stream(c);
  const size_t lds_n = lm_normal_lds(P), lds_t = lm_trials_lds(P);
  if (lds_n > 48 * 1024) PK_LM_HIP(c, hipFuncSetAttribute((const void*)lm_normal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_n));
  if (lds_t > 48 * 1024) PK_LM_HIP(c, hipFuncSetAttribute((const void*)lm_trials_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_t));
  const double* y0_solve = y0_is_batched ? y0_w : y0;
  const auto gather_grid = [&](int64_t n) { return dim3((unsigned)std::min<int64_t>((n * std::max(P, S) + 255) / 256, 65535)); };

  // start values and initial residuals: p = clip(P0), mu = mu0, one solve launch, r and cost of every row
  hipLaunchKernelGGL(lm_gather_kernel, gather_grid(R), dim3(256), 0, stream, pr, (long long)R, (long long)R, (const int32_t*)nullptr, P0, 1, p, theta_w, y0_w);
  if ((rc = pk_solve_protein_batch(c, model, n_sites, R, theta_w, y0_solve, y0_is_batched, t, T, &so, nullptr, flat_w, nullptr, 0, status_w, nullptr))) return rc;
  hipLaunchKernelGGL(lm_accept_kernel, dim3((unsigned)R), dim3(kLmThreads), 0, stream, pr, (const int32_t*)nullptr, (long long)R, 1, flat_w,
                     (const double*)nullptr, (const double*)nullptr, 1, (int32_t*)nullptr);
  PK_LM_HIP(c, hipGetLastError());
  counters[1] += R; counters[2] += 1;

  std::vector<unsigned char> active((size_t)R, 1);
  std::vector<int32_t> why((size_t)R, 3), idx, pend, next;
  for (int64_t it = 1; it <= fo.max_iter; ++it) {
    idx.clear();
    for (int64_t k = 0; k < R; ++k) if (active[k]) idx.push_back((int32_t)k);
    if (idx.empty()) break;
    counters[0] = it;
    // Jacobian phase: gather, sensitivity launch, normal equations -- per chunk of rows; ONE wait for the done flags
    const int64_t k = (int64_t)idx.size();
    std::memcpy(rows_h, idx.data(), k * sizeof(int32_t));
    PK_LM_HIP(c, hipMemcpyAsync(rows_d, rows_h, k * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    for (int64_t c0 = 0; c0 < k; c0 += kc_max) {
      const int64_t kc = std::min(kc_max, k - c0);
      hipLaunchKernelGGL(lm_gather_kernel, gather_grid(kc), dim3(256), 0, stream, pr, (long long)kc, (long long)kc, (const int32_t*)(rows_d + c0),
                         (const double*)p, 1, (double*)nullptr, theta_w, y0_w);
      if ((rc = pk_solve_protein_sens_batch(c, model, n_sites, kc, theta_w, y0_solve, y0_is_batched, t, T, &so, flat_w, dflat_w, status_w, nullptr))) return rc;
      hipLaunchKernelGGL(lm_normal_kernel, dim3((unsigned)kc), dim3(kLmThreads), lds_n, stream, pr, (const int32_t*)(rows_d + c0), (const double*)dflat_w, flags_d + c0);
      PK_LM_HIP(c, hipGetLastError());
      counters[2] += 3;
    }
    PK_LM_HIP(c, hipMemcpyAsync(flags_h, flags_d, k * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    PK_LM_HIP(c, hipStreamSynchronize(stream));
    counters[1] += k; counters[3] += 1; counters[4] += 1;
    pend.clear();
    for (int64_t j = 0; j < k; ++j) {
      if (flags_h[j]) { active[idx[j]] = 0; why[idx[j]] = 1; }
      else pend.push_back(idx[j]);
    }
    // trial rounds: damped steps of K levels, their solves, the accept rule; ONE wait for the flags
    int tries = 0;
    while (tries < kLmMaxTries && !pend.empty()) {
      const int64_t m = (int64_t)pend.size();
      const int K = lm_round_levels(fo.trial_levels, m, tries);
      tries += K;
      std::memcpy(rows_h, pend.data(), m * sizeof(int32_t));
      PK_LM_HIP(c, hipMemcpyAsync(rows_d, rows_h, m * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      hipLaunchKernelGGL(lm_trials_kernel, dim3((unsigned)m, (unsigned)K), dim3(lm_trials_threads(P)), lds_t, stream, pr, (const int32_t*)rows_d, (long long)m,
                         trials_w, pred_w, theta_w, y0_w);
      if ((rc = pk_solve_protein_batch(c, model, n_sites, K * m, theta_w, y0_solve, y0_is_batched, t, T, &so, nullptr, flat_w, nullptr, 0, status_w, nullptr))) return rc;
      hipLaunchKernelGGL(lm_accept_kernel, dim3((unsigned)m), dim3(kLmThreads), 0, stream, pr, (const int32_t*)rows_d, (long long)m, K, (const double*)flat_w,
                         (const double*)trials_w, (const double*)pred_w, 0, flags_d);
      PK_LM_HIP(c, hipGetLastError());
      PK_LM_HIP(c, hipMemcpyAsync(flags_h, flags_d, m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      PK_LM_HIP(c, hipStreamSynchronize(stream));
      counters[1] += K * m; counters[2] += 3; counters[3] += 1; counters[5] += 1;
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
    std::memcpy(rows_h, why.data(), R * sizeof(int32_t));
    PK_LM_HIP(c, hipMemcpyAsync(reason, rows_h, R * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    PK_LM_HIP(c, hipStreamSynchronize(stream));
  }
  return PK_OK;
}

}  // extern "C"
