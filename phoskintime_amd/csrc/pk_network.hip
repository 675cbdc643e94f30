// pk_network.hip -- kernels and C ABI of the network (global_model) path: batched RHS, analytic Jacobian, softplus unpack.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <mutex>
#include <vector>
#include "../../include/phoskin.h"
#include "pk_network.hpp"
#include "pk_network_solve.hpp"
#include "pk_network_solve_reg.hpp"
#include "pk_network_rk45.hpp"
#include "pk_network_sens.hpp"
#include "pk_net_plan.hpp"
#include "pk_env.hpp"
namespace pk {
// persistent grid: min(B, workgroups of `kernel` at `threads` each resident on the current device at once)
hipError_t net_persistent_grid(const void* kernel, int threads, long long B, int* grid);
// ROS34PW2-W with every per-candidate vector in an HBM workspace (net_solve_ws_kernel, pk_inst_net_ws.hip): no size limit
hipError_t net_ws_grid(const NetDev& n, long long B, int* grid);
hipError_t launch_net_ws(const NetDev& n, const NetSolveArgs& a, long long B, int grid, double* ws, hipStream_t st);
// the same two kernels scoring the three-objective loss as they integrate (pk_inst_net_rosw_fused.hip)
hipError_t net_ws_fused_grid(const NetDev& n, long long B, int* grid);
hipError_t launch_net_ws_fused(const NetDev& n, const NetSolveArgs& a, long long B, int grid, double* ws, hipStream_t st);
hipError_t launch_net_lds_fused(const NetDev& n, const NetSolveArgs& a, long long B, int threads, size_t lds, hipStream_t st);
// ... and measuring the fold-change observables and their scalar Morris metric (pk_inst_net_rosw_measure.hip)
hipError_t net_ws_measure_grid(const NetDev& n, long long B, int* grid);
hipError_t launch_net_ws_measure(const NetDev& n, const NetSolveArgs& a, long long B, int grid, double* ws, hipStream_t st);
hipError_t launch_net_lds_measure(const NetDev& n, const NetSolveArgs& a, long long B, int threads, size_t lds, hipStream_t st);
// ... and carrying forward parameter sensitivities, one workgroup per (candidate, column chunk) (pk_inst_net_rosw_sens.hip)
hipError_t launch_net_lds_sens(const NetDev& n, const NetSolveArgs& a, const NetSensArgs& s, long long B, int threads, size_t lds, hipStream_t st);
// ... and scoring the loss and its gradient from those tangents as they land (pk_inst_net_rosw_sens_score.hip)
hipError_t launch_net_lds_sens_score(const NetDev& n, const NetSolveArgs& a, const NetSensArgs& s, const NetSensScoreArgs& sc, long long B, int threads,
                                     size_t lds, hipStream_t st);
// ... and the same two flavours on HBM-workspace slabs, a persistent grid over (candidate, column chunk) items (pk_inst_net_rosw_sens_ws.hip)
hipError_t net_sens_ws_grid(const NetDev& n, bool score, long long items, int* grid);
hipError_t launch_net_ws_sens(const NetDev& n, const NetSolveArgs& a, const NetSensArgs& s, const NetSensScoreArgs* sc, long long B, int grid,
                              double* ws, hipStream_t st);
// order-4 additive integrator (pk_network_solve_ark.hpp), its own translation unit: returns the dynamic LDS it needs, or launches
size_t net_ark_lds_bytes(const NetDev& n, int nnzT, int max_sites, int threads);
hipError_t launch_net_ark(const NetDev& n, const NetSolveArgs& a, int max_sites, long long B, int threads, size_t lds, hipStream_t st);
// register-resident order-3 integrator, one thread per protein (pk_network_solve_reg.hpp, _reg2.hpp; pk_inst_net_reg.hip)
void launch_net_reg(const NetDev& n, const NetSolveArgs& a, int max_sites, long long B, int threads, size_t lds, hipStream_t st);
// the same method in the dense two-lanes-per-protein layout (pk_network_solve_arkp.hpp; arrow topologies): n.lane_unit must be set
bool net_arkp_enabled();
bool net_arkp_fits(const NetDev& n, int max_sites);
bool net_arkp_fuses_loss();                      // the register-diet kernel (PK_ARK_PAIR=3, the default) scores observations at its output times
hipError_t launch_net_arkp(const NetDev& n, const NetSolveArgs& a, int nnzT, int max_sites, long long B, hipStream_t st);
}
#include <algorithm>
#include <cstdlib>

struct pk_ctx;                                   // defined in pk_capi.hip
extern "C" int pk_ctx_device(pk_ctx*);
extern "C" void* pk_ctx_stream(pk_ctx*);
extern "C" int pk_ctx_fail(pk_ctx*, int code, const char* msg);
extern "C" int pk_ctx_scratch_launch(pk_ctx*, size_t bytes, hipError_t (*launch)(void* scratch, hipStream_t stream, void* user), void* user);

namespace pk {

// dydt[b, :] = f(t_b, y_b; x_b) with the work area L (LDS, or a workspace slab)
__device__ __forceinline__ void net_rhs_one(const NetDev& n, const NetLds& L, const long long b, const double* __restrict__ x, const int x_is_raw,
                                            const double* __restrict__ y, const int y_batched, const double* __restrict__ t, const int t_batched,
                                            double* __restrict__ dydt) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* xb = x + b * n.n_var;
  for (int k = tid; k < n.n_var; k += nt) L.p[k] = x_is_raw ? softplus(xb[k]) : xb[k];
  const double* yb = y + (y_batched ? b * n.S : 0);
  for (int k = tid; k < n.S; k += nt) L.y[k] = yb[k];
  const int jb = net_bucket(t[t_batched ? b : 0], n.kin_grid, n.n_grid);
  __syncthreads();
  net_prepare<false>(n, L, jb);
  for (int k = tid; k < n.S; k += nt) dydt[b * n.S + k] = net_state_rhs(n, L, k);
}

__global__ __launch_bounds__(256) void net_rhs_kernel(const NetDev n, const double* __restrict__ x, const int x_is_raw,
                                                      const double* __restrict__ y, const int y_batched,
                                                      const double* __restrict__ t, const int t_batched, double* __restrict__ dydt) {
  extern __shared__ __align__(16) double lds[];
  net_rhs_one(n, NetLds(lds, n), blockIdx.x, x, x_is_raw, y, y_batched, t, t_batched, dydt);
}

// J[b, r, c] = d f_r / d y_c, row-major, analytic
__device__ __forceinline__ void net_jac_one(const NetDev& n, const NetLds& L, const long long b, const double* __restrict__ x, const int x_is_raw,
                                            const double* __restrict__ y, const int y_batched, const double* __restrict__ t, const int t_batched,
                                            double* __restrict__ J) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* xb = x + b * n.n_var;
  for (int k = tid; k < n.n_var; k += nt) L.p[k] = x_is_raw ? softplus(xb[k]) : xb[k];
  const double* yb = y + (y_batched ? b * n.S : 0);
  for (int k = tid; k < n.S; k += nt) L.y[k] = yb[k];
  const int jb = net_bucket(t[t_batched ? b : 0], n.kin_grid, n.n_grid);
  __syncthreads();
  net_prepare<true>(n, L, jb);
  double* Jb = J + b * (size_t)n.S * n.S;
  // block-diagonal part: one thread per row, its protein's columns; everything else zero
  for (int r = tid; r < n.S; r += nt) {
    double* row = Jb + (size_t)r * n.S;
    for (int c = 0; c < n.S; ++c) row[c] = 0.0;
    const int i = n.state_prot[r], lr = n.state_local[r];
    const int st = n.offset_y[i];
    const int cnt = (n.model == 2) ? 1 + (1 << n.n_sites[i]) : 2 + n.n_sites[i];
    for (int lc = 0; lc < cnt; ++lc) row[st + lc] = net_block_jac(n, L, i, lr, lc);
    if (lr == 0) {
      // TF coupling of the mRNA row: d synth_i / d y_c = dsyn_i * TF_ij * [c is a protein-form state of an undriven regulator j]
      for (int q = n.TF_indptr[i]; q < n.TF_indptr[i + 1]; ++q) {
        const int j = n.TF_indices[q];
        if (n.model != 2 && n.driver_map[j] >= 0) continue;
        const double w = L.dsyn[i] * n.TF_data[q];
        const int sj = n.offset_y[j];
        const int cj = (n.model == 2) ? (1 << n.n_sites[j]) : 1 + n.n_sites[j];
        for (int m = 0; m < cj; ++m) row[sj + 1 + m] += w;
      }
    }
  }
}

__global__ __launch_bounds__(256) void net_jac_kernel(const NetDev n, const double* __restrict__ x, const int x_is_raw,
                                                      const double* __restrict__ y, const int y_batched,
                                                      const double* __restrict__ t, const int t_batched, double* __restrict__ J) {
  extern __shared__ __align__(16) double lds[];
  net_jac_one(n, NetLds(lds, n), blockIdx.x, x, x_is_raw, y, y_batched, t, t_batched, J);
}

// networks whose work area exceeds 160 KiB of LDS: the same bodies on a workspace slab per workgroup, persistent over the batch
__host__ __device__ inline size_t net_rhs_ws_slab_doubles(const NetDev& n) {
  return ((size_t)n.n_var + n.S + n.n_K + n.sites + 3 * (size_t)n.N + 15) / 16 * 16;
}
template <bool JAC>
__global__ __launch_bounds__(256) void net_rhs_ws_kernel(const NetDev n, const long long B, double* __restrict__ ws, const size_t slab,
                                                         const double* __restrict__ x, const int x_is_raw, const double* __restrict__ y,
                                                         const int y_batched, const double* __restrict__ t, const int t_batched, double* __restrict__ out) {
  const NetLds L(ws + (size_t)blockIdx.x * slab, n);
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();                                   // the previous candidate of this workgroup is done with the slab
    if (JAC) net_jac_one(n, L, b, x, x_is_raw, y, y_batched, t, t_batched, out);
    else     net_rhs_one(n, L, b, x, x_is_raw, y, y_batched, t, t_batched, out);
  }
}

__global__ void net_unpack_kernel(const double* __restrict__ x, double* __restrict__ out, const long long total) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < total) out[k] = softplus(x[k]);
}

}  // namespace pk

struct pk_net {
  pk::NetDev d;
  std::vector<void*> allocs;
  size_t lds_bytes;
  size_t solve_lds_bytes;
  size_t solve_reg_lds_bytes;
  int max_sites;
  int nnzT = 0;
  std::vector<double> kin_grid_host;
  double* stops_dev = nullptr; int32_t* stop_out_dev = nullptr; size_t stops_cap = 0;
  std::mutex mu;       // a network handle may be shared by the threads of a process (each with its own pk_ctx): guards the stop buffers
};

namespace {
template <class T>
const T* upload(pk_net* n, const T* host, size_t count, bool& ok) {
  if (!ok) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, (count ? count : 1) * sizeof(T)) != hipSuccess) { ok = false; return nullptr; }
  n->allocs.push_back(p);
  if (count && hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { ok = false; return nullptr; }
  return (const T*)p;
}
}  // namespace

extern "C" {

pk_net* pk_network_create(pk_ctx* c, const pk_network_desc* d) {
  if (!c || !d) return nullptr;
  if (!(d->model == 0 || d->model == 1 || d->model == 2 || d->model == 4)) { pk_ctx_fail(c, PK_ERR_ARG, "network model must be 0, 1, 2 or 4"); return nullptr; }
  if (d->N < 1 || d->n_K < 1 || d->total_sites < 0 || d->n_grid < 1) { pk_ctx_fail(c, PK_ERR_ARG, "bad network dimensions"); return nullptr; }
  if (!d->offset_y || !d->offset_s || !d->n_sites || !d->W_indptr || !d->TF_indptr || !d->tf_deg || !d->driver_map || !d->kin_grid || !d->kin_Kmat) {
    pk_ctx_fail(c, PK_ERR_ARG, "null array in pk_network_desc"); return nullptr;
  }
  // validate the layout on the host: a wrong offset would become an out-of-bounds access on the GPU
  int S = 0, sites = 0;
  std::vector<int32_t> sp, sl;
  for (int i = 0; i < d->N; ++i) {
    const int ns = d->n_sites[i];
    if (ns < 0 || (d->model == 2 && ns > 10)) { pk_ctx_fail(c, PK_ERR_ARG, "n_sites out of range (model 2: <= 10)"); return nullptr; }
    if (d->offset_y[i] != S || d->offset_s[i] != sites) { pk_ctx_fail(c, PK_ERR_ARG, "offset_y / offset_s are not the running sums of the block sizes"); return nullptr; }
    const int cnt = (d->model == 2) ? 1 + (1 << ns) : 2 + ns;
    for (int l = 0; l < cnt; ++l) { sp.push_back(i); sl.push_back(l); }
    S += cnt; sites += ns;
    if (d->driver_map[i] >= d->n_K) { pk_ctx_fail(c, PK_ERR_ARG, "driver_map entry >= n_K"); return nullptr; }
  }
  if (sites != d->total_sites) { pk_ctx_fail(c, PK_ERR_ARG, "sum(n_sites) != total_sites"); return nullptr; }
  if (d->W_indptr[0] != 0 || d->TF_indptr[0] != 0) { pk_ctx_fail(c, PK_ERR_ARG, "CSR indptr must start at 0"); return nullptr; }
  for (int r = 0; r < sites; ++r) if (d->W_indptr[r + 1] < d->W_indptr[r]) { pk_ctx_fail(c, PK_ERR_ARG, "W_indptr not monotone"); return nullptr; }
  for (int r = 0; r < d->N; ++r) if (d->TF_indptr[r + 1] < d->TF_indptr[r]) { pk_ctx_fail(c, PK_ERR_ARG, "TF_indptr not monotone"); return nullptr; }
  const int nnzW = d->W_indptr[sites], nnzT = d->TF_indptr[d->N];
  for (int q = 0; q < nnzW; ++q) if (d->W_indices[q] < 0 || d->W_indices[q] >= d->n_K) { pk_ctx_fail(c, PK_ERR_ARG, "W_indices out of range"); return nullptr; }
  for (int q = 0; q < nnzT; ++q) if (d->TF_indices[q] < 0 || d->TF_indices[q] >= d->N) { pk_ctx_fail(c, PK_ERR_ARG, "TF_indices out of range"); return nullptr; }
  for (int g = 1; g < d->n_grid; ++g) if (!(d->kin_grid[g] > d->kin_grid[g - 1])) { pk_ctx_fail(c, PK_ERR_ARG, "kin_grid must increase"); return nullptr; }

  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return nullptr;
  pk_net* n = new pk_net();
  bool ok = true;
  pk::NetDev& v = n->d;
  v.model = d->model; v.N = d->N; v.n_K = d->n_K; v.sites = sites; v.S = S; v.n_grid = d->n_grid; v.n_var = d->n_K + 5 * d->N + sites + 1;
  v.offset_y = upload(n, d->offset_y, d->N, ok); v.offset_s = upload(n, d->offset_s, d->N, ok); v.n_sites = upload(n, d->n_sites, d->N, ok);
  v.state_prot = upload(n, sp.data(), sp.size(), ok); v.state_local = upload(n, sl.data(), sl.size(), ok);
  v.W_indptr = upload(n, d->W_indptr, sites + 1, ok); v.W_indices = upload(n, d->W_indices, nnzW, ok); v.W_data = upload(n, d->W_data, nnzW, ok);
  v.TF_indptr = upload(n, d->TF_indptr, d->N + 1, ok); v.TF_indices = upload(n, d->TF_indices, nnzT, ok); v.TF_data = upload(n, d->TF_data, nnzT, ok);
  v.tf_deg = upload(n, d->tf_deg, d->N, ok); v.driver_map = upload(n, d->driver_map, d->N, ok);
  v.kin_grid = upload(n, d->kin_grid, d->n_grid, ok); v.kin_Kmat = upload(n, d->kin_Kmat, (size_t)d->n_K * d->n_grid, ok);
  n->lds_bytes = ((size_t)v.n_var + v.S + v.n_K + v.sites + 3 * (size_t)v.N) * sizeof(double);
  n->solve_lds_bytes = pk::net_solve_lds_bytes(v, nnzT);
  n->solve_reg_lds_bytes = pk::net_solve_reg_lds_bytes(v, nnzT);
  n->nnzT = nnzT;
  n->max_sites = 0;
  for (int i = 0; i < d->N; ++i) n->max_sites = std::max(n->max_sites, (int)d->n_sites[i]);
  n->kin_grid_host.assign(d->kin_grid, d->kin_grid + d->n_grid);
  v.lane_unit = nullptr; v.n_lanes = 0;
  if ((d->model == 0 || d->model == 1 || d->model == 4) && n->max_sites <= 8) {
    // dense lane table: a lane holds (2 + site class) / 2 rows; proteins with more sites than fit beside mRNA and protein take a second lane
    const int cls = n->max_sites <= 4 ? 4 : n->max_sites <= 6 ? 6 : 8, nrl = (2 + cls) / 2;
    std::vector<int32_t> lanes;
    // ... and so do proteins with more than 4 regulators: the lanes of a pair split the TF row, 4 register-resident entries each
    auto two = [&](int i) { return d->n_sites[i] > nrl - 2 || d->TF_indptr[i + 1] - d->TF_indptr[i] > 4; };
    for (int i = 0; i < d->N; ++i) if (two(i)) { lanes.push_back((i << 2) | 2); lanes.push_back((i << 2) | 3); }
    for (int i = 0; i < d->N; ++i) if (!two(i)) lanes.push_back(i << 2);
    v.n_lanes = (int)lanes.size();
    v.lane_unit = upload(n, lanes.data(), lanes.size(), ok);
  }
  if (!ok) {
    pk_ctx_fail(c, PK_ERR_NOMEM, "hipMalloc / hipMemcpy failed");
    pk_network_destroy(n);
    return nullptr;
  }
  // beyond 160 KiB the RHS / Jacobian run on workspace slabs instead of dynamic LDS (net_rhs_ws_kernel)
  if (n->lds_bytes > 48 * 1024 && n->lds_bytes <= 160 * 1024) {
    (void)hipFuncSetAttribute((const void*)pk::net_rhs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n->lds_bytes);
    (void)hipFuncSetAttribute((const void*)pk::net_jac_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n->lds_bytes);
  }
  if (n->solve_lds_bytes > 48 * 1024 && n->solve_lds_bytes <= 160 * 1024) {
    (void)hipFuncSetAttribute((const void*)pk::net_solve_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n->solve_lds_bytes);
    (void)hipFuncSetAttribute((const void*)pk::net_solve_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n->solve_lds_bytes);
    (void)hipFuncSetAttribute((const void*)pk::net_solve_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n->solve_lds_bytes);
    (void)hipFuncSetAttribute((const void*)pk::net_solve_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n->solve_lds_bytes);
  }
  return n;
}

void pk_network_destroy(pk_net* n) {
  if (!n) return;
  for (void* p : n->allocs) (void)hipFree(p);
  if (n->stops_dev) (void)hipFree(n->stops_dev);
  if (n->stop_out_dev) (void)hipFree(n->stop_out_dev);
  delete n;
}

const pk::NetDev* pk_net_dev(const pk_net* n) { return &n->d; }
int pk_network_n_states(const pk_net* n) { return n ? n->d.S : PK_ERR_ARG; }
int pk_network_n_var(const pk_net* n) { return n ? n->d.n_var : PK_ERR_ARG; }

static int net_args_ok(pk_ctx* c, pk_net* n, int64_t B, const void* x, const void* y, const void* t, const void* out) {
  if (!c || !n) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (B > 0 && (!x || !y || !t || !out)) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (B > 0x7fffffffLL) return pk_ctx_fail(c, PK_ERR_ARG, "batch too large for one launch");
  return PK_OK;
}

// RHS / Jacobian of a network whose work area exceeds 160 KiB: a persistent grid of min(B, resident workgroups) on slabs of the context's
// scratch arena
struct NetRhsWsLaunch {
  const pk::NetDev* d; long long B; int grid; bool jac;
  const double *x, *y, *t; int x_is_raw, y_batched, t_batched; double* out;
};
static hipError_t net_rhs_ws_launch(void* scratch, hipStream_t st, void* user) {
  const NetRhsWsLaunch& q = *(const NetRhsWsLaunch*)user;
  const size_t slab = pk::net_rhs_ws_slab_doubles(*q.d);
  if (q.jac) hipLaunchKernelGGL(pk::net_rhs_ws_kernel<true>, dim3((unsigned)q.grid), dim3(256), 0, st, *q.d, q.B, (double*)scratch, slab, q.x,
                                q.x_is_raw, q.y, q.y_batched, q.t, q.t_batched, q.out);
  else       hipLaunchKernelGGL(pk::net_rhs_ws_kernel<false>, dim3((unsigned)q.grid), dim3(256), 0, st, *q.d, q.B, (double*)scratch, slab, q.x,
                                q.x_is_raw, q.y, q.y_batched, q.t, q.t_batched, q.out);
  return hipGetLastError();
}
static int net_rhs_ws(pk_ctx* c, pk_net* n, bool jac, int64_t B, const double* x, int x_is_raw, const double* y, int y_is_batched,
                      const double* t, int t_is_batched, double* out) {
  NetRhsWsLaunch q{&n->d, (long long)B, 0, jac, x, y, t, x_is_raw, y_is_batched ? 1 : 0, t_is_batched ? 1 : 0, out};
  const void* k = jac ? (const void*)pk::net_rhs_ws_kernel<true> : (const void*)pk::net_rhs_ws_kernel<false>;
  if (pk::net_persistent_grid(k, 256, (long long)B, &q.grid) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "occupancy query");
  return pk_ctx_scratch_launch(c, (size_t)q.grid * pk::net_rhs_ws_slab_doubles(n->d) * sizeof(double), net_rhs_ws_launch, &q);
}

int pk_network_rhs_batch(pk_ctx* c, pk_net* n, int64_t B, const double* x, int x_is_raw, const double* y, int y_is_batched,
                         const double* t, int t_is_batched, double* dydt) {
  int rc = net_args_ok(c, n, B, x, y, t, dydt);
  if (rc || B == 0) return rc;
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  if (n->lds_bytes > 160 * 1024) return net_rhs_ws(c, n, false, B, x, x_is_raw, y, y_is_batched, t, t_is_batched, dydt);
  hipLaunchKernelGGL(pk::net_rhs_kernel, dim3((unsigned)B), dim3(256), n->lds_bytes, (hipStream_t)pk_ctx_stream(c), n->d, x, x_is_raw, y,
                     y_is_batched, t, t_is_batched, dydt);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PK_OK : pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(e));
}

int pk_network_jacobian_batch(pk_ctx* c, pk_net* n, int64_t B, const double* x, int x_is_raw, const double* y, int y_is_batched,
                              const double* t, int t_is_batched, double* J) {
  int rc = net_args_ok(c, n, B, x, y, t, J);
  if (rc || B == 0) return rc;
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  if (n->lds_bytes > 160 * 1024) return net_rhs_ws(c, n, true, B, x, x_is_raw, y, y_is_batched, t, t_is_batched, J);
  hipLaunchKernelGGL(pk::net_jac_kernel, dim3((unsigned)B), dim3(256), n->lds_bytes, (hipStream_t)pk_ctx_stream(c), n->d, x, x_is_raw, y,
                     y_is_batched, t, t_is_batched, J);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PK_OK : pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(e));
}

// Which kernel a network launch runs, with which method, or why not: net_plan of pk_net_plan.hpp, the single source of truth for every
// flavour (the Python host layer picks its default tolerances from the method).  Here: what the plan is told about this network
// (net_facts) and about the environment (net_switches), both read at every call: PK_NET_SENS_KC and PK_NET_THREADS are the live
// switches of pk_env.hpp.
using pk::NetFlavour; using pk::NetKernel; using pk::NetPlan;

// Columns one workgroup of the sensitivity kernel carries on this network: the largest count whose LDS request (net_sens_lds_bytes; `score`:
// net_sens_score_lds_bytes -- the rna baseline, its tangents and the accumulators come on top) stays within 160 KiB, at most n_var; 0 where
// not even one fits or the network is beyond the LDS kernel's thread layout.  Host arithmetic only (dev knob PK_NET_SENS_KC: a smaller count)
static int net_sens_lds_columns(const pk_net* n, bool score) {
  if (n->d.S > 1024 || n->d.N > 512) return 0;
  const int fit = score ? pk::net_sens_score_max_columns(n->d, n->nnzT, pk::kNetLdsLimit) : pk::net_sens_max_columns(n->d, n->nnzT, pk::kNetLdsLimit);
  return pk::net_sens_kc(pk::env_live(), std::min(fit, n->d.n_var));
}

static pk::NetFacts net_facts(const pk_net* n) {
  const pk::NetDev& d = n->d;
  return {d.model, d.N, d.S, d.n_var, n->max_sites,
          n->solve_lds_bytes, pk::net_solve_fused_lds_bytes(d, n->nnzT), n->solve_reg_lds_bytes, pk::net_rk45_lds_bytes(d),
          pk::net_ark_lds_bytes(d, n->nnzT, n->max_sites, ((d.N + 63) / 64) * 64),
          pk::net_arkp_fits(d, n->max_sites), pk::net_arkp_fuses_loss(), net_sens_lds_columns(n, false), net_sens_lds_columns(n, true)};
}

static pk::NetSwitches net_switches() {
  const pk::Env e = pk::env_live();
  return {e.net_threads, pk::net_sens_kc(e, 16)};
}

static pk_solver_opts net_opts(const pk_solver_opts* opts) {
  pk_solver_opts o;
  if (opts) o = *opts; else pk_default_opts(&o);
  return o;
}

int pk_network_resolve_method(const pk_net* n, const pk_solver_opts* opts) {
  return n ? pk::net_plan(net_facts(n), net_opts(opts), NetFlavour::Plain, 0, net_switches()).method : PK_ERR_ARG;
}

// The columns of a tangent launch (cols: HOST pointer, K >= 1) with the plan their entry point made for them -- it answers the plan's
// refusals before it checks cols.  score: the scoring flavour's outputs (pk_network_simulate_objective_grad_batch)
struct NetSensReq { const int32_t* cols_host; int K; double* dY; const pk::NetSensScoreArgs* score; NetPlan plan; };

// Landing points of a launch: every output time after t[0] plus every bucket edge strictly inside (t[0], t[T-1]); the explicit integrator
// interpolates its outputs and needs the T output times only.  Up to 64 travel in the kernel arguments, more through a per-network buffer
static int net_landing_points(pk_ctx* c, pk_net* n, const double* t_host, int T, bool dp5, pk::NetSolveArgs& a) {
  std::vector<std::pair<double, int>> st;
  for (int k = dp5 ? 0 : 1; k < T; ++k) st.push_back({t_host[k], k});
  if (!dp5) {
    for (double gk : n->kin_grid_host) {
      if (gk > t_host[0] && gk < t_host[T - 1]) {
        bool dup = false;
        for (int k = 1; k < T; ++k) if (t_host[k] == gk) { dup = true; break; }
        if (!dup) st.push_back({gk, -1});
      }
    }
    std::sort(st.begin(), st.end());
  }
  a.n_stops = (int)st.size();
  if (st.size() <= 64) {
    for (size_t i = 0; i < st.size(); ++i) { a.stops_v[i] = st[i].first; a.stop_out_v[i] = st[i].second; }
    return PK_OK;
  }
  // long output grids: stage through a per-network device buffer (the previous launch on it must have finished)
  std::lock_guard<std::mutex> g(n->mu);
  if (hipDeviceSynchronize() != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipDeviceSynchronize");      // any stream of any context
  if (n->stops_cap < st.size()) {
    if (n->stops_dev) (void)hipFree(n->stops_dev);
    if (n->stop_out_dev) (void)hipFree(n->stop_out_dev);
    n->stops_dev = nullptr; n->stop_out_dev = nullptr; n->stops_cap = 0;
    if (hipMalloc((void**)&n->stops_dev, st.size() * 8) != hipSuccess || hipMalloc((void**)&n->stop_out_dev, st.size() * 4) != hipSuccess)
      return pk_ctx_fail(c, PK_ERR_NOMEM, "hipMalloc");
    n->stops_cap = st.size();
  }
  std::vector<double> sv(st.size()); std::vector<int32_t> so(st.size());
  for (size_t i = 0; i < st.size(); ++i) { sv[i] = st[i].first; so[i] = st[i].second; }
  if (hipMemcpy(n->stops_dev, sv.data(), sv.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(n->stop_out_dev, so.data(), so.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return pk_ctx_fail(c, PK_ERR_HIP, "hipMemcpy");
  a.stops_p = n->stops_dev; a.stop_out_p = n->stop_out_dev;
  return PK_OK;
}

// Tangent launch: B x ceil(K / KC) workgroups of the LDS kernel, or with plan.hbm a persistent grid over as many (candidate, chunk) items
// on workspace slabs.  The context's scratch arena holds the column indices and, on slabs, behind them (whole 128-B lines) grid x slab;
// status is OR-ed over the chunks, so it is zeroed first
struct NetSensLaunch {
  const pk::NetDev* d; const pk::NetSolveArgs* a; const NetSensReq* s; long long B;
  int threads; size_t lds;                       // LDS route
  int grid; size_t cols_bytes;                   // slabs
};
static hipError_t net_sens_launch(void* scratch, hipStream_t st, void* user) {
  const NetSensLaunch& r = *(const NetSensLaunch*)user;
  const NetSensReq& s = *r.s;
  hipError_t e = hipMemcpyAsync(scratch, s.cols_host, (size_t)s.K * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && r.a->status) e = hipMemsetAsync(r.a->status, 0, (size_t)r.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  const pk::NetSensArgs sa{(const int32_t*)scratch, s.K, s.plan.KC, s.dY};
  if (s.plan.hbm) return pk::launch_net_ws_sens(*r.d, *r.a, sa, s.score, r.B, r.grid, (double*)((char*)scratch + r.cols_bytes), st);
  if (s.score) return pk::launch_net_lds_sens_score(*r.d, *r.a, sa, *s.score, r.B, r.threads, r.lds, st);
  return pk::launch_net_lds_sens(*r.d, *r.a, sa, r.B, r.threads, r.lds, st);
}
static int net_simulate_sens(pk_ctx* c, pk_net* n, const pk::NetSolveArgs& a, const NetSensReq& s, int64_t B) {
  const bool score = s.score != nullptr;
  const int kcl = std::min(s.K, s.plan.KC), n_chunks = (s.K + s.plan.KC - 1) / s.plan.KC;
  NetSensLaunch q{&n->d, &a, &s, (long long)B, s.plan.threads, 0, 0, 0};
  if (!s.plan.hbm) {
    q.lds = score ? pk::net_sens_score_lds_bytes(n->d, n->nnzT, kcl) : pk::net_sens_lds_bytes(n->d, n->nnzT, kcl);
    return pk_ctx_scratch_launch(c, (size_t)s.K * sizeof(int32_t), net_sens_launch, &q);
  }
  q.cols_bytes = ((size_t)s.K * sizeof(int32_t) + 127) / 128 * 128;
  if (pk::net_sens_ws_grid(n->d, score, (long long)B * n_chunks, &q.grid) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "occupancy query");
  return pk_ctx_scratch_launch(c, q.cols_bytes + (size_t)q.grid * pk::net_sens_ws_slab_doubles(n->d, kcl, score) * sizeof(double), net_sens_launch, &q);
}

// Every network launch.  `a`: zeroed, with the loss and measurement fields that `fl` reads filled in by the entry point (Y may be null for
// every flavour but Plain); the rest is filled here.  `sens`: the columns of the two tangent flavours with their plan, else null
static int net_simulate_impl(pk_ctx* c, pk_net* n, int64_t B, const double* x, int x_is_raw, const double* y0, int y0_is_batched,
                             const double* t_host, int T, const pk_solver_opts* opts_in, double* Y, int32_t* status, int32_t* n_steps,
                             NetFlavour fl, pk::NetSolveArgs& a, const NetSensReq* sens = nullptr) {
  if (!c || !n) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (T < 1 || !t_host) return pk_ctx_fail(c, PK_ERR_ARG, "t must hold >= 1 time points (host pointer)");
  if (B == 0) return PK_OK;
  if (!x || !y0 || (!Y && fl == NetFlavour::Plain)) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (B > 0x7fffffffLL) return pk_ctx_fail(c, PK_ERR_ARG, "batch too large for one launch");
  if (n->d.model == 2 && n->max_sites > 16) return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "combinatorial topology: <= 16 sites per protein");
  pk_solver_opts o = net_opts(opts_in);
  const NetPlan plan = sens ? sens->plan : pk::net_plan(net_facts(n), o, fl, 0, net_switches());
  if (plan.code != PK_OK) return pk_ctx_fail(c, plan.code, plan.refusal);
  const bool dp5 = plan.kernel == NetKernel::DP5;
  for (int k = 1; k < T; ++k) if (!(t_host[k] > t_host[k - 1])) return pk_ctx_fail(c, PK_ERR_ARG, "t must be strictly increasing");
  if (!(o.rtol > 0.0 && o.atol >= 0.0)) return pk_ctx_fail(c, PK_ERR_ARG, "rtol must be > 0 and atol >= 0");
  if (o.max_steps <= 0) o.max_steps = dp5 ? 2000000 : 1000000;      // solvers.py:294 max_steps = 2_000_000
  if (o.err_norm < PK_NORM_DEFAULT || o.err_norm > PK_NORM_RMS) return pk_ctx_fail(c, PK_ERR_ARG, "unknown opts->err_norm");
  a.x = x; a.x_is_raw = x_is_raw; a.y0 = y0; a.y0_batched = y0_is_batched ? 1 : 0; a.t0 = t_host[0]; a.T = T; a.Y = Y;
  a.status = status; a.n_steps = n_steps; a.rtol = o.rtol; a.atol = o.atol; a.h0 = o.h0; a.max_steps = o.max_steps;
  a.err_rms = (o.err_norm == PK_NORM_RMS) ? 1 : 0;
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  hipStream_t stream = (hipStream_t)pk_ctx_stream(c);
  if (const int rc = net_landing_points(c, n, t_host, T, dp5, a)) return rc;
  if (sens) return net_simulate_sens(c, n, a, *sens, B);
  const bool measure = fl == NetFlavour::Measure, rosw_fused = measure || fl == NetFlavour::ScoreLists;
  const int M = n->d.model;
  switch (plan.kernel) {
    case NetKernel::Workspace: {
      // ROS34PW2 on workspace slabs (net_solve_ws_kernel): grid = min(B, resident workgroups), workspace = grid x slab of the scratch arena
      struct Q { const pk::NetDev* d; const pk::NetSolveArgs* a; long long B; int grid; decltype(&pk::launch_net_ws) launch; }
          q{&n->d, &a, (long long)B, 0, measure ? pk::launch_net_ws_measure : rosw_fused ? pk::launch_net_ws_fused : pk::launch_net_ws};
      if ((measure ? pk::net_ws_measure_grid : rosw_fused ? pk::net_ws_fused_grid : pk::net_ws_grid)(n->d, (long long)B, &q.grid) != hipSuccess)
        return pk_ctx_fail(c, PK_ERR_HIP, "occupancy query");
      auto launch = [](void* scratch, hipStream_t s, void* user) -> hipError_t {
        const Q& r = *(const Q*)user;
        return r.launch(*r.d, *r.a, r.B, r.grid, (double*)scratch, s);
      };
      // a fused launch's slab is N doubles longer (the rna baseline), a measuring launch's too
      const size_t slab = rosw_fused ? pk::net_ws_fused_slab_doubles(n->d) : pk::net_ws_slab_doubles(n->d);
      return pk_ctx_scratch_launch(c, (size_t)q.grid * slab * sizeof(double), launch, &q);
    }
    case NetKernel::DP5: {
      const size_t lb = pk::net_rk45_lds_bytes(n->d);
#define PK_RK_LAUNCH(M)                                                                                                              \
      do {                                                                                                                             \
        if (lb > 48 * 1024) (void)hipFuncSetAttribute((const void*)pk::net_rk45_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb); \
        hipLaunchKernelGGL(pk::net_rk45_kernel<M>, dim3((unsigned)B), dim3(256), lb, stream, n->d, a);                                 \
      } while (0)
      if (M == 0) PK_RK_LAUNCH(0); else if (M == 1) PK_RK_LAUNCH(1); else if (M == 2) PK_RK_LAUNCH(2); else PK_RK_LAUNCH(4);
#undef PK_RK_LAUNCH
      break;
    }
    case NetKernel::ArkPair:
    case NetKernel::Ark: {
      // The order-4 method runs at 0.25 x the requested tolerances: at that factor its error equals the order-3 method's at the SAME nominal
      // tolerance.  Measured at rtol = atol = 1e-8, band widths from the converged solution (tools/gpu_ark_population*.py, bench.py):
      //   BASELINE config 5's population (8 192 candidates, log-normal 0.5 around the defaults), fixture candidate vs LSODA@1e-12:
      //     factor 1: 914 steps, 0.085;  0.5: 1 102, 0.048;  0.25: 1 329, 0.023;  ROS34PW2: 5 516 steps, 0.022  (reference's LSODA@1e-8: 0.054)
      //   2 048 candidates UNIFORM IN THE OPTIMISER'S RAW BOUNDS (extreme rates, strong TF coupling):
      //     factor 0.5: 4 217 steps, median 0.21, p99 0.85, 0.7 % beyond the band;  0.25: 5 114 steps, median 0.11, p99 0.41, 0.5 % beyond;
      //     ROS34PW2: 7 478 steps, median 0.16, p99 0.31, 0.05 % beyond  (both methods: worst candidates 6-7 band widths off)
      // (dev knob: PK_ARK_TOLFAC)
      const pk::Env& env = pk::env();
      pk::NetSolveArgs aa = a;
      aa.rtol *= env.ark_tolfac; aa.atol *= env.ark_tolfac;
      aa.ctl_safety = env.ark_safety; aa.ctl_grow = env.ark_grow;      // dev knobs of the controller: PK_ARK_SAFETY, PK_ARK_GROW
      // [r3] arrow topologies: the dense two-lanes-per-protein layout, every stage vector in registers (PK_ARK_PAIR=0: round 2's kernel)
      const hipError_t ea = plan.kernel == NetKernel::ArkPair
                                ? pk::launch_net_arkp(n->d, aa, n->nnzT, n->max_sites, (long long)B, stream)
                                : pk::launch_net_ark(n->d, aa, n->max_sites, (long long)B, plan.threads,
                                                     pk::net_ark_lds_bytes(n->d, n->nnzT, n->max_sites, plan.threads), stream);
      if (ea != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(ea));
      break;
    }
    case NetKernel::CombReg:
    case NetKernel::Reg:
      pk::launch_net_reg(n->d, a, n->max_sites, (long long)B, plan.threads, n->solve_reg_lds_bytes, stream);
      break;
    case NetKernel::Lds: {
      const int threads = plan.threads;              // every thread owns <= 4 states and <= 2 proteins (register-cached contexts in the kernel)
      if (rosw_fused) {
        const size_t lb = pk::net_solve_fused_lds_bytes(n->d, n->nnzT);
        const hipError_t ef = measure ? pk::launch_net_lds_measure(n->d, a, (long long)B, threads, lb, stream)
                                      : pk::launch_net_lds_fused(n->d, a, (long long)B, threads, lb, stream);
        if (ef != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(ef));
        break;
      }
      if (M == 0)      hipLaunchKernelGGL(pk::net_solve_kernel<0>, dim3((unsigned)B), dim3(threads), n->solve_lds_bytes, stream, n->d, a);
      else if (M == 1) hipLaunchKernelGGL(pk::net_solve_kernel<1>, dim3((unsigned)B), dim3(threads), n->solve_lds_bytes, stream, n->d, a);
      else if (M == 2) hipLaunchKernelGGL(pk::net_solve_kernel<2>, dim3((unsigned)B), dim3(threads), n->solve_lds_bytes, stream, n->d, a);
      else             hipLaunchKernelGGL(pk::net_solve_kernel<4>, dim3((unsigned)B), dim3(threads), n->solve_lds_bytes, stream, n->d, a);
      break;
    }
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PK_OK : pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(e));
}

int64_t pk_network_workspace_bytes(pk_ctx* c, const pk_net* n, int64_t B) {
  if (!c || !n) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  int grid = 0;
  if (pk::net_ws_grid(n->d, (long long)B, &grid) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "occupancy query");
  return (int64_t)grid * (int64_t)(pk::net_ws_slab_doubles(n->d) * sizeof(double));
}

int pk_network_simulate_batch(pk_ctx* c, pk_net* n, int64_t B, const double* x, int x_is_raw, const double* y0, int y0_is_batched,
                              const double* t_host, int T, const pk_solver_opts* opts_in, double* Y, int32_t* status, int32_t* n_steps) {
  pk::NetSolveArgs a;
  std::memset(&a, 0, sizeof(a));
  return net_simulate_impl(c, n, B, x, x_is_raw, y0, y0_is_batched, t_host, T, opts_in, Y, status, n_steps, NetFlavour::Plain, a);
}

// the caller's scoring arguments of the two loss entry points; without lambdas the three objectives weigh 1 and the prior 0
static void net_fill_loss(pk::NetSolveArgs& f, int loss_mode, const double* defaults, const double* lambdas, double fail_value, double* loss_sums,
                          double* F) {
  f.loss_defaults = defaults; f.loss_mode = loss_mode; f.loss_fail = fail_value; f.loss_sums = loss_sums; f.loss_F = F;
  for (int k = 0; k < 4; ++k) f.loss_lam[k] = lambdas ? lambdas[k] : k < 3 ? 1.0 : 0.0;
}

// simulate + three-objective loss in ONE launch (SURVEY fused op (i), VERDICT r2 item 4 iii): the integrator scores the observations of the
// loss handle at its output times; the trajectory is written only when Y != null.  Same F / loss_sums as pk_network_simulate_batch followed
// by pk_network_objective_batch (up to the order of the sums).  PK_ERR_UNSUPPORTED when the network / options / loss data do not take the path.
// By default that path is the dense-lane additive kernel (topologies 0 / 1 / 4).  On request -- opts->method = PK_METHOD_ROS34PW2 or
// opts->kernel = PK_KERNEL_WORKSPACE -- the order-3 LDS / workspace kernels score the loss handle's time-bucketed lists: every topology,
// every size, duplicate observations allowed.
int pk_loss_fused_tables(const pk_loss* l, const double** obs, const double** w, double* norms, int* T, int* rna_base);
int pk_loss_fused_lists(const pk_loss* l, const int32_t** ptr, const int32_t** prot, const int32_t** site, const double** obs, const double** w,
                        double* norms, int* T, int* rna_base);
int pk_network_simulate_objective_batch(pk_ctx* c, pk_net* n, pk_loss* l, int64_t B, const double* x, int x_is_raw, const double* y0,
                                        int y0_is_batched, const double* t_host, int T, const pk_solver_opts* opts, int loss_mode,
                                        const double* defaults, const double* lambdas, double fail_value, double* Y, int32_t* status,
                                        int32_t* n_steps, double* loss_sums, double* F) {
  if (!c || !n || !l) return PK_ERR_ARG;
  if (B == 0) return PK_OK;
  if (!loss_sums && !F) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (F && !lambdas) return pk_ctx_fail(c, PK_ERR_ARG, "lambdas (protein, rna, phospho, prior) are required for F");
  if (loss_mode < 0 || loss_mode > 7) return pk_ctx_fail(c, PK_ERR_ARG, "loss_mode must be 0..7");
  pk::NetSolveArgs f;
  std::memset(&f, 0, sizeof(f));
  int Tl = 0;
  const bool lists = opts && (opts->method == PK_METHOD_ROS34PW2 || opts->kernel == PK_KERNEL_WORKSPACE);
  if (lists) {
    if (!pk_loss_fused_lists(l, &f.loss_ptr, &f.loss_prot, &f.loss_site, &f.loss_lobs, &f.loss_lw, f.loss_norm, &Tl, &f.loss_rna_base))
      return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "fused objective: protein / phospho baselines must be time index 0 and rna observations not earlier "
                                                "than the rna baseline");
  } else if (!pk_loss_fused_tables(l, &f.loss_obs, &f.loss_w, f.loss_norm, &Tl, &f.loss_rna_base))
    return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "fused objective: protein / phospho baselines must be time index 0, rna observations not earlier than "
                                              "the rna baseline, and no (state, time) observed twice");
  if (Tl != T) return pk_ctx_fail(c, PK_ERR_ARG, "T differs from the grid the loss data were created for");
  net_fill_loss(f, loss_mode, defaults, lambdas, fail_value, loss_sums, F);
  return net_simulate_impl(c, n, B, x, x_is_raw, y0, y0_is_batched, t_host, T, opts, Y, status, n_steps,
                           lists ? NetFlavour::ScoreLists : NetFlavour::ScoreTables, f);
}

// simulate + fold-change observables + scalar Morris metric in ONE launch (SURVEY fused op (iii) on the network path; the reference's
// sensitivity worker, sensitivity.py:143-168): the order-3 LDS / workspace kernels measure the handle's time-bucketed index lists at their
// output rows and reduce them per candidate.  Same status / n_steps / Y as pk_network_simulate_batch for the same opts; pred equals
// pk_network_observables_batch on that trajectory (same operands, same order).
int pk_loss_measure_lists(const pk_loss* l, const int32_t** ptr, const int32_t** prot, const int32_t** site, const int32_t** perm, int* n_obs,
                          int* T, int* rna_base);
int pk_network_simulate_measure_batch(pk_ctx* c, pk_net* n, pk_loss* l, int64_t B, const double* x, int x_is_raw, const double* y0,
                                      int y0_is_batched, const double* t_host, int T, const pk_solver_opts* opts, double eps, int metric_id,
                                      double* Y, double* pred, double* metric, int32_t* status, int32_t* n_steps) {
  if (!c || !n || !l) return PK_ERR_ARG;
  if (metric_id < PK_NET_METRIC_TOTAL_SIGNAL || metric_id > PK_NET_METRIC_L2_NORM) return pk_ctx_fail(c, PK_ERR_ARG, "metric_id must be PK_NET_METRIC_* (0..3)");
  if (B == 0) return PK_OK;
  if (!metric && !pred && !Y) return pk_ctx_fail(c, PK_ERR_ARG, "metric, pred and Y are all NULL: nothing to compute");
  pk::NetSolveArgs f;
  std::memset(&f, 0, sizeof(f));
  int Tl = 0;
  if (!pk_loss_measure_lists(l, &f.loss_ptr, &f.loss_prot, &f.loss_site, &f.meas_perm, &f.meas_n, &Tl, &f.loss_rna_base))
    return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "fused measurement: protein / phospho baselines must be time index 0 and rna observations not earlier than "
                                              "the rna baseline; call pk_network_simulate_batch + pk_network_observables_batch");
  if (Tl != T) return pk_ctx_fail(c, PK_ERR_ARG, "T differs from the grid the index lists were created for");
  f.meas = 1; f.meas_id = metric_id; f.meas_eps = eps; f.meas_pred = pred; f.meas_metric = metric;
  return net_simulate_impl(c, n, B, x, x_is_raw, y0, y0_is_batched, t_host, T, opts, Y, status, n_steps, NetFlavour::Measure, f);
}

int pk_network_sens_columns_per_launch(pk_net* n) { return n ? net_sens_lds_columns(n, false) : PK_ERR_ARG; }
int pk_network_objective_grad_columns_per_launch(pk_net* n) { return n ? net_sens_lds_columns(n, true) : PK_ERR_ARG; }

// Columns one work item of the slab route carries: min(K, n_var, W), W = 16 (DESIGN 5.9 records the measurement behind it); the dev knob
// PK_NET_SENS_KC lowers W as it lowers the LDS counts (read at every call).  The width is the same for both flavours: `scoring` is part of
// the signature so that it may differ one day.  Host arithmetic only
int pk_network_sens_hbm_columns(pk_net* n, int K, int scoring) {
  if (!n || K < 0) return PK_ERR_ARG;
  (void)scoring;
  return pk::net_sens_hbm_columns(K, n->d.n_var, net_switches().sens_hbm_width);
}

// Bytes of slabs a launch of the slab route reserves: grid x slab, grid = min(B x chunks, resident workgroups of the flavour's kernel) -- bounded
// in B.  (The launch stages the K column indices in front of the slabs: 4 K bytes, in whole 128-B lines, on top of this figure)
int64_t pk_network_sens_workspace_bytes(pk_ctx* c, pk_net* n, int64_t B, int K, int scoring) {
  if (!c || !n) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (K < 1 || K > n->d.n_var) return pk_ctx_fail(c, PK_ERR_ARG, "K must be in [1, n_var]");
  if (B > 0x7fffffffLL) return pk_ctx_fail(c, PK_ERR_ARG, "batch too large for one launch");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  const int kc = pk_network_sens_hbm_columns(n, K, scoring), n_chunks = (K + kc - 1) / kc;
  int grid = 0;
  if (pk::net_sens_ws_grid(n->d, scoring != 0, (long long)B * n_chunks, &grid) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "occupancy query");
  return (int64_t)grid * (int64_t)(pk::net_sens_ws_slab_doubles(n->d, kc, scoring != 0) * sizeof(double));
}

// cols (HOST pointer, not null) names K distinct parameters
static int net_check_cols(pk_ctx* c, const pk_net* n, const int32_t* cols_host, int K) {
  std::vector<char> seen((size_t)n->d.n_var, 0);
  for (int k = 0; k < K; ++k) {
    const int col = cols_host[k];
    if (col < 0 || col >= n->d.n_var) return pk_ctx_fail(c, PK_ERR_ARG, "cols: index outside [0, n_var)");
    if (seen[col]) return pk_ctx_fail(c, PK_ERR_ARG, "cols: an index is repeated");
    seen[col] = 1;
  }
  return PK_OK;
}

// Y and dY / dx[cols] from one integration of the augmented system (pk_network_sens.hpp).  Always the order-3 method: on the general LDS
// kernel where a column fits beside the state, else -- and with PK_KERNEL_HBM -- on HBM slabs.  K = 0 is pk_network_simulate_batch on the
// general LDS kernel (PK_KERNEL_HBM: on the workspace kernel)
int pk_network_simulate_sens_batch(pk_ctx* c, pk_net* n, int64_t B, const double* x, int x_is_raw, const double* y0, int y0_is_batched,
                                   const double* t_host, int T, const pk_solver_opts* opts, const int32_t* cols_host, int K, double* Y,
                                   double* dY, int32_t* status, int32_t* n_steps) {
  if (!c || !n) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (K < 0) return pk_ctx_fail(c, PK_ERR_ARG, "K must be >= 0");
  const pk_solver_opts asked = net_opts(opts), o = pk::net_tangent_opts(asked);
  const NetSensReq req{cols_host, K, dY, nullptr, pk::net_plan(net_facts(n), asked, NetFlavour::Sens, K, net_switches())};
  if (req.plan.code != PK_OK) return pk_ctx_fail(c, req.plan.code, req.plan.refusal);
  if (K > 0) {
    if (!cols_host) return pk_ctx_fail(c, PK_ERR_ARG, "cols is NULL with K > 0");
    if (!dY) return pk_ctx_fail(c, PK_ERR_ARG, "dY is NULL with K > 0");
    if (const int rc = net_check_cols(c, n, cols_host, K)) return rc;
  } else if (!Y && B > 0) return pk_ctx_fail(c, PK_ERR_ARG, "K = 0 and Y is NULL: nothing to compute");
  if (B == 0) return PK_OK;
  pk::NetSolveArgs a;
  std::memset(&a, 0, sizeof(a));
  if (K == 0) return net_simulate_impl(c, n, B, x, x_is_raw, y0, y0_is_batched, t_host, T, &o, Y, status, n_steps, NetFlavour::Plain, a);
  return net_simulate_impl(c, n, B, x, x_is_raw, y0, y0_is_batched, t_host, T, &o, Y, status, n_steps, NetFlavour::Sens, a, &req);
}

// The three objectives AND their derivative with respect to x[cols] from one integration of the augmented system: the scoring flavour of
// the sensitivity kernel differentiates the loss where state and tangents land on an output row (pk_network_sens.hpp); neither the
// trajectory nor the tangent trajectory reaches HBM as an output unless Y / dY are asked for.  Rules of pk_network_simulate_sens_batch (order-3
// method, general LDS kernel or HBM slabs, cols checked here) and of the order-3 fused objective (the time-bucketed lists).  K = 0 is
// pk_network_simulate_objective_batch with PK_METHOD_ROS34PW2 / PK_LINSOLVE_STRUCTURED (PK_KERNEL_HBM: with PK_KERNEL_WORKSPACE)
int pk_network_simulate_objective_grad_batch(pk_ctx* c, pk_net* n, pk_loss* l, int64_t B, const double* x, int x_is_raw, const double* y0,
                                             int y0_is_batched, const double* t_host, int T, const pk_solver_opts* opts, const int32_t* cols_host,
                                             int K, int loss_mode, const double* defaults, const double* lambdas, double fail_value, double* Y,
                                             double* dY, double* pred, double* dpred, double* loss_sums, double* dsums, double* F, double* dF,
                                             int32_t* status, int32_t* n_steps) {
  if (!c || !n || !l) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (K < 0) return pk_ctx_fail(c, PK_ERR_ARG, "K must be >= 0");
  const pk_solver_opts asked = net_opts(opts), o = pk::net_tangent_opts(asked);
  const pk::NetSensScoreArgs sc{dpred, dsums, dF};
  const NetSensReq req{cols_host, K, dY, &sc, pk::net_plan(net_facts(n), asked, NetFlavour::SensScore, K, net_switches())};
  if (req.plan.code != PK_OK) return pk_ctx_fail(c, req.plan.code, req.plan.refusal);
  if (loss_mode < 0 || loss_mode > 7) return pk_ctx_fail(c, PK_ERR_ARG, "loss_mode must be 0..7");
  if (!Y && !dY && !pred && !dpred && !loss_sums && !dsums && !F && !dF)
    return pk_ctx_fail(c, PK_ERR_ARG, "every output pointer is NULL: pass at least one of Y, dY, pred, dpred, loss_sums, dsums, F, dF");
  if (K > 0 && !dY && !dpred && !dsums && !dF)
    return pk_ctx_fail(c, PK_ERR_ARG, "K > 0 but dY, dpred, dsums and dF are all NULL: pass one of them, or K = 0 for the objectives alone");
  if ((F || dF) && !lambdas) return pk_ctx_fail(c, PK_ERR_ARG, "lambdas (protein, rna, phospho, prior) are required for F and dF");
  if (K > 0) {
    if (!cols_host) return pk_ctx_fail(c, PK_ERR_ARG, "cols is NULL with K > 0");
    if (const int rc = net_check_cols(c, n, cols_host, K)) return rc;
  }
  if (K == 0) {
    if (pred || (!loss_sums && !F))
      return pk_ctx_fail(c, PK_ERR_ARG, "K = 0 computes loss_sums / F (and Y) as pk_network_simulate_objective_batch does: pass one of them, and ask "
                                        "pk_network_simulate_measure_batch for pred");
    return pk_network_simulate_objective_batch(c, n, l, B, x, x_is_raw, y0, y0_is_batched, t_host, T, &o, loss_mode, defaults, lambdas, fail_value, Y,
                                               status, n_steps, loss_sums, F);
  }
  pk::NetSolveArgs f;
  std::memset(&f, 0, sizeof(f));
  int Tl = 0, Tm = 0, rb = 0;
  const int32_t *p2 = nullptr, *pr2 = nullptr, *si2 = nullptr;
  if (!pk_loss_fused_lists(l, &f.loss_ptr, &f.loss_prot, &f.loss_site, &f.loss_lobs, &f.loss_lw, f.loss_norm, &Tl, &f.loss_rna_base) ||
      !pk_loss_measure_lists(l, &p2, &pr2, &si2, &f.meas_perm, &f.meas_n, &Tm, &rb))
    return pk_ctx_fail(c, PK_ERR_UNSUPPORTED, "objective gradients: protein / phospho baselines must be time index 0 and rna observations not earlier "
                                              "than the rna baseline; difference pk_network_simulate_batch + pk_network_objective_batch");
  if (Tl != T) return pk_ctx_fail(c, PK_ERR_ARG, "T differs from the grid the loss data were created for");
  if (B == 0) return PK_OK;
  net_fill_loss(f, loss_mode, defaults, lambdas, fail_value, loss_sums, F);
  f.meas_pred = pred;
  return net_simulate_impl(c, n, B, x, x_is_raw, y0, y0_is_batched, t_host, T, &o, Y, status, n_steps, NetFlavour::SensScore, f, &req);
}

int pk_network_unpack_batch(pk_ctx* c, pk_net* n, int64_t B, const double* x_raw, double* x_phys) {
  if (!c || !n) return PK_ERR_ARG;
  if (B < 0) return pk_ctx_fail(c, PK_ERR_ARG, "B must be >= 0");
  if (B == 0) return PK_OK;
  if (!x_raw || !x_phys) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  const long long total = (long long)B * n->d.n_var;
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  hipLaunchKernelGGL(pk::net_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)pk_ctx_stream(c), x_raw, x_phys, total);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PK_OK : pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(e));
}

}  // extern "C"
