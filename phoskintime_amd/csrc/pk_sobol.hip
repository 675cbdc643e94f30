// pk_sobol.hip -- variance-based (Sobol') sensitivity around the solve: the Saltelli design is BUILT in HBM from the two base samples and
// the first-order / total indices of M outputs, with their bootstrap spread, are reduced from the [N (D + 2), M] output matrix without
// leaving the GPU.
//
// Reference: scripts/temporal_sensitivity.py:143-188 calls SALib's saltelli.sample(calc_second_order=False) -> N (D + 2) x D host matrix ->
// process pool -> sobol.analyze once per time point (100 bootstrap resamples each), and all of that once per protein.  SALib is absent
// here; the estimator is the one of its analyze(calc_second_order=False) (Saltelli et al. 2010, first order; Jansen 1999, total), restated
// in sensitivity/sobol.py, which is also the host twin these kernels are held to.
//
// Row layout (saltelli.sample): for each i: A_i, then AB_i1 .. AB_iD (A_i with column j taken from B_i), then B_i.
//
// Indices.  One thread owns one (j, m) pair and a chunk of kSlots "slots": slot 0 is the plain estimate (weight 1), slot s >= 1 is
// bootstrap resample s - 1 (weight counts[s - 1, i]).  Lanes run along m, so a row of Y is read coalesced; the weight of a slot depends on
// the block and on i only, so its load is wave-uniform.  A thread walks i = 0 .. N - 1 in increasing order and keeps 4 sums per slot in
// registers; there are no atomics and no cross-lane sums over i, so a (j, m) entry does not depend on D, M, R or the grid around it.
// The remaining chunks and the j range go over the grid: Y is re-read ceil((R + 1) / kSlots) times, not R times.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include "../../include/phoskin.h"

struct pk_ctx;
extern "C" int pk_ctx_device(pk_ctx*);
extern "C" void* pk_ctx_stream(pk_ctx*);
extern "C" int pk_ctx_fail(pk_ctx*, int code, const char* msg);
extern "C" int pk_ctx_scratch_launch(pk_ctx*, size_t bytes, hipError_t (*launch)(void* scratch, hipStream_t stream, void* user), void* user);

namespace pk {

constexpr int kSlots = 8;        // slots per thread: 4 kSlots sums in registers (see the resource ledger in DESIGN)
constexpr int kLanes = 64;       // block = kLanes columns x kRowsJ values of j; one wave = one j
constexpr int kRowsJ = 4;

// X[(i (D + 2) + s) D + k], one thread per element: s = 0 -> A, s = D + 1 -> B, else A with column s - 1 from B; scaled to [lb_k, ub_k]
__global__ void sobol_build_kernel(const long long total, const int D, const double* __restrict__ A, const double* __restrict__ B,
                                   const double* __restrict__ lb, const double* __restrict__ ub, double* __restrict__ X) {
#pragma clang fp contract(off)      // separately rounded mul / add: the matrix is bit-identical to the host builder (sensitivity/sobol.py build())
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const int k = (int)(g % D);
  const long long row = g / D;
  const int s = (int)(row % (D + 2));
  const long long i = row / (D + 2);
  const bool from_b = (s == D + 1) || (s == k + 1);
  const double u = from_b ? B[i * D + k] : A[i * D + k];
  X[g] = lb[k] + u * (ub[k] - lb[k]);
}

// First pass: mean[m] = mean over all rows of y - y[0] in column m, NaN when the column's maximum equals its minimum (the constant-column
// rule: the NaN then runs through every sum of that column).  Row r goes to partial r mod kRowsJ; the partials are added in a fixed
// order, so the mean depends on the column alone.  A value is centred as (y - y[0]) - mean[m]: nothing is rounded at the size of the
// column's offset, which may dwarf its spread.
__global__ __launch_bounds__(kLanes * kRowsJ) void sobol_colstat_kernel(const long long rows, const long long M, const double* __restrict__ Y,
                                                                         double* __restrict__ mean) {
  __shared__ double s_sum[kRowsJ][kLanes], s_min[kRowsJ][kLanes], s_max[kRowsJ][kLanes];
  const long long m = (long long)blockIdx.x * kLanes + threadIdx.x;
  const int q = threadIdx.y;
  double sum = 0.0, lo = INFINITY, hi = -INFINITY, y0 = 0.0;
  if (m < M) {
    y0 = Y[m];
    for (long long r = q; r < rows; r += kRowsJ) {
      const double y = Y[r * M + m];
      sum += y - y0;
      lo = fmin(lo, y); hi = fmax(hi, y);
    }
  }
  s_sum[q][threadIdx.x] = sum; s_min[q][threadIdx.x] = lo; s_max[q][threadIdx.x] = hi;
  __syncthreads();
  if (q == 0 && m < M) {
    for (int k = 1; k < kRowsJ; ++k) {
      sum += s_sum[k][threadIdx.x];
      lo = fmin(lo, s_min[k][threadIdx.x]); hi = fmax(hi, s_max[k][threadIdx.x]);
    }
    mean[m] = (hi == lo) ? (double)NAN : sum / (double)rows;
  }
}

// Main pass.  grid = (ceil(M / kLanes), ceil(D / kRowsJ), ceil((R + 1) / kSlots)), block = (kLanes, kRowsJ).
//   per slot:  s1 = sum c (a + b),  s2 = sum c (a^2 + b^2),  p1 = sum c b (ab - a),  pt = sum c (a - ab)^2      (a, b, ab centred)
//   var = s2 / 2N - (s1 / 2N)^2,   S1 = p1 / N / var,   ST = pt / 2N / var                                      (sum c = N in every slot)
// Slot 0 writes S1 / ST [D, M] (and var [M] from j = 0); slot s >= 1 writes its pair to r1 / rt [R, D, M] for the spread kernel.
__global__ __launch_bounds__(kLanes * kRowsJ) void sobol_sums_kernel(const int N, const int D, const long long M, const int R,
                                                                      const double* __restrict__ Y, const int32_t* __restrict__ counts,
                                                                      const double* __restrict__ mean, double* __restrict__ S1,
                                                                      double* __restrict__ ST, double* __restrict__ var,
                                                                      double* __restrict__ r1, double* __restrict__ rt) {
  const long long m = (long long)blockIdx.x * kLanes + threadIdx.x;
  const int j = (int)blockIdx.y * kRowsJ + (int)threadIdx.y;
  const int slot0 = (int)blockIdx.z * kSlots;
  if (m >= M || j >= D) return;
  const double y0 = Y[m], mu = mean[m];
  double s1[kSlots], s2[kSlots], p1[kSlots], pt[kSlots];
#pragma unroll
  for (int q = 0; q < kSlots; ++q) s1[q] = s2[q] = p1[q] = pt[q] = 0.0;
  const long long stride = (long long)(D + 2) * M;
  const double* ya = Y + m;
  for (int i = 0; i < N; ++i, ya += stride) {
    const double a = (ya[0] - y0) - mu;
    const double ab = (ya[(long long)(j + 1) * M] - y0) - mu;
    const double b = (ya[(long long)(D + 1) * M] - y0) - mu;
    const double t1 = a + b, t2 = a * a + b * b, d = ab - a, u = b * d, v = d * d;
#pragma unroll
    for (int q = 0; q < kSlots; ++q) {
      const int s = slot0 + q;                                               // wave-uniform: block index and loop counters only
      const double c = s == 0 ? 1.0 : (s <= R ? (double)counts[(long long)(s - 1) * N + i] : 0.0);
      s1[q] += c * t1; s2[q] += c * t2; p1[q] += c * u; pt[q] += c * v;
    }
  }
  const double n2 = 2.0 * (double)N;
  const long long dm = (long long)D * M, jm = (long long)j * M + m;
#pragma unroll
  for (int q = 0; q < kSlots; ++q) {
    const int s = slot0 + q;
    const double e = s1[q] / n2;
    const double vr = s2[q] / n2 - e * e;
    const double f = p1[q] / (double)N / vr, g = pt[q] / n2 / vr;
    if (s == 0) {
      S1[jm] = f; ST[jm] = g;
      if (j == 0 && var) var[m] = vr;
    } else if (s <= R) {
      r1[(long long)(s - 1) * dm + jm] = f; rt[(long long)(s - 1) * dm + jm] = g;
    }
  }
}

// ddof-1 standard deviation over the R resamples of every (j, m), two passes in resample order; one thread per entry
__global__ void sobol_spread_kernel(const long long dm, const int R, const double* __restrict__ r1, const double* __restrict__ rt,
                                    double* __restrict__ S1_sd, double* __restrict__ ST_sd) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= dm) return;
  double m1 = 0.0, mt = 0.0;
  for (int r = 0; r < R; ++r) { m1 += r1[(long long)r * dm + g]; mt += rt[(long long)r * dm + g]; }
  m1 /= (double)R; mt /= (double)R;
  double q1 = 0.0, qt = 0.0;
  for (int r = 0; r < R; ++r) {
    const double d1 = r1[(long long)r * dm + g] - m1, dt = rt[(long long)r * dm + g] - mt;
    q1 += d1 * d1; qt += dt * dt;
  }
  S1_sd[g] = sqrt(q1 / (double)(R - 1)); ST_sd[g] = sqrt(qt / (double)(R - 1));
}

struct SobolArgs {
  int N, D, R; long long M;
  const double* Y; const int32_t* counts;
  double *S1, *ST, *S1_sd, *ST_sd, *var;
};

size_t sobol_align(size_t b) { return (b + 255) / 256 * 256; }

// scratch: mean [M] | r1 [R, D, M] | rt [R, D, M]
hipError_t sobol_launch(void* scratch, hipStream_t stream, void* user) {
  const SobolArgs& a = *static_cast<const SobolArgs*>(user);
  const long long dm = (long long)a.D * a.M;
  double* mean = static_cast<double*>(scratch);
  double* r1 = reinterpret_cast<double*>(static_cast<char*>(scratch) + sobol_align(sizeof(double) * (size_t)a.M));
  double* rt = r1 + (size_t)a.R * (size_t)dm;
  const unsigned gx = (unsigned)((a.M + kLanes - 1) / kLanes);
  hipLaunchKernelGGL(sobol_colstat_kernel, dim3(gx), dim3(kLanes, kRowsJ), 0, stream, (long long)a.N * (a.D + 2), a.M, a.Y, mean);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sobol_sums_kernel, dim3(gx, (unsigned)((a.D + kRowsJ - 1) / kRowsJ), (unsigned)((a.R + kSlots) / kSlots)), dim3(kLanes, kRowsJ), 0,
                     stream, a.N, a.D, a.M, a.R, a.Y, a.counts, mean, a.S1, a.ST, a.var, r1, rt);
  e = hipGetLastError();
  if (e != hipSuccess || a.R == 0) return e;
  hipLaunchKernelGGL(sobol_spread_kernel, dim3((unsigned)((dm + 255) / 256)), dim3(256), 0, stream, dm, a.R, r1, rt, a.S1_sd, a.ST_sd);
  return hipGetLastError();
}

}  // namespace pk

extern "C" {

int pk_sobol_build_batch(pk_ctx* c, int64_t N, int D, const double* A, const double* B, const double* lb, const double* ub, double* X) {
  if (!c) return PK_ERR_ARG;
  if (N < 1 || D < 1) return pk_ctx_fail(c, PK_ERR_ARG, "N must be >= 1 and D >= 1");
  if (!A || !B || !lb || !ub || !X) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (N > 0x7fffffffffffLL / ((long long)(D + 2) * D)) return pk_ctx_fail(c, PK_ERR_ARG, "sample too large for one launch");
  const long long total = (long long)N * (D + 2) * D;
  if ((total + 255) / 256 > 0x7fffffffLL) return pk_ctx_fail(c, PK_ERR_ARG, "sample too large for one launch");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  hipLaunchKernelGGL(pk::sobol_build_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)pk_ctx_stream(c), total, D, A, B, lb, ub, X);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PK_OK : pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(e));
}

int pk_sobol_indices_batch(pk_ctx* c, int64_t N, int D, int64_t M, const double* Y, const int32_t* counts, int R, double* S1, double* ST,
                           double* S1_sd, double* ST_sd, double* var) {
  if (!c) return PK_ERR_ARG;
  if (N < 1 || D < 1 || M < 0 || R < 0 || R == 1) return pk_ctx_fail(c, PK_ERR_ARG, "N >= 1, D >= 1, M >= 0 and R = 0 or R >= 2 required");
  if (M == 0) return PK_OK;
  if (!Y || !S1 || !ST) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (R >= 2 && (!counts || !S1_sd || !ST_sd)) return pk_ctx_fail(c, PK_ERR_ARG, "R >= 2 needs counts, S1_sd and ST_sd");
  // grid limits: x < 2^31 blocks, y and z <= 65535; N is the trip count of an int loop; the element counts must fit 64-bit indices
  const long long gx = (M + pk::kLanes - 1) / pk::kLanes, gy = ((long long)D + pk::kRowsJ - 1) / pk::kRowsJ, gz = ((long long)R + pk::kSlots) / pk::kSlots;
  if (N > 0x7fffffffLL || gx > 0x7fffffffLL || gy > 65535 || gz > 65535 || M > 0x7fffffffffffLL / ((long long)D + 2) / N ||
      ((long long)D * M + 255) / 256 > 0x7fffffffLL || (R > 0 && (long long)D * M > 0x3fffffffffffLL / R))
    return pk_ctx_fail(c, PK_ERR_ARG, "indices: too large for one launch");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  pk::SobolArgs a{(int)N, D, R, (long long)M, Y, counts, S1, ST, S1_sd, ST_sd, var};
  const size_t bytes = pk::sobol_align(sizeof(double) * (size_t)M) + 2 * sizeof(double) * (size_t)R * (size_t)D * (size_t)M;
  return pk_ctx_scratch_launch(c, bytes, pk::sobol_launch, &a);
}

}  // extern "C"
