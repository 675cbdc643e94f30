// pk_moo.hip -- the bookkeeping of a reference-direction many-objective search (U-NSGA-III as the reference's calibration runs it,
// global_model/runner.py:663-699: pymoo's UNSGA3 with SBX / PM) without a host round trip: non-dominated ranks, association with the
// reference directions, niching survival and mating (tournament, bounded SBX, bounded polynomial mutation) on arrays that stay in HBM.
// global_model/search.py is the loop around these four entry points; tests/moo_reference.py is the numpy twin they are held to.
//
// Rank.       Peeling, front after front, with one remembered dominator per row.  A row is alive while its rank is < 0.  A pass is three
//             launches: (1) every alive row whose remembered dominator is still alive stays dominated and does nothing; the others are
//             appended to a work list; (2) the list is scanned against every alive row j -- grid = list chunks x kSlices slices of j,
//             one thread per listed row, the j rows of a slice staged through LDS in tiles of kTile rows; a dead or non-finite j is
//             staged as a row of +inf, which dominates nothing, and a non-finite row i is compared as a row of +inf, which every finite
//             row dominates and no +inf row does; the first dominator a thread finds is remembered (slices race for the slot; every
//             value they can leave there is a true dominator, and the ranks do not depend on which); (3) listed rows without a
//             dominator form the front and are counted into one int32 in HBM (n_fronts[0] serves as that counter until the last
//             launch writes the front count there), which the host reads -- 4 bytes per front -- to decide whether to go on.  A row is
//             rescanned only when its remembered dominator is peeled, so the compares of all passes together stay near those of the
//             first, P^2, instead of P^2 per front.  No P x P object exists anywhere; scratch is two int32 per row.
// Associate.  One thread per row, the H directions in LDS (dynamic, H M doubles <= 128 KiB); argmin over h in increasing h, strict <.
// Survive.    Three launches.  (1) one workgroup: the last front l by bisection on #{rank < l}; the niche counts rho (taken rows) and
//             a (last-front rows) by LDS atomics; the water level L by bisection on S(L) = sum_j min(a_j, max(0, L -
//             rho_j)); the per-niche quota c_j, with the remainder dealt one each to the lowest-j niches standing at L by a block scan.
//             (2) every last-front row counts the rows of its niche and front that stand before it in (dist, index) -- grid = row
//             chunks x kSlices slices of j, LDS tiles again, dist as a monotone integer key with NaN last, the slices' counts added
//             atomically (integers: the sum does not depend on their order).  (3) one workgroup keeps the rows of earlier fronts and the
//             last-front rows whose count is below their niche's quota c_j, compacted into ascending indices.
// Mate.       One wave per offspring pair, lanes over variables; every random number is a pure function of (seed, gen, stream, row, var).
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

constexpr int kTile = 256;            // rows per LDS tile = threads per block of the pairwise kernels
constexpr int kOne = 1024;            // threads of the single-workgroup kernels
constexpr int kMaxP = 65536, kMaxH = 4096;

// ---------------------------------------------------------------- rank

constexpr int kSlices = 16;           // the j range of a scan is cut into this many slices (grid.y): 64 list chunks x 16 = 1024 blocks at P = 16384

// dom[i]: a row known to dominate row i, -1 when none is known.  list / list_n[2]: the rows to scan in this pass and their count; pass f
// appends through list_n[f & 1] and clears the other one for the next pass.
__global__ void moo_rank_init_kernel(const int P, int32_t* __restrict__ rank, int32_t* __restrict__ dom, int32_t* __restrict__ list_n,
                                     int32_t* __restrict__ counter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) { rank[i] = -1; dom[i] = -1; }
  if (i == 0) { counter[0] = 0; list_n[0] = 0; list_n[1] = 0; }
}

__global__ __launch_bounds__(kTile) void moo_rank_list_kernel(const int P, const int front, const int32_t* __restrict__ rank, int32_t* __restrict__ dom,
                                                              int32_t* __restrict__ list, int32_t* __restrict__ list_n) {
  __shared__ int s_n, s_at;
  const int i = blockIdx.x * kTile + threadIdx.x;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  bool scan = false;
  if (i < P && rank[i] < 0) {
    const int d = dom[i];
    scan = d < 0 || rank[d] >= 0;                          // no dominator known, or the known one has been peeled
  }
  int at = 0;
  if (scan) { at = atomicAdd(&s_n, 1); dom[i] = -1; }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) s_at = atomicAdd(&list_n[front & 1], s_n);
  __syncthreads();
  if (scan) list[s_at + at] = i;                           // s_at + at < P: every row is appended at most once
}

template <int M>
__global__ __launch_bounds__(kTile) void moo_rank_scan_kernel(const int P, const int front, const int slice, const double* __restrict__ F,
                                                              const int32_t* __restrict__ rank, const int32_t* __restrict__ list,
                                                              const int32_t* __restrict__ list_n, int32_t* __restrict__ dom) {
  __shared__ double s_f[kTile][M];
  const int n_list = list_n[front & 1];
  if ((int)blockIdx.x * kTile >= n_list) return;           // block-uniform
  const int q = blockIdx.x * kTile + threadIdx.x;
  const int i = q < n_list ? list[q] : -1;
  double fi[M];
  bool fin = true;
#pragma unroll
  for (int m = 0; m < M; ++m) { fi[m] = i >= 0 ? F[(size_t)i * M + m] : 0.0; fin = fin && isfinite(fi[m]); }
  if (!fin) {
#pragma unroll
    for (int m = 0; m < M; ++m) fi[m] = INFINITY;
  }
  int found = i >= 0 ? -1 : 0;                             // idle threads count as settled
  const int j_begin = (int)blockIdx.y * slice, j_end = min(P, j_begin + slice);
  for (int j0 = j_begin; j0 < j_end; j0 += kTile) {
    const int j = j0 + threadIdx.x;
    const bool live = j < j_end && rank[j] < 0;
    double fj[M];
    bool finj = live;
#pragma unroll
    for (int m = 0; m < M; ++m) { fj[m] = live ? F[(size_t)j * M + m] : INFINITY; finj = finj && isfinite(fj[m]); }
    __syncthreads();                                       // the previous tile has been read
#pragma unroll
    for (int m = 0; m < M; ++m) s_f[threadIdx.x][m] = finj ? fj[m] : INFINITY;
    if (!__syncthreads_or(finj)) continue;                 // a tile without a live finite row dominates nothing
    if (found < 0) {
      const int n = min(kTile, j_end - j0);
      for (int k = 0; k < n && found < 0; ++k) {
        bool le = true, lt = false;
#pragma unroll
        for (int m = 0; m < M; ++m) { const double a = s_f[k][m]; le = le && (a <= fi[m]); lt = lt || (a < fi[m]); }
        if (le && lt) found = j0 + k;
      }
    }
  }
  if (i >= 0 && found >= 0) dom[i] = found;
}

__global__ __launch_bounds__(kTile) void moo_rank_assign_kernel(const int front, const int32_t* __restrict__ list, int32_t* __restrict__ list_n,
                                                                const int32_t* __restrict__ dom, int32_t* __restrict__ rank,
                                                                int32_t* __restrict__ counter) {
  __shared__ int s_cnt;
  const int n_list = list_n[front & 1];
  if (blockIdx.x == 0 && threadIdx.x == 0) list_n[(front + 1) & 1] = 0;      // nobody reads that slot in this pass
  if ((int)blockIdx.x * kTile >= n_list) return;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int q = blockIdx.x * kTile + threadIdx.x;
  if (q < n_list) {
    const int i = list[q];
    if (dom[i] < 0) { rank[i] = front; atomicAdd(&s_cnt, 1); }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(counter, s_cnt);
}

__global__ void moo_rank_finish_kernel(const int P, const int n_fronts, int32_t* __restrict__ rank, int32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P && rank[i] < 0) rank[i] = n_fronts;
  if (i == 0) out[0] = n_fronts;
}

struct RankArgs {
  int P, M, stop_at;
  const double* F; int32_t *rank, *n_fronts;
};

size_t moo_align(size_t b) { return (b + 255) / 256 * 256; }

// scratch: list_n [2] | dom [P] | list [P].  The loop of passes lives here: the scratch stays reserved from the first launch to the last.
hipError_t rank_launch(void* scratch, hipStream_t st, void* user) {
  const RankArgs& a = *static_cast<const RankArgs*>(user);
  const int P = a.P;
  char* p = static_cast<char*>(scratch);
  int32_t* list_n = reinterpret_cast<int32_t*>(p); p += 256;
  int32_t* dom = reinterpret_cast<int32_t*>(p); p += moo_align(sizeof(int32_t) * (size_t)P);
  int32_t* list = reinterpret_cast<int32_t*>(p);
  const unsigned nb = (unsigned)((P + kTile - 1) / kTile);
  const int slices = (int)nb < kSlices ? (int)nb : kSlices;
  const int slice = (int)((nb + slices - 1) / slices) * kTile;               // rows of j per slice, a whole number of tiles; slices x slice >= P
  hipError_t e;
  hipLaunchKernelGGL(moo_rank_init_kernel, dim3(nb), dim3(kTile), 0, st, P, a.rank, dom, list_n, a.n_fronts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  int front = 0;
  for (int32_t ranked = 0; ranked < P && (a.stop_at == 0 || ranked < a.stop_at); ++front) {
    hipLaunchKernelGGL(moo_rank_list_kernel, dim3(nb), dim3(kTile), 0, st, P, front, a.rank, dom, list, list_n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid(nb, (unsigned)slices);
    switch (a.M) {
      case 2: hipLaunchKernelGGL(moo_rank_scan_kernel<2>, grid, dim3(kTile), 0, st, P, front, slice, a.F, a.rank, list, list_n, dom); break;
      case 3: hipLaunchKernelGGL(moo_rank_scan_kernel<3>, grid, dim3(kTile), 0, st, P, front, slice, a.F, a.rank, list, list_n, dom); break;
      default: hipLaunchKernelGGL(moo_rank_scan_kernel<4>, grid, dim3(kTile), 0, st, P, front, slice, a.F, a.rank, list, list_n, dom); break;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(moo_rank_assign_kernel, dim3(nb), dim3(kTile), 0, st, front, list, list_n, dom, a.rank, a.n_fronts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int32_t was = ranked;
    if ((e = hipMemcpyAsync(&ranked, a.n_fronts, sizeof(int32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;     // the 4 bytes of this front
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (ranked <= was) return hipErrorAssert;              // every pass ranks at least one row: a guard, not a path
  }
  hipLaunchKernelGGL(moo_rank_finish_kernel, dim3(nb), dim3(kTile), 0, st, P, front, a.rank, a.n_fronts);
  return hipGetLastError();
}

// ---------------------------------------------------------------- associate

template <int M>
__global__ __launch_bounds__(kTile) void moo_associate_kernel(const int P, const int H, const double* __restrict__ F,
                                                              const double* __restrict__ ideal, const double* __restrict__ nadir,
                                                              const double* __restrict__ dirs, int32_t* __restrict__ niche,
                                                              double* __restrict__ dist) {
  extern __shared__ double s_w[];                          // [H, M]
  for (int k = threadIdx.x; k < H * M; k += kTile) s_w[k] = dirs[k];
  __syncthreads();
  const int i = blockIdx.x * kTile + threadIdx.x;
  if (i >= P) return;
  double f[M];
  bool fin = true;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double v = F[(size_t)i * M + m];
    fin = fin && isfinite(v);
    f[m] = (v - ideal[m]) / fmax(nadir[m] - ideal[m], 1e-12);
  }
  int best_h = -1;
  double best = INFINITY;
  if (fin) {
    for (int h = 0; h < H; ++h) {
      double fw = 0.0, ww = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) { const double w = s_w[h * M + m]; fw += f[m] * w; ww += w * w; }
      const double s = fw / ww;
      double d2 = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) { const double r = f[m] - s * s_w[h * M + m]; d2 += r * r; }
      const double d = sqrt(d2);
      if (d < best) { best = d; best_h = h; }
    }
  }
  niche[i] = best_h;
  dist[i] = best_h >= 0 ? best : (double)INFINITY;
}

// ---------------------------------------------------------------- survive

// sum of v over the block (every thread gets it); s_red holds kOne / 64 partials
__device__ inline long long block_sum(long long v, long long* s_red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();                                         // s_red free from the previous call
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += s_red[k];
  return t;
}

// plan[0] = last front l, plan[1] = rows of the last front without a niche still to take; quota[j] = c_j; cnt [P] is cleared
__global__ __launch_bounds__(kOne) void moo_survive_plan_kernel(const int P, const int K, const int H, const int32_t* __restrict__ rank,
                                                                const int32_t* __restrict__ niche, int32_t* __restrict__ quota,
                                                                int32_t* __restrict__ plan, int32_t* __restrict__ cnt) {
  __shared__ long long s_red[kOne / 64];
  __shared__ int s_scan[kOne];
  __shared__ int rho[kMaxH], a[kMaxH];                     // taken rows / last-front rows per niche
  const int t = threadIdx.x;
  for (int i = t; i < P; i += kOne) cnt[i] = 0;            // the count kernel adds into it
  // the last front: the largest l with #{rank < l} <= K  (l = P + 1 always counts every row, so K = P ends above every rank)
  int lo = 0, hi = P + 1;                                  // count(lo) = 0 <= K always
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    long long c = 0;
    for (int i = t; i < P; i += kOne) c += rank[i] < mid;
    c = block_sum(c, s_red);
    if (c <= K) lo = mid; else hi = mid - 1;
  }
  const int l = lo;
  for (int j = t; j < H; j += kOne) { rho[j] = 0; a[j] = 0; }
  __syncthreads();
  long long taken = 0, n_niched = 0;
  for (int i = t; i < P; i += kOne) {
    const int r = rank[i], h = niche[i];
    const bool ok = h >= 0 && h < H;
    if (r < l) { ++taken; if (ok) atomicAdd(&rho[h], 1); }
    else if (r == l && ok) { ++n_niched; atomicAdd(&a[h], 1); }
  }
  taken = block_sum(taken, s_red);
  n_niched = block_sum(n_niched, s_red);                   // its barriers also order the LDS atomics above before the reads below
  const long long k_rest = (long long)K - taken;
  const long long k_niched = k_rest < n_niched ? k_rest : n_niched;
  // the water level: the largest L in [0, P] with S(L) <= k_niched  (S(P) counts every last-front row: rho_j + a_j <= P)
  lo = 0; hi = P;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    long long s = 0;
    for (int j = t; j < H; j += kOne) s += min(a[j], max(0, mid - rho[j]));
    s = block_sum(s, s_red);
    if (s <= k_niched) lo = mid; else hi = mid - 1;
  }
  const int L = lo;
  long long s = 0;
  for (int j = t; j < H; j += kOne) s += min(a[j], max(0, L - rho[j]));
  long long rem = k_niched - block_sum(s, s_red);
  // one more each to the lowest-j niches standing at L with rows left; thread t owns the contiguous niches [t per, (t + 1) per)
  const int per = (H + kOne - 1) / kOne;
  int mine = 0;
  for (int j = t * per; j < min(H, (t + 1) * per); ++j) {
    const int c = min(a[j], max(0, L - rho[j]));
    mine += (rho[j] <= L && c < a[j]);
  }
  s_scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < kOne; o <<= 1) {                     // inclusive Hillis-Steele scan
    const int v = t >= o ? s_scan[t - o] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  long long before = s_scan[t] - mine;
  for (int j = t * per; j < min(H, (t + 1) * per); ++j) {
    int c = min(a[j], max(0, L - rho[j]));
    if (rho[j] <= L && c < a[j]) { if (before < rem) ++c; ++before; }
    quota[j] = c;
  }
  if (t == 0) { plan[0] = l; plan[1] = (int)(k_rest - k_niched); }
}

// The place of a row within its niche as one integer: the bits of dist made monotone (negative numbers below positive, -0 = +0, every
// NaN above +inf), so "(dist, index) before" is two integer compares whatever dist holds.  Rows without a niche go by index alone.
__device__ inline unsigned long long moo_dist_key(const double d, const bool niched) {
  if (!niched) return 0ULL;
  if (d != d) return ~0ULL;
  const unsigned long long b = (unsigned long long)__double_as_longlong(d + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

// cnt[i] += the rows of slice blockIdx.y that stand before last-front row i in its niche (or, without a niche, among the niche-less
// rows).  grid = (row chunks, slices of j), as in the rank scan; cnt was cleared by the plan kernel.
__global__ __launch_bounds__(kTile) void moo_survive_count_kernel(const int P, const int H, const int slice, const int32_t* __restrict__ rank,
                                                                  const int32_t* __restrict__ niche, const double* __restrict__ dist,
                                                                  const int32_t* __restrict__ plan, int32_t* __restrict__ cnt) {
  __shared__ int s_h[kTile];                               // niche of a last-front row; -1: no niche; -2: not in the last front
  __shared__ unsigned long long s_key[kTile];
  const int l = plan[0];
  const int i = blockIdx.x * kTile + threadIdx.x;
  const bool last = i < P && rank[i] == l;
  if (!__syncthreads_or(last)) return;
  int hi = last ? niche[i] : -3;                           // -3 matches no staged row
  if (last && (hi < 0 || hi >= H)) hi = -1;
  const unsigned long long ki = moo_dist_key(last ? dist[i] : 0.0, hi >= 0);
  int before = 0;
  const int j_begin = (int)blockIdx.y * slice, j_end = min(P, j_begin + slice);
  for (int j0 = j_begin; j0 < j_end; j0 += kTile) {
    const int j = j0 + threadIdx.x;
    int hj = -2;
    if (j < j_end && rank[j] == l) { hj = niche[j]; if (hj < 0 || hj >= H) hj = -1; }
    __syncthreads();                                       // the previous tile has been read
    s_h[threadIdx.x] = hj;
    s_key[threadIdx.x] = moo_dist_key(hj >= 0 ? dist[j] : 0.0, hj >= 0);
    if (!__syncthreads_or(hj != -2)) continue;             // no last-front row in this tile
    if (last) {
      const int n = min(kTile, j_end - j0);
      for (int k = 0; k < n; ++k) {
        const unsigned long long kk = s_key[k];
        before += (s_h[k] == hi) && (kk < ki || (kk == ki && j0 + k < i));
      }
    }
  }
  if (last && before) atomicAdd(&cnt[i], before);
}

__device__ inline bool moo_survives(const int i, const int H, const int l, const int k_neg, const int32_t* __restrict__ rank,
                                    const int32_t* __restrict__ niche, const int32_t* __restrict__ quota, const int32_t* __restrict__ cnt) {
  const int r = rank[i];
  if (r != l) return r < l;
  const int h = niche[i];
  return cnt[i] < ((h >= 0 && h < H) ? quota[h] : k_neg);
}

__global__ __launch_bounds__(kOne) void moo_survive_compact_kernel(const int P, const int K, const int H, const int32_t* __restrict__ rank,
                                                                   const int32_t* __restrict__ niche, const int32_t* __restrict__ quota,
                                                                   const int32_t* __restrict__ plan, const int32_t* __restrict__ cnt,
                                                                   int32_t* __restrict__ keep) {
  __shared__ int s_scan[kOne];
  const int t = threadIdx.x;
  const int l = plan[0], k_neg = plan[1];
  const int per = (P + kOne - 1) / kOne;
  const int i0 = min(P, t * per), i1 = min(P, (t + 1) * per);
  int mine = 0;
  for (int i = i0; i < i1; ++i) mine += moo_survives(i, H, l, k_neg, rank, niche, quota, cnt);
  s_scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < kOne; o <<= 1) {
    const int v = t >= o ? s_scan[t - o] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  int at = s_scan[t] - mine;
  for (int i = i0; i < i1; ++i)
    if (moo_survives(i, H, l, k_neg, rank, niche, quota, cnt)) { if (at < K) keep[at] = i; ++at; }
}

struct SurviveArgs {
  int P, K, H;
  const int32_t *rank, *niche; const double* dist; int32_t* keep;
};

// scratch: plan [2] | quota [H] | cnt [P]
hipError_t survive_launch(void* scratch, hipStream_t stream, void* user) {
  const SurviveArgs& s = *static_cast<const SurviveArgs*>(user);
  char* p = static_cast<char*>(scratch);
  int32_t* plan = reinterpret_cast<int32_t*>(p); p += 256;
  const size_t hb = moo_align(sizeof(int32_t) * (size_t)(s.H > 0 ? s.H : 1));
  int32_t* quota = reinterpret_cast<int32_t*>(p); p += hb;
  int32_t* cnt = reinterpret_cast<int32_t*>(p);
  const unsigned nb = (unsigned)((s.P + kTile - 1) / kTile);
  const int slices = (int)nb < kSlices ? (int)nb : kSlices;
  const int slice = (int)((nb + slices - 1) / slices) * kTile;               // as in rank_launch: slices x slice >= P
  hipLaunchKernelGGL(moo_survive_plan_kernel, dim3(1), dim3(kOne), 0, stream, s.P, s.K, s.H, s.rank, s.niche, quota, plan, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(moo_survive_count_kernel, dim3(nb, (unsigned)slices), dim3(kTile), 0, stream, s.P, s.H, slice, s.rank, s.niche, s.dist, plan, cnt);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(moo_survive_compact_kernel, dim3(1), dim3(kOne), 0, stream, s.P, s.K, s.H, s.rank, s.niche, quota, plan, cnt, s.keep);
  return hipGetLastError();
}

// ---------------------------------------------------------------- mate

__device__ inline uint64_t moo_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

struct MooRng {
  uint64_t seed, gen, P, n_var;
  __device__ double u(uint64_t stream, uint64_t row, uint64_t var) const {
    const uint64_t ctr = 1ULL + ((gen * 8ULL + stream) * P + row) * n_var + var;
    return (double)(moo_mix(seed + 0x9E3779B97F4A7C15ULL * ctr) >> 11) * 0x1.0p-53;
  }
};

__device__ inline int moo_tournament(const MooRng& g, const int c, const int P, const int32_t* __restrict__ rank,
                                     const int32_t* __restrict__ niche, const double* __restrict__ dist) {
  const int a = min(P - 1, (int)(g.u(0, (uint64_t)c, 0) * (double)P));
  const int b = min(P - 1, (int)(g.u(1, (uint64_t)c, 0) * (double)P));
  const int ra = rank[a], rb = rank[b];
  if (rb < ra) return b;
  if (rb == ra && niche[a] == niche[b] && dist[b] < dist[a]) return b;
  return a;
}

__device__ inline double moo_clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

__device__ inline double moo_pm(const MooRng& g, const int c, const int v, double x, const double lo, const double hi, const double pm,
                                const double eta_m) {
  if (!(hi > lo) || !(g.u(6, (uint64_t)c, (uint64_t)v) <= pm)) return x;
  const double u = g.u(7, (uint64_t)c, (uint64_t)v);
  const double w = hi - lo, d1 = (x - lo) / w, d2 = (hi - x) / w, e = eta_m + 1.0;
  double dq;
  if (u < 0.5) dq = pow(2.0 * u + (1.0 - 2.0 * u) * pow(1.0 - d1, e), 1.0 / e) - 1.0;
  else dq = 1.0 - pow(2.0 * (1.0 - u) + 2.0 * (u - 0.5) * pow(1.0 - d2, e), 1.0 / e);
  return moo_clip(x + dq * w, lo, hi);
}

__device__ inline double moo_betaq(const double u, const double beta, const double e) {
  const double alpha = 2.0 - pow(beta, -e);
  return u <= 1.0 / alpha ? pow(u * alpha, 1.0 / e) : pow(1.0 / (2.0 - u * alpha), 1.0 / e);
}

// block = one wave = offspring pair q (slots 2 q and 2 q + 1; with odd P the last pair has the first slot only)
__global__ __launch_bounds__(64) void moo_mate_kernel(const int P, const int n_var, const double* __restrict__ X,
                                                      const int32_t* __restrict__ rank, const int32_t* __restrict__ niche,
                                                      const double* __restrict__ dist, const double* __restrict__ xl,
                                                      const double* __restrict__ xu, const uint64_t seed, const uint64_t gen, const double pc,
                                                      const double eta_c, const double pm, const double eta_m, double* __restrict__ Xc,
                                                      int32_t* __restrict__ parents) {
  const int q = blockIdx.x;
  const int c0 = 2 * q, c1 = 2 * q + 1;
  if (c0 >= P) return;
  const bool two = c1 < P;
  const MooRng g{seed, gen, (uint64_t)P, (uint64_t)n_var};
  const int p0 = moo_tournament(g, c0, P, rank, niche, dist);
  const int p1 = two ? moo_tournament(g, c1, P, rank, niche, dist) : p0;
  if (threadIdx.x == 0 && parents) { parents[c0] = p0; if (two) parents[c1] = p1; }
  const bool cross = two && g.u(2, (uint64_t)q, 0) <= pc;
  const double e = eta_c + 1.0;
  for (int v = threadIdx.x; v < n_var; v += 64) {
    const double lo = xl[v], hi = xu[v];
    double x0 = X[(size_t)p0 * n_var + v], x1 = two ? X[(size_t)p1 * n_var + v] : x0;
    if (cross && g.u(3, (uint64_t)q, (uint64_t)v) <= 0.5 && fabs(x0 - x1) > 1e-14 && hi > lo) {
      const double y1 = fmin(x0, x1), y2 = fmax(x0, x1), dy = y2 - y1;
      const double u = g.u(4, (uint64_t)q, (uint64_t)v);
      const double b1 = moo_betaq(u, 1.0 + 2.0 * (y1 - lo) / dy, e), b2 = moo_betaq(u, 1.0 + 2.0 * (hi - y2) / dy, e);
      const double k1 = moo_clip(0.5 * ((y1 + y2) - b1 * dy), lo, hi), k2 = moo_clip(0.5 * ((y1 + y2) + b2 * dy), lo, hi);
      const bool swap = g.u(5, (uint64_t)q, (uint64_t)v) <= 0.5;
      x0 = swap ? k2 : k1; x1 = swap ? k1 : k2;
    }
    Xc[(size_t)c0 * n_var + v] = moo_pm(g, c0, v, x0, lo, hi, pm, eta_m);
    if (two) Xc[(size_t)c1 * n_var + v] = moo_pm(g, c1, v, x1, lo, hi, pm, eta_m);
  }
}

}  // namespace pk

extern "C" {

int pk_moo_rank_batch(pk_ctx* c, int P, int M, const double* F, int stop_at, int32_t* rank, int32_t* n_fronts) {
  if (!c) return PK_ERR_ARG;
  if (P < 0 || P > pk::kMaxP || M < 2 || M > 4 || stop_at < 0) return pk_ctx_fail(c, PK_ERR_ARG, "rank: 0 <= P <= 65536, M in 2..4 and stop_at >= 0 required");
  if (P == 0) return PK_OK;
  if (!F || !rank || !n_fronts) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  pk::RankArgs a{P, M, stop_at, F, rank, n_fronts};
  return pk_ctx_scratch_launch(c, 256 + 2 * pk::moo_align(sizeof(int32_t) * (size_t)P), pk::rank_launch, &a);
}

#define PK_MOO_CHECK(call) do { if ((e = (call)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, hipGetErrorString(e)); } while (0)
int pk_moo_associate_batch(pk_ctx* c, int P, int M, const double* F, const double* ideal, const double* nadir, int H, const double* dirs,
                           int32_t* niche, double* dist) {
  if (!c) return PK_ERR_ARG;
  if (P < 0 || P > pk::kMaxP || M < 2 || M > 4 || H < 1 || H > pk::kMaxH) return pk_ctx_fail(c, PK_ERR_ARG, "associate: 0 <= P <= 65536, M in 2..4 and 1 <= H <= 4096 required");
  if (P == 0) return PK_OK;
  if (!F || !ideal || !nadir || !dirs || !niche || !dist) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  hipStream_t st = (hipStream_t)pk_ctx_stream(c);
  const unsigned nb = (unsigned)((P + pk::kTile - 1) / pk::kTile);
  const size_t lds = sizeof(double) * (size_t)H * (size_t)M;
  hipError_t e;
  const void* fn = M == 2 ? (const void*)pk::moo_associate_kernel<2> : M == 3 ? (const void*)pk::moo_associate_kernel<3> : (const void*)pk::moo_associate_kernel<4>;
  if (lds > 48 * 1024) PK_MOO_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  switch (M) {
    case 2: hipLaunchKernelGGL(pk::moo_associate_kernel<2>, dim3(nb), dim3(pk::kTile), lds, st, P, H, F, ideal, nadir, dirs, niche, dist); break;
    case 3: hipLaunchKernelGGL(pk::moo_associate_kernel<3>, dim3(nb), dim3(pk::kTile), lds, st, P, H, F, ideal, nadir, dirs, niche, dist); break;
    default: hipLaunchKernelGGL(pk::moo_associate_kernel<4>, dim3(nb), dim3(pk::kTile), lds, st, P, H, F, ideal, nadir, dirs, niche, dist); break;
  }
  PK_MOO_CHECK(hipGetLastError());
  return PK_OK;
}

int pk_moo_survive_batch(pk_ctx* c, int P, int K, const int32_t* rank, const int32_t* niche, const double* dist, int H, int32_t* keep) {
  if (!c) return PK_ERR_ARG;
  if (P < 0 || P > pk::kMaxP || K < 0 || K > P || H < 1 || H > pk::kMaxH) return pk_ctx_fail(c, PK_ERR_ARG, "survive: 0 <= K <= P <= 65536 and 1 <= H <= 4096 required");
  if (K == 0) return PK_OK;
  if (!rank || !niche || !dist || !keep) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  pk::SurviveArgs s{P, K, H, rank, niche, dist, keep};
  const size_t bytes = 256 + pk::moo_align(sizeof(int32_t) * (size_t)H) + pk::moo_align(sizeof(int32_t) * (size_t)P);
  return pk_ctx_scratch_launch(c, bytes, pk::survive_launch, &s);
}

int pk_moo_mate_batch(pk_ctx* c, int P, int n_var, const double* X, const int32_t* rank, const int32_t* niche, const double* dist,
                      const double* xl, const double* xu, uint64_t seed, int gen, double pc, double eta_c, double pm, double eta_m,
                      double* Xc, int32_t* parents) {
  if (!c) return PK_ERR_ARG;
  if (P < 0 || P > pk::kMaxP || n_var < 1 || gen < 0 || !(pc >= 0.0) || !(pm >= 0.0) || !(eta_c >= 0.0) || !(eta_m >= 0.0))
    return pk_ctx_fail(c, PK_ERR_ARG, "mate: 0 <= P <= 65536, n_var >= 1, gen >= 0 and non-negative pc, pm, eta_c, eta_m required");
  if (P == 0) return PK_OK;
  if (!X || !rank || !niche || !dist || !xl || !xu || !Xc) return pk_ctx_fail(c, PK_ERR_ARG, "null pointer");
  if (hipSetDevice(pk_ctx_device(c)) != hipSuccess) return pk_ctx_fail(c, PK_ERR_HIP, "hipSetDevice");
  hipLaunchKernelGGL(pk::moo_mate_kernel, dim3((unsigned)((P + 1) / 2)), dim3(64), 0, (hipStream_t)pk_ctx_stream(c), P, n_var, X, rank, niche, dist,
                     xl, xu, seed, (uint64_t)gen, pc, eta_c, pm, eta_m, Xc, parents);
  hipError_t e;
  PK_MOO_CHECK(hipGetLastError());
  return PK_OK;
}
#undef PK_MOO_CHECK

}  // extern "C"
