/* phoskin.h -- C ABI of libphoskin_hip.so: the MI355X (gfx950) batched stiff-ODE engine for
 * PhosKinTime's per-protein parameter-estimation hot path.
 *
 * The reference (bibymaths/phoskintime) has no FFI: the seam is a set of plain Python callables
 * (SURVEY.md section 8b).  Every entry point below names the reference callable(s) it replaces.
 * Signatures use only plain pointers and sizes (no torch / numpy types).  Unless a function name
 * ends in `_host`, every array pointer is a DEVICE pointer (HBM) and the call is asynchronous on
 * the context's stream; `_host` variants take host pointers, stage through HBM and synchronise.
 *
 * Conventions
 *   model      0 = distmod (models/distmod.py), 1 = succmod (models/succmod.py), 2 = randmod (models/randmod.py)
 *   state      y = [R, P, X_1..X_m], m = n_sites (dist/succ) or 2^n_sites - 1 (rand); S = 2 + m.  Up to 64 states a replica is a lane
 *              group of a wavefront; beyond that (distmod / succmod n_sites 63..1276, randmod n_sites 7..20) one workgroup owns a
 *              replica: distmod / succmod keep the default LRP12 with exact structured solves; randmod n_sites = 7 keeps LRP12 too, the
 *              128 x 128 inverse spread over the registers of the workgroup (csrc/pk_rand_dense.hpp); randmod n_sites >= 8 integrates with
 *              the order-4 additive method ARK4(3)6L[2]SA on the n-cube at 0.02 x the requested tolerances (csrc/pk_wide.hpp)
 *   theta      [A, B, C, D, S_1..S_n, D_1..D_m], P = 4 + n + m      (reference unpack_params, distmod.py:68-91,
 *              succmod.py:94-112, randmod.py:88-119); batched as a row-major [B, P] f64 matrix
 *   return     0 = ok; < 0 = argument / runtime error (see pk_last_error); never throws or aborts.
 *   status[b]  per-replica bit flags: PK_ST_NONFINITE | PK_ST_MAXSTEPS | PK_ST_HMIN.  A flagged replica's
 *              remaining output rows are NaN (the reference only warns: odeint returns garbage and callers
 *              test np.isfinite, e.g. global_model/optproblem.py:125-133).
 */
#ifndef PHOSKIN_H
#define PHOSKIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PK_VERSION 200

enum { PK_MODEL_DIST = 0, PK_MODEL_SUCC = 1, PK_MODEL_RAND = 2 };

/* Integrators (all adaptive ones: max-norm local error control, steps land exactly on every t[k]).
 * LRP12 is the default: the three per-protein models are affine in y (constant Jacobian), which the LRP methods exploit. */
enum {
  PK_METHOD_RODAS4 = 0, /* 6-stage L-stable Rosenbrock 4(3) (Hairer-Wanner RODAS), analytic Jacobian, 1 factorisation / step */
  PK_METHOD_BDF2   = 1, /* variable-step BDF2 (BDF1 start), analytic Jacobian, 1 factorisation / step (BASELINE config 3) */
  PK_METHOD_RK4    = 2, /* classical explicit RK4, fixed step h <= rk4_h (BASELINE config 2); stability-bound when stiff */
  PK_METHOD_LRP8   = 3, /* L-stable restricted-Pade one-step method for affine systems: 8 resolvent solves, 1 rhs and
                           1 factorisation per step, order 7 with an embedded order-6 estimate */
  PK_METHOD_LRP12  = 5, /* the same construction with 12 solves: order 11, embedded order 10, gamma = 0.16 (L-stable; |R(iy)| <= 1 + 4.5e-9);
                           about half the steps of LRP8 at equal accuracy.  Default. */
  PK_METHOD_DP5    = 4, /* pk_network_simulate_batch only: the reference's opt-in explicit integrator, step for step -- Dormand-Prince
                           5(4), PI controller, dt in [1e-6, 1], bucket-edge landing, Hermite output (global_model/solvers.py:293-758) */
  PK_METHOD_ARK436 = 6, /* pk_network_simulate_batch only: ARK4(3)6L[2]SA (Kennedy-Carpenter) as a linearly implicit additive method, implicit
                           on the per-protein block Jacobian: order 4 for any Jacobian approximation, 5 block solves per step.  The network
                           default wherever the one-thread-per-protein layout applies (topologies 0 / 1 / 4, <= 8 sites, N <= 256); on
                           request also for the combinatorial topology (<= 3 sites), where the order-3 kernel is the faster one     */
  PK_METHOD_ROS34PW2 = 7 /* pk_network_simulate_batch only: the round-1 integrator, Rosenbrock-W of order 3 (4 block solves per step); every
                           network / topology; the default where ARK436 does not apply                                                       */
};

/* Linear solver for the implicit stage equations (g I - J) x = r. */
enum {
  PK_LINSOLVE_AUTO       = 0, /* fastest available: resolvent methods (LRP12 / LRP8 / RODAS4) -> the throughput kernels (distmod: 4-16 lanes per
                                 replica; randmod: bit-mask rows; small systems at large B: one lane per replica); else structured / dense */
  PK_LINSOLVE_DENSE      = 1, /* dense: in-register Gauss-Jordan to the explicit inverse, one matrix row per lane; every solve is a mat-vec (any model) */
  PK_LINSOLVE_STRUCTURED = 2  /* arrow (distmod) / tridiagonal (succmod) elimination; randmod falls back to dense */
};

/* Scalar Morris outputs, sensitivity/analysis.py:90-176 (_compute_Y; Y_METRIC, config/constants.py:104). */
enum {
  PK_METRIC_TOTAL_SIGNAL = 0, PK_METRIC_MEAN_ACTIVITY = 1, PK_METRIC_VARIANCE = 2,
  PK_METRIC_DYNAMICS = 3, PK_METRIC_L2_NORM = 4
};

enum { PK_ST_OK = 0, PK_ST_NONFINITE = 1, PK_ST_MAXSTEPS = 2, PK_ST_HMIN = 4 };

enum {
  PK_OK = 0, PK_ERR_ARG = -1, PK_ERR_UNSUPPORTED = -2, PK_ERR_HIP = -3, PK_ERR_NOMEM = -4
};

typedef struct pk_solver_opts {
  int32_t method;       /* PK_METHOD_*                                                        */
  int32_t linsolve;     /* PK_LINSOLVE_*                                                      */
  double  rtol, atol;   /* local error tolerances (max-norm); defaults 1e-6 / 1e-8 (chosen for LRP12: worst error 0.05 of the
                           parity band; RODAS4 / LRP8 / BDF2 need 1e-7 / 1e-9 for the same margin) */
  double  h0;           /* first step; 0 = automatic                                          */
  double  rk4_h;        /* RK4 only: largest fixed step (each output interval is split evenly) */
  int32_t max_steps;    /* per replica, accepted + rejected; default 100000                   */
  int32_t clip_nonneg;  /* np.clip(sol, 0, None) as in distmod.py:112-113 (default 1)         */
  int32_t normalize;    /* NORMALIZE_MODEL_OUTPUT: sol *= 1 / y0 (distmod.py:116-122)         */
  int32_t stage_form;   /* RODAS4: 0 = resolvent form (1 rhs + 6 solves / step; exact for the affine per-protein models),
                           1 = classical 6-stage Rosenbrock form (same method; kept for nonlinear right-hand sides) */
  int32_t kernel;       /* PK_KERNEL_*: which kernel family runs a small system.  AUTO picks by batch size (thread-per-replica above a
                           measured threshold), so the SAME replica can take different roundings / step sequences in batches of
                           different size -- a sharded run that must reproduce the single-GPU bits pins GROUP or TPR on every rank. */
  int32_t err_norm;     /* PK_NORM_*: how the local error of a step is measured against rtol / atol (pk_network_simulate_batch; the per-protein
                           kernels always use the max norm)                                                                          */
} pk_solver_opts;

enum {
  PK_NORM_DEFAULT = 0,  /* = PK_NORM_MAX                                                                                              */
  PK_NORM_MAX     = 1,  /* max_i |e_i| / (atol + rtol |y_i|): every component inside its tolerance (1.4-1.7x the steps of RMS at S ~ 550)   */
  PK_NORM_RMS     = 2   /* sqrt(mean_i (e_i / (atol + rtol |y_i|))^2): ODEPACK's vnorm, i.e. what the reference's LSODA controls with the
                           same rtol / atol (scipy.integrate.odeint, global_model/simulate.py:69-79).  Opt-in: 1.4-1.7x fewer steps, accuracy
                           of the reference run's own class on the fixtures but outside the parity band on some populations   */
};

enum {
  PK_KERNEL_AUTO  = 0,  /* by batch size (default)                                                             */
  PK_KERNEL_GROUP = 1,  /* lane-group kernels (several lanes per replica) at every batch size                  */
  PK_KERNEL_TPR   = 2,  /* thread-per-replica kernels wherever one exists for (model, n_sites), else lane-group */
  PK_KERNEL_WORKSPACE = 3, /* pk_network_simulate_batch only: ROS34PW2 on the HBM-workspace kernel at any network size (the kernel
                              networks beyond one workgroup's LDS take by themselves)                                           */
  PK_KERNEL_HBM = 4        /* pk_network_simulate_sens_batch and pk_network_simulate_objective_grad_batch only: state AND tangents on
                              HBM slabs at any network size (the route networks beyond one workgroup's LDS take by themselves).
                              Every other network entry point answers PK_ERR_UNSUPPORTED for it (pk_network_resolve_method too) and the
                              per-protein entry points PK_ERR_ARG ("unknown opts->kernel"), as they do for PK_KERNEL_WORKSPACE     */
};

typedef struct pk_ctx pk_ctx;

int         pk_version(void);
/* One context per GPU / per thread.  Owns a HIP stream, grow-only HBM arenas (staging of the `_host` entry points; per-replica
 * scratch of the largest random-model systems; the state of pk_fit_protein_rows_batch) and a page-locked host buffer for small `_host` calls -- no hipMalloc / hipFree per call. */
pk_ctx*     pk_create(int device_id);          /* NULL on failure: reason in pk_create_error() */
const char* pk_create_error(void);          /* thread-local; empty string after a successful pk_create */
void        pk_destroy(pk_ctx*);
const char* pk_last_error(pk_ctx*);            /* valid until the next call on this context */
/* Launch on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; NULL is HIP's default
 * stream).  pk_use_own_stream switches back to the context's private non-blocking stream. */
int         pk_set_stream(pk_ctx*, void* hip_stream);
int         pk_use_own_stream(pk_ctx*);
int         pk_synchronize(pk_ctx*);
void        pk_default_opts(pk_solver_opts*);
/* {staging allocations so far, staging bytes, scratch allocations, scratch bytes, page-locked allocations, page-locked bytes}: serial
 * callers (the reference calls solve_ode once per parameter vector: paramest/normest.py:55, paramest/core.py:111,141,154) allocate once. */
int         pk_workspace_stats(pk_ctx*, int64_t out[6]);

/* Shapes (pure host arithmetic, usable without a GPU). */
int pk_protein_n_states(int model, int n_sites);           /* S, or PK_ERR_* */
int pk_protein_n_params(int model, int n_sites);           /* P */
int pk_protein_flat_len(int model, int n_sites, int T);    /* (T-5) + T + n_sites*T  (distmod.py:125-134) */

/* (state conventions, [r3]: randmod n_sites = 7, 8 integrate with the default LRP12 on EXACT solves -- the odd-popcount block of I - q J is
 *  diagonal, its even Schur complement is inverted in the registers of one workgroup, csrc/pk_rand_parity.hpp; n_sites >= 9: the additive
 *  method on the n-cube, csrc/pk_wide.hpp.)
 *
 * Replaces, for a whole batch of parameter vectors, models.solve_ode(params, init_cond, num_psites, t)
 *   -> (sol, flat)   [models/__init__.py:12; distmod.py:93-134, succmod.py:114-152, randmod.py:249-305]
 * and, fused behind it, sensitivity.analysis._compute_Y (sensitivity/analysis.py:90-176).
 *   theta [B,P]; y0 [S] (shared) or [B,S]; t [T] with t[0] the initial time, strictly increasing;
 *   sol [B,T,S] | NULL; flat [B,F] | NULL; metric [B] | NULL; status [B] | NULL; n_steps [B,2] | NULL
 *   (accepted, rejected).  sol is clipped / normalised per opts exactly like the reference's return value. */
int pk_solve_protein_batch(pk_ctx*, int model, int n_sites, int64_t B,
                           const double* theta, const double* y0, int y0_is_batched,
                           const double* t, int T, const pk_solver_opts* opts,
                           double* sol, double* flat, double* metric, int metric_id,
                           int32_t* status, int32_t* n_steps);

/* flat(theta) AND its parameter Jacobian d flat / d theta from ONE integration (forward sensitivities: S' = J S + df/dtheta solved with the
 * factors of the state solve, differentiated stage by stage: csrc/pk_sens.hpp).  Replaces the 1 + P calls of models.solve_ode per Jacobian
 * that scipy.optimize.curve_fit's '2-point' differences make under paramest/normest.py:167-326 and paramest/toggle.py.
 *   flat [B,F]; dflat [B,F,P] (row-major: the P derivatives of one flat entry are contiguous); status / n_steps as above.
 * The derivative follows flat's own post-processing: scaled by 1 / y0 under opts->normalize, and 0 where the value was clipped at 0 -- where
 * the state is below -atol, that is: a state within atol of 0 is not known to be negative (a site whose rate sits on the bound 0 decays to
 * +-1e-24), so its value is clipped but its derivative row is kept; it is the row that can move the rate off the bound.
 * Tangents are held to the same rtol / atol as the states (maximum norm over all columns).  Method LRP12 only.
 * Sizes: pk_protein_sens_available(model, n_sites) != 0 -- distmod / succmod n_sites <= 62 (one column per lane, csrc/pk_sens.hpp: exists up to 14, the
 * default below the measured crossover, distmod n_sites < 10 and succmod n_sites < 6; from there on: rows across the lanes, eight columns
 * per lane, chunked columns, csrc/pk_sens_rows.hpp -- PK_SENS_ROWS=2 keeps the column kernel up to 14, =1 takes the rows kernel at every
 * size), randmod n_sites <= 7 (6 and 7: the
 * parity-eliminated inverse in registers serving eight columns per workgroup, csrc/pk_rand_sens.hpp); PK_ERR_UNSUPPORTED beyond (callers
 * difference pk_solve_protein_batch there, as phoskintime_amd.paramest.fit_rows_batch does).  Kernels that cut the columns of a replica
 * into chunks integrate the state once per chunk with its own step-size control: every column is within rtol / atol of the exact
 * derivative, the chunks are not bit-coupled; `status` is the OR over the chunks. */
int pk_protein_sens_available(int model, int n_sites);
int pk_solve_protein_sens_batch(pk_ctx*, int model, int n_sites, int64_t B,
                                const double* theta, const double* y0, int y0_is_batched,
                                const double* t, int T, const pk_solver_opts* opts,
                                double* flat, double* dflat, int32_t* status, int32_t* n_steps);

/* The scalar Morris output m = _compute_Y (PK_METRIC_*, as pk_solve_protein_batch forms it) AND its gradient d m / d theta from ONE
 * integration: the metric flavour of the output stage of the kernels behind pk_solve_protein_sens_batch.  The gradient cannot be rebuilt
 * from dflat: the metric sums ALL observed rows i < 2 + n_sites at ALL T output times, and flat has no slot for the mRNA row at the first
 * five times.
 *   metric [B]; dmetric [B,P]; flat [B,F] | NULL; dflat [B,F,P] | NULL (NULL = not written: B (1 + P) doubles leave the kernel instead of
 *   B F (1 + P)); status / n_steps as above.  All arrays are device pointers; the call is asynchronous on the context's stream.
 * With v[i,k] the post-processed value of observed row i at output time k (clipped at 0 under opts->clip_nonneg, scaled by 1 / y0[i]
 * under opts->normalize: exactly as flat), d[i,k,p] its post-processed derivative (scaled alike; 0 where the state is below -atol under
 * clip_nonneg, the rule of dflat; 0 at k = 0, the initial values being data), L = T (2 + n_sites) and vbar the mean of v:
 *   total_signal    g[p] = sum d
 *   mean_activity   g[p] = sum d / L
 *   variance        g[p] = (2 / L) sum (v - vbar) d      (accumulated as sum (v - c) d and sum d with c the mean at t0, never as the
 *                                                         difference of the raw sums)
 *   dynamics        g[p] = 2 sum_i sum_{k >= 1} (v[i,k] - v[i,k-1]) (d[i,k,p] - d[i,k-1,p])
 *   l2_norm         g[p] = sum v d / m, and 0 where m = 0
 * Failure follows dflat's NaN fill, the NaN entries entering the sums: a flagged replica has metric = NaN, and NaN in the columns of
 * dmetric whose chunk was flagged (kernels that cut the columns into chunks: chunk 0 forms metric, every chunk integrates the state itself
 * and forms its own columns; status is the OR over the chunks).  T = 1: metric is the metric of the post-processed y0, dmetric is 0.
 * Same sizes (pk_protein_sens_available), options (LRP12 only) and kernel per size, PK_SENS_ROWS included, as pk_solve_protein_sens_batch,
 * and PK_ERR_UNSUPPORTED in the same cases; PK_ERR_ARG for a metric_id outside PK_METRIC_* and for a null metric or dmetric.
 * flat, dflat, status and n_steps are bit-equal to those of pk_solve_protein_sens_batch for the same inputs; metric and dmetric do not
 * depend on whether flat and dflat were asked for, nor on the batch around a replica (every reduction runs in a fixed order). */
int pk_solve_protein_sens_metric_batch(pk_ctx*, int model, int n_sites, int64_t B,
                                       const double* theta, const double* y0, int y0_is_batched,
                                       const double* t, int T, const pk_solver_opts* opts, int metric_id,
                                       double* metric, double* dmetric, double* flat, double* dflat,
                                       int32_t* status, int32_t* n_steps);

/* A weighted sum over the entries of flat AND its gradient from ONE integration: the VJP flavour of the output stage of the kernels behind
 * pk_solve_protein_sens_batch.  It is the vector-Jacobian product w^T d flat / d theta a backward pass needs, and the weighted least-squares
 * cost with its gradient J^T r that an optimiser other than Levenberg-Marquardt takes -- without dflat [B,F,P] in memory.
 *   w [F] | [B,F]; target NULL | [F] | [B,F]; value [B]; grad [B,P]; flat [B,F] | NULL (NULL = not written: B (1 + P) doubles leave the
 *   kernel instead of B F (1 + P)); status / n_steps as above.  All arrays are device pointers; the call is asynchronous on the context's stream.
 * With v[f] the post-processed value of flat entry f (clipped at 0 under opts->clip_nonneg, scaled by 1 / y0 under opts->normalize: exactly as
 * flat stores it) and d[f,p] its post-processed derivative (scaled alike; 0 where the state is below -atol under clip_nonneg, the rule of
 * dflat; 0 at output time 0, the initial values being data):
 *   linear mode        (target == NULL)   c[f] = w[f]                                   value = sum_f w[f] v[f]
 *   least-squares mode (target != NULL)   r[f] = w[f] (v[f] - target[f]),  c[f] = w[f] r[f]   value = 1/2 sum_f r[f]^2     (w = 1 / sigma)
 *   both                                  grad[p] = sum_f c[f] d[f,p]
 * Least-squares mode is the cost and J^T r of the data rows of pk_fit_protein_rows_batch's residual.  The sum index is the FLAT index: the
 * mRNA row at the first five output times has no slot in flat and contributes nothing (the opposite of the metric flavour, which sums it);
 * with T <= 5 the mRNA block is empty.  Every column keeps one running sum over its entries in output order, stored once; no atomics, no
 * order that depends on the batch.
 * Failure follows dflat's NaN fill, the NaN entries entering the sums: a flagged replica has value = NaN, and NaN in the columns of grad whose
 * chunk was flagged (kernels that cut the columns into chunks: chunk 0 forms value and flat, every chunk integrates the state itself and
 * forms its own columns -- in least-squares mode with c[f] from its own state values, which differ from flat's within rtol / atol; status
 * is the OR over the chunks).  T = 1: value is that of the post-processed y0, grad is 0.
 * Same sizes (pk_protein_sens_available), options (LRP12 only) and kernel per size, PK_SENS_ROWS included, as pk_solve_protein_sens_batch,
 * and PK_ERR_UNSUPPORTED in the same cases; PK_ERR_ARG for a null w, value or grad; B = 0 is PK_OK.
 * flat, status and n_steps are bit-equal to those of pk_solve_protein_sens_batch for the same inputs; value and grad do not depend on
 * whether flat was asked for, nor on the batch around a replica. */
int pk_solve_protein_sens_vjp_batch(pk_ctx*, int model, int n_sites, int64_t B,
                                    const double* theta, const double* y0, int y0_is_batched,
                                    const double* t, int T, const pk_solver_opts* opts,
                                    const double* w, int w_is_batched, const double* target, int target_is_batched,
                                    double* value, double* grad, double* flat,
                                    int32_t* status, int32_t* n_steps);

/* The bounded least-squares fit itself, for R independent rows in lockstep -- the numerical core of paramest.normest's
 * _curve_fit_multistart / find_best_lambda / bootstrap loop (paramest/normest.py:167-326, one scipy.optimize.curve_fit per start there), as
 * phoskintime_amd.paramest.fit_rows_batch runs it with jacobian="sens": row k fits [flat(theta_k) ; lam_k / P * p_k^2] to [target_k ; 0] with
 * weights 1 / sigma_k inside the box [lb, ub] from the start point clip(P0_k), by Levenberg-Marquardt with Marquardt scaling, projection on
 * the box and gain-ratio damping (mu0 = 1e-3; up to 12 damping values mu, 4 mu, 16 mu ... per iteration, trial_levels of them per launch,
 * the first acceptable one taken).  p is the fitted space: theta = exp(p) under log_space (randmod in the reference), else theta = p.
 *   P0, p [R,P]; y0 [S] | [R,S]; t [T]; target [F] | [R,F]; sigma NULL (= 1) | [Nr] | [R,Nr] with Nr = F + (use_reg ? P : 0); lam [R], or NULL
 *   without use_reg; lb, ub [P] | [R,P]; cost [R] = 0.5 |r|^2; r [R,Nr] | NULL the final weighted residuals; JTJ [R,P,P] | NULL, J^T J of the
 *   weighted residuals at each row's last Jacobian evaluation (what a covariance needs); reason [R] | NULL why the row stopped: 0 ftol / xtol,
 *   1 gradient / empty free set, 2 damping budget, 3 max_iter.  All of these are DEVICE pointers; counters is a HOST array:
 *   {iterations, solves, launches, host waits, Jacobian phases, trial rounds}.
 *   JTJ belongs to the point the row's last Jacobian phase was taken AT, which is the point BEFORE that iteration's step: a row that stops
 *   in its first iteration (for any reason, max_iter = 1 included) holds J^T J at clip(P0), not at the p it returns, and in general JTJ is
 *   one accepted step behind p unless the row's last iteration took no step (reasons 1 and 2).  With max_iter = 0 no
 *   Jacobian phase runs: JTJ is NOT WRITTEN and the caller's buffer keeps what it held; p = clip(P0), r and cost are the start point's,
 *   reason = 3 and counters = {0, R, 1, 0, 0, 0}.
 * Every iteration is a Jacobian phase (gather, pk_solve_protein_sens_batch on the active rows, normal equations: 3 launches, in row chunks
 * where the Jacobians of a launch would pass 1 GiB) and trial rounds (damped steps, pk_solve_protein_batch on levels x pending rows, accept
 * rule: 3 launches); the host waits once per phase and once per round, for one flag per row, and nothing else crosses PCIe but the row
 * lists.  `launches` counts those and the one solve launch of the initial residuals.  State and scratch live in a grow-only arena of the context
 * that only this entry point uses (no allocation per iteration; pk_workspace_stats does not count it); the call holds the context's lock and returns after its last wait.
 * A failed solve is very bad, not fatal: its residuals count 1e6 each and its Jacobian entries 0.
 * Batch independence: all row algebra (csrc/pk_lm.hpp) has one code path and sums in a fixed order, so p, cost, r and JTJ of a row do not
 * depend on the rows around it, their order, or trial_levels -- PROVIDED the solves do not: opts->kernel = PK_KERNEL_AUTO lets a small system
 * change kernel family with the batch size (see pk_solver_opts.kernel); a caller who needs the bits pins PK_KERNEL_GROUP or PK_KERNEL_TPR.
 * opts (NULL = defaults) goes to every solve.  PK_ERR_UNSUPPORTED exactly where pk_solve_protein_sens_batch answers it (sizes without a
 * sensitivity kernel: difference pk_solve_protein_batch there, as phoskintime_amd.paramest.fit_rows_batch does; a method other than LRP12);
 * PK_ERR_ARG for a null required pointer, R < 0, T < 1, trial_levels outside 0..12, max_iter < 0; R = 0 is PK_OK. */
typedef struct pk_fit_opts {
  int32_t max_iter;      /* iterations (Jacobian evaluations) per row; default 100                                  */
  int32_t trial_levels;  /* damping values per trial launch; 0 = auto: 3 while <= 256 rows pend, else 1             */
  int32_t log_space;     /* theta = exp(p)                                                                          */
  int32_t use_reg;       /* the P ridge rows (lam / P) p^2 are part of the residual                                 */
  double  ftol, xtol;    /* an accepted step ends the row when dcost <= ftol cost or |dp| <= xtol (xtol + |p|); 1e-10 */
} pk_fit_opts;
void pk_default_fit_opts(pk_fit_opts*);
int  pk_fit_protein_rows_batch(pk_ctx*, int model, int n_sites, int64_t R,
                               const double* P0, const double* y0, int y0_is_batched, const double* t, int T,
                               const double* target, int target_is_batched, const double* sigma, int sigma_is_batched,
                               const double* lam, const double* lb, const double* ub, int bounds_are_batched,
                               const pk_solver_opts* opts, const pk_fit_opts* fit,
                               double* p, double* cost, double* r, double* JTJ, int32_t* reason, int64_t counters[6]);

/* Replaces models.{distmod,succmod}.ode_core / models.randmod.ode_system (distmod.py:7-65, succmod.py:9-90,
 * randmod.py:122-247) evaluated for a batch: y [B,S] -> dydt [B,S]. */
int pk_rhs_protein_batch(pk_ctx*, int model, int n_sites, int64_t B,
                         const double* theta, const double* y, double* dydt);

/* Analytic Jacobian d f_i / d y_j, row-major J [B,S,S] (the reference has none for this path: LSODA
 * finite-differences ode_core; row-major as global_model/simulate.py:75 col_deriv=False). */
int pk_jacobian_protein_batch(pk_ctx*, int model, int n_sites, int64_t B,
                              const double* theta, double* J);

/* Steady state y* of dy/dt = J(theta) y + b(theta) = 0 for B parameter vectors: y_ss [B,S] (device), status [B] (or NULL;
 * PK_ST_NONFINITE + a NaN row when J is singular, e.g. no degradation).  Generalises steady.initial_condition(num_psites)
 * (steady/initdist.py:9-50, initsucc.py:9-55, initrand.py:9-77: SLSQP on the steady-state equations with every rate fixed to 1,
 * called once per protein at paramest/core.py:83) to per-replica theta.  Beyond 64 states one workgroup owns a replica: closed form (distmod),
 * cyclic reduction (succmod), symmetric Gauss-Seidel on the n-cube (randmod, n_sites <= 12; PK_ST_MAXSTEPS + NaN row if it does not converge). */
int pk_steady_state_protein_batch(pk_ctx*, int model, int n_sites, int64_t B, const double* theta, double* y_ss, int32_t* status);

/* Morris screening without a host round trip (reference: SALib morris.sample / morris.analyze as called at
 * sensitivity/analysis.py:221-265 and global_model/sensitivity.py:210-277; SALib itself is absent from the reference tree).
 * The N x D random draws -- base[r,i] on the level grid of the unit cube, sign[r,i] = +-1, rank[r,i] = position of coordinate i in
 * trajectory r's random order -- come from the host (KB); the N (D + 1) x D sample matrix is built in HBM:
 *   X[(r (D+1) + s), i] = lb_i + clip(base + sign * delta * [rank < s], 0, 1) * (ub_i - lb_i),       delta = p / (2 (p - 1)).
 * rank[r, :] must be a permutation of 0..D-1 (not checked on the device).  All pointers are device pointers. */
int pk_morris_build_batch(pk_ctx*, int64_t N, int D, double delta, const double* base, const double* sign, const int32_t* rank,
                          const double* lb, const double* ub, double* X);
/* Elementary effects EE [N,D] from the per-row outputs Y [N (D+1)] of the same design: (Y[r, rank+1] - Y[r, rank]) / (sign * delta). */
int pk_morris_effects_batch(pk_ctx*, int64_t N, int D, double delta, const double* sign, const int32_t* rank, const double* Y, double* EE);

/* Variance-based (Sobol') indices without a host round trip (reference: SALib saltelli.sample / sobol.analyze with
 * calc_second_order=False as called at scripts/temporal_sensitivity.py:169,185).  The two N x D base samples A, B on the unit cube come
 * from the host (KB); the N (D + 2) x D design is built in HBM in saltelli.sample's row order: for each i the row A_i, then
 * AB_i1 .. AB_iD (A_i with column j taken from B_i), then B_i, each scaled as lb + u (ub - lb) with separately rounded multiply and add.
 * All pointers are device pointers. */
int pk_sobol_build_batch(pk_ctx*, int64_t N, int D, const double* A, const double* B, const double* lb, const double* ub, double* X);
/* First-order and total indices S1, ST [D,M] of the M output columns Y [N (D + 2), M] (row-major, rows in the design's order), each column
 * centred by its mean over all rows:  S1_j = mean(B (AB_j - A)) / var([A; B]),  ST_j = mean((A - AB_j)^2) / 2 / var([A; B])  with the
 * population variance, also written to var [M] (optional).  counts [R,N] (int32): row r holds how often resample r draws each i; its
 * indices are the same formulas with weights counts[r,i] / N (its own variance included), and S1_sd, ST_sd [D,M] are their ddof-1
 * standard deviations over the R resamples (no normal quantile).  R = 0: no resampling, counts / S1_sd / ST_sd ignored; R = 1 is an error.
 * A column whose maximum equals its minimum is NaN in every output.  Every sum is one thread's sequential sum over i: an entry (j, m)
 * is bit-equal whatever D, M and R surround it.  M = 0 is PK_OK. */
int pk_sobol_indices_batch(pk_ctx*, int64_t N, int D, int64_t M, const double* Y, const int32_t* counts, int R,
                           double* S1, double* ST, double* S1_sd, double* ST_sd, double* var);

/* The bookkeeping of a reference-direction many-objective search without a host round trip (reference: pymoo's UNSGA3 with
 * das-dennis(3, 20) directions, SBX(0.9, 15) and PM(1 / n_var, 10) as built at global_model/runner.py:663-699; pymoo is optional).
 * global_model/search.py is the generation loop around these four calls; X, F, ranks and niches stay in HBM.  All pointers are device
 * pointers; the calls are asynchronous on the context's stream, except that pk_moo_rank_batch reads 4 bytes per front.
 *
 * Non-dominated ranks of the rows of F [P,M] (M in 2..4, P <= 65536; P = 0 is PK_OK).  Row a dominates row b iff a_m <= b_m for all m and
 * a_m < b_m for some m; a row with a non-finite entry dominates nothing and is dominated by every all-finite row; two non-finite rows, or
 * two equal rows, do not dominate each other.  rank = 0 where nothing dominates the row, else 1 + the largest rank among its dominators
 * (the result of peeling front after front).  n_fronts [1] is the number of fronts formed.  stop_at > 0: peeling stops after the first
 * front with which at least stop_at rows are ranked, and every row still unranked gets rank = n_fronts; stop_at = 0 ranks every row. */
int pk_moo_rank_batch(pk_ctx*, int P, int M, const double* F, int stop_at, int32_t* rank, int32_t* n_fronts);
/* Reference-direction association: f' = (F - ideal) / max(nadir - ideal, 1e-12) per column, dist_h = || f' - (f'.w_h / w_h.w_h) w_h || for
 * the H <= 4096 rows w_h of dirs [H,M]; niche [P] = argmin_h dist_h (the lowest h among equals), dist [P] = that distance.  A row of F with
 * a non-finite entry gets niche = -1 and dist = +inf. */
int pk_moo_associate_batch(pk_ctx*, int P, int M, const double* F, const double* ideal, const double* nadir, int H, const double* dirs,
                           int32_t* niche, double* dist);
/* The K survivors of P ranked and associated rows as ascending row indices keep [K] (K > P is an error; K = 0 is PK_OK).  Whole fronts
 * are taken while they fit.  The first front that does not fit fills the rest by niching: with rho_j the taken rows of niche j, repeatedly
 * the niche with the smallest rho_j (lowest j among equals) that still has a row of that front gives its row of smallest dist (lowest
 * index among equals) and rho_j += 1.  Evaluated in closed form: with a_j the rows of that front in niche j and L the largest integer with
 * sum_j min(a_j, max(0, L - rho_j)) <= the rows still wanted, niche j gives c_j = min(a_j, max(0, L - rho_j)) rows, one more for the
 * lowest-j niches with rho_j <= L and c_j < a_j until the count is met.  Rows of that front with niche = -1 are taken last, by index.
 * Within a niche a NaN dist orders after every number (by index among NaNs); pk_moo_associate_batch writes none. */
int pk_moo_survive_batch(pk_ctx*, int P, int K, const int32_t* rank, const int32_t* niche, const double* dist, int H, int32_t* keep);
/* Offspring Xc [P,n_var] of the population X [P,n_var]: binary tournament, bounded simulated binary crossover, bounded polynomial
 * mutation.  Every random number is a function of its coordinates only:
 *   u(stream, row, var) = (mix(seed + 0x9E3779B97F4A7C15 (1 + ((gen 8 + stream) P + row) n_var + var)) >> 11) 2^-53       (mod 2^64),
 * mix = the SplitMix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31).
 *   tournament  slot c: a = floor(u(0, c, 0) P), b = floor(u(1, c, 0) P); the lower rank wins; with equal rank and the same niche the
 *               smaller dist wins; otherwise a.  parents [P] (optional) = the winner of each slot.  Pair q mates the winners of slots 2 q
 *               and 2 q + 1 into offspring rows 2 q and 2 q + 1; with odd P the last slot copies its winner (and is then mutated).
 *   SBX         the pair crosses iff u(2, q, 0) <= pc; variable v of it iff u(3, q, v) <= 0.5, |x1 - x2| > 1e-14 and xu_v > xl_v.  With
 *               y1 < y2 the two values, u = u(4, q, v) and e = eta_c + 1:  beta = 1 + 2 (y1 - xl) / (y2 - y1), alpha = 2 - beta^-e,
 *               betaq = (u alpha)^(1/e) if u <= 1 / alpha else (1 / (2 - u alpha))^(1/e), c1 = ((y1 + y2) - betaq (y2 - y1)) / 2; c2 its mirror
 *               image with beta = 1 + 2 (xu - y2) / (y2 - y1); both clipped to [xl, xu].  Row 2 q gets c1 and row 2 q + 1 gets c2,
 *               exchanged iff u(5, q, v) <= 0.5.
 *   PM          offspring row c, variable v mutates iff u(6, c, v) <= pm and xu_v > xl_v.  With u = u(7, c, v), e = eta_m + 1,
 *               d1 = (x - xl) / (xu - xl), d2 = (xu - x) / (xu - xl):  dq = (2 u + (1 - 2 u) (1 - d1)^e)^(1/e) - 1 for u < 0.5, else
 *               1 - (2 (1 - u) + 2 (u - 0.5) (1 - d2)^e)^(1/e);  x += dq (xu - xl), clipped.
 * A value that is neither crossed nor mutated is its parent's, bit for bit. */
int pk_moo_mate_batch(pk_ctx*, int P, int n_var, const double* X, const int32_t* rank, const int32_t* niche, const double* dist,
                      const double* xl, const double* xu, uint64_t seed, int gen, double pc, double eta_c, double pm, double eta_m,
                      double* Xc, int32_t* parents);

/* Replaces config.config.score_fit(params, target, prediction, alpha, beta, gamma, delta, mu) (config/config.py:176-226) for B
 * candidates: theta [B,P], target [N] (shared), pred [B,N] (e.g. the `flat` output) -> out [B].  weights = {alpha (rmse), beta (mae),
 * gamma (var), delta (mse), mu (l2)} as a HOST pointer, NULL = all 1 (config/constants.py:77-83). */
int pk_score_fit_batch(pk_ctx*, int64_t B, const double* theta, int P, const double* target, const double* pred, int N,
                       const double* weights, double* out);

/* Host-pointer conveniences (stage through HBM, synchronise before returning). */
int pk_solve_protein_batch_host(pk_ctx*, int model, int n_sites, int64_t B,
                                const double* theta, const double* y0, int y0_is_batched,
                                const double* t, int T, const pk_solver_opts* opts,
                                double* sol, double* flat, double* metric, int metric_id,
                                int32_t* status, int32_t* n_steps);
int pk_solve_protein_sens_batch_host(pk_ctx*, int model, int n_sites, int64_t B,
                                     const double* theta, const double* y0, int y0_is_batched,
                                     const double* t, int T, const pk_solver_opts* opts,
                                     double* flat, double* dflat, int32_t* status, int32_t* n_steps);
int pk_rhs_protein_batch_host(pk_ctx*, int model, int n_sites, int64_t B,
                              const double* theta, const double* y, double* dydt);
int pk_jacobian_protein_batch_host(pk_ctx*, int model, int n_sites, int64_t B,
                                   const double* theta, double* J);

/* ------------------------------------------------------------------------------------------------------------------
 * Network (global_model) path -- SURVEY.md section 8 rows a9-a16, a21, a23.
 * pk_network_desc mirrors what global_model.network.System.odeint_args() packs (network.py:443-526) minus the per-candidate
 * parameters; all pointers are HOST pointers and are copied to HBM by pk_network_create.
 * A candidate is one row of x [B, n_var], n_var = n_K + 5 N + total_sites + 1, laid out as the optimiser's decision vector
 * (global_model/params.py:60-96):  [c_k | A_i | B_i | C_i | D_i | Dp_i | E_i | tf_scale];  x_is_raw != 0 applies the softplus of
 * params.unpack_params (params.py:106-132, utils.py:229-241) on load.
 * State layout: per protein i at offset_y[i]: models 0/1/4 [R, P, site_1..site_ns]; model 2 [R, state_0 .. state_{2^ns - 1}]. */
typedef struct pk_network_desc {
  int32_t model;                 /* 0 distributive, 1 sequential, 2 combinatorial, 4 saturating (global_model/config.py:59-61) */
  int32_t N, n_K, total_sites, n_grid;
  const int32_t *offset_y, *offset_s, *n_sites;                        /* [N] */
  const int32_t *W_indptr, *W_indices; const double* W_data;           /* CSR, total_sites x n_K  (kinase -> site) */
  const int32_t *TF_indptr, *TF_indices; const double* TF_data;        /* CSR, N x N              (TF -> target)   */
  const double*  tf_deg;                                               /* [N] */
  const int32_t* driver_map;                                           /* [N] kinase index driving protein i, or -1 */
  const double*  kin_grid;                                             /* [n_grid] bucket edges of the kinase input */
  const double*  kin_Kmat;                                             /* [n_K, n_grid] row-major */
} pk_network_desc;
typedef struct pk_net pk_net;

pk_net* pk_network_create(pk_ctx*, const pk_network_desc*);            /* NULL on error: see pk_last_error */
void    pk_network_destroy(pk_net*);
int     pk_network_n_states(const pk_net*);
int     pk_network_n_var(const pk_net*);

/* Replaces global_model.jacspeedup.rhs_odeint(y, t, *args) (jacspeedup.py:392-394 -> rhs_nb_* :176-388) for B candidates:
 * x [B,n_var]; y [S] or [B,S]; t [1] or [B] (device pointers); dydt [B,S]. */
int pk_network_rhs_batch(pk_ctx*, pk_net*, int64_t B, const double* x, int x_is_raw, const double* y, int y_is_batched,
                         const double* t, int t_is_batched, double* dydt);
/* Analytic Jacobian, row-major [B,S,S]; stands where the reference uses the finite-difference fd_jacobian_odeint
 * (jacspeedup.py:398-588) as odeint's Dfun. */
int pk_network_jacobian_batch(pk_ctx*, pk_net*, int64_t B, const double* x, int x_is_raw, const double* y, int y_is_batched,
                              const double* t, int t_is_batched, double* J);
/* Replaces global_model.simulate.simulate_odeint(sys, t_eval, rtol, atol, mxstep) -> Y[T,S] (simulate.py:34-80) for B candidates
 * of one network: x [B,n_var] and y0 ([S] or [B,S]) are device pointers, t is a HOST pointer to T strictly increasing times
 * (t[0] = initial time), Y [B,T,S] device.  Integrator: linearly implicit with the per-protein diagonal blocks of the analytic Jacobian
 * (DESIGN.md): PK_METHOD_ARK436 (order 4) where its kernel applies, else PK_METHOD_ROS34PW2 (order 3); either can be requested by name,
 * every other opts->method value means "the default"; PK_METHOD_DP5 selects the reference's explicit RK45 (jacspeedup.solve_custom,
 * jacspeedup.py:31-64; h0 = dt_init, 0 -> 0.05; max_steps <= 0 -> 2 000 000).  opts->rtol / atol / h0 / max_steps / err_norm are honoured.
 * All four topologies; combinatorial blocks (2) up to 3 sites per protein run out of registers, larger ones (<= 16 sites) in the LDS kernel.
 * Networks beyond one workgroup's LDS (S > 1024, N > 512 or a work area over 160 KiB) integrate with ROS34PW2 in the workspace kernel:
 * every per-candidate vector in a slab of the context's scratch arena (pk_network_workspace_bytes), no size limit but device memory;
 * opts->kernel = PK_KERNEL_WORKSPACE selects that kernel on any network.  ARK436 and DP5 stay limited to their one-workgroup kernels. */
int pk_network_simulate_batch(pk_ctx*, pk_net*, int64_t B, const double* x, int x_is_raw, const double* y0, int y0_is_batched,
                              const double* t_host, int T, const pk_solver_opts* opts, double* Y, int32_t* status, int32_t* n_steps);
/* The integrator pk_network_simulate_batch will run for `opts` (NULL = defaults) on this network: PK_METHOD_DP5, PK_METHOD_ARK436 or
 * PK_METHOD_ROS34PW2 (always ROS34PW2 on networks beyond one workgroup's LDS and with opts->kernel = PK_KERNEL_WORKSPACE);
 * PK_ERR_UNSUPPORTED when ARK436 was requested and its kernel does not fit (N, sites per protein, 160 KB of LDS), or ARK436 / DP5 together
 * with PK_KERNEL_WORKSPACE.  Pure host arithmetic.  Host layers derive integrator-dependent defaults (tolerances) from this answer instead
 * of re-stating the rule. */
int pk_network_resolve_method(const pk_net*, const pk_solver_opts* opts);
/* Bytes of the context's scratch arena the workspace kernel reserves for B candidates on this network: grid x slab, grid = min(B, workgroups
 * resident on the context's GPU), slab = 8 (n_var + 8 S + n_K + total_sites + 6 N) bytes rounded up to 128 B -- bounded in B.  < 0 on error. */
int64_t pk_network_workspace_bytes(pk_ctx*, const pk_net*, int64_t B);
/* global_model.params.unpack_params (softplus of the raw decision vectors): x_raw [B,n_var] -> x_phys [B,n_var]. */
int pk_network_unpack_batch(pk_ctx*, pk_net*, int64_t B, const double* x_raw, double* x_phys);

/* Discrete Frechet distance between observed and predicted curves for B candidates x n_series series -- replaces
 * frechet.distance.frechet_distance (frechet/distance.py:9-56) inside the Pareto pick loop of global_model/runner.py:780-841.
 * Series s compares the observed points (obs_t, obs_v)[obs_ptr[s] .. obs_ptr[s+1]) with the predicted points
 * (pred_t[k], pred[b, pred_idx[k]]) for k in [pred_ptr[s], pred_ptr[s+1]); points are 2-D (time, value), both lists sorted by time by the
 * caller; pred [B, n_obs] is e.g. the output of pk_network_observables_batch.  max_points = longest curve (<= 32; checked here because
 * the kernel keeps the DP row in registers).  out [B, n_series]; a series with an empty side gives 0.  All pointers device pointers. */
int pk_frechet_batch(pk_ctx*, int64_t B, int n_series, const int32_t* obs_ptr, const double* obs_t, const double* obs_v,
                     const int32_t* pred_ptr, const double* pred_t, const int32_t* pred_idx, const double* pred, int n_obs,
                     int max_points, double* out);

/* Fused objective of one optimiser candidate after the simulation -- replaces global_model.lossfn.LOSS_FN (lossfn.py:114-382; all eight
 * LOSS_MODEs) and the assembly in GlobalODE_MOO._evaluate (optproblem.py:99-160).  pk_loss_data mirrors cache.prepare_fast_loss_data's
 * arrays (HOST pointers, copied to HBM and index-checked by pk_network_loss_create for a time grid of T points).
 *   Y [B,T,S] device; x [B,n_var] + defaults [n_var] (device; both optional: the prior penalty on A,B,C,D,E);
 *   lambdas = {protein, rna, phospho, prior} (host); status [B] from the simulation (optional: flagged => fail_value);
 *   loss_sums [B,3] raw weighted sums (LOSS_FN's return value) and / or F [B,3] the three objectives. */
typedef struct pk_loss_data {
  int32_t n_prot, n_rna, n_pho;
  const int32_t *p_prot, *t_prot; const double *obs_prot, *w_prot;
  const int32_t *p_rna, *t_rna;   const double *obs_rna, *w_rna;
  const int32_t *p_pho, *s_pho, *t_pho; const double *obs_pho, *w_pho;
  int32_t prot_base_idx, rna_base_idx, pho_base_idx;
} pk_loss_data;
typedef struct pk_loss pk_loss;
pk_loss* pk_network_loss_create(pk_ctx*, pk_net*, const pk_loss_data*, int T);
void     pk_network_loss_destroy(pk_loss*);
int      pk_network_objective_batch(pk_ctx*, pk_net*, pk_loss*, int64_t B, const double* Y, int T, int loss_mode,
                                    const double* x, int x_is_raw, const double* defaults, const double* lambdas, double fail_value,
                                    const int32_t* status, double* loss_sums, double* F);

/* [r3] simulate + objective in ONE launch (SURVEY fused op (i): optproblem.py:99-160 calls simulate_odeint -> LOSS_FN -> prior per candidate):
 * the additive integrator scores the loss handle's observations at its output times out of registers and writes F [B,3] / loss_sums [B,3];
 * the trajectory Y [B,T,S] is written only if Y != NULL.  Results equal pk_network_simulate_batch followed by pk_network_objective_batch
 * up to the order of the sums.  Takes: topologies 0 / 4 on the default integrator (PK_METHOD_LRP12 = "default" or PK_METHOD_ARK436), loss
 * data whose three baselines are time index 0 and that observe no (state, time) twice.  Otherwise PK_ERR_UNSUPPORTED (the message says
 * which): call the two functions above instead.  x, y0, defaults, Y, status, n_steps, loss_sums, F: DEVICE pointers; t, lambdas: HOST.
 * On request -- opts->method = PK_METHOD_ROS34PW2 or opts->kernel = PK_KERNEL_WORKSPACE -- the order-3 integrator scores the loss instead: all
 * four topologies at every size, wherever pk_network_simulate_batch would run the general LDS kernel or the workspace kernel for these opts
 * (opts->linsolve = PK_LINSOLVE_STRUCTURED forces the LDS kernel, as for simulate; a plan on the register-resident kernels answers
 * PK_ERR_UNSUPPORTED).  It scores the observation lists bucketed by time index, so a (state, time) may be observed twice; the protein /
 * phospho baselines must be time index 0 and no rna observation may precede the rna baseline.  A fused launch keeps N more doubles per
 * candidate (the rna baseline): a larger LDS request, or past 160 KiB the workspace kernel with slabs N doubles longer than
 * pk_network_workspace_bytes reports for plain launches.  Default opts answer exactly as before. */
int      pk_network_simulate_objective_batch(pk_ctx*, pk_net*, pk_loss*, int64_t B, const double* x, int x_is_raw, const double* y0,
                                             int y0_is_batched, const double* t_host, int T, const pk_solver_opts* opts, int loss_mode,
                                             const double* defaults, const double* lambdas, double fail_value, double* Y, int32_t* status,
                                             int32_t* n_steps, double* loss_sums, double* F);

/* global_model.lossfn.LOSS_FN with its own positional argument list (lossfn.py:114-121; :386 picks loss_function_comb when MODEL == 2):
 *   LOSS_FN(Y, p_prot, t_prot, obs_prot, w_prot, p_rna, t_rna, obs_rna, w_rna, p_pho, s_pho, t_pho, obs_pho, w_pho, prot_map,
 *           prot_base_idx, rna_base_idx, pho_base_idx) -> (loss_p, loss_r, loss_ph)          [called at optproblem.py:137-145]
 * for B trajectories and WITHOUT a network handle: the state offsets come from prot_map [N,2] int32 = (block start, n_sites) -- for the
 * combinatorial topology (block start, n_states = 2^n_sites).  HOST pointers throughout (the reference passes numpy arrays): indices are
 * checked on the host, arrays staged to HBM, one launch, synchronised.  Y [B,T,S]; loss_sums [B,3]; loss_mode = LOSS_MODE 0..7. */
int pk_loss_fn_batch_host(pk_ctx*, int combinatorial, int loss_mode, int64_t B, const double* Y, int T, int S, const pk_loss_data*,
                          const int32_t* prot_map, int N, double* loss_sums);

/* Array form of the pred_fc columns of global_model.simulate.simulate_and_measure (simulate.py:119-202): fold changes for the index
 * lists of a pk_loss (protein | rna | phospho, obs / w ignored), floor eps (the reference uses 1e-12 there): pred [B, n_prot+n_rna+n_pho]. */
int pk_network_observables_batch(pk_ctx*, pk_net*, pk_loss*, int64_t B, const double* Y, int T, double eps, double* pred);

/* simulate + fold-change observables + scalar Morris metric in ONE launch (SURVEY fused op (iii) on the network path: the body of the
 * reference's sensitivity worker, sensitivity.py:143-168 = simulate_and_measure -> _compute_scalar_metric): the order-3 integrator forms the
 * fold changes of `lists` (a pk_loss; its obs / w arrays are ignored) at its output times exactly as pk_network_observables_batch forms them
 * from a stored trajectory (floor eps), and reduces them per candidate to metric [B]:
 *   PK_NET_METRIC_TOTAL_SIGNAL sum p, _MEAN sum p / n, _VARIANCE the population variance (Welford partials merged pairwise in a fixed order,
 *   never E[p^2] - E[p]^2), _L2_NORM sqrt(sum p^2); all four are 0.0 for empty lists.  A candidate's value does not depend on B.
 * pred [B, n_prot + n_rna + n_pho] (optional) receives the fold changes in the order of the lists as they were given to
 * pk_network_loss_create; Y [B,T,S] (optional) the trajectory; at least one of metric, pred, Y must be non-NULL.  status, n_steps and Y equal
 * pk_network_simulate_batch's for the same opts bit for bit.  A flagged candidate (status != 0) gets metric = NaN and an all-NaN pred row.
 * Runs wherever the plan for opts (pk_network_resolve_method) is PK_METHOD_ROS34PW2 on the general LDS kernel or on the workspace kernel --
 * by default on networks beyond one workgroup -- and moves from the LDS kernel to the workspace kernel where the LDS request (N doubles
 * more than a plain launch: the rna baseline) passes 160 KiB.  PK_ERR_UNSUPPORTED, with the remedy in pk_last_error: a plan on the
 * register-resident kernels (ask for the LDS kernel: opts->linsolve = PK_LINSOLVE_STRUCTURED), on PK_METHOD_ARK436 or PK_METHOD_DP5 (ask for
 * PK_METHOD_ROS34PW2), lists whose protein / phospho baseline is not time index 0 or that hold an rna observation before the rna baseline
 * (call pk_network_simulate_batch + pk_network_observables_batch).  PK_ERR_ARG: metric_id outside 0..3; metric, pred and Y all NULL.
 * x, y0, Y, pred, metric, status, n_steps: DEVICE pointers; t: HOST. */
enum { PK_NET_METRIC_TOTAL_SIGNAL = 0, PK_NET_METRIC_MEAN = 1, PK_NET_METRIC_VARIANCE = 2, PK_NET_METRIC_L2_NORM = 3 };
int pk_network_simulate_measure_batch(pk_ctx*, pk_net*, pk_loss* lists, int64_t B, const double* x, int x_is_raw, const double* y0,
                                      int y0_is_batched, const double* t_host, int T, const pk_solver_opts* opts, double eps, int metric_id,
                                      double* Y, double* pred, double* metric, int32_t* status, int32_t* n_steps);

/* Y(t) AND dY / dx_c for K chosen entries c = cols[k] of the candidate vector from ONE integration (forward sensitivities: the augmented
 * system s_c' = f_y s_c + df / dx_c, s_c(t0) = 0 -- y0 is data --, integrated with the state by the order-3 Rosenbrock-W method; every
 * tangent stage is solved with the state's per-protein block factors of that step and its right-hand side is the exact directional
 * derivative of the network right-hand side: csrc/pk_network_sens.hpp).  Replaces differencing pk_network_simulate_batch by hand.
 *   cols [K] HOST pointer: indices into x in its own order [c_k | A | B | C | D | Dp | E | tf_scale]; an index outside [0, n_var) or a
 *   repeated one is PK_ERR_ARG.  dY [B,T,S,K], the K derivatives of one state at one time contiguous; row t = 0 of dY is 0.  Y [B,T,S] | NULL.
 *   With x_is_raw the derivative is with respect to the RAW entry: the physical derivative times softplus'(raw), exactly 1 where softplus
 *   returns its argument (raw > 20).  x, y0, Y, dY, status, n_steps: DEVICE pointers; t, cols: HOST.
 * Always PK_METHOD_ROS34PW2, whatever opts->method / linsolve say -- except that an explicit PK_METHOD_ARK436, PK_METHOD_DP5 or
 * PK_KERNEL_WORKSPACE is PK_ERR_UNSUPPORTED (pk_last_error names the remedy).  Route: the general LDS kernel where at least one column fits
 * beside the state in 160 KiB of LDS (pk_network_sens_columns_per_launch >= 1); the slab route -- state and tangents in slabs of the
 * context's scratch arena, no size limit but device memory -- on every other network (S > 1024, N > 512, or no column fits) and, at any
 * size, with opts->kernel = PK_KERNEL_HBM.  On slabs KC = pk_network_sens_hbm_columns, the launch is a persistent grid of
 * min(B x ceil(K / KC), resident workgroups) over the (candidate, chunk) items, and pk_network_sens_workspace_bytes reports the slabs; every
 * rule below holds on both routes, and a candidate's numbers agree between them within rounding, not bit for bit.
 * Tangents are held to the same rtol / atol as the states, in the norm opts->err_norm selects (maximum over states and columns; RMS: over
 * all S (1 + columns of the workgroup) entries).
 * Column chunks: one workgroup integrates one candidate with up to KC = pk_network_sens_columns_per_launch columns, the launch is
 * B x ceil(K / KC) workgroups.  Every chunk integrates the state itself with its own step-size control: each column is within rtol / atol
 * of the exact derivative, the chunks are not bit-coupled.  Chunk 0 writes Y; status is the OR over the chunks; n_steps is chunk 0's.
 * Failure: a flagged chunk leaves NaN in its own columns at the rows it did not reach, and in every row when it is PK_ST_NONFINITE (a
 * non-finite state, parameter or tangent, or a tangent beyond 1e100 in magnitude, at a step whose error is not finite); Y follows
 * pk_network_simulate_batch's rule.
 * K = 0 with Y set is pk_network_simulate_batch with PK_METHOD_ROS34PW2 / PK_LINSOLVE_STRUCTURED, bit for bit (with PK_KERNEL_HBM: with
 * PK_KERNEL_WORKSPACE); B = 0 is PK_OK; dY NULL with K > 0 is PK_ERR_ARG.  A candidate's results do not depend on the batch around it. */
int pk_network_simulate_sens_batch(pk_ctx*, pk_net*, int64_t B, const double* x, int x_is_raw, const double* y0, int y0_is_batched,
                                   const double* t_host, int T, const pk_solver_opts* opts, const int32_t* cols_host, int K,
                                   double* Y, double* dY, int32_t* status, int32_t* n_steps);
/* KC of pk_network_simulate_sens_batch on this network: the largest column count whose LDS request stays within 160 KiB (at most n_var);
 * 0 = not one column fits or the network is beyond the LDS kernel (the slab route then runs).  Pure host arithmetic. */
int pk_network_sens_columns_per_launch(pk_net*);
/* KC of the slab route for a request of K columns: min(K, n_var, W) with W = 16 -- not bound by LDS; the dev knob PK_NET_SENS_KC lowers W
 * as it lowers the LDS counts.  scoring: 0 = pk_network_simulate_sens_batch, 1 = pk_network_simulate_objective_grad_batch (the same width
 * today).  PK_ERR_ARG for a null handle or K < 0.  Pure host arithmetic. */
int pk_network_sens_hbm_columns(pk_net*, int K, int scoring);
/* Bytes of slabs the slab route reserves in the context's scratch arena for B candidates and K columns (1 <= K <= n_var): grid x slab, grid =
 * min(B x ceil(K / KC), workgroups of the flavour's kernel resident on the context's GPU) -- bounded in B --, slab = the plain work area of
 * pk_network_workspace_bytes plus the sensitivity area the LDS kernels keep behind the plain request (2 N + KC (7 S + total_sites + N + 2)
 * doubles; scoring: N + 4 + KC (N + 3) more), rounded up to 128 B.  The K column indices are staged in front of the slabs (4 K bytes in
 * whole 128-B lines, not counted here).  < 0 on error. */
int64_t pk_network_sens_workspace_bytes(pk_ctx*, pk_net*, int64_t B, int K, int scoring);

/* The three objectives of pk_network_simulate_objective_batch AND their exact discrete derivative with respect to K chosen entries
 * cols[k] of the candidate vector, from ONE launch: the sensitivity integrator above differentiates the loss where the state and the
 * chunk's tangents land on an output row (csrc/pk_network_sens.hpp, scoring flavour; csrc/pk_network_loss_grad.hpp for the point-loss
 * and fold-change derivatives).  Neither the trajectory nor the tangent trajectory is written unless Y / dY are asked for.
 *   Outputs, all DEVICE pointers, each optional (NULL): Y [B,T,S], dY [B,T,S,K] (as pk_network_simulate_sens_batch), pred [B,n_obs] and
 *   dpred [B,n_obs,K] (fold changes with LOSS_FN's floor 1e-9 and their derivative -- 0 through an active floor --, in the caller's
 *   (protein | rna | phospho) list order), loss_sums [B,3] and dsums [B,3,K] (the weighted sums and their derivative),
 *   F [B,3] and dF [B,3,K] = dsums norm_m lambda_m + d prior / d x_c; the prior term lambda_prior 2 (p - d) / (d + 1e-6)^2 / (5 N) is non-zero
 *   for columns in A, B, C, D, E and enters all three objectives.  With x_is_raw every derivative is with respect to the raw entry.
 * Rules of pk_network_simulate_sens_batch: always PK_METHOD_ROS34PW2, on the general LDS kernel where
 * pk_network_objective_grad_columns_per_launch >= 1 and on HBM slabs elsewhere or with PK_KERNEL_HBM; an explicit PK_METHOD_ARK436,
 * PK_METHOD_DP5 or PK_KERNEL_WORKSPACE is PK_ERR_UNSUPPORTED; cols (HOST) is checked on the host; column chunks of
 * KC = pk_network_objective_grad_columns_per_launch (slabs: pk_network_sens_hbm_columns), each integrating the state itself; chunk 0 writes Y, pred, loss_sums, F and n_steps;
 * status is the OR over the chunks.  Rules of the order-3 fused objective: protein / phospho baselines are time index 0 and no rna
 * observation lies before the rna baseline (else PK_ERR_UNSUPPORTED); a (state, time) may be observed twice; loss_mode 0..7; T equals the
 * handle's; lambdas is required for F / dF.  PK_ERR_ARG when every output pointer is NULL, or K > 0 and dY, dpred, dsums, dF are all NULL.
 * Every sum is one thread's sequential sum in list order (no atomics): a candidate's numbers are bit-equal alone and in any batch, and
 * permuting cols permutes the outputs (K <= KC, maximum norm).
 * Failure: a flagged chunk has NaN in its own columns of dsums, dF and dpred; F = fail_value and an all-NaN pred row when chunk 0 is
 * flagged or a state of a scored row is not finite.
 * K = 0 is pk_network_simulate_objective_batch with PK_METHOD_ROS34PW2 / PK_LINSOLVE_STRUCTURED, bit for bit (with PK_KERNEL_HBM: with
 * PK_KERNEL_WORKSPACE; loss_sums or F required, pred must be NULL).  pk_last_error names the remedy for every refusal. */
int pk_network_simulate_objective_grad_batch(pk_ctx*, pk_net*, pk_loss*, int64_t B, const double* x, int x_is_raw, const double* y0,
                                             int y0_is_batched, const double* t_host, int T, const pk_solver_opts* opts,
                                             const int32_t* cols_host, int K, int loss_mode, const double* defaults, const double* lambdas,
                                             double fail_value, double* Y, double* dY, double* pred, double* dpred, double* loss_sums,
                                             double* dsums, double* F, double* dF, int32_t* status, int32_t* n_steps);
/* KC of pk_network_simulate_objective_grad_batch: as pk_network_sens_columns_per_launch, with the rna baseline, its tangents and the
 * accumulators on top (8 N + 32 bytes, and 8 N + 24 per column).  Pure host arithmetic. */
int pk_network_objective_grad_columns_per_launch(pk_net*);

/* Bounded Levenberg-Marquardt polish of B network candidates in lockstep over K chosen entries cols[k] of the candidate vector, every
 * other entry held: the Gauss-Newton consumer of pk_network_simulate_objective_grad_batch's pred / dpred, with its state in HBM
 * (csrc/pk_net_fit.hip; residual rows in csrc/pk_net_fit.hpp, row algebra in csrc/pk_lm.hpp).  Candidate b minimises
 *   cost = 1/2 sum_m obj_w[m] F_m(x),  F = pk_network_simulate_objective_batch's F [3] for loss_mode 0 (the only loss this fit has: a robust
 *   loss would need reweighting), obj_w [3] >= 0 the caller's scalarisation,
 * as a least-squares problem with the rows sqrt(obj_w[m] norm_m lambda_m w_i) (pred_i - obs_i) for every observation i of modality m, in the
 * caller's (protein | rna | phospho) list order, and sqrt((sum_m obj_w[m]) lambda_prior / (5 N)) (p_c - d_c) / (d_c + 1e-6) for every FITTED
 * column c in A, B, C, D, E (defaults != NULL); the prior of the held entries is a constant of the fit.  With x_is_raw the fit runs on the
 * raw entries: dpred is the raw derivative, the prior row's carries softplus'.  lb, ub bound the fitted entries in the space of x.
 *   x0, x [B,n_var]; y0 [S] | [B,S]; defaults [n_var] | NULL; lb, ub [K] | [B,K], both NULL = no box; cost [B]; F [B,3]; JTJ [B,K,K] | NULL;
 *   reason [B] | NULL; status [B] | NULL: DEVICE pointers.  t [T], cols [K], lambdas [4] = {protein, rna, phospho, prior}, obj_w [3],
 *   counters [6] = {iterations, simulated candidates, launches, host waits, Jacobian phases, trial rounds}: HOST.
 * The rules and constants are pk_fit_protein_rows_batch's (Marquardt scaling, mu0 = 1e-3, levels mu, 4 mu, 16 mu ... up to 12 per
 * iteration, fit->trial_levels of them per launch, the first acceptable one taken, projection on the box, ftol / xtol); fit->log_space and
 * fit->use_reg must be 0.  reason: 0 ftol / xtol, 1 gradient / empty free set, 2 damping budget, 3 max_iter, 4 the Jacobian launch flagged
 * the candidate (any chunk): the row stops at its last accepted point and never steps from NaN.
 * One iteration is a Jacobian phase -- gather, ONE tangent launch on the active rows (pk_network_simulate_objective_grad_batch with its
 * route rules: LDS where columns fit, HBM slabs elsewhere or with PK_KERNEL_HBM, chunks of KC columns), the normal-equations kernel; in row
 * chunks where dpred would pass 1 GiB -- and trial rounds: the trials kernel, ONE plain order-3 fused-objective launch on (levels x pending
 * rows) trial candidates (that entry point with no columns), the accept kernel.  The host waits once per phase and once per round, for one
 * flag per row.  State and scratch live in the grow-only fit arena of the context (no allocation per iteration); the call holds the
 * context's lock and returns after its last wait.
 * Cost consistency: a tangent launch controls its steps on state and tangents together, so its trajectory lies within rtol / atol of the
 * plain launch's, not on it.  Every cost the gain ratio compares comes from PLAIN launches: the start cost from one at clip(x0), every
 * trial's from its round's, and an accepted trial's cost and F become the row's own.  The Jacobian phase contributes A = J^T J and
 * g = J^T r only, r from its own pred.  Hence F equals pk_network_simulate_objective_batch at the returned x BIT FOR BIT (same opts with
 * PK_METHOD_ROS34PW2 / PK_LINSOLVE_STRUCTURED; PK_KERNEL_HBM: PK_KERNEL_WORKSPACE), and cost = 1/2 ((obj_w0 F0 + obj_w1 F1) + obj_w2 F2).
 * Failures: a flagged trial has F = fail_value and is never acceptable; a flagged Jacobian launch is reason 4.  status is the row's last
 * Jacobian launch OR-ed with the trial launches looked at in the iteration that followed (max_iter = 0: the start launch).
 * JTJ belongs to the point of the row's last Jacobian phase (one accepted step behind x unless the last iteration took none); a row
 * whose only Jacobian launch was flagged leaves its JTJ unwritten.  max_iter = 0: x = clip(x0), its cost and F, reason 3, JTJ NOT WRITTEN,
 * counters = {0, B, 3, 0, 0, 0}.  Every sum is one thread's sequential sum in list order, prior rows last (no atomics): a row's x, cost,
 * F and JTJ do not depend on the rows around it, their order, or trial_levels.
 * PK_ERR_ARG: K < 1 or > n_var, a repeated or out-of-range column, a null required pointer, one of lb / ub alone, a negative obj_w,
 * log_space / use_reg, trial_levels outside 0..12, max_iter < 0, T other than the loss handle's.  PK_ERR_UNSUPPORTED wherever the two
 * launches answer it, and for a K whose damped system (K (K + 1) / 2 + 9 K doubles) passes 160 KiB of LDS.  B = 0 is PK_OK. */
int pk_network_fit_batch(pk_ctx*, pk_net*, pk_loss*, int64_t B, const double* x0, int x_is_raw, const double* y0, int y0_is_batched,
                         const double* t_host, int T, const pk_solver_opts* opts, const int32_t* cols_host, int K, const double* defaults,
                         const double* lambdas, const double* obj_w, const double* lb, const double* ub, int bounds_are_batched,
                         const pk_fit_opts* fit, double fail_value, double* x, double* cost, double* F, double* JTJ, int32_t* reason,
                         int32_t* status, int64_t counters[6]);

/* Timing hook for bench.py: runs `iters` back-to-back launches of pk_solve_protein_batch on the context's
 * stream between two hipEvents and returns the mean kernel time per launch in milliseconds (< 0 on error). */
double pk_time_solve_protein_batch(pk_ctx*, int iters, int model, int n_sites, int64_t B,
                                   const double* theta, const double* y0, int y0_is_batched,
                                   const double* t, int T, const pk_solver_opts* opts,
                                   double* sol, double* flat, double* metric, int metric_id,
                                   int32_t* status, int32_t* n_steps);

/* Wave pacing of the parked one-wave LRP12 distmod kernels.  The policy is the environment variable PK_DIST_SCHED, read
 * once per process: off | lead | level | lead+level (pk_dist_sched_names); unset, the four-lane layouts (17 <= n_sites <= 32) run
 * lead+level on grids of up to 4/3 of the device's resident waves and everything else runs off.  pk_dist_sched_parse returns the policy's bits (0 = off) or -1 for a value that is none of them; with such a value set, pk_solve_protein_batch fails with PK_ERR_ARG and names the valid ones.
 * Results do not depend on the policy.  Pure host code, usable without a GPU. */
int         pk_dist_sched_parse(const char* value);
const char* pk_dist_sched_names(void);
/* Wave timeline of the diagnostic kernel that PK_DIST_TRACE=1 selects for the n_sites = 27-30 trajectory + running-sum configuration
 * (tools/dist_wave_timeline.py): `records` is a DEVICE buffer of `capacity` 32-byte records {u64 t_entry, t_exit (100 MHz); u32 block,
 * hw_id, xcc_id, iterations}, one per workgroup, which every later traced launch of the process fills; NULL detaches it.  Synchronous. */
int         pk_dist_trace_set(pk_ctx*, void* records, int64_t capacity);

/* Machine peaks measured on the context's GPU, for bench.py's roofline fractions (the spec-sheet values are printed beside them):
 * sustained HBM copy rate in GB/s (read + written bytes; `bytes` >= 1 MiB per buffer, choose it well beyond the 256 MiB Infinity Cache)
 * and sustained FP64 vector FMA rate in TFLOP/s.  Both allocate and free their own buffers; < 0 on error. */
double pk_measure_hbm_gbs(pk_ctx*, int64_t bytes, int iters);
/* one-directional rates, bytes moved per second: mode 0 = read-only, 1 = write-only (a copy pays the bus turnarounds between the two) */
double pk_measure_hbm_stream_gbs(pk_ctx*, int64_t bytes, int iters, int mode);
double pk_measure_fp64_fma_tflops(pk_ctx*, int iters);

/* ---- multi-GPU for an embedder without torch.distributed: one process per GPU, each rank integrates ITS rows with the
 * batch entry points above and gathers the per-row results with ONE all-gather (RCCL over xGMI, on the context's stream) -- candidates /
 * replicas never move.  Rank 0 makes an id (pk_comm_unique_id), the embedder ships its PK_COMM_ID_BYTES to every rank by its own means
 * (MPI, a file, a socket), every rank calls pk_comm_init(ctx, id, rank, world); pk_allgather_f64(ctx, send, count, recv): send [count],
 * recv [world * count] DEVICE pointers, rank r's block at recv + r * count.  Interleave rows as phoskintime_amd/distributed.py does
 * (rank = position mod world in decreasing order of a cost proxy) to balance step counts.  RCCL is bound at run time: PK_ERR_UNSUPPORTED
 * when librccl cannot be loaded.  pk_destroy frees the communicator too. */
#define PK_COMM_ID_BYTES 128
int pk_comm_unique_id(pk_ctx*, char* id_out /* [PK_COMM_ID_BYTES] */);
int pk_comm_init(pk_ctx*, const char* id /* [PK_COMM_ID_BYTES] */, int rank, int world);
int pk_comm_rank(pk_ctx*);
int pk_comm_world(pk_ctx*);
int pk_allgather_f64(pk_ctx*, const double* send, int64_t count, double* recv);
int pk_comm_destroy(pk_ctx*);

#ifdef __cplusplus
}
#endif
#endif /* PHOSKIN_H */
