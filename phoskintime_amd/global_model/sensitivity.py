"""Network Morris screening (reference: global_model/sensitivity.py), batched and shardable.

  compute_bounds / _reconstruct_params / _compute_scalar_metric     sensitivity.py:41-140  (host helpers, same semantics)
  run_sensitivity_batch                                             the numerical core of run_sensitivity_analysis (:171-277): sample ->
        candidates -> ONE simulate launch (rtol 1e-5 / atol 1e-7 as simulate_and_measure) -> fold-change observables -> scalar metric per
        candidate -> (multi-GPU: one all-gather of Y) -> elementary-effects analysis.  The reference pickles the whole System per task."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ..sensitivity import morris
from ..sensitivity import sobol
from ..distributed import interleaved_rows, all_gather_interleaved_with_status, shared_seed
from . import config
from .engine import NetworkEngine

_ORDER = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")


def compute_bounds(params_dict, perturbation=config.SENSITIVITY_PERTURBATION):
    bounds, names = [], []
    for key, value in params_dict.items():
        if isinstance(value, np.ndarray):
            for i, v in enumerate(value):
                lb, ub = v * (1 - perturbation), v * (1 + perturbation)
                if abs(v) < 1e-6:
                    lb, ub = 0.0, 0.01
                bounds.append([max(0.0, lb), ub]); names.append(f"{key}_{i}")
        else:
            v = float(value)
            lb, ub = v * (1 - perturbation), v * (1 + perturbation)
            if abs(v) < 1e-6:
                lb, ub = 0.0, 0.01
            bounds.append([max(0.0, lb), ub]); names.append(key)
    return {"num_vars": len(names), "names": names, "bounds": bounds}


def _reconstruct_params(param_vector, names_map, original_shapes):
    p_out, curr = {}, 0
    for key, shape in original_shapes.items():
        if shape == ():
            p_out[key] = param_vector[curr]; curr += 1
        else:
            size = int(np.prod(shape))
            p_out[key] = np.array(param_vector[curr: curr + size]); curr += size
    return p_out


def _compute_scalar_metric(df_prot, df_rna, df_phos, metric="total_signal"):
    parts = [d["pred_fc"].values for d in (df_prot, df_rna, df_phos) if d is not None]
    combined = np.concatenate(parts) if parts else np.array([])
    if len(combined) == 0:
        return 0.0
    if metric == "mean":
        return np.mean(combined)
    if metric == "variance":
        return np.var(combined)
    if metric == "l2_norm":
        return np.linalg.norm(combined)
    return np.sum(combined)


def scalar_metric_batch(pred: torch.Tensor, metric: str = "total_signal") -> torch.Tensor:
    """_compute_scalar_metric over the rows of pred [B, n_obs] (GPU).  The row sums run as a fixed pairwise tree over the columns
    (elementwise adds of column halves): a row's value does not depend on how many rows share the launch -- a library reduction picks its
    split by the whole shape, and a rank that owns half the rows would then round differently from the one-process run."""
    def rowsum(a: torch.Tensor) -> torch.Tensor:
        n = a.shape[1]
        if n == 0:
            return a.new_zeros(a.shape[0])
        m = 1 << (n - 1).bit_length()
        if m != n:
            a = torch.cat([a, a.new_zeros(a.shape[0], m - n)], dim=1)
        while m > 1:
            m >>= 1
            a = a[:, :m] + a[:, m:]
        return a[:, 0]
    n = max(pred.shape[1], 1)
    if metric == "mean":
        return rowsum(pred) / n
    if metric == "variance":
        mu = rowsum(pred) / n
        return rowsum((pred - mu[:, None]) ** 2) / n
    if metric == "l2_norm":
        return torch.sqrt(rowsum(pred * pred))
    return rowsum(pred)


def run_sensitivity_batch(eng: NetworkEngine, fitted_params: Dict, times_p, times_r, times_ph, perturbation: float = config.SENSITIVITY_PERTURBATION,
                          trajectories: int = config.SENSITIVITY_TRAJECTORIES, num_levels: int = config.SENSITIVITY_LEVELS,
                          metric: str = config.SENSITIVITY_METRIC, seed: Optional[int] = None,
                          param_values: Optional[np.ndarray] = None, y0=None, conf_level: float = 0.95, rtol: Optional[float] = None, atol: Optional[float] = None,
                          vary=None, return_pred: bool = False, fused: bool = False, method: str = "auto", kernel: str = "auto"):
    """Returns dict(Si, problem, param_values, Y, status).  ``fitted_params`` maps the eight parameter groups (System.update order)
    to arrays / a scalar; every entry is varied, as in the reference (sensitivity.py:196-215) -- unless ``vary`` names a subset: indices
    into the flat parameter vector (or parameter names ``"A_i_3"``, ``"tf_scale"``); the design then has len(vary) dimensions
    (trajectories x (len(vary) + 1) simulations: BASELINE config 4 is 128 x (200 + 1)) and every other entry stays at its fitted value.
    ``param_values`` (a ready sample matrix) has one column per varied entry.  ``return_pred``: also return the fold-change observables
    ``pred`` [rows of this rank, n_obs] (GPU tensor) and their ``layout``.  ``method`` / ``kernel`` go to ``simulate_batch``.
    ``fused=True``: one ``simulate_measure_batch`` launch measures and reduces every row inside the integrator instead of the three steps
    simulate -> observables -> metric, so neither the trajectories [rows, T, S] nor (without ``return_pred``) the observables
    [rows, n_obs] are allocated; it integrates with the order-3 method -- ``method="rosw"``, ``kernel="lds"`` unless the caller names one
    (the library moves to the workspace kernel where the LDS kernel does not fit) -- so compare it with the unfused call at those settings.
    ``metric`` must then be one of the four named metrics; a refused launch raises ``PhoskinError`` with the library's reason."""
    params = {k: (np.asarray(fitted_params[k], float) if k != "tf_scale" else float(fitted_params[k])) for k in _ORDER}
    from .simulate import measure_tolerances                  # the settings of simulate_and_measure, which the reference's workers call
    tol = measure_tolerances(eng)
    rtol = tol["rtol"] if rtol is None else rtol
    atol = tol["atol"] if atol is None else atol
    problem = compute_bounds(params, perturbation)
    center = None
    if vary is not None:
        names = problem["names"]
        pos = {nm: i for i, nm in enumerate(names)}
        vidx = np.array([pos[v] if isinstance(v, str) else int(v) for v in vary], dtype=np.int64)
        if vidx.size == 0 or np.unique(vidx).size != vidx.size or vidx.min() < 0 or vidx.max() >= len(names):
            raise ValueError("vary must hold distinct indices (or names) of the flat parameter vector")
        center = eng.pack_params(*(params[k] for k in _ORDER))
        problem = {"num_vars": int(vidx.size), "names": [names[i] for i in vidx], "bounds": [problem["bounds"][i] for i in vidx]}
    design = None
    seed = shared_seed(seed)              # N > 1 ranks: every rank must build the SAME design (seed=None would give each its own)
    if param_values is None:
        # the design is built in HBM from the draws (pk_morris_build_batch): no N (D + 1) x D matrix crosses PCIe on the way in
        Xd, design = morris.sample_device(problem, N=trajectories, num_levels=num_levels, seed=seed, device=eng.ctx.device)
    else:
        Xd = torch.as_tensor(np.ascontiguousarray(param_values, dtype=np.float64), device=torch.device("cuda", eng.ctx.device))
    if Xd.shape[1] != problem["num_vars"]:
        raise ValueError(f"the sample matrix has {Xd.shape[1]} columns, the problem {problem['num_vars']} variables")
    Xv = Xd                                                             # the design in its own (varied) coordinates
    if center is not None:                                              # scatter the varied columns into copies of the fitted vector (in HBM)
        Xd = torch.as_tensor(center, device=Xv.device).repeat(Xv.shape[0], 1)
        Xd[:, torch.as_tensor(vidx, device=Xv.device)] = Xv
    if Xd.shape[1] != eng.n_var:                                        # flat vector order == candidate row order (both System.update order)
        raise ValueError(f"parameter vector has {Xd.shape[1]} entries, the network expects {eng.n_var}")
    total = Xd.shape[0]
    times = np.unique(np.concatenate([times_p, times_r, times_ph]).astype(np.float64))
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    # rows are dealt round-robin over the ranks: a Morris design walks through parameter space trajectory by trajectory, so contiguous
    # blocks would hand each rank its own region (and its own step counts); interleaved, every rank integrates the same mix
    rows = interleaved_rows(total, rank, world).to(Xd.device)
    lists, ld = eng.make_index_lists(times, times_p, times_r, times_ph)
    n_obs = ld["p_prot"].size + ld["p_rna"].size + ld["p_pho"].size
    pred = None
    mean_steps = None
    try:
        if rows.numel() > 0:
            Xloc = Xd if world == 1 else Xd[rows]
            if fused:
                out = eng.simulate_measure_batch(lists, Xloc, times, y0=y0, rtol=rtol, atol=atol, max_steps=5000 * times.size, metric=metric, eps=1e-12,
                                                 want_pred=return_pred, method=("rosw" if method == "auto" else method),
                                                 kernel=("lds" if kernel == "auto" else kernel))
                if out is None:
                    from .. import _capi
                    raise _capi.PhoskinError("run_sensitivity_batch(fused=True): the fused launch was refused: "
                                             + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode() + " -- or call with fused=False")
                yloc, pred, status, nst, _ = out
            else:
                Y, status, nst = eng.simulate_batch(Xloc, times, y0=y0, rtol=rtol, atol=atol, max_steps=5000 * times.size, method=method, kernel=kernel)
                pred = eng.observables_batch(lists, Y, n_obs, eps=1e-12)
                yloc = scalar_metric_batch(pred, metric)
            mean_steps = nst.double().mean(dim=0)
            yloc = torch.where(status != 0, torch.zeros_like(yloc), yloc)          # failed simulations contribute Y = 0
        else:
            dev = torch.device("cuda", eng.ctx.device)
            yloc = torch.empty(0, dtype=torch.float64, device=dev); status = torch.empty(0, dtype=torch.int32, device=dev)
        Yall, stat = all_gather_interleaved_with_status(yloc, status, total) if world > 1 else (yloc, status)      # the ONE collective
        Yall = torch.nan_to_num(Yall, nan=0.0, posinf=0.0, neginf=0.0)
        if design is not None:
            ee = morris.elementary_effects_device(design, Yall).cpu().numpy()      # EE [N, D] on the GPU: 8 N D bytes come back
        torch.cuda.current_stream().synchronize()
    finally:
        eng.free_loss(lists)
    Yh = Yall.cpu().numpy()
    X = Xv.cpu().numpy()
    if design is not None:
        Si = morris.analyze_effects(ee, problem.get("names"), conf_level=conf_level, seed=seed)
    else:
        Si = morris.analyze(problem, X, Yh, num_levels=num_levels, conf_level=conf_level, seed=seed)
    out = {"Si": Si, "problem": problem, "param_values": X, "Y": Yh, "status": stat.cpu().numpy(),
           "mean_steps": (None if mean_steps is None else [float(v) for v in mean_steps.cpu()])}      # accepted, rejected: this rank's rows
    if return_pred:
        out.update(pred=pred, layout=ld, rows=rows.cpu().numpy(), times=times)
    return out


def temporal_gsa_batch(eng: NetworkEngine, params: Dict, time_grid=(0, 5, 15, 30, 60, 90, 120), vary=None, perturbation: float = 0.5,
                       n_samples: int = 128, seed: Optional[int] = None, num_resamples: int = 100, conf_level: float = 0.95, proteins=None,
                       y0=None, rtol: Optional[float] = None, atol: Optional[float] = None, fused: bool = False, method: str = "auto",
                       kernel: str = "auto", return_pred: bool = False) -> Dict:
    """Time-resolved Sobol' indices of EVERY protein's fold-change trajectory from ONE Saltelli batch: the numerical core of
    ``run_full_gsa`` (scripts/temporal_sensitivity.py:143-188) for all proteins at once.  The reference draws the same design once per
    protein, runs its n_samples (D + 2) LSODA solves, keeps one protein's trajectory of each and analyses it once per time point; here the
    design is built in HBM (``sobol.sample_device``), scattered into copies of the packed vector, integrated in one launch, and the
    [n_samples (D + 2), N_prot T] fold changes are reduced to indices, bootstrap included, on the device (``sobol.indices_device``).

    ``params`` maps the eight parameter groups (``run_sensitivity_batch``'s ``fitted_params``).  ``vary=None`` is the reference's problem:
    every ``c_k`` plus ``E_i`` of every protein that acts as a TF -- read from the column indices of the engine's TF matrix, the one
    deviation: the engine keeps the matrix, not the edge table the reference looks the names up in.  ``vary`` also takes names
    (``"c_k_0"``, ``"E_i_3"``) or indices into the flat parameter vector.  Bounds are [v (1 - perturbation), v (1 + perturbation)] with no
    special case for zero values.  ``fused=True`` forms the fold changes inside the order-3 integrator (``simulate_measure_batch``;
    ``method`` / ``kernel`` defaults as ``run_sensitivity_batch(fused=True)``); a refused launch raises ``PhoskinError`` with the
    library's reason.  Tolerances default to ``measure_tolerances``, ``max_steps`` is 5000 T.  Rows with ``status != 0`` and non-finite
    entries become 0, as the reference's worker returns zeros.  ``seed=None`` draws one; the bootstrap uses
    ``sobol.resample_counts(n_samples, num_resamples, seed)`` (``num_resamples`` 0 or >= 2).  Single process: the rows are not sharded.

    Returns a dict: ``ST``, ``S1``, ``ST_conf``, ``S1_conf`` [T, N_prot, D] (only the rows ``proteins`` when given); ``heatmap`` =
    max(ST, 0) with NaN -> 0 (the reference's ``max(0, st_val)``; ST is NaN where a column is constant, as at the baseline time);
    ``names``, ``problem``, ``times``, ``param_values`` [n_samples (D + 2), D], ``status``, ``mean_steps``, ``seed``; with
    ``return_pred``: ``pred`` [rows, N_prot T] (GPU tensor, column p T + k, after the zeroing) and ``layout``."""
    p = {k: (np.asarray(params[k], float) if k != "tf_scale" else float(params[k])) for k in _ORDER}
    from .simulate import measure_tolerances
    tol = measure_tolerances(eng)
    rtol = tol["rtol"] if rtol is None else rtol
    atol = tol["atol"] if atol is None else atol
    names_all = compute_bounds(p, perturbation)["names"]
    center = eng.pack_params(*(p[k] for k in _ORDER))
    if vary is None:
        e0 = eng.n_K + 4 * eng.N + eng.total_sites                         # [c_k | A_i | B_i | C_i | D_i | Dp_i | E_i | tf_scale]
        vidx = np.concatenate([np.arange(eng.n_K), e0 + np.unique(eng._keep[7]).astype(np.int64)]).astype(np.int64)
    else:
        pos = {nm: i for i, nm in enumerate(names_all)}
        vidx = np.array([pos[v] if isinstance(v, str) else int(v) for v in vary], dtype=np.int64)
    if vidx.size == 0 or np.unique(vidx).size != vidx.size or vidx.min() < 0 or vidx.max() >= len(names_all):
        raise ValueError("vary must hold distinct indices (or names) of the flat parameter vector")
    v = center[vidx]
    problem = {"num_vars": int(vidx.size), "names": [names_all[i] for i in vidx],
               "bounds": [[float(x * (1 - perturbation)), float(x * (1 + perturbation))] for x in v]}
    times = np.asarray(time_grid, dtype=np.float64)
    if times.ndim != 1 or times.size < 1 or np.any(np.diff(times) <= 0):
        raise ValueError("time_grid must be strictly increasing")
    T, D = times.size, int(vidx.size)
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    counts = sobol.resample_counts(n_samples, num_resamples, seed) if num_resamples else None
    Xv, design = sobol.sample_device(problem, N=n_samples, seed=seed, device=eng.ctx.device)
    Xd = torch.as_tensor(center, device=Xv.device).repeat(Xv.shape[0], 1)  # scatter the varied columns into copies of the packed vector (in HBM)
    Xd[:, torch.as_tensor(vidx, device=Xv.device)] = Xv
    lists, ld = eng.make_index_lists(times, times, [], [])                  # protein fold changes only: column p T + k
    n_obs = ld["p_prot"].size
    try:
        if fused:
            out = eng.simulate_measure_batch(lists, Xd, times, y0=y0, rtol=rtol, atol=atol, max_steps=5000 * T, eps=1e-12, want_pred=True,
                                             method=("rosw" if method == "auto" else method), kernel=("lds" if kernel == "auto" else kernel))
            if out is None:
                from .. import _capi
                raise _capi.PhoskinError("temporal_gsa_batch(fused=True): the fused launch was refused: "
                                         + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode() + " -- or call with fused=False")
            _, pred, status, nst, _ = out
        else:
            Y, status, nst = eng.simulate_batch(Xd, times, y0=y0, rtol=rtol, atol=atol, max_steps=5000 * T, method=method, kernel=kernel)
            pred = eng.observables_batch(lists, Y, n_obs, eps=1e-12)
        pred = torch.where((status != 0)[:, None], torch.zeros_like(pred), pred)      # a failed simulation contributes a zero trajectory
        pred = torch.nan_to_num(pred, nan=0.0, posinf=0.0, neginf=0.0)
        idx = sobol.indices_device(design, pred, counts, conf_level)
        torch.cuda.current_stream().synchronize()
    finally:
        eng.free_loss(lists)
    sel = np.arange(eng.N) if proteins is None else np.asarray(proteins, dtype=np.int64)
    shape = lambda a: np.ascontiguousarray(a.cpu().numpy().reshape(D, eng.N, T).transpose(2, 1, 0)[:, sel, :])      # [D, p T + k] -> [T, N_prot, D]
    res = {k: shape(idx[k]) for k in ("ST", "S1", "ST_conf", "S1_conf")}
    res["heatmap"] = np.where(np.isnan(res["ST"]), 0.0, np.maximum(res["ST"], 0.0))
    res.update(names=problem["names"], problem=problem, times=times, param_values=Xv.cpu().numpy(), status=status.cpu().numpy(),
               mean_steps=[float(x) for x in nst.double().mean(dim=0).cpu()], seed=seed)
    if return_pred:
        res.update(pred=pred, layout=ld)
    return res


_METRICS = ("total_signal", "mean", "variance", "l2_norm")


def observable_weights(eng: NetworkEngine, ld: dict) -> np.ndarray:
    """W [n_obs, S] with pred's numerator = W @ Y[t] and baseline = W @ Y[base], rows in (protein | rna | phospho) order of the index
    lists ``ld`` (``make_index_lists``): the total protein (P plus all sites / all 2^ns states), the mRNA row, a site's row (combinatorial
    topology: all masks with the site's bit)."""
    oy, ns, comb = eng._keep[0], eng._keep[2], eng.model == 2
    n_obs = ld["p_prot"].size + ld["p_rna"].size + ld["p_pho"].size
    W = np.zeros((n_obs, eng.S))
    r = 0
    for i in ld["p_prot"]:
        cnt = (1 << int(ns[i])) if comb else 1 + int(ns[i])
        W[r, oy[i] + 1: oy[i] + 1 + cnt] = 1.0; r += 1
    for i in ld["p_rna"]:
        W[r, oy[i]] = 1.0; r += 1
    for i, j in zip(ld["p_pho"], ld["s_pho"]):
        if comb:
            m = np.arange(1 << int(ns[i]))
            W[r, oy[i] + 1 + m[(m >> int(j)) & 1 == 1]] = 1.0
        else:
            W[r, oy[i] + 2 + int(j)] = 1.0
        r += 1
    return W


def fold_change_derivatives(W: np.ndarray, ld: dict, Y: np.ndarray, dY: np.ndarray, eps: float = 1e-12):
    """(pred [n_obs], dpred [n_obs, K]) of one trajectory Y [T, S] with tangents dY [T, S, K]: pred = max(a, eps) / max(c, eps) with
    numerator a at the entry's time and baseline c at its modality's baseline index, differentiated through both; a floor that is active
    has derivative 0."""
    t_idx = np.concatenate([ld["t_prot"], ld["t_rna"], ld["t_pho"]]).astype(np.int64)
    b_idx = np.concatenate([np.full(ld["p_prot"].size, int(ld["prot_base_idx"])), np.full(ld["p_rna"].size, int(ld["rna_base_idx"])),
                            np.full(ld["p_pho"].size, int(ld["pho_base_idx"]))]).astype(np.int64)
    a = np.einsum("os,os->o", W, Y[t_idx]); c = np.einsum("os,os->o", W, Y[b_idx])
    da = np.einsum("os,osk->ok", W, dY[t_idx]); dc = np.einsum("os,osk->ok", W, dY[b_idx])
    am, cm = np.maximum(a, eps), np.maximum(c, eps)
    da = np.where((a > eps)[:, None], da, 0.0); dc = np.where((c > eps)[:, None], dc, 0.0)
    return am / cm, da / cm[:, None] - (am / (cm * cm))[:, None] * dc


def metric_derivatives(pred: np.ndarray, dpred: np.ndarray) -> Dict:
    """{metric: (value, gradient [K])} of the four ``_compute_scalar_metric`` outputs over pred [n_obs] with d pred [n_obs, K]: sum;
    sum / n; (2 / n) sum (p - mean) dp; sum p dp / |p| (0 where |p| = 0).  Empty lists give 0."""
    n, K = pred.size, dpred.shape[1]
    if n == 0:
        return {m: (0.0, np.zeros(K)) for m in _METRICS}
    mu, nrm = float(np.mean(pred)), float(np.linalg.norm(pred))
    return {"total_signal": (float(np.sum(pred)), dpred.sum(axis=0)), "mean": (mu, dpred.sum(axis=0) / n),
            "variance": (float(np.var(pred)), (2.0 / n) * ((pred - mu) @ dpred)),
            "l2_norm": (nrm, (pred @ dpred) / nrm if nrm > 0.0 else np.zeros(K))}


def local_sensitivity_batch(eng: NetworkEngine, params: Dict, t_prot, t_rna, t_pho, vary=None, metric: str = config.SENSITIVITY_METRIC,
                            perturbation: float = config.SENSITIVITY_PERTURBATION, y0=None, rtol: Optional[float] = None,
                            atol: Optional[float] = None, eps: float = 1e-12, max_steps: int = 1000000) -> Dict:
    """Local sensitivities of the network's fold-change observables and of the Morris output at ``params`` (the eight parameter groups,
    as ``run_sensitivity_batch`` takes them) from ONE ``simulate_sens_batch`` launch -- exact tangents of the discrete solution, where
    differencing ``simulate_batch`` takes two solves per entry and loses accuracy at the tolerances in use.  The network twin of
    ``sensitivity.analysis.local_sensitivity_batch``.  ``vary``: names (``"c_k_0"``, ``"A_i_1"``, ``"tf_scale"``, as ``compute_bounds``
    names them) or indices into the flat parameter vector; None = every entry -- but this is a tool for a chosen handful of entries: a
    launch costs about (1 + KC) / KC state integrations per column (KC = ``eng.sens_columns_per_launch()``; on networks beyond one
    workgroup's LDS the launch runs on HBM slabs by itself, KC = ``eng.sens_hbm_columns(K)``), a full gradient needs an adjoint.
    Returns a dict with

      names       the K varied entries
      layout      the index lists (``make_index_lists``) pred's rows follow, times the union grid
      pred        [n_obs]     fold-change observables (protein | rna | phospho), floors ``eps``
      dpred       [n_obs, K]  their derivatives through numerator and baseline (0 through an active floor)
      Y, dY       the scalar metric ``metric`` and d Y / d x [K]; ``metrics``: {name: (Y, dY)} for all four
      elasticity  [K]  x_c dY_c / Y, 0 where Y == 0
      scaled      [K]  dY_c (ub_c - lb_c) with the bounds of ``compute_bounds(params, perturbation)``
      status      [1]  the solver's flags (OR over the column chunks); a flagged run has NaN entries

    The chain from dY [T, S, K] to dpred and the metrics is host arithmetic."""
    if metric not in _METRICS:
        raise ValueError(f"metric must be one of {_METRICS}")
    p = {k: (np.asarray(params[k], float) if k != "tf_scale" else float(params[k])) for k in _ORDER}
    problem = compute_bounds(p, perturbation)
    names = problem["names"]
    if vary is None:
        vidx = np.arange(len(names), dtype=np.int64)
    else:
        pos = {nm: i for i, nm in enumerate(names)}
        vidx = np.array([pos[v] if isinstance(v, str) else int(v) for v in vary], dtype=np.int64)
        if vidx.size == 0 or np.unique(vidx).size != vidx.size or vidx.min() < 0 or vidx.max() >= len(names):
            raise ValueError("vary must hold distinct indices (or names) of the flat parameter vector")
    x = eng.pack_params(*(p[k] for k in _ORDER))
    times = np.unique(np.concatenate([t_prot, t_rna, t_pho]).astype(np.float64))
    lists, ld = eng.make_index_lists(times, t_prot, t_rna, t_pho)
    eng.free_loss(lists)
    out = eng.simulate_sens_batch(x, times, vidx.astype(np.int32), y0=y0, rtol=rtol, atol=atol, max_steps=max_steps)
    if out is None:
        from .. import _capi
        raise _capi.PhoskinError("local_sensitivity_batch: the sensitivity launch was refused: "
                                 + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode())
    dYt, Yt, status, _ = out
    Yh, dYh = Yt[0].cpu().numpy(), dYt[0].cpu().numpy()
    pred, dpred = fold_change_derivatives(observable_weights(eng, ld), ld, Yh, dYh, eps)
    mets = metric_derivatives(pred, dpred)
    val, grad = mets[metric]
    xv = x[vidx]
    width = np.array([problem["bounds"][i][1] - problem["bounds"][i][0] for i in vidx])
    elasticity = np.zeros_like(grad) if val == 0.0 else xv * grad / val
    return {"names": [names[i] for i in vidx], "layout": ld, "times": times, "pred": pred, "dpred": dpred, "Y": val, "dY": grad,
            "metrics": mets, "elasticity": elasticity, "scaled": grad * width, "status": status.cpu().numpy()}


def _worker_simulation(task_args):
    """``(idx, param_vector, names_map, original_shapes, sys, idx_sys, times_p, times_r, times_ph, metric) -> (idx, y, dfp, dfr, dfph)``:
    the reference's pool worker (sensitivity.py:143-168), one simulation.  ``run_sensitivity_analysis`` does not use it: all samples are
    one launch and no ``System`` is pickled."""
    from .simulate import simulate_and_measure
    (i, param_vector, names_map, original_shapes, sys, idx_sys, times_p, times_r, times_ph, metric) = task_args
    sys.update(**_reconstruct_params(param_vector, names_map, original_shapes))
    dfp, dfr, dfph = simulate_and_measure(sys, idx_sys, times_p, times_r, times_ph)
    return i, _compute_scalar_metric(dfp, dfr, dfph, metric), dfp, dfr, dfph


def run_sensitivity_analysis(sys, idx, fitted_params, output_dir, metric="total_signal", seed: Optional[int] = None,
                             param_values: Optional[np.ndarray] = None, fused: bool = False):
    """Morris screening of the network around ``fitted_params`` with the reference's argument list (sensitivity.py:171-297) -> the
    DataFrame ``Parameter, mu_star, sigma, mu_star_conf`` sorted by influence, also written to ``<output_dir>/sensitivity_indices.csv``.

    N = ``config.SENSITIVITY_TRAJECTORIES`` trajectories on ``config.SENSITIVITY_LEVELS`` levels within +-``config.SENSITIVITY_PERTURBATION``
    of every entry; the N (D + 1) simulations are ONE launch on the engine of ``sys`` (the reference pickles the whole System into every
    task of a process pool); under an initialised ``torch.distributed`` group the rows are sharded over the ranks with one all-gather of Y.
    ``<output_dir>/sensitivity_trajectories.csv`` lists the ``config.SENSITIVITY_TOP_CURVES`` samples of largest Y (id, y_val and the
    sampled parameter values; the reference stores whole DataFrames in that table's cells).  The two plots (:290-296) are not drawn.
    ``seed`` defaults to ``config.SEED``; ``param_values`` (keyword, not in the reference) takes a ready sample matrix such as SALib's;
    ``fused`` (keyword, not in the reference) is ``run_sensitivity_batch``'s: measure and reduce inside the integrator."""
    import os
    import pandas as pd
    from .simulate import engine_for
    eng = engine_for(sys)
    params = {}
    for k in _ORDER:
        v = fitted_params[k]
        params[k] = float(v) if k == "tf_scale" else np.asarray(v, dtype=float)
    res = run_sensitivity_batch(eng, params, config.TIME_POINTS_PROTEIN, config.TIME_POINTS_RNA, config.TIME_POINTS_PHOSPHO, metric=metric,
                                perturbation=config.SENSITIVITY_PERTURBATION, trajectories=config.SENSITIVITY_TRAJECTORIES,
                                num_levels=config.SENSITIVITY_LEVELS, seed=config.SEED if seed is None else seed, param_values=param_values, y0=np.asarray(sys.y0(), dtype=np.float64),
                                fused=fused)
    Si = res["Si"]
    df_sens = pd.DataFrame({"Parameter": res["problem"]["names"], "mu_star": Si["mu_star"], "sigma": Si["sigma"], "mu_star_conf": Si["mu_star_conf"]})
    df_sens = df_sens.sort_values("mu_star", ascending=False)
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        df_sens.to_csv(os.path.join(output_dir, "sensitivity_indices.csv"), index=False)
        top = np.argsort(-res["Y"], kind="stable")[:config.SENSITIVITY_TOP_CURVES]
        traj = pd.DataFrame(res["param_values"][top], columns=res["problem"]["names"])
        traj.insert(0, "y_val", res["Y"][top]); traj.insert(0, "id", top)
        traj.to_csv(os.path.join(output_dir, "sensitivity_trajectories.csv"), index=False)
    return df_sens
