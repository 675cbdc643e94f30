"""Variance-based (Sobol') sensitivity: Saltelli design and first-order / total index estimator with its bootstrap (host side, numpy),
the twin of ``morris.py``.

The reference delegates both to SALib (``saltelli.sample`` / ``sobol.analyze`` with ``calc_second_order=False``,
scripts/temporal_sensitivity.py:169,185), a third-party package that is absent from this image.  Parity for this row is therefore
"same X in => same indices out": ``analyze`` takes the outputs of any Saltelli sample matrix (SALib's included) and is pinned by
known-answer tests (tests/test_sobol_cpu.py); ``build`` lays the rows out as SALib does, ``draw`` takes the base samples from SciPy's
scrambled Sobol' sequence."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np


@dataclass
class Draws:
    """The random part of a Saltelli design: the two base samples on the unit cube."""
    A: np.ndarray          # [N, D]
    B: np.ndarray          # [N, D]


def draw(D: int, N: int, seed: Optional[int] = None) -> Draws:
    """Columns [:D] and [D:] of N points of ``scipy.stats.qmc.Sobol(d=2 D, scramble=True, seed=seed)`` (``random_base2`` when N is a
    power of two, ``random(N)`` otherwise).  SALib's own stream -- the unscrambled sequence after its skip values -- is NOT reproduced:
    feed SALib's matrix to the solver and its outputs to ``analyze`` where that stream matters."""
    from scipy.stats import qmc
    D, N = int(D), int(N)
    if D < 1 or N < 1:
        raise ValueError("D and N must be >= 1")
    eng = qmc.Sobol(d=2 * D, scramble=True, seed=seed)
    if N & (N - 1) == 0:
        u = eng.random_base2(N.bit_length() - 1)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)      # "balance properties require n to be a power of 2": the caller chose N
            u = eng.random(N)
    return Draws(A=np.ascontiguousarray(u[:, :D]), B=np.ascontiguousarray(u[:, D:]))


def build(draws: Draws, bounds) -> np.ndarray:
    """Sample matrix [N (D + 2), D] in the row order of ``saltelli.sample(..., calc_second_order=False)``: for each i the row A_i, then
    AB_i1 .. AB_iD (A_i with column j taken from B_i), then B_i; scaled as lb + u (ub - lb)."""
    A, B = np.asarray(draws.A, float), np.asarray(draws.B, float)
    N, D = A.shape
    U = np.repeat(A[:, None, :], D + 2, axis=1)
    j = np.arange(D)
    U[:, j + 1, j] = B[:, j]
    U[:, D + 1, :] = B
    b = np.asarray(bounds, dtype=float).reshape(D, 2)
    return (b[:, 0] + U * (b[:, 1] - b[:, 0])).reshape(N * (D + 2), D)


def sample(problem: Dict, N: int, seed: Optional[int] = None) -> np.ndarray:
    """N base points -> [N (D + 2), D], scaled to ``problem['bounds']``."""
    return build(draw(int(problem["num_vars"]), N, seed), problem["bounds"])


def resample_counts(N: int, R: int, seed: Optional[int] = None) -> np.ndarray:
    """int32 [R, N]: how often bootstrap resample r draws base point i -- the row-wise bincount of
    ``default_rng(seed).integers(0, N, (R, N))``, the index matrix SALib's analyser draws."""
    idx = np.random.default_rng(seed).integers(0, N, size=(int(R), int(N)))
    return np.stack([np.bincount(row, minlength=N) for row in idx]).astype(np.int32) if R > 0 else np.zeros((0, N), np.int32)


def analyze(Y, D: int, counts=None, conf_level: float = 0.95) -> Dict:
    """S1, ST, S1_conf, ST_conf [D, M] and var [M] of the outputs Y [N (D + 2), M] of a Saltelli design (a 1-D Y is one column; the
    results then lose the M axis): ``SALib.analyze.sobol.analyze(calc_second_order=False)`` column by column.

        A = Y[0::D+2], B = Y[D+1::D+2], AB_j = Y[j+1::D+2], each column centred by its mean over all rows
        S1_j = mean(B (AB_j - A)) / var([A; B])          ST_j = mean((A - AB_j)^2) / 2 / var([A; B])          (population variance)

    SALib also divides the centred column by its standard deviation; both indices are invariant under scaling, so that division is
    dropped.  ``counts`` [R, N] (``resample_counts``): resample r is the same formulas with weights counts[r, i] / N, its own variance
    included -- exactly what gathering A[idx], AB[idx], B[idx] gives -- and ``*_conf`` = norm.ppf(0.5 + conf_level / 2) x the ddof-1 standard
    deviation over the resamples.  R must be 0 (``counts=None``; the ``*_conf`` are then NaN) or >= 2.  A column whose maximum equals its
    minimum over all rows gives NaN in every output (SALib: through std = 0; a fold change at the baseline time is exactly 1).  The
    arithmetic runs in Y's own precision when Y is ``np.longdouble`` (the tests' reference), in float64 otherwise."""
    Y = np.asarray(Y)
    dt = np.longdouble if Y.dtype == np.longdouble else np.float64
    Y = Y.astype(dt, copy=False)
    one = Y.ndim == 1
    Y2 = Y.reshape(Y.shape[0], -1)
    D = int(D)
    if D < 1 or Y2.shape[0] < D + 2 or Y2.shape[0] % (D + 2):
        raise ValueError("Y must hold N (D + 2) rows")
    N, M = Y2.shape[0] // (D + 2), Y2.shape[1]
    R = 0
    if counts is not None:
        counts = np.asarray(counts)
        R = counts.shape[0]
        if counts.ndim != 2 or counts.shape[1] != N:
            raise ValueError("counts must be [R, N]")
    if R == 1:
        raise ValueError("R must be 0 or >= 2")
    const = (Y2.max(axis=0) == Y2.min(axis=0)) if M else np.zeros(0, bool)
    # centred as (y - y[0]) - mean(y - y[0]), as the kernel does: no rounding at the size of a column's offset, which may dwarf its spread
    Yr = Y2 - Y2[0]
    Yr = (Yr - Yr.mean(axis=0)).reshape(N, D + 2, M)
    A, B, AB = Yr[:, 0], Yr[:, D + 1], Yr[:, 1:D + 1]                      # [N, M], [N, M], [N, D, M]
    P1 = B[:, None, :] * (AB - A[:, None, :])
    PT = (A[:, None, :] - AB) ** 2
    nan = np.asarray(np.nan, dtype=dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where(const, nan, np.var(np.concatenate([A, B], axis=0), axis=0))
        S1 = P1.mean(axis=0) / var
        ST = PT.mean(axis=0) / 2 / var
        S1c = np.full((D, M), nan); STc = np.full((D, M), nan)
        if R:
            w = counts.astype(dt) / N                                        # [R, N]
            S1r = np.empty((R, D, M), dtype=dt); STr = np.empty((R, D, M), dtype=dt)
            for r in range(R):
                mu = (w[r] @ (A + B)) / 2
                vr = np.where(const, nan, (w[r] @ ((A - mu) ** 2 + (B - mu) ** 2)) / 2)
                S1r[r] = np.tensordot(w[r], P1, axes=(0, 0)) / vr
                STr[r] = np.tensordot(w[r], PT, axes=(0, 0)) / 2 / vr
            from scipy.stats import norm
            z = dt(norm.ppf(0.5 + conf_level / 2.0))
            S1c = z * S1r.std(axis=0, ddof=1); STc = z * STr.std(axis=0, ddof=1)
    out = {"S1": S1, "ST": ST, "S1_conf": S1c, "ST_conf": STc, "var": var}
    return {k: v[..., 0] for k, v in out.items()} if one else out


def sample_device(problem: Dict, N: int, seed: Optional[int] = None, device: Optional[int] = None):
    """The same design built in HBM (``pk_sobol_build_batch``): only the two base samples cross PCIe.  Returns (X [N (D+2), D] GPU tensor,
    handle for ``indices_device``).  Bit-identical to ``sample`` with the same seed."""
    import torch
    from .. import batch
    ctx = batch.get_context(device)
    dev = torch.device("cuda", ctx.device)
    D = int(problem["num_vars"])
    d = draw(D, N, seed)
    b = np.asarray(problem["bounds"], dtype=float).reshape(D, 2)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    h = dict(draws=d, A=t(d.A), B=t(d.B), lb=t(b[:, 0]), ub=t(b[:, 1]), ctx=ctx, N=int(N), D=D)
    X = torch.empty((N * (D + 2), D), dtype=torch.float64, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ctx.check(ctx.lib.pk_sobol_build_batch(ctx.handle, N, D, h["A"].data_ptr(), h["B"].data_ptr(), h["lb"].data_ptr(), h["ub"].data_ptr(),
                                           X.data_ptr()))
    return X, h


def indices_device(h: dict, Y, counts=None, conf_level: float = 0.95) -> Dict:
    """``analyze`` on the GPU (``pk_sobol_indices_batch``) for a design made by ``sample_device``: Y [N (D + 2), M] or [N (D + 2)] (GPU
    tensor) -> dict of GPU tensors S1, ST, S1_conf, ST_conf [D, M] and var [M] (without the M axis for a 1-D Y).  ``counts`` [R, N] int32
    (``resample_counts``; array or tensor), None = no bootstrap: the ``*_conf`` are then NaN."""
    import torch
    ctx, N, D = h["ctx"], h["N"], h["D"]
    one = Y.dim() == 1
    Y = Y.to(dtype=torch.float64).reshape(Y.shape[0], -1).contiguous()
    if Y.shape[0] != N * (D + 2):
        raise ValueError("Y must hold one row per row of the design")
    M = Y.shape[1]
    R = 0
    cd = None
    if counts is not None:
        cd = (counts if isinstance(counts, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(counts, dtype=np.int32)))
        cd = cd.to(device=Y.device, dtype=torch.int32).contiguous()
        if cd.dim() != 2 or cd.shape[1] != N:
            raise ValueError("counts must be [R, N]")
        R = cd.shape[0]
    if R == 1:
        raise ValueError("R must be 0 or >= 2")
    new = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=Y.device)
    S1, ST, S1_sd, ST_sd, var = new(D, M), new(D, M), new(D, M), new(D, M), new(M)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    ctx.set_stream(torch.cuda.current_stream(Y.device).cuda_stream)
    ctx.check(ctx.lib.pk_sobol_indices_batch(ctx.handle, N, D, M, p(Y), p(cd) if R else None, R, p(S1), p(ST), p(S1_sd), p(ST_sd), p(var)))
    from scipy.stats import norm
    z = float(norm.ppf(0.5 + conf_level / 2.0))
    out = {"S1": S1, "ST": ST, "S1_conf": z * S1_sd, "ST_conf": z * ST_sd, "var": var}
    if one:
        out = {k: v[..., 0] for k, v in out.items()}
    out["S1"]._keepalive = (Y, cd)  # type: ignore[attr-defined]
    return out
