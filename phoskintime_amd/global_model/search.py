"""Device-resident reference-direction population search for the network calibration -- the loop of the reference's
``run_global_calibration`` (global_model/runner.py:663-699: pymoo's ``UNSGA3(pop_size, ref_dirs=das-dennis(3, 20), sampling=LHS(),
crossover=SBX(0.9, 15), mutation=PM(1 / n_var, 10))`` under ``minimize``) without pymoo and without a host round trip.

One generation is: mate (``pk_moo_mate_batch``: tournament, bounded SBX, bounded PM) -> ``problem.evaluate_device`` on the offspring ->
parents and offspring concatenated in HBM -> ideal / nadir (torch reductions) -> non-dominated ranks (``pk_moo_rank_batch`` with
``stop_at = pop``) -> association with the reference directions (``pk_moo_associate_batch``) -> niching survival
(``pk_moo_survive_batch``) -> gather.  X and F never leave the device inside the loop; per generation the host sees the 4 bytes per
front the ranking reads and, after the generation's launches are queued, ``ideal`` and the size of front 0 for ``history``.

Stated deviations from pymoo's UNSGA3:
  * no duplicate elimination;
  * a fixed generation count (or a ``callback`` returning True) instead of ``DefaultMultiObjectiveTermination``;
  * deterministic tie-breaks where pymoo draws (niche choice: lowest index; within a niche: smallest distance, lowest index; the
    tournament's fall-through: the first contestant), and counter-based random numbers (include/phoskin.h), so a run is a function of
    ``seed`` alone;
  * the nadir point is the column maximum over front 0, and, in a column where that leaves ``nadir - ideal < 1e-6``, the column maximum
    over all finite rows -- the fallback of pymoo's hyperplane through the extreme points, used always;
  * one process: a sharded search is not part of this.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import torch


def das_dennis(M: int, p: int) -> np.ndarray:
    """The simplex lattice {k / p : k in N^M, sum k = p} as [C(p + M - 1, M - 1), M] float64, in lexicographic order of the integer
    vectors k (k_0 ascending, then k_1, ...; the last entry is what remains): 91 rows at (3, 12), 231 at (3, 20).  Row 0 is the last
    axis, the last row the first axis."""
    M, p = int(M), int(p)
    if M < 1 or p < 1:
        raise ValueError("M and p must be >= 1")
    rows: List[List[int]] = []

    def rec(prefix, left):
        if len(prefix) == M - 1:
            rows.append(prefix + [left])
            return
        for k in range(left + 1):
            rec(prefix + [k], left - k)

    rec([], p)
    return np.asarray(rows, dtype=np.float64) / float(p)


def lhs(P: int, n_var: int, xl, xu, seed: int, device=None) -> torch.Tensor:
    """Latin hypercube [P, n_var] on the device: in every column each of the P strata [k / P, (k + 1) / P) holds exactly one point (a
    random permutation of the strata plus a uniform offset inside the stratum), scaled to [xl, xu].  A function of ``seed`` alone."""
    dev = torch.device("cuda" if device is None else device)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    perm = torch.argsort(torch.rand((P, n_var), generator=g, device=dev, dtype=torch.float64), dim=0).to(torch.float64)
    u = (perm + torch.rand((P, n_var), generator=g, device=dev, dtype=torch.float64)) / float(P)
    lo = torch.as_tensor(np.asarray(xl, dtype=np.float64), device=dev)
    hi = torch.as_tensor(np.asarray(xu, dtype=np.float64), device=dev)
    return torch.minimum(torch.maximum(lo + u * (hi - lo), lo), hi)


@dataclass
class SearchResult:
    X: torch.Tensor                # [pop, n_var] raw candidates (device)
    F: torch.Tensor                # [pop, 3] their objectives, as evaluate_device returned them (device)
    rank: torch.Tensor             # [pop] int32 non-dominated rank within the last merged population (device)
    niche: torch.Tensor            # [pop] int32 reference direction, -1 for a non-finite row (device)
    history: List[dict] = field(default_factory=list)       # per generation: {"gen", "ideal" [3] numpy, "front0", "fronts" peeled}
    dist: Optional[torch.Tensor] = None                      # [pop] distance to the niche's direction (device)
    ref_dirs: Optional[np.ndarray] = None


class _Kernels:
    """The four pk_moo_* calls on torch tensors of one device, on torch's current stream."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.dev = torch.device("cuda", ctx.device)

    def _go(self):
        self.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)

    def rank(self, F, stop_at=0):
        P, M = F.shape
        rank = torch.empty(P, dtype=torch.int32, device=self.dev)
        nf = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._go()
        self.ctx.check(self.ctx.lib.pk_moo_rank_batch(self.ctx.handle, P, M, F.data_ptr(), int(stop_at), rank.data_ptr(), nf.data_ptr()))
        return rank, nf

    def associate(self, F, ideal, nadir, dirs):
        P, M = F.shape
        niche = torch.empty(P, dtype=torch.int32, device=self.dev)
        dist = torch.empty(P, dtype=torch.float64, device=self.dev)
        self._go()
        self.ctx.check(self.ctx.lib.pk_moo_associate_batch(self.ctx.handle, P, M, F.data_ptr(), ideal.data_ptr(), nadir.data_ptr(), dirs.shape[0],
                                                           dirs.data_ptr(), niche.data_ptr(), dist.data_ptr()))
        return niche, dist

    def survive(self, rank, niche, dist, H, K):
        keep = torch.empty(K, dtype=torch.int32, device=self.dev)
        self._go()
        self.ctx.check(self.ctx.lib.pk_moo_survive_batch(self.ctx.handle, rank.shape[0], int(K), rank.data_ptr(), niche.data_ptr(), dist.data_ptr(),
                                                         int(H), keep.data_ptr() if K else None))
        return keep

    def mate(self, X, rank, niche, dist, xl, xu, seed, gen, pc, eta_c, pm, eta_m, want_parents=False):
        P, n_var = X.shape
        Xc = torch.empty_like(X)
        par = torch.empty(P, dtype=torch.int32, device=self.dev) if want_parents else None
        self._go()
        self.ctx.check(self.ctx.lib.pk_moo_mate_batch(self.ctx.handle, P, n_var, X.data_ptr(), rank.data_ptr(), niche.data_ptr(), dist.data_ptr(),
                                                      xl.data_ptr(), xu.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(gen), float(pc), float(eta_c),
                                                      float(pm), float(eta_m), Xc.data_ptr(), par.data_ptr() if par is not None else None))
        return (Xc, par) if want_parents else Xc


def kernels(ctx) -> _Kernels:
    """The four device calls as methods on torch tensors (``rank``, ``associate``, ``survive``, ``mate``) for a ``_capi.Context``: the
    array-level layer under ``search``, as ``NetworkEngine.fit_batch`` is under ``polish``."""
    return _Kernels(ctx)


def _rank_associate(k: _Kernels, F, ideal, dirs, pop, tick):
    """Ranks and niches of the rows of F; ``ideal`` is updated to min(ideal, column minima over finite rows).  Returns
    (ideal, rank, n_fronts [1], niche, dist)."""
    fin = torch.isfinite(F).all(dim=1, keepdim=True)
    inf = torch.full_like(F, float("inf"))
    ideal = torch.minimum(ideal, torch.where(fin, F, inf).min(dim=0).values)
    tick("torch")
    rank, nf = k.rank(F, stop_at=pop)
    tick("rank")
    top = torch.where(fin & (rank == 0)[:, None], F, -inf).max(dim=0).values
    every = torch.where(fin, F, -inf).max(dim=0).values
    nadir = torch.where(top - ideal < 1e-6, every, top)
    # a population without one finite row has no ideal or nadir point: the kernel marks every row niche -1 whatever these hold
    ideal_k = torch.where(torch.isfinite(ideal), ideal, torch.zeros_like(ideal)).contiguous()
    nadir_k = torch.where(torch.isfinite(nadir), nadir, torch.ones_like(nadir)).contiguous()
    tick("torch")
    niche, dist = k.associate(F, ideal_k, nadir_k, dirs)
    tick("associate")
    return ideal, rank, nf, niche, dist


def search(problem, pop: int, n_gen: int, seed: int, ref_partitions: int = 20, pc: float = 0.9, eta_c: float = 15.0, pm: Optional[float] = None,
           eta_m: float = 10.0, callback: Optional[Callable] = None, X0=None, timer: Optional[Callable] = None) -> SearchResult:
    """Minimise the problem's three objectives with ``pop`` candidates over ``n_gen`` generations from a Latin hypercube inside the
    problem's bounds (or from ``X0`` [pop, n_var], raw).  ``pm`` None = 1 / n_var.  ``callback(gen, state)`` is called after every
    generation (gen = 0: the evaluated start) with ``state`` = dict(X, F, rank, niche, dist, ideal) of device tensors and may return True
    to stop.  Returns the last population; its ``F`` is what ``problem.evaluate_device`` returned for its ``X``.  Beyond the five fields
    the loop is defined by, the result carries ``dist`` (each row's distance to its direction, what the next tournament would use) and
    ``ref_dirs`` (the lattice, so that ``niche`` can be read); ``history`` holds {gen, ideal, front0, fronts} per generation.

    ``timer(phase)``, for measurements (tools/moo_generation_split.py): called on the host with "start" when a generation begins and
    with "mate", "evaluate", "rank", "associate", "survive" or "torch" (concatenation, reductions, gather) when the launches of that
    phase have been queued; record a device event there.  It changes nothing else."""
    tick = timer if timer is not None else (lambda phase: None)
    if getattr(problem, "xl", None) is None or getattr(problem, "xu", None) is None:
        raise ValueError("search needs the problem's bounds xl / xu")
    pop, n_gen, n_var = int(pop), int(n_gen), int(problem.n_var)
    if pop < 1 or n_gen < 0:
        raise ValueError("pop must be >= 1 and n_gen >= 0")
    xl_h = np.broadcast_to(np.asarray(problem.xl, dtype=np.float64), (n_var,)).copy()
    xu_h = np.broadcast_to(np.asarray(problem.xu, dtype=np.float64), (n_var,)).copy()
    if not (xu_h >= xl_h).all():
        raise ValueError("xu must be >= xl")
    k = _Kernels(problem.eng.ctx)
    dev = k.dev
    xl, xu = torch.as_tensor(xl_h, device=dev), torch.as_tensor(xu_h, device=dev)
    ref = das_dennis(problem.n_obj, ref_partitions)
    dirs = torch.as_tensor(ref, device=dev).contiguous()
    pm = 1.0 / n_var if pm is None else float(pm)
    if X0 is None:
        X = lhs(pop, n_var, xl_h, xu_h, seed, dev)
    else:
        X = (X0 if isinstance(X0, torch.Tensor) else torch.as_tensor(np.asarray(X0, dtype=np.float64))).to(device=dev, dtype=torch.float64)
        if tuple(X.shape) != (pop, n_var):
            raise ValueError("X0 must be [pop, n_var]")
    X = X.contiguous().clone()
    F = problem.evaluate_device(X).contiguous()
    ideal = torch.full((F.shape[1],), float("inf"), dtype=torch.float64, device=dev)
    ideal, rank, nf, niche, dist = _rank_associate(k, F, ideal, dirs, pop, tick)      # the start: nothing to discard yet
    history: List[dict] = []

    def record(gen):
        history.append(dict(gen=gen, ideal=ideal.cpu().numpy(), front0=int((rank == 0).sum().item()), fronts=int(nf.item())))
        return bool(callback(gen, dict(X=X, F=F, rank=rank, niche=niche, dist=dist, ideal=ideal))) if callback is not None else False

    stop = record(0)
    for gen in range(1, n_gen + 1):
        if stop:
            break
        tick("start")
        Xc = k.mate(X, rank, niche, dist, xl, xu, seed, gen, pc, eta_c, pm, eta_m)
        tick("mate")
        Fc = problem.evaluate_device(Xc)
        tick("evaluate")
        Xa, Fa = torch.cat([X, Xc], dim=0), torch.cat([F, Fc], dim=0).contiguous()
        ideal, ra, nf, na, da = _rank_associate(k, Fa, ideal, dirs, pop, tick)
        keep = k.survive(ra, na, da, dirs.shape[0], pop)
        tick("survive")
        keep = keep.long()
        X, F = Xa[keep].contiguous(), Fa[keep].contiguous()
        rank, niche, dist = ra[keep].contiguous(), na[keep].contiguous(), da[keep].contiguous()
        tick("torch")
        stop = record(gen)
    return SearchResult(X=X, F=F, rank=rank, niche=niche, history=history, dist=dist, ref_dirs=ref)
