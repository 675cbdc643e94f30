"""GPU: the four ``pk_moo_*`` kernels (csrc/pk_moo.hip) against the numpy twin tests/moo_reference.py, and the generation loop
``GlobalODEBatch.search`` (global_model/search.py) on the smallest network fixture.

Bounds.  Ranks, niches, survivors and tournament winners are integers: equality.  Association distances: 1e-12 (1 + dist) -- a 3-term
norm in doubles is good to a few 2^-53 of its terms, four orders below that; a wrong formula errs at O(1); the twin's best and
second-best distances of every row are first shown to differ by > 1e-9, so the integer comparison cannot hinge on rounding.  Offspring:
1e-12 (xu - xl) -- the kernel and the twin follow the same branches on the same random numbers and differ by ``pow`` rounding only."""
import numpy as np
import pytest

import moo_reference as mr

pytestmark = pytest.mark.gpu
_K = {}


def _k():
    if "k" not in _K:
        from phoskintime_amd import batch
        from phoskintime_amd.global_model import search
        _K["k"] = search.kernels(batch.get_context(None))
    return _K["k"]


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=_k().dev)


def _rank(F, stop_at=0):
    import torch
    r, nf = _k().rank(_t(F, torch.float64), stop_at)
    return r.cpu().numpy(), int(nf.item())


def _random_F():
    return np.random.default_rng(101).random((1000, 3))


# ---------------------------------------------------------------- rank

def _rank_cases():
    rng = np.random.default_rng(3)
    chain = (np.arange(7.0)[::-1, None] * np.ones((1, 3)))[[3, 0, 6, 2, 5, 1, 4]]
    dup = rng.integers(0, 3, (12, 3)).astype(float)
    dup = np.concatenate([dup, dup[:6], dup[:3]])
    bad = rng.integers(0, 4, (70, 3)).astype(float)
    bad[5] = np.nan; bad[17, 1] = np.inf; bad[18, 0] = -np.inf; bad[30] = 1e12; bad[44, 2] = 1e12; bad[69] = np.nan
    return {"one": np.array([[0.3, 0.1, 0.2]]), "chain7": chain, "duplicates": dup,
            "integer300": rng.integers(0, 5, (300, 3)).astype(float), "random1000": _random_F(),
            "m2": rng.random((130, 2)), "m4": rng.random((130, 4)), "nonfinite": bad}


@pytest.mark.parametrize("name", ["one", "chain7", "duplicates", "integer300", "random1000", "m2", "m4", "nonfinite"])
def test_rank_equals_the_twin(name):
    F = _rank_cases()[name]
    want, nf = mr.rank_peel(F)
    got, gnf = _rank(F)
    print(name, "fronts", nf, gnf)
    assert np.array_equal(got, want) and gnf == nf
    if name == "chain7":
        assert nf == 7
    if name == "nonfinite":
        assert (want[~np.isfinite(F).all(axis=1)] == nf - 1).all()


def test_rank_stop_at():
    F = _random_F()
    full, _ = mr.rank_peel(F)
    want, nf = mr.rank_peel(F, stop_at=40)
    got, gnf = _rank(F, stop_at=40)
    assert gnf == nf and np.array_equal(got, want)
    assert np.array_equal(got[got < nf], full[got < nf]) and (full[got == nf] >= nf).all() and (got < nf).sum() >= 40
    assert (full < nf - 1).sum() < 40                       # the front before the last one had not reached stop_at


def _big_rank_case(P):
    """More than one LDS tile in every slice of the scan (P > 4096; P = 5000 is no multiple of the tile): random rows, a third of them
    on a 12-level integer grid (ties, duplicates), non-finite rows and 1e12, and rows 0 .. 255 an antichain below everything else --
    front 0 is exactly the first tile, so from the second pass on the first slice walks a dead tile and then a live one."""
    rng = np.random.default_rng(P)
    F = rng.random((P, 3))
    F[P // 3:2 * P // 3] = rng.integers(0, 12, (2 * P // 3 - P // 3, 3)) / 12.0
    t = np.linspace(0.0, 1.0, 256)
    F[:256] = np.stack([t, 1.0 - t, np.zeros(256)], axis=1) * 1e-3 - 1.0
    F[300] = np.nan; F[P - 1, 1] = np.inf; F[P // 2] = 1e12
    return F


@pytest.mark.parametrize("P", [5000, 16384])
def test_rank_with_several_tiles_per_slice(P):
    F = _big_rank_case(P)
    D = mr.dominance(F)
    want, nf = mr.rank_peel(F, D=D)
    got, gnf = _rank(F)
    assert gnf == nf and np.array_equal(got, want)
    assert (want == 0).sum() == 256 and (want[:256] == 0).all() and nf > 10
    bad = ~np.isfinite(F).all(axis=1)
    assert bad.sum() == 2 and (want[bad] == nf - 1).all()
    want, nf = mr.rank_peel(F, stop_at=P // 2, D=D)
    got, gnf = _rank(F, stop_at=P // 2)
    print("P", P, "fronts to rank half:", nf)
    assert gnf == nf and np.array_equal(got, want) and (want == nf).any()


def test_rank_argument_errors():
    import torch
    from phoskintime_amd import _capi
    k = _k()
    F = _t(np.zeros((4, 3)), torch.float64); r = torch.zeros(4, dtype=torch.int32, device=k.dev); nf = torch.zeros(1, dtype=torch.int32, device=k.dev)
    call = lambda P, M: k.ctx.lib.pk_moo_rank_batch(k.ctx.handle, P, M, F.data_ptr(), 0, r.data_ptr(), nf.data_ptr())
    assert call(0, 3) == _capi.PK_OK and call(4, 1) == _capi.PK_ERR_ARG and call(4, 5) == _capi.PK_ERR_ARG and call(65537, 3) == _capi.PK_ERR_ARG
    assert k.ctx.lib.pk_moo_survive_batch(k.ctx.handle, 4, 5, r.data_ptr(), r.data_ptr(), F.data_ptr(), 3, r.data_ptr()) == _capi.PK_ERR_ARG


# ---------------------------------------------------------------- associate

ASSOC_SEED = 0


def _assoc_case(p):
    from phoskintime_amd.global_model.search import das_dennis
    rng = np.random.default_rng([ASSOC_SEED, p])
    F = rng.random((333, 3)) * np.array([2.0, 30.0, 0.5]) + np.array([1.0, -4.0, 0.0])
    return F, F.min(axis=0), F.max(axis=0), das_dennis(3, p)


@pytest.mark.parametrize("p,H", [(12, 91), (20, 231)])
def test_associate_equals_the_twin(p, H):
    import torch
    F, ideal, nadir, W = _assoc_case(p)
    assert W.shape[0] == H
    niche, dist, d = mr.associate(F, ideal, nadir, W)
    two = np.sort(d, axis=1)[:, :2]
    gap = float((two[:, 1] - two[:, 0]).min())
    print("smallest gap between the best and second-best distance:", gap)
    assert gap > 1e-9
    Fb = F.copy(); Fb[7] = np.nan; Fb[100, 2] = np.inf
    nb, db, _ = mr.associate(Fb, ideal, nadir, W)
    for Fx, nx, dx in ((F, niche, dist), (Fb, nb, db)):
        gn, gd = _k().associate(_t(Fx, torch.float64), _t(ideal), _t(nadir), _t(W))
        gn, gd = gn.cpu().numpy(), gd.cpu().numpy()
        fin = np.isfinite(dx)
        err = float(np.max(np.abs(gd[fin] - dx[fin]) / (1.0 + dx[fin])))
        print("H", H, "max |dist - twin| / (1 + dist) =", err)
        assert np.array_equal(gn, nx)
        assert err <= 1e-12 and np.array_equal(gd[~fin], dx[~fin])
    assert nb[7] == -1 and nb[100] == -1 and np.isinf(db[7])


def _assoc_big_case():
    from phoskintime_amd.global_model.search import das_dennis
    F = np.random.default_rng(4).random((50, 4))
    return F, np.zeros(4), np.ones(4), das_dennis(4, 27)


def test_associate_with_directions_beyond_the_default_lds_limit():
    """H = 4060, M = 4: 127 KiB of directions, the launch that has to raise the kernel's dynamic LDS limit first."""
    import torch
    F, ideal, nadir, W = _assoc_big_case()
    assert W.shape == (4060, 4)
    niche, dist, d = mr.associate(F, ideal, nadir, W)
    two = np.sort(d, axis=1)[:, :2]
    assert float((two[:, 1] - two[:, 0]).min()) > 1e-9
    gn, gd = _k().associate(_t(F, torch.float64), _t(ideal), _t(nadir), _t(W))
    assert np.array_equal(gn.cpu().numpy(), niche)
    assert float(np.max(np.abs(gd.cpu().numpy() - dist) / (1.0 + dist))) <= 1e-12


def test_associate_degenerate_column_and_tie():
    """A column with nadir = ideal divides by 1e-12; a row on the bisector of two directions goes to the lower one."""
    import torch
    W = np.array([[1.0, 0.0], [0.0, 1.0]])
    F = np.array([[1.0, 1.0], [3.0, 0.5], [0.25, 2.0]])
    gn, gd = _k().associate(_t(F, torch.float64), _t(np.zeros(2)), _t(np.ones(2)), _t(W))
    assert gn.cpu().numpy().tolist() == [0, 0, 1] and gd.cpu().numpy().tolist() == [1.0, 0.5, 0.25]
    ideal, nadir = np.array([0.0, 1.0]), np.array([1.0, 1.0])
    F = np.array([[0.5, 1.0], [0.5, 1.0 + 1e-6]])
    wn, wd, _ = mr.associate(F, ideal, nadir, W)
    gn, gd = _k().associate(_t(F, torch.float64), _t(ideal), _t(nadir), _t(W))
    assert np.array_equal(gn.cpu().numpy(), wn) and np.allclose(gd.cpu().numpy(), wd, rtol=1e-12, atol=0)


# ---------------------------------------------------------------- survive

def _survive(rank, niche, dist, H, K):
    import torch
    return _k().survive(_t(rank, torch.int32), _t(niche, torch.int32), _t(dist, torch.float64), H, K).cpu().numpy()


def _survive_cases():
    rng = np.random.default_rng(8)
    out = []
    for k, (P, H, nr) in enumerate([(50, 91, 3), (300, 420, 4), (700, 231, 5), (1500, 91, 3), (64, 4096, 2), (257, 7, 6)]):
        rank = rng.integers(0, nr, P).astype(np.int32)
        rank = np.unique(rank, return_inverse=True)[1].astype(np.int32)
        niche = rng.integers(0, H if k % 2 else max(1, H // 3), P).astype(np.int32)      # H // 3: two thirds of the niches stay empty
        dist = rng.random(P)
        out.append((rank, niche, dist, H))
    # tied distances from duplicated rows, rows without a niche
    rank, niche, dist, H = out[2]
    dist = np.round(dist * 4) / 4
    niche = niche.copy(); niche[::9] = -1
    out.append((rank, niche, np.where(niche < 0, np.inf, dist), H))
    # one front only, every row without a niche
    out.append((np.zeros(40, np.int32), np.full(40, -1, np.int32), np.full(40, np.inf), 5))
    # everything in one niche of one front
    out.append((np.zeros(130, np.int32), np.full(130, 3, np.int32), rng.integers(0, 5, 130) / 5.0, 12))
    # NaN distances (the entry point takes any dist): they order last within their niche, by index
    rank, niche, dist, H = out[1]
    dist = np.round(dist * 4) / 4
    dist[::7] = np.nan
    out.append((rank, niche, dist, H))
    return out


@pytest.mark.parametrize("case", range(10))
def test_survive_equals_the_sequential_loop(case):
    rank, niche, dist, H = _survive_cases()[case]
    P = rank.size
    fronts = np.cumsum(np.bincount(rank))
    for K in sorted({0, 1, P // 5, P // 2, P - 1, P, *map(int, fronts), int(fronts[0]) + 1}):
        if not 0 <= K <= P:
            continue
        want = mr.survive_loop(rank, niche, dist, H, K)
        got = _survive(rank, niche, dist, H, K)
        assert got.shape == (K,) and np.array_equal(got, want), (case, K)


def _big_survive_case():
    """P = 5000: two LDS tiles in every slice of the count kernel, the last tile cut short; tied and NaN distances, rows without a niche."""
    rng = np.random.default_rng(12)
    P, H = 5000, 91
    rank = rng.integers(0, 3, P).astype(np.int32)
    niche = rng.integers(0, 60, P).astype(np.int32)
    niche[::11] = -1
    dist = np.round(rng.random(P) * 64) / 64
    dist[5::97] = np.nan
    return rank, niche, np.where(niche < 0, np.inf, dist), H


@pytest.mark.parametrize("K", [2500, 4990])
def test_survive_with_several_tiles_per_slice(K):
    rank, niche, dist, H = _big_survive_case()
    assert (rank == 0).sum() < 2500 < (rank <= 1).sum() and (rank <= 1).sum() < 4990       # the last front is front 1, then front 2
    want = mr.survive_loop(rank, niche, dist, H, K)
    got = _survive(rank, niche, dist, H, K)
    assert got.shape == (K,) and np.array_equal(got, want)


# ---------------------------------------------------------------- mate

def _mate_case(P, n):
    rng = np.random.default_rng([P, n])
    xl = rng.uniform(-3, 0, n); xu = xl + rng.uniform(0.5, 4, n)
    if n > 1:
        xu[n // 2] = xl[n // 2]                            # a fixed column
    X = rng.uniform(xl, xu, (P, n))
    X[1] = X[0]                                            # identical parents: |x1 - x2| <= 1e-14
    X[2, 0] = xl[0]; X[3, 0] = xu[0]                       # on the bounds
    rank = rng.integers(0, 3, P).astype(np.int32)
    niche = rng.integers(0, 4, P).astype(np.int32)
    dist = np.round(rng.random(P) * 8) / 8
    return X, rank, niche, dist, xl, xu


def _mate(X, rank, niche, dist, xl, xu, seed, gen, pc, eta_c, pm, eta_m):
    import torch
    Xc, par = _k().mate(_t(X, torch.float64), _t(rank, torch.int32), _t(niche, torch.int32), _t(dist, torch.float64), _t(xl), _t(xu),
                        seed, gen, pc, eta_c, pm, eta_m, want_parents=True)
    return Xc.cpu().numpy(), par.cpu().numpy()


@pytest.mark.parametrize("P", [37, 256])
@pytest.mark.parametrize("n", [1, 5, 130])
def test_mate_equals_the_twin(P, n):
    X, rank, niche, dist, xl, xu = _mate_case(P, n)
    seed, gen = 0xDEADBEEFCAFEF00D, 3
    pm = max(0.3, 1.0 / n)
    want, wpar = mr.mate(X, rank, niche, dist, xl, xu, seed, gen, 0.9, 15.0, pm, 10.0)
    got, gpar = _mate(X, rank, niche, dist, xl, xu, seed, gen, 0.9, 15.0, pm, 10.0)
    assert np.array_equal(gpar, wpar)
    err = float(np.max(np.abs(got - want) / np.where(xu > xl, xu - xl, 1.0)))
    print("P", P, "n_var", n, "max |Xc - twin| / (xu - xl) =", err, "changed entries:", int((want != X[wpar]).sum()))
    assert err <= 1e-12
    assert (got >= xl).all() and (got <= xu).all()
    assert (want != X[wpar]).any()                                             # the case does cross and mutate
    if n > 1:
        assert np.array_equal(got[:, n // 2], X[gpar][:, n // 2])              # xl == xu: unchanged
    same, spar = _mate(X, rank, niche, dist, xl, xu, seed, gen, 0.0, 15.0, 0.0, 10.0)
    assert np.array_equal(spar, wpar) and np.array_equal(same, X[wpar])        # pc = pm = 0: the parents bit for bit
    again, _ = _mate(X, rank, niche, dist, xl, xu, seed, gen, 0.9, 15.0, pm, 10.0)
    other, opar = _mate(X, rank, niche, dist, xl, xu, seed, gen + 1, 0.9, 15.0, pm, 10.0)
    assert np.array_equal(again, got) and not np.array_equal(other, got)
    if P > 37:
        assert not np.array_equal(opar, gpar)


# ---------------------------------------------------------------- driver

def _problem():
    if "prob" not in _K:
        import net_objgrad_reference as og
        import net_sens_reference as ref
        from oracle import network_models as nm
        from phoskintime_amd.global_model import NetworkEngine
        from phoskintime_amd.global_model.optproblem import GlobalODEBatch
        s = og.fixture_data("network_m0_small")
        eng = NetworkEngine.from_npz(s["g"])
        keys = ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")
        sl = ref.slices(s["net"])
        defaults = {k: (s["defaults"][sl[k][0]:sl[k][1]] if k != "tf_scale" else float(s["defaults"][sl[k][0]])) for k in keys}
        raw0 = nm.inv_softplus(s["defaults"])
        _K["prob"] = GlobalODEBatch(eng, None, s["ld"], defaults, og.LAMD, s["g"]["t_eval"], xl=raw0 - 1.0, xu=raw0 + 1.0, y0=s["g"]["y0"],
                                    rtol=1e-8, atol=1e-10)
    return _K["prob"]


def _run(seed):
    key = ("run", seed)
    if key not in _K:
        states = []

        def cb(gen, st):
            states.append({k: v.cpu().numpy().copy() for k, v in st.items()})

        res = _problem().search(40, 6, seed, callback=cb)
        _K[key] = (res, states)
    return _K[key]


def test_search_returns_what_evaluate_device_computes():
    prob = _problem()
    res, states = _run(5)
    assert res.X.is_cuda and res.F.is_cuda and tuple(res.X.shape) == (40, prob.n_var) and tuple(res.F.shape) == (40, 3)
    assert len(states) == 7 and len(res.history) == 7
    X = res.X.cpu().numpy()
    assert (X >= prob.xl).all() and (X <= prob.xu).all()
    assert np.array_equal(prob.evaluate_device(res.X).cpu().numpy(), res.F.cpu().numpy())
    assert np.array_equal(states[-1]["F"], res.F.cpu().numpy()) and np.array_equal(states[-1]["rank"], res.rank.cpu().numpy())
    assert np.isfinite(res.F.cpu().numpy()).all()


def test_search_is_a_function_of_the_seed():
    import torch
    res, _ = _run(5)
    again = _problem().search(40, 6, 5)
    other, _ = _run(6)
    assert torch.equal(again.X, res.X) and torch.equal(again.F, res.F) and torch.equal(again.rank, res.rank) and torch.equal(again.niche, res.niche)
    assert not torch.equal(other.X, res.X)


def test_search_start_is_a_latin_hypercube():
    prob = _problem()
    _, states = _run(5)
    X0 = states[0]["X"]
    u = (X0 - prob.xl) / (prob.xu - prob.xl)
    strata = np.sort(np.minimum(np.floor(u * 40).astype(int), 39), axis=0)
    assert np.array_equal(strata, np.tile(np.arange(40)[:, None], (1, prob.n_var)))


def test_search_never_loses_ground():
    res, states = _run(5)
    ideals = np.stack([h["ideal"] for h in res.history])
    assert (np.diff(ideals, axis=0) <= 0).all()
    for g in range(len(states) - 1):
        front = states[g + 1]["F"][states[g + 1]["rank"] == 0]
        assert front.shape[0] == res.history[g + 1]["front0"] and front.shape[0] > 0
        D = mr.dominance(np.concatenate([states[g]["F"], front]))
        n = states[g]["F"].shape[0]
        assert not D[:n, n:].any(), g
    first, last = states[0]["F"].sum(axis=1).min(), states[-1]["F"].sum(axis=1).min()
    print("best sum of objectives: start", first, "after 6 generations", last)
    assert last < first


def test_search_callback_can_stop():
    res = _problem().search(40, 6, 5, callback=lambda gen, st: gen == 2)
    assert [h["gen"] for h in res.history] == [0, 1, 2]
