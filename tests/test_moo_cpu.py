"""CPU: the numpy twin of the many-objective bookkeeping agrees with itself (peeling = chain rule, sequential niching loop = closed form),
the reference-direction lattice has its size and order, the four ``pk_moo_*`` entry points are declared in include/phoskin.h, listed in
``_capi.SYMBOLS``, exported by the library and answer a null context with an error code (no kernel is launched here), and ``search``
refuses a problem without bounds."""
import re
from pathlib import Path

import numpy as np
import pytest

import moo_reference as mr

ROOT = Path(__file__).resolve().parents[1]
NEW = ("pk_moo_rank_batch", "pk_moo_associate_batch", "pk_moo_survive_batch", "pk_moo_mate_batch")


def _cases_F():
    rng = np.random.default_rng(11)
    for k in range(12):
        P, M = int(rng.integers(1, 90)), int(rng.integers(2, 5))
        yield rng.random((P, M))                                             # random
        yield rng.integers(0, 4, (P, M)).astype(float)                      # tie-heavy
    F = rng.integers(0, 3, (40, 3)).astype(float)
    F[3] = np.nan; F[7, 1] = np.inf; F[9] = 1e12; F[11] = F[12]
    yield F


def test_peeling_equals_the_chain_rule():
    for F in _cases_F():
        r, nf = mr.rank_peel(F)
        assert np.array_equal(r, mr.rank_chain(F)) and nf == r.max() + 1


def test_nonfinite_rows_rank_behind_every_finite_row():
    F = np.array([[1.0, 2.0], [np.nan, 0.0], [2.0, 1.0], [np.inf, np.inf], [3.0, 3.0], [1e12, 1e12]])
    r, nf = mr.rank_peel(F)
    assert list(r) == [0, 3, 0, 3, 1, 2] and nf == 4
    D = mr.dominance(F)
    assert not D[1].any() and not D[3].any() and not D[1, 3] and D[5, 1]


def test_stop_at_marks_the_unranked_rows():
    F = np.arange(7.0)[:, None] * np.ones((1, 3))
    r, nf = mr.rank_peel(F, stop_at=3)
    assert nf == 3 and list(r) == [0, 1, 2, 3, 3, 3, 3]


def _cases_survive():
    rng = np.random.default_rng(5)
    for k in range(60):
        P, H = int(rng.integers(1, 70)), int(rng.integers(1, 100))
        rank = np.sort(rng.integers(0, rng.integers(1, 6), P)).astype(np.int32)
        rank = (np.unique(rank, return_inverse=True)[1]).astype(np.int32)[rng.permutation(P)]
        niche = rng.integers(-1 if k % 3 == 0 else 0, max(1, H // (1 + k % 4)), P).astype(np.int32)
        dist = rng.integers(0, 4, P) / 4.0 if k % 2 else rng.random(P)      # tied distances every other case
        dist = np.where(niche < 0, np.inf, dist)
        for K in sorted({0, 1, P // 3, P // 2, P - 1, P, int((rank == 0).sum()), int((rank <= 1).sum())}):
            if 0 <= K <= P:
                yield rank, niche, dist, H, K


def test_sequential_niching_equals_the_closed_form():
    n = 0
    for rank, niche, dist, H, K in _cases_survive():
        a, b = mr.survive_loop(rank, niche, dist, H, K), mr.survive_closed(rank, niche, dist, H, K)
        assert np.array_equal(a, b), (rank, niche, dist, H, K)
        assert a.size == K and (np.diff(a) > 0).all()
        n += 1
    assert n > 300


def test_nan_distances_order_last_in_both_forms():
    rng = np.random.default_rng(9)
    rank = rng.integers(0, 3, 60).astype(np.int32); niche = rng.integers(0, 5, 60).astype(np.int32)
    dist = rng.integers(0, 3, 60) / 3.0
    dist[::4] = np.nan
    for K in range(0, 61, 7):
        a = mr.survive_loop(rank, niche, dist, 5, K)
        assert np.array_equal(a, mr.survive_closed(rank, niche, dist, 5, K))
    last = np.nonzero((rank == 0) & (niche == 0))[0]                          # K = 1: front 0 does not fit; niche 0 gives its best row
    best = min(last, key=lambda i: (np.isnan(dist[i]), dist[i], i))
    assert not np.isnan(dist[best]) and mr.survive_loop(rank, niche, dist, 5, 1).tolist() == [best]


def test_das_dennis():
    from phoskintime_amd.global_model.search import das_dennis
    for p, rows in ((12, 91), (20, 231)):
        W = das_dennis(3, p)
        assert W.shape == (rows, 3) and np.allclose(W.sum(axis=1), 1.0, atol=1e-15) and (W >= 0).all()
        assert len({tuple(np.rint(w * p).astype(int)) for w in W}) == rows
        k = np.rint(W * p).astype(int)
        assert sorted(map(tuple, k)) == list(map(tuple, k))                  # the documented (lexicographic) order
    assert das_dennis(2, 3).tolist() == [[0.0, 1.0], [1 / 3, 2 / 3], [2 / 3, 1 / 3], [1.0, 0.0]]
    assert das_dennis(4, 5).shape == (56, 4)


def test_rng_is_splitmix64_of_the_counter():
    # SplitMix64 finaliser: mix(0x9E3779B97F4A7C15) is the generator's first output for state 0 (known answer 0xE220A8397B1DCDAF)
    assert int(mr._mix(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF
    u = mr.uniform(0, 0, 0, 0, 0, 5, 3)                                     # counter 1, seed 0
    assert float(u) == (0xE220A8397B1DCDAF >> 11) * 2.0 ** -53
    U = mr.uniform(12345, 3, 6, np.arange(64)[:, None], np.arange(50)[None, :], 64, 50)
    assert U.shape == (64, 50) and (U >= 0).all() and (U < 1).all() and abs(U.mean() - 0.5) < 0.02 and np.unique(U).size == U.size


def test_mate_twin_properties():
    rng = np.random.default_rng(2)
    P, n = 9, 6
    xl, xu = -np.ones(n), np.ones(n) * 2.0
    xl[2] = xu[2] = 0.5
    X = rng.uniform(xl, xu, (P, n))
    rank = rng.integers(0, 3, P); niche = rng.integers(0, 4, P); dist = rng.random(P)
    Xc, par = mr.mate(X, rank, niche, dist, xl, xu, 7, 1, 0.0, 15.0, 0.0, 10.0)
    assert np.array_equal(Xc, X[par])                                        # no crossover, no mutation: the parents bit for bit
    Xc, par2 = mr.mate(X, rank, niche, dist, xl, xu, 7, 1, 0.9, 15.0, 0.5, 10.0)
    assert np.array_equal(par, par2) and (Xc >= xl).all() and (Xc <= xu).all() and np.array_equal(Xc[:, 2], X[par][:, 2])
    assert not np.array_equal(Xc, X[par])


def test_declared_listed_and_exported(built_lib):
    from phoskintime_amd import _capi
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "phoskin.h").read_text(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _capi.SYMBOLS and hasattr(built_lib, name), name
    assert built_lib.pk_version() == 200


def test_null_handles_are_errors(built_lib):
    from phoskintime_amd import _capi
    assert built_lib.pk_moo_rank_batch(None, 1, 3, None, 0, None, None) == _capi.PK_ERR_ARG
    assert built_lib.pk_moo_associate_batch(None, 1, 3, None, None, None, 1, None, None, None) == _capi.PK_ERR_ARG
    assert built_lib.pk_moo_survive_batch(None, 1, 1, None, None, None, 1, None) == _capi.PK_ERR_ARG
    assert built_lib.pk_moo_mate_batch(None, 1, 1, None, None, None, None, None, None, 0, 0, 0.9, 15.0, 0.1, 10.0, None, None) == _capi.PK_ERR_ARG


def test_python_layers_exist_and_search_needs_bounds():
    import types
    from phoskintime_amd import global_model
    from phoskintime_amd.global_model import search
    from phoskintime_amd.global_model.optproblem import GlobalODEBatch
    assert global_model.search is search and callable(search.search) and callable(search.lhs) and callable(GlobalODEBatch.search)
    with pytest.raises(ValueError):
        search.search(types.SimpleNamespace(xl=None, xu=None, n_var=4, n_obj=3), 8, 2, 0)
    prob = object.__new__(GlobalODEBatch)
    prob.xl, prob.xu, prob.n_var, prob.n_obj = np.zeros(4), None, 4, 3
    with pytest.raises(ValueError):
        prob.search(8, 2, 0)
