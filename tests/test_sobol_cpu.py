"""CPU: the host side of the Sobol' path (phoskintime_amd/sensitivity/sobol.py) -- the Saltelli row layout, the estimator against two
models with analytic indices, the constant-column rule, the bootstrap against a restatement that gathers rows, and the float64 rounding
error E_ROUND of the estimator on the inputs the GPU comparison uses (tests/test_gpu_sobol.py takes its limit from the same figure).

Known answers.  Ishigami (a = 7, b = 0.1): S1 = (0.3139, 0.4424, 0), ST = (0.5576, 0.4424, 0.2437).  At N = 4096 with this construction
(scrambled Sobol' base samples, the estimators of ``analyze``) the worst of seeds 0 .. 7 is 0.0025 (0.022 at N = 1024); the limit 0.01
leaves a factor of 4."""
import numpy as np
import pytest

import sobol_reference as ref
from phoskintime_amd.sensitivity import sobol

LIMIT = 0.01
N_KNOWN = 4096


def test_build_two_by_two_rows_written_out():
    d = sobol.Draws(A=np.array([[0.1, 0.2], [0.3, 0.4]]), B=np.array([[0.5, 0.6], [0.7, 0.8]]))
    X = sobol.build(d, [[0.0, 1.0], [10.0, 20.0]])
    want = np.array([[0.1, 12.0],     # A_0
                     [0.5, 12.0],     # AB_01: column 0 from B_0
                     [0.1, 16.0],     # AB_02: column 1 from B_0
                     [0.5, 16.0],     # B_0
                     [0.3, 14.0],     # A_1
                     [0.7, 14.0],     # AB_11
                     [0.3, 18.0],     # AB_12
                     [0.7, 18.0]])    # B_1
    np.testing.assert_allclose(X, want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("N,D", [(8, 1), (5, 3)])
def test_shape_and_order_of_a_ab_b(N, D):
    d = sobol.draw(D, N, seed=3)
    assert d.A.shape == (N, D) and d.B.shape == (N, D)
    assert (d.A >= 0).all() and (d.A < 1).all() and (d.B >= 0).all() and (d.B < 1).all()
    lb, ub = np.arange(D) - 2.0, np.arange(D) + 3.0
    X = sobol.build(d, np.stack([lb, ub], axis=1))
    assert X.shape == (N * (D + 2), D)
    sc = lambda u: lb + u * (ub - lb)
    np.testing.assert_array_equal(X[0::D + 2], sc(d.A))
    np.testing.assert_array_equal(X[D + 1::D + 2], sc(d.B))
    for j in range(D):
        want = d.A.copy(); want[:, j] = d.B[:, j]
        np.testing.assert_array_equal(X[j + 1::D + 2], sc(want))
    # the draws are the two halves of one 2 D-dimensional scrambled Sobol' point set; sample() is draw + build
    from scipy.stats import qmc
    e = qmc.Sobol(d=2 * D, scramble=True, seed=3)
    u = e.random_base2(3) if N == 8 else None
    if u is not None:
        np.testing.assert_array_equal(np.hstack([d.A, d.B]), u)
    problem = {"num_vars": D, "bounds": np.stack([lb, ub], axis=1).tolist()}
    np.testing.assert_array_equal(sobol.sample(problem, N, seed=3), X)


def test_resample_counts_are_the_bincount_of_the_index_draw():
    c = sobol.resample_counts(6, 4, seed=9)
    idx = np.random.default_rng(9).integers(0, 6, (4, 6))
    assert c.dtype == np.int32 and c.shape == (4, 6) and (c.sum(axis=1) == 6).all()
    for r in range(4):
        np.testing.assert_array_equal(c[r], np.bincount(idx[r], minlength=6))


@pytest.mark.parametrize("seed", range(8))
def test_ishigami_known_indices(seed):
    X = sobol.sample(ref.ISHIGAMI_PROBLEM, N_KNOWN, seed=seed)
    r = sobol.analyze(ref.ishigami(X), 3)
    e1, et = np.max(np.abs(r["S1"] - ref.ISHIGAMI_S1)), np.max(np.abs(r["ST"] - ref.ISHIGAMI_ST))
    print(f"ishigami seed {seed}: max |S1 - analytic| = {e1:.4f}, max |ST - analytic| = {et:.4f}")
    assert r["S1"].shape == (3,) and r["var"].shape == ()
    assert e1 <= LIMIT and et <= LIMIT


@pytest.mark.parametrize("seed", range(8))
def test_linear_model_known_indices(seed):
    a = np.array([1.0, 2.0, 0.5, 3.0])
    problem = {"num_vars": 4, "bounds": [[0.0, 1.0]] * 4}
    X = sobol.sample(problem, N_KNOWN, seed=seed)
    r = sobol.analyze(X @ a, 4)
    want = a ** 2 / np.sum(a ** 2)
    e1, et = np.max(np.abs(r["S1"] - want)), np.max(np.abs(r["ST"] - want))
    print(f"linear seed {seed}: max |S1 - analytic| = {e1:.4f}, max |ST - analytic| = {et:.4f}")
    assert e1 <= LIMIT and et <= LIMIT


def test_constant_column_is_nan_and_leaves_its_neighbours_alone():
    N, D = 16, 3
    Y, _ = ref.random_outputs(N, D, 5)
    counts = sobol.resample_counts(N, 6, seed=1)
    Yc = Y.copy(); Yc[:, 2] = 0.1 + 0.2                      # a value whose column mean need not reproduce it exactly
    full = sobol.analyze(Yc, D, counts)
    rest = sobol.analyze(np.delete(Yc, 2, axis=1), D, counts)
    for k in ("S1", "ST", "S1_conf", "ST_conf"):
        assert np.isnan(full[k][:, 2]).all(), k
        assert np.isnan(full[k][:, 4]).all(), k              # random_outputs' own constant column
        # numpy's matrix products pick their summation order by the whole shape: a few ulps of O(1) numbers, not bit equality
        np.testing.assert_allclose(np.delete(full[k], 2, axis=1), rest[k], rtol=0, atol=1e-14)
        assert np.isfinite(np.delete(full[k], [2, 4], axis=1)).all(), k
    assert np.isnan(full["var"][[2, 4]]).all() and np.isfinite(np.delete(full["var"], [2, 4])).all()


def test_bootstrap_equals_gathering_the_rows():
    N, D, M, R = 12, 3, 4, 9
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((N * (D + 2), M)) + np.array([0.0, 1.0, -3.0, 10.0])
    idx = np.random.default_rng(4).integers(0, N, (R, N))
    counts = sobol.resample_counts(N, R, seed=4)
    S1r, STr = ref.analyze_gather(Y, D, idx)
    from scipy.stats import norm
    z = norm.ppf(0.975)
    r = sobol.analyze(Y, D, counts, conf_level=0.95)
    # the same numbers summed in another order: a few hundred terms of size <= 100 (offset 10, squared) -> 1e-12 is generous
    np.testing.assert_allclose(r["S1_conf"], z * S1r.std(axis=0, ddof=1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["ST_conf"], z * STr.std(axis=0, ddof=1), rtol=0, atol=1e-12)
    # the plain estimate is the resample that draws every row once
    one = sobol.analyze(Y, D, np.ones((2, N), np.int32))
    np.testing.assert_allclose(one["S1"], r["S1"], rtol=0, atol=1e-13)
    assert np.all(one["S1_conf"] <= 1e-13) and np.all(one["ST_conf"] <= 1e-13)
    plain = sobol.analyze(Y, D)
    np.testing.assert_array_equal(plain["S1"], r["S1"]); np.testing.assert_array_equal(plain["ST"], r["ST"])
    assert np.isnan(plain["S1_conf"]).all()


def test_one_resample_is_refused():
    Y, _ = ref.random_outputs(4, 2, 3)
    with pytest.raises(ValueError):
        sobol.analyze(Y, 2, np.ones((1, 4), np.int32))
    with pytest.raises(ValueError):
        sobol.analyze(Y[:-1], 2)


def test_float64_rounding_error_on_the_gpu_comparison_inputs():
    """E_ROUND = worst |float64 analyze - np.longdouble analyze| over the shapes, offsets and resample counts of the GPU comparison.
    Measured: 3.7e-15 overall (3.7e-15, 2.6e-15 and 2.3e-15 at offsets 0, 1 and 1e3: centring relative to a column's first row keeps the
    offset out of the rounding; centring by the mean itself gave 5e-13 at offset 1e3, the rounding of a mean of size 1e3)."""
    per_offset = {}
    for Y, D, counts, const, N, M in ref.index_cases():
        assert ref.input_condition(Y, const) <= 2e3
        for k, off in enumerate(ref.OFFSETS):
            cols = [m for m in range(M) if m % 3 == k and m != const]
            if cols:
                per_offset[off] = max(per_offset.get(off, 0.0), ref.e_round([(Y[:, cols], D, counts)]))
    E_ROUND = max(per_offset.values())
    print("E_ROUND per offset:", {k: f"{v:.2e}" for k, v in per_offset.items()}, f"overall {E_ROUND:.2e}")
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not wider than float64 on this platform"
    assert E_ROUND <= 1e-11                                   # the comparison's limit max(1e-12, 100 E_ROUND) stays meaningful
