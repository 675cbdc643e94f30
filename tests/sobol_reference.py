"""Shared by tests/test_sobol_cpu.py and tests/test_gpu_sobol.py: the inputs of the index-kernel comparison, an independent (gathering)
restatement of the bootstrap, and the two known-answer models.  Nothing here is a test."""
import numpy as np

# (N, D, M) of the index-kernel comparison: M = 1 with odd N; M one lane past a wave; M one column past a 256-wide tile
SHAPES = ((7, 3, 1), (16, 2, 65), (8, 5, 257))
OFFSETS = (0.0, 1.0, 1e3)
RESAMPLES = (0, 2, 17)                # 17 is no multiple of any chunk width

ISHIGAMI_S1 = np.array([0.3139, 0.4424, 0.0])
ISHIGAMI_ST = np.array([0.5576, 0.4424, 0.2437])
ISHIGAMI_PROBLEM = {"num_vars": 3, "names": ["x1", "x2", "x3"], "bounds": [[-np.pi, np.pi]] * 3}


def ishigami(X, a=7.0, b=0.1):
    return np.sin(X[:, 0]) + a * np.sin(X[:, 1]) ** 2 + b * X[:, 2] ** 4 * np.sin(X[:, 0])


def random_outputs(N, D, M, seed=0):
    """(Y [N (D + 2), M], index of the constant column or None): standard normal spread around the column offsets 0, 1, 1e3 (cycled); where
    there is more than one column, the last one is exactly constant."""
    rng = np.random.default_rng(1000 * seed + 100 * N + 10 * D + M)
    Y = rng.standard_normal((N * (D + 2), M)) + np.resize(np.asarray(OFFSETS), M)[None, :]
    const = M - 1 if M > 1 else None
    if const is not None:
        Y[:, const] = 1.0
    return Y, const


def input_condition(Y, const):
    """max |mean| / std over the non-constant columns: the comparison's own condition on its inputs (<= 2e3)."""
    keep = np.arange(Y.shape[1]) != (-1 if const is None else const)
    return float(np.max(np.abs(Y[:, keep].mean(axis=0)) / Y[:, keep].std(axis=0)))


def analyze_gather(Y, D, idx):
    """The bootstrap as SALib states it: for every resample gather A[idx], AB[idx], B[idx] and apply the plain formulas.  Y [N (D + 2), M]
    centred by the column means over all rows, idx [R, N] -> (S1r, STr) [R, D, M]."""
    Y = np.asarray(Y, float)
    Yc = Y - Y.mean(axis=0)
    A, B = Yc[0::D + 2], Yc[D + 1::D + 2]
    S1r = np.empty((idx.shape[0], D, Y.shape[1])); STr = np.empty_like(S1r)
    for r, ix in enumerate(idx):
        a, b = A[ix], B[ix]
        var = np.var(np.concatenate([a, b], axis=0), axis=0)
        for j in range(D):
            ab = Yc[j + 1::D + 2][ix]
            S1r[r, j] = np.mean(b * (ab - a), axis=0) / var
            STr[r, j] = 0.5 * np.mean((a - ab) ** 2, axis=0) / var
    return S1r, STr


def worst(got, ref):
    """max |got - ref| over the entries where ref is finite (NaN positions are compared separately)."""
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    ok = np.isfinite(ref)
    return float(np.max(np.abs(got[ok] - ref[ok]))) if ok.any() else 0.0


def e_round(cases):
    """E_ROUND: the worst |float64 analyze - longdouble analyze| over ``cases`` = iterable of (Y, D, counts)."""
    from phoskintime_amd.sensitivity import sobol
    e = 0.0
    for Y, D, counts in cases:
        lo, hi = sobol.analyze(Y, D, counts), sobol.analyze(Y.astype(np.longdouble), D, counts)
        keys = ("S1", "ST", "var") + (("S1_conf", "ST_conf") if counts is not None else ())
        e = max(e, max(worst(lo[k], hi[k]) for k in keys))
    return e


def index_cases():
    """(Y, D, counts, const, N, M) for every shape x resample count of the index-kernel comparison."""
    from phoskintime_amd.sensitivity import sobol
    for N, D, M in SHAPES:
        Y, const = random_outputs(N, D, M)
        for R in RESAMPLES:
            yield Y, D, (sobol.resample_counts(N, R, seed=R) if R else None), const, N, M
