"""GPU: pk_solve_protein_sens_vjp_batch -- a weighted sum over flat and its gradient (linear mode: w^T dflat; least-squares mode: the cost
0.5 |w (flat - target)|^2 and J^T r) from the output stage of every sensitivity kernel family, and its consumers autograd.solve_flat and
paramest.multistart.cost_and_grad_rows.  tests/sens_vjp_reference.py states the two modes.

(a) against pk_solve_protein_sens_batch with the same options, roundoff only: flat / status / n_steps bit-equal, and with u = 2^-53
        |grad_p - sum_f c_f dflat_fp| <= 4 F u sum_f |c_f dflat_fp|,        |value - sum terms| <= 4 F u sum |terms|
    (the kernel's serial sum of F terms and numpy's are each within (F + 3) u sum |terms|), c_f formed from the returned flat.
(b) least-squares mode on the kernels that cut the columns into chunks: a chunk forms c_f from its own integration of the state, so
    2 sum_f w_f^2 eps_v(f) |dflat_fp| is added, eps_v the flat limit of tests/test_gpu_sens_regimes.py: 0.1 (1e-8 + 1e-6 |v|) at rtol 1e-9 /
    atol 1e-11, 1e-8 + 1e-6 |v| at the default tolerances.
(c) against the oracle's exact derivative (oracle.protein_models.sens_exact_lti through flat_and_jacobian and the reference's two modes):
    no tolerance of its own, the (eps_v, eps_d) pairs of tests/test_gpu_sens_metric.py (_eps) propagated to first order
    (sens_vjp_reference.bounds).
Every comparison prints its worst err / bound first (FIG lines, collected in profiles/r17_a_sens_vjp_summary.txt) and asserts <= 1.

Sizes: FAMILIES of tests/test_gpu_sens_metric.py; B = 5 up to 64 states and 2 beyond, replicas 0 and B - 1 compared.  Grids: the regimes
test's, the first five points of the reference's grid (the mRNA block of flat is EMPTY: an output stage keyed on (row, time) instead of the
flat index fails here), the first six (exactly one mRNA slot) and T = 1.

Measured on an MI355X (worst err / bound; profiles/r17_a_sens_vjp_summary.txt has every case):
  (a) / (b) against pk_solve_protein_sens_batch: value 0.095 (distmod 1, five points, batched w), gradient 0.082 (same size); on the
  chunked kernels in least-squares mode: gradient 2.2e-3 at the default tolerances (succmod 6), 1.2e-5 at rtol 1e-9 / atol 1e-11.
  (c) against the exact derivative: default tolerances value 1.0e-4 (distmod 33, uniform, linear), gradient 3.3e-4 (distmod 30,
  log-uniform, linear); rtol 1e-9 / atol 1e-11 value 3.2e-6, gradient 1.2e-4 (distmod 33, log-uniform, linear); normalised / unclipped /
  forced kernels <= 4.0e-6.  autograd 5.8e-5 (distmod 4); cost_and_grad_rows 0.03 (distmod 4).
"""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import protein_models as pm
import sens_vjp_reference as ref
from test_gpu_sens_metric import DEFAULT, FAMILIES, FAMILY_OF, ONE_PER_FAMILY, REGIMES, SIZES, TIGHT, _case, _eps, _ratio
from test_gpu_sens_regimes import _cols, _grid

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CHUNKED = {s for fam in ("rows16", "rows32", "rows64", "randsens") for s in FAMILIES[fam]}
GRIDS = {"regimes": _grid, "t5": lambda model, n: pm.TIME_POINTS[:5], "t6": lambda model, n: pm.TIME_POINTS[:6],
         "t1": lambda model, n: np.array([0.0])}
OPTS = {"tight": TIGHT, "default": DEFAULT}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _np(x):
    return x.cpu().numpy()


def _eps_v(tol, v):
    return _eps(tol, v, np.zeros(1))[0]


@functools.lru_cache(maxsize=None)
def _inputs(model, n):
    """(theta [B, P] on U(0, 20), y0 [S]) for the comparisons with pk_solve_protein_sens_batch: no exact reference needed."""
    mid = pm.MODEL_IDS[model]
    B = 5 if pm.n_states(mid, n) <= 64 else 2
    th, y0 = pm.sens_regime("uniform", mid, n, np.random.default_rng([23, mid, n]), B)
    th.setflags(write=False); y0.setflags(write=False)
    return th, y0


def _weights(rng, like):
    """Shared and batched weights, shared weights with exact zeros, shared and batched targets near `like` [B, F] (but not on it)."""
    B, F = like.shape
    w_sh = rng.uniform(0.5, 2.0, size=F); w_b = rng.uniform(0.5, 2.0, size=(B, F))
    w_z = w_sh.copy(); w_z[rng.random(F) < 0.3] = 0.0
    tg_b = like * (1.0 + 0.1 * rng.normal(size=(B, F))) + 0.05 * rng.normal(size=(B, F))
    return w_sh, w_b, w_z, tg_b[0].copy(), tg_b


def _row(a, b):
    return None if a is None else (a[b] if a.ndim == 2 else a)


# ------------------------------------------------------------------------------------------------ (a), (b): against the existing entry point
@pytest.mark.parametrize("tol", ["tight", "default"])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("model,n", SIZES)
def test_against_sens_batch(eng, model, n, grid, tol):
    mid = pm.MODEL_IDS[model]
    th, y0 = _inputs(model, n)
    B = th.shape[0]
    t = GRIDS[grid](model, n)
    plain = eng.solve_ode_sens_batch(model, th, y0, n, t, **OPTS[tol])
    flat, dflat = _np(plain.flat), _np(plain.dflat)
    F = flat.shape[1]
    assert not _np(plain.status).any() and np.isfinite(dflat).all()
    w_sh, w_b, w_z, tg_sh, tg_b = _weights(np.random.default_rng([5, mid, n, len(t)]), flat)
    variants = [("linear_shared", w_sh, None), ("linear_batched", w_b, None), ("linear_zeros", w_z, None),
                ("ls_shared", w_sh, tg_sh), ("ls_batched", w_b, tg_b), ("ls_zeros_batched_target", w_z, tg_b)]
    chunked = (model, n) in CHUNKED
    for k, (name, w, tg) in enumerate(variants):
        r = eng.solve_ode_vjp_batch(model, th, y0, n, t, w, tg, want_flat=(k % 3 == 0), **OPTS[tol])
        value, grad = _np(r.value), _np(r.grad)
        assert np.array_equal(_np(r.status), _np(plain.status)) and np.array_equal(_np(r.n_steps), _np(plain.n_steps)), name
        if k % 3 == 0:
            assert np.array_equal(_np(r.flat), flat), name
        else:
            assert r.flat is None
        assert np.isfinite(value).all() and np.isfinite(grad).all(), name
        rv = rg = 0.0
        for b in (0, B - 1):
            wb, tgb = _row(w, b), _row(tg, b)
            v_ref, g_ref, sv, sg = ref.vjp(flat[b], dflat[b], wb, tgb)
            bound_g = 4 * F * U * sg
            if tg is not None and chunked:                                    # (b): a chunk's own state values
                bound_g = bound_g + 2.0 * ((wb * wb * _eps_v(tol, flat[b]))[:, None] * np.abs(dflat[b])).sum(axis=0)
            rv = max(rv, _ratio(abs(value[b] - v_ref), 4 * F * U * sv)); rg = max(rg, _ratio(np.abs(grad[b] - g_ref), bound_g))
        print(f"FIG sens_batch {FAMILY_OF[(model, n)]} {model} {n} {grid} {tol} {name}: value_ratio={rv:.3e} grad_ratio={rg:.3e}")
        assert rv <= 1.0, name
        assert rg <= 1.0, name
    if grid == "t1":                                                          # the value of the post-processed y0, a gradient of exact zeros
        assert np.all(grad == 0.0)


# ------------------------------------------------------------------------------------------------ (c): against the exact derivative
@functools.lru_cache(maxsize=None)
def _exact_flat(model, n, regime, clip_nonneg=True, normalize=False):
    """{replica: (v [F], d [F, len(cols)])} of test_gpu_sens_metric._case, computed once per process and never written."""
    _, y0, raw = _case(model, n, regime)
    out = {}
    for b, (sol, dsol) in raw.items():
        v, d = ref.flat_reference(model, sol, dsol, y0, n, clip_nonneg=clip_nonneg, normalize=normalize)
        v.setflags(write=False); d.setflags(write=False)
        out[b] = (v, d)
    return out


def _exact_weights(model, n, regime, refs, B):
    mid = pm.MODEL_IDS[model]
    rng = np.random.default_rng([7, mid, n, pm.SENS_REGIMES.index(regime)])
    like = np.stack([refs[b][0] if b in refs else refs[0][0] for b in range(B)])
    w_sh, _, _, _, tg_b = _weights(rng, like)
    return w_sh, tg_b


def _compare_exact(tag, model, n, regime, tol, w, tg, value, grad, status, **post):
    cols = _cols(model, n)
    T = _grid(model, n).size
    rv = rg = 0.0
    for b, (v, d) in _exact_flat(model, n, regime, **post).items():
        tgb = _row(tg, b)
        v_ref, g_ref, _, _ = ref.vjp(v, d, w, tgb)
        bv, bg = ref.bounds(v, d, w, tgb, *_eps(tol, v, d), n, T)
        rv = max(rv, _ratio(abs(value[b] - v_ref), bv)); rg = max(rg, _ratio(np.abs(grad[b][cols] - g_ref), bg))
    mode = "linear" if tg is None else "least_squares"
    print(f"FIG {tag} {FAMILY_OF.get((model, n), '-')} {model} {n} {regime} {mode}: value_ratio={rv:.3e} grad_ratio={rg:.3e}")
    assert not np.asarray(status).any()
    assert np.isfinite(value).all() and np.isfinite(grad).all()
    assert rv <= 1.0
    assert rg <= 1.0


@pytest.mark.parametrize("tol", ["tight", "default"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("model,n", ONE_PER_FAMILY)
def test_against_the_exact_derivative(eng, model, n, regime, tol):
    th, y0, _ = _case(model, n, regime)
    w, tg = _exact_weights(model, n, regime, _exact_flat(model, n, regime), th.shape[0])
    for target in (None, tg):
        r = eng.solve_ode_vjp_batch(model, th, y0, n, _grid(model, n), w, target, **OPTS[tol])
        _compare_exact(tol, model, n, regime, tol, w, target, _np(r.value), _np(r.grad), _np(r.status))


# ------------------------------------------------------------------------------------------------ (d): post-processing, kernels, independence
@pytest.mark.parametrize("post", ["normalize", "noclip"])
@pytest.mark.parametrize("model,n", ONE_PER_FAMILY)
def test_normalize_and_unclipped(eng, model, n, post):
    kw = dict(normalize=True) if post == "normalize" else dict(clip_nonneg=False)
    th, y0, _ = _case(model, n, "uniform")
    w, tg = _exact_weights(model, n, "uniform", _exact_flat(model, n, "uniform", **kw), th.shape[0])
    for target in (None, tg):
        r = eng.solve_ode_vjp_batch(model, th, y0, n, _grid(model, n), w, target, **TIGHT, **kw)
        _compare_exact(post, model, n, "uniform", "tight", w, target, _np(r.value), _np(r.grad), _np(r.status), **kw)


_FORCED = {"2": [("distmod", 10), ("succmod", 6)],       # the column kernel where it is no longer the default
           "1": [("distmod", 9), ("succmod", 5)]}        # the 16-lane rows kernel below its default range

_FORCED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from phoskintime_amd import batch
inp = np.load(sys.argv[2])
out = {}
for key in inp["keys"]:
    model, n = key.split("_")
    for mode in ("linear", "ls"):
        r = batch.solve_ode_vjp_batch(model, inp[key + "_th"], inp[key + "_y0"], int(n), inp["t"], inp[key + "_w"],
                                      inp[key + "_tg"] if mode == "ls" else None, rtol=1e-9, atol=1e-11)
        out[f"{key}_{mode}_v"] = r.value.cpu().numpy(); out[f"{key}_{mode}_g"] = r.grad.cpu().numpy(); out[f"{key}_{mode}_status"] = r.status.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize("rows_env", ["2", "1"])
def test_forced_kernels(eng, tmp_path, rows_env):
    """PK_SENS_ROWS is read once per process: a fresh child computes with the forced kernel, this process compares with the same exact
    reference and bound."""
    cases = _FORCED[rows_env]
    inp = {"keys": np.array([f"{m}_{n}" for m, n in cases]), "t": pm.TIME_POINTS}
    wt = {}
    for m, n in cases:
        th, y0, _ = _case(m, n, "uniform")
        wt[(m, n)] = _exact_weights(m, n, "uniform", _exact_flat(m, n, "uniform"), th.shape[0])
        inp[f"{m}_{n}_th"], inp[f"{m}_{n}_y0"], inp[f"{m}_{n}_w"], inp[f"{m}_{n}_tg"] = th, y0, wt[(m, n)][0], wt[(m, n)][1]
    np.savez(tmp_path / "in.npz", **inp)
    root = str(Path(__file__).resolve().parents[1])
    subprocess.run([sys.executable, "-c", _FORCED_SCRIPT, root, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True,
                   env=dict(os.environ, PK_SENS_ROWS=rows_env), timeout=300)
    out = np.load(tmp_path / "out.npz")
    for m, n in cases:
        w, tg = wt[(m, n)]
        for mode, target in (("linear", None), ("ls", tg)):
            key = f"{m}_{n}_{mode}"
            _compare_exact(f"forced-PK_SENS_ROWS={rows_env}", m, n, "uniform", "tight", w, target, out[key + "_v"], out[key + "_g"], out[key + "_status"])


@pytest.mark.parametrize("model,n", ONE_PER_FAMILY)
def test_batch_independence_and_flat_request(eng, model, n):
    """A replica alone, in a batch of 5 and in the reversed batch gives equal bits (w and target batched, so that they travel with the
    replica); value and grad do not depend on whether flat was asked for."""
    mid = pm.MODEL_IDS[model]
    th2, y0 = _inputs(model, n)
    th = np.concatenate([th2, th2[::-1] * 1.25, th2[:1] * 0.5])[:5]
    t = _grid(model, n)
    F = max(t.size - 5, 0) + t.size + n * t.size
    rng = np.random.default_rng([29, mid, n])
    w = rng.uniform(0.5, 2.0, size=(5, F)); tg = rng.uniform(0.1, 1.0, size=(5, F))
    for target in (None, tg):
        full = eng.solve_ode_vjp_batch(model, th, y0, n, t, w, target, want_flat=True)
        bare = eng.solve_ode_vjp_batch(model, th, y0, n, t, w, target)
        rev = eng.solve_ode_vjp_batch(model, th[::-1].copy(), y0, n, t, w[::-1].copy(), None if target is None else target[::-1].copy())
        assert not _np(full.status).any() and np.isfinite(_np(bare.grad)).all()
        assert np.array_equal(_np(bare.value), _np(full.value)) and np.array_equal(_np(bare.grad), _np(full.grad))
        assert np.array_equal(_np(rev.value)[::-1], _np(bare.value)) and np.array_equal(_np(rev.grad)[::-1], _np(bare.grad))
        for b in (0, 2, 4):
            alone = eng.solve_ode_vjp_batch(model, th[b:b + 1], y0, n, t, w[b:b + 1], None if target is None else target[b:b + 1])
            assert np.array_equal(_np(alone.value)[0], _np(bare.value)[b]) and np.array_equal(_np(alone.grad)[0], _np(bare.grad)[b])
        assert not np.array_equal(_np(bare.grad)[0], _np(bare.grad)[4])


# ------------------------------------------------------------------------------------------------ (e): failure and refusals
@pytest.mark.parametrize("model,n", ONE_PER_FAMILY)
def test_step_limit_gives_nan(eng, model, n):
    """max_steps = 5 with the first output time out of reach (a step grows at most sixfold): PK_ST_MAXSTEPS on every replica and in every
    chunk, value NaN, every column of grad NaN, flat finite at t0 and NaN after it; the clean launch after it is unaffected."""
    from phoskintime_amd._capi import ST_MAXSTEPS
    mid = pm.MODEL_IDS[model]
    th, y0 = _inputs(model, n)
    t = np.array([0.0, 1e5, 2e5])
    F = 3 + 3 * n
    w = np.full(F, 0.5)
    for target in (None, np.full(F, 0.25)):
        before = eng.solve_ode_vjp_batch(model, th, y0, n, pm.TIME_POINTS[:6], np.ones(7 + 6 * n), None if target is None else np.ones(7 + 6 * n))
        cut = eng.solve_ode_vjp_batch(model, th, y0, n, t, w, target, want_flat=True, max_steps=5)
        after = eng.solve_ode_vjp_batch(model, th, y0, n, pm.TIME_POINTS[:6], np.ones(7 + 6 * n), None if target is None else np.ones(7 + 6 * n))
        assert ((_np(cut.status) & ST_MAXSTEPS) != 0).all()
        assert np.isnan(_np(cut.value)).all() and np.isnan(_np(cut.grad)).all()
        flat = _np(cut.flat)
        assert np.isfinite(flat[:, ref.t0_entries(n, 3)]).all() and np.isnan(flat[:, ref.t0_entries(n, 3) + 1]).all()
        for k in ("value", "grad", "status", "n_steps"):
            assert np.array_equal(_np(getattr(after, k)), _np(getattr(before, k))), k


def _raw_call(eng, model, n, null=None, method=None):
    import torch
    from phoskintime_amd import _capi
    ctx = eng.get_context()
    dev = torch.device("cuda", ctx.device)
    mid = pm.MODEL_IDS[model]
    P, S = pm.n_params(mid, n), pm.n_states(mid, n)
    F = 2 + 2 * n
    z = lambda *shape: torch.ones(shape, dtype=torch.float64, device=dev)
    th, y0, t, w, value, grad = z(1, P), z(S), torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev), z(F), z(1), z(1, P)
    p = lambda name, x: C.c_void_p(None) if null == name else C.c_void_p(x.data_ptr())
    opts = _capi.default_opts(method=method)
    rc = ctx.lib.pk_solve_protein_sens_vjp_batch(ctx.handle, mid, n, 1, p("theta", th), p("y0", y0), 0, p("t", t), 2, C.byref(opts), p("w", w), 0,
                                                 C.c_void_p(None), 0, p("value", value), p("grad", grad), C.c_void_p(None), C.c_void_p(None),
                                                 C.c_void_p(None))
    torch.cuda.synchronize()
    return rc


def test_refusals(eng):
    from phoskintime_amd import _capi
    assert _raw_call(eng, "distmod", 4) == _capi.PK_OK
    assert _raw_call(eng, "distmod", 63) == _capi.PK_ERR_UNSUPPORTED
    assert _raw_call(eng, "randmod", 8) == _capi.PK_ERR_UNSUPPORTED
    assert _raw_call(eng, "distmod", 4, method="rodas4") == _capi.PK_ERR_UNSUPPORTED
    for name in ("w", "value", "grad"):
        assert _raw_call(eng, "distmod", 4, null=name) == _capi.PK_ERR_ARG, name
    with pytest.raises(_capi.PhoskinError):
        eng.solve_ode_vjp_batch("randmod", np.ones((1, pm.n_params(2, 8))), np.ones(pm.n_states(2, 8)), 8, [0.0, 1.0], np.ones(2 + 2 * 8))
    with pytest.raises(ValueError):
        eng.solve_ode_vjp_batch("distmod", np.ones((1, 12)), np.ones(6), 4, [0.0, 1.0], np.ones(9))          # F = 10
    with pytest.raises(ValueError):
        eng.solve_ode_vjp_batch("distmod", np.ones((1, 12)), np.ones(6), 4, [0.0, 1.0], np.ones(10), np.ones((2, 10)))
    r = eng.solve_ode_vjp_batch("distmod", np.ones((0, 12)), np.ones(6), 4, [0.0, 1.0], np.ones(10))          # B = 0 is PK_OK
    assert r.value.shape == (0,) and r.grad.shape == (0, 12)


# ------------------------------------------------------------------------------------------------ (f): the consumers
@pytest.mark.parametrize("model,n", [("distmod", 4), ("randmod", 3), ("distmod", 30)])
def test_autograd_solve_flat(eng, model, n):
    """loss = 0.5 sum (w (solve_flat(theta) - target))^2; loss.backward() against the least-squares entry point's grad.  The backward
    pass forms c_f = w_f^2 (flat_f - target_f) from the THROUGHPUT kernel's flat, the entry point from the sensitivity kernel's own state
    values; both are within eps_v of the exact value, so beside the roundoff of (a) (two sums) the difference is bounded by
    2 sum_f w_f^2 eps_v(f) |dflat_fp|, and by (b)'s term once more on the chunked kernels.  Default tolerances."""
    import torch
    from phoskintime_amd import autograd
    mid = pm.MODEL_IDS[model]
    th, y0 = _inputs(model, n)
    B = th.shape[0]
    t = _grid(model, n)
    plain = eng.solve_ode_sens_batch(model, th, y0, n, t)
    flat, dflat = _np(plain.flat), _np(plain.dflat)
    F = flat.shape[1]
    w_sh, _, _, _, tg_b = _weights(np.random.default_rng([31, mid, n]), flat)
    dev = plain.flat.device
    theta = torch.tensor(th, device=dev, requires_grad=True)
    w_d, tg_d = torch.tensor(w_sh, device=dev), torch.tensor(tg_b, device=dev)
    out = autograd.solve_flat(model, theta, y0, n, t)
    fwd = eng.solve_ode_batch(model, th, y0, n, t, want_sol=False, want_flat=True).flat
    assert torch.equal(out.detach(), fwd) and out.requires_grad
    loss = (((out - tg_d) ** 2) * w_d ** 2).sum() / 2
    loss.backward()
    ls = eng.solve_ode_vjp_batch(model, th, y0, n, t, w_sh, tg_b)
    got, want = _np(theta.grad), _np(ls.grad)
    worst = 0.0
    for b in (0, B - 1):
        c = w_sh * (w_sh * (flat[b] - tg_b[b]))
        ev = ((w_sh * w_sh * _eps_v("default", flat[b]))[:, None] * np.abs(dflat[b])).sum(axis=0)
        bound = 2 * 4 * F * U * np.abs(c[:, None] * dflat[b]).sum(axis=0) + 2.0 * ev * (2 if (model, n) in CHUNKED else 1)
        worst = max(worst, _ratio(np.abs(got[b] - want[b]), bound))
    print(f"FIG autograd {model} {n}: grad_ratio={worst:.3e}")
    assert worst <= 1.0
    assert float(loss) == pytest.approx(float(_np(ls.value).sum()), rel=1e-4)
    # a single parameter vector, and no gradient for the other arguments
    th1 = torch.tensor(th[0], device=dev, requires_grad=True)
    y0_d = torch.tensor(y0, device=dev, requires_grad=True)
    o1 = autograd.solve_flat(model, th1, y0_d, n, t)
    assert o1.shape == (F,)
    o1.sum().backward()
    assert th1.grad.shape == th1.shape and y0_d.grad is None
    lin = eng.solve_ode_vjp_batch(model, th[:1], y0, n, t, np.ones(F))
    assert np.array_equal(_np(th1.grad), _np(lin.grad)[0])                   # backward IS the linear mode with w = grad_output


def test_autograd_backward_refuses_sizes_without_a_kernel(eng):
    import torch
    from phoskintime_amd import autograd
    from phoskintime_amd._capi import PhoskinError
    n = 63
    dev = torch.device("cuda", eng.get_context().device)
    theta = torch.full((1, pm.n_params(0, n)), 0.5, dtype=torch.float64, device=dev, requires_grad=True)
    out = autograd.solve_flat("distmod", theta, np.ones(pm.n_states(0, n)), n, [0.0, 1.0])          # forward: every size
    assert out.shape == (1, 2 + 2 * n) and torch.isfinite(out).all()
    with pytest.raises(PhoskinError):
        out.sum().backward()
    # another method: the forward pass runs it, the sensitivity kernels (LRP12 only) have no backward pass for it
    th4 = torch.full((2, 12), 0.5, dtype=torch.float64, device=dev, requires_grad=True)
    out4 = autograd.solve_flat("distmod", th4, np.ones(6), 4, [0.0, 1.0], method="rodas4")
    with pytest.raises(PhoskinError):
        out4.sum().backward()
    autograd.solve_flat("distmod", th4, np.ones(6), 4, [0.0, 1.0], method="lrp12", rtol=1e-8).sum().backward()
    assert th4.grad.shape == (2, 12) and torch.isfinite(th4.grad).all()


@pytest.mark.parametrize("model,n,log_space", [("distmod", 4, False), ("randmod", 3, True)])
def test_cost_and_grad_rows(eng, model, n, log_space):
    """Against the same quantities assembled in numpy from ONE solve_ode_sens_batch call (column-per-lane sizes: one integration of the
    state, roundoff only).  Bound: the kernel's and numpy's sums of F terms, (F + 3) u each, the chain-rule product and the ridge term's
    three operations: (2 F + 12) u sum |terms|."""
    import torch
    from phoskintime_amd.paramest import multistart
    mid = pm.MODEL_IDS[model]
    P, S = pm.n_params(mid, n), pm.n_states(mid, n)
    rng = np.random.default_rng([37, mid, n])
    R = 5
    theta = rng.uniform(0.2, 5.0, size=(R, P))
    p = np.log(theta) if log_space else theta
    y0 = rng.uniform(0.3, 1.5, size=S)
    t = pm.TIME_POINTS
    # theta = exp(p) by the function the code under test calls: numpy's and torch's exp may differ in the last bit, and one ulp of theta
    # moves the solution by more than the roundoff this test allows
    th_eff = torch.exp(torch.as_tensor(p)).numpy() if log_space else p
    plain = eng.solve_ode_sens_batch(model, th_eff, y0, n, t)
    flat, dflat = _np(plain.flat), _np(plain.dflat)
    F = flat.shape[1]
    target = flat * (1.0 + 0.1 * rng.normal(size=(R, F))) + 0.05 * rng.normal(size=(R, F))
    sigma = rng.uniform(0.5, 2.0, size=(R, F + P))
    lam = np.array([0.0, 0.3, 1.0, 0.0, 2.5])
    cost, grad = multistart.cost_and_grad_rows(model, n, t, p, y0, target, sigma=sigma, lam=lam)
    cost, grad = _np(cost), _np(grad)
    wv = 1.0 / sigma[:, :F]
    r = wv * (flat - target)
    rr = (lam / P)[:, None] * p * p / sigma[:, F:]
    cost_terms = np.concatenate([r * r, rr * rr], axis=1)
    cost_ref = 0.5 * cost_terms.sum(axis=1)
    jac = dflat * th_eff[:, None, :] if log_space else dflat
    data_terms = (wv * r)[:, :, None] * jac                                  # [R, F, P]
    ridge = rr * (2.0 * (lam / P)[:, None] * p / sigma[:, F:])
    grad_ref = data_terms.sum(axis=1) + ridge
    bound_c = (2 * F + 12) * U * 0.5 * np.abs(cost_terms).sum(axis=1)
    bound_g = (2 * F + 12) * U * (np.abs(data_terms).sum(axis=1) + np.abs(ridge))
    rc, rg = _ratio(np.abs(cost - cost_ref), bound_c), _ratio(np.abs(grad - grad_ref), bound_g)
    print(f"FIG cost_and_grad_rows {model} {n}: cost_ratio={rc:.3e} grad_ratio={rg:.3e} (entries where numpy's exp differs: {int((np.exp(p) != th_eff).sum()) if log_space else 0})")
    assert rc <= 1.0
    assert rg <= 1.0
    assert (ridge[[0, 3]] == 0.0).all() and (ridge[[1, 2, 4]] != 0.0).any()
