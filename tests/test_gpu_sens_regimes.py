"""GPU: every sensitivity kernel family behind pk_solve_protein_sens_batch against the oracle's EXACT derivative
(oracle.protein_models.sens_exact_lti) where the fits take it: rates on U(0, 20), log-uniform on 1e-8 .. 20, exact zeros (variables on the
lower bound of the box), a start at the steady state with fast rates (only the tangents move: the step controller must watch them), the
library's default tolerances, the kernels PK_SENS_ROWS forces, irregular grids, a non-zero start time, a forced first step and a step limit.

Sizes: the smallest that reach each code path.
  column kernel (csrc/pk_sens.hpp), its default range ........ distmod 1, 9; succmod 1, 5
  randmod in registers / LDS (CubeSys / CubeLdsSys) .......... 1, 3 / 4, 5
  rows kernel (csrc/pk_sens_rows.hpp), 16-lane groups ........ distmod 10 (first default size), 12 (P = 28 = 4 x 7: no partial chunk);
                                                               succmod 6 (first default size) -- S <= 16 states: 16 lanes by default too
  rows kernel, 32-lane groups ................................ distmod 19 (P = 42 = 6 x 7), 30 (P = 64: the last chunk holds one
                                                               column); succmod 30
  rows kernel, 64-lane groups ................................ distmod 31, 33 (P = 70 = 10 x 7), 62; succmod 31, 62
  csrc/pk_rand_sens.hpp ...................................... randmod 6, 7
For n >= 31 and randmod 6, 7 the reference is formed on a 5-point grid for a column subset: all of chunk 0 and of the last chunk, the first
and last column of every other chunk; every other column must be finite.

Measured on an MI355X (worst over the sizes of a family and replicas 0, B - 1; profiles/r14_a_sens_regimes_summary.txt has every family):
  rtol 1e-9 / atol 1e-11, |d - d_ref| / (1 + |d_ref|), limit 1e-7: U(0, 20) 5.9e-12, log-uniform 3.7e-10 (distmod 33), zeros 1.9e-11,
    steady start 2.7e-12; forced kernels 4.4e-12; t up to 1e5 3.5e-10, intervals down to 1e-6 8.8e-16.
  default tolerances, tangent band error max |d - d_ref| / (1e-8 + 1e-6 |d_ref|), limit 1: U(0, 20) 4.0e-3, log-uniform 0.14 (succmod
    30), zeros 2.3e-2, steady start 2.4e-3 -- the states of the same runs: 1.8e-2, 1.6e-2, 1.1e-2, 1.6e-8.  No family exceeds the band.
  Before the derivative rows of states within atol of 0 were kept (csrc/pk_sens_out.hpp, sens_post_entry), the zeros regime missed both limits in every
  family: 0.01 .. 1.0 in the first metric, 1e6 band units (a row of zeros against a derivative of order 1).
"""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import protein_models as pm

pytestmark = pytest.mark.gpu

SENS_RTOL = 1e-7          # tests/test_gpu_sens.py: |d - d_ref| <= SENS_RTOL (1 + |d_ref|) at rtol 1e-9 / atol 1e-11
TIGHT = dict(rtol=1e-9, atol=1e-11)
DEFAULT = {}              # the library's defaults (rtol 1e-6 / atol 1e-8): what the fits run at
KT = 7                    # tangent columns per chunk in the chunked kernels (kSensRowsKC - 1, kRandSensKC - 1)
GRID5 = np.array([0.0, 0.5, 4.0, 60.0, 960.0])

FAMILIES = {
    "column": [("distmod", 1), ("distmod", 9), ("succmod", 1), ("succmod", 5)],
    "cube": [("randmod", 1), ("randmod", 3), ("randmod", 4), ("randmod", 5)],
    "rows16": [("distmod", 10), ("distmod", 12), ("succmod", 6)],
    "rows32": [("distmod", 19), ("distmod", 30), ("succmod", 30)],
    "rows64": [("distmod", 31), ("distmod", 33), ("distmod", 62), ("succmod", 31), ("succmod", 62)],
    "randsens": [("randmod", 6), ("randmod", 7)],
}
SIZES = [s for fam in FAMILIES.values() for s in fam]
FAMILY_OF = {s: name for name, fam in FAMILIES.items() for s in fam}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from phoskintime_amd import batch
    batch.get_context()
    return batch


def _subset(model, n):
    return (model != "randmod" and n >= 31) or (model == "randmod" and n >= 6)


def _chunks(P):
    return [np.arange(c, min(c + KT, P)) for c in range(0, P, KT)]


def _cols(model, n):
    """Columns compared with the reference: all of them, or for the large sizes all of chunk 0 and of the last chunk and the first and
    last column of every other chunk."""
    P = pm.n_params(pm.MODEL_IDS[model], n)
    if not _subset(model, n):
        return np.arange(P)
    ch = _chunks(P)
    keep = [ch[0], ch[-1]] + [c[[0, -1]] for c in ch[1:-1]]
    return np.unique(np.concatenate(keep))


def _grid(model, n):
    return GRID5 if _subset(model, n) else pm.TIME_POINTS


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


REF_MAX = 1e6             # largest derivative the double-precision reference is trusted with (_case): it was off by 1.8e-14 x its largest
                          # entry on the draw that showed it, which 1e6 keeps five times below SENS_RTOL


def _exact(model, n, th, y0, t, cols):
    mid = pm.MODEL_IDS[model]
    sol, dsol = pm.sens_exact_lti(mid, th, y0, n, t, cols=cols)
    return _freeze(*pm.flat_and_jacobian(mid, sol, dsol, y0, n))


@functools.lru_cache(maxsize=None)
def _case(model, n, regime):
    """(theta [B, P], y0, {replica: (flat [F], dflat [F, len(cols)])} for replicas 0 and B - 1): drawn and computed once, shared by every
    test, never written.  A draw whose exact derivative exceeds REF_MAX anywhere is drawn again: with rates near 1e-8 the derivatives grow
    like t^3 (distmod n = 1, first log-uniform draw: 3.5e9), and scipy's Frechet derivative then leaves entries that are 0 or small short of
    SENS_RTOL by rounding alone -- on that draw it is 6.3e-5 from a 60-digit evaluation of the block exponential, and 4.8e-5 from the same
    construction in double precision, while the column kernel is within 1.3e-12 of the 60 digits.  The rule looks at the reference only."""
    mid = pm.MODEL_IDS[model]
    S = pm.n_states(mid, n)
    B = 5 if S <= 64 else 2                             # not a multiple of the replicas per wave: the last wave carries shadow groups
    for attempt in range(20):
        rng = np.random.default_rng([mid, n, pm.SENS_REGIMES.index(regime), attempt])
        th, y0 = pm.sens_regime(regime, mid, n, rng, B)
        ref = {b: _exact(model, n, th[b], y0[b] if y0.ndim == 2 else y0, _grid(model, n), _cols(model, n)) for b in (0, B - 1)}
        if max(np.abs(r[1]).max() for r in ref.values()) <= REF_MAX:
            return th, y0, ref
    raise AssertionError("no draw with derivatives below REF_MAX")


def _inputs(model, n, regime):
    return _case(model, n, regime)[:2]


def _reference(model, n, regime):
    return _case(model, n, regime)[2]


def _sens_err(d, ref):
    return float(np.max(np.abs(d - ref) / (1.0 + np.abs(ref))))


def _run(eng, model, n, regime, opts):
    th, y0 = _inputs(model, n, regime)
    r = eng.solve_ode_sens_batch(model, th, y0, n, _grid(model, n), **opts)
    return r.status.cpu().numpy(), r.flat.cpu().numpy(), r.dflat.cpu().numpy()


def _figures(tag, model, n, regime, flat, dflat):
    """Worst state band error, tangent error in the (1 + |d|) metric and tangent band error over replicas 0 and B - 1, printed before
    anything is asserted on them."""
    th, _ = _inputs(model, n, regime)
    cols = _cols(model, n)
    ref = _reference(model, n, regime)
    fb = max(pm.band_error(flat[b], ref[b][0]) for b in ref)
    se = max(_sens_err(dflat[b][:, cols], ref[b][1]) for b in ref)
    tb = max(pm.band_error(dflat[b][:, cols], ref[b][1]) for b in ref)
    lg = max(_sens_err(dflat[b][:, cols] * th[b][None, cols], ref[b][1] * th[b][None, cols]) for b in ref)
    print(f"FIG {tag} {FAMILY_OF[(model, n)]} {model} {n} {regime}: flat_band={fb:.3e} sens_err={se:.3e} tangent_band={tb:.3e} log_sens_err={lg:.3e}")
    return fb, se, tb, lg


@pytest.mark.parametrize("regime", ["uniform", "loguniform", "zeros"])
@pytest.mark.parametrize("model,n", SIZES)
def test_regimes_of_the_fits_at_tight_tolerance(eng, model, n, regime):
    """U(0, 20), log-uniform 1e-8 .. 20 and U(0, 20) with 30 % exact zeros at rtol 1e-9 / atol 1e-11: unflagged, flat within 0.1 band of
    the closed form, dflat within SENS_RTOL of the exact derivative -- and for randmod also dflat * theta, the log-space Jacobian its
    fits use."""
    st, flat, dflat = _run(eng, model, n, regime, TIGHT)
    fb, se, _, lg = _figures("tight", model, n, regime, flat, dflat)
    assert not st.any()
    assert np.isfinite(dflat).all()
    assert fb < 0.1
    assert se < SENS_RTOL
    if model == "randmod":
        assert lg < SENS_RTOL


@pytest.mark.parametrize("tol", ["default", "tight"])
@pytest.mark.parametrize("model,n", SIZES)
def test_steady_start_is_controlled_by_the_tangents(eng, model, n, tol):
    """y0 = y*(theta), theta ~ U(2, 20): the states stay where they are, so a controller that looked at them alone would take the first
    interval [0, 0.5] in a few long steps; the tangents have transients at rate ~ 20 there and are right only if the kernel holds its
    steps to them.  Asserted on the reference, not on the kernel: the states do not move and the tangents reach 1e-2.  Not in every chunk,
    nor in every replica: these inputs cannot give that -- the steady state thins out along a chain or up the cube, and the 5-point grid
    of the large sizes has no R block (succmod n = 62: 3e-24 in the last chunk, randmod n = 5: 3e-6, distmod n = 62: 1e-4 there and 3e-3
    in chunk 0 of replica 0).  Chunks that hold only such columns are compared like the others but discriminate less; their number is
    printed."""
    mid = pm.MODEL_IDS[model]
    th, y0 = _inputs(model, n, "steady")
    ref = _reference(model, n, "steady")
    cols = _cols(model, n)
    T = _grid(model, n).size
    largest = 0.0
    for b in ref:
        const = pm.flatten_observables(mid, np.repeat(y0[b][None, :], T, axis=0), n)
        assert pm.band_error(ref[b][0], const) < 1e-3                                   # the reference itself does not move
        size = [np.abs(ref[b][1][:, np.isin(cols, ch)]).max() for ch in _chunks(th.shape[1])]
        print(f"FIG steady-reference {model} {n} b={b}: {sum(s >= 1e-2 for s in size)} of {len(size)} chunks reach 1e-2, smallest {min(size):.1e}")
        largest = max(largest, max(size))
    assert largest >= 1e-2
    st, flat, dflat = _run(eng, model, n, "steady", TIGHT if tol == "tight" else DEFAULT)
    fb, se, tb, _ = _figures(tol, model, n, "steady", flat, dflat)
    assert not st.any()
    assert np.isfinite(dflat).all()
    for b in ref:
        const = pm.flatten_observables(mid, np.repeat(y0[b][None, :], _grid(model, n).size, axis=0), n)
        assert pm.band_error(flat[b], const) < 0.1
    if tol == "tight":
        assert se < SENS_RTOL
    else:
        assert tb <= 1.0


@pytest.mark.parametrize("regime", pm.SENS_REGIMES)
@pytest.mark.parametrize("model,n", SIZES)
def test_tangents_hold_the_band_at_default_tolerances(eng, model, n, regime):
    """The tolerances the fits run at (rtol 1e-6 / atol 1e-8).  include/phoskin.h: "Tangents are held to the same rtol / atol as the states"
    -- so the parity gate of BASELINE.json, max |d - d_ref| / (1e-8 + 1e-6 |d_ref|) <= 1, is applied to dflat as it is to flat."""
    st, flat, dflat = _run(eng, model, n, regime, DEFAULT)
    fb, _, tb, _ = _figures("default", model, n, regime, flat, dflat)
    assert not st.any()
    assert np.isfinite(dflat).all()
    assert fb <= 1.0
    assert tb <= 1.0


# ------------------------------------------------------------------------------------------------ forced kernels (child processes)
_FORCED = {"2": [("distmod", 10), ("distmod", 14), ("succmod", 6), ("succmod", 14)],       # the column kernel where it is no longer the default
           "1": [("distmod", 1), ("distmod", 9), ("succmod", 1), ("succmod", 5)]}          # the 16-lane rows kernel below its default range

_FORCED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from phoskintime_amd import batch
inp = np.load(sys.argv[2])
out = {}
for key in inp["keys"]:
    model, n, regime = key.split("_")
    r = batch.solve_ode_sens_batch(model, inp[key + "_th"], inp[key + "_y0"], int(n), inp["t"], rtol=1e-9, atol=1e-11)
    out[key + "_flat"] = r.flat.cpu().numpy(); out[key + "_dflat"] = r.dflat.cpu().numpy(); out[key + "_status"] = r.status.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize("rows_env", ["2", "1"])
def test_forced_kernels_against_the_exact_derivative(eng, tmp_path, rows_env):
    """PK_SENS_ROWS=2 runs the column kernel at distmod 10 .. 14 / succmod 6 .. 14, PK_SENS_ROWS=1 the 16-lane rows kernel below distmod 10 / succmod 6: the
    switch is read once per process, so a fresh child computes and this process compares -- with the exact derivative at SENS_RTOL (U(0, 20)
    and the steady start, tight tolerance), and with its own default kernel, whose bits the forced one must not reproduce."""
    cases = [(m, n, regime) for m, n in _FORCED[rows_env] for regime in ("uniform", "steady")]
    inp = {"keys": np.array([f"{m}_{n}_{regime}" for m, n, regime in cases]), "t": pm.TIME_POINTS}
    for m, n, regime in cases:
        th, y0 = _inputs(m, n, regime)
        inp[f"{m}_{n}_{regime}_th"], inp[f"{m}_{n}_{regime}_y0"] = th, y0
    np.savez(tmp_path / "in.npz", **inp)
    root = str(Path(__file__).resolve().parents[1])
    subprocess.run([sys.executable, "-c", _FORCED_SCRIPT, root, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], check=True,
                   env=dict(os.environ, PK_SENS_ROWS=rows_env), timeout=300)
    out = np.load(tmp_path / "out.npz")
    for m, n, regime in cases:
        key = f"{m}_{n}_{regime}"
        th, y0 = _inputs(m, n, regime)
        flat, dflat = out[key + "_flat"], out[key + "_dflat"]
        assert not out[key + "_status"].any(), key
        worst_f = worst_d = 0.0
        for b, (ref_f, ref_d) in _reference(m, n, regime).items():          # n <= 14: the 14-point grid, every column
            worst_f = max(worst_f, pm.band_error(flat[b], ref_f)); worst_d = max(worst_d, _sens_err(dflat[b], ref_d))
        print(f"FIG forced PK_SENS_ROWS={rows_env} {key}: flat_band={worst_f:.3e} sens_err={worst_d:.3e}")
        assert worst_f < 0.1, key
        assert worst_d < SENS_RTOL, key
        if "PK_SENS_ROWS" not in os.environ:
            own = eng.solve_ode_sens_batch(m, th, y0, n, pm.TIME_POINTS, **TIGHT).dflat.cpu().numpy()
            assert not np.array_equal(own, dflat), key                                  # another kernel ran in the child


# ------------------------------------------------------------------------------------------------ grids and options
OPTION_SIZES = [("distmod", 4), ("distmod", 30), ("succmod", 31), ("randmod", 4), ("randmod", 6)]


@functools.lru_cache(maxsize=None)
def _option_inputs(model, n):
    mid = pm.MODEL_IDS[model]
    rng = np.random.default_rng([7, mid, n])
    return rng.uniform(0.05, 5.0, size=(3, pm.n_params(mid, n))), rng.uniform(0.3, 1.5, size=pm.n_states(mid, n))


@pytest.mark.parametrize("grid", ["longt", "shortt"])
@pytest.mark.parametrize("model,n", OPTION_SIZES)
def test_very_long_and_very_short_grids(eng, model, n, grid):
    """The "longt" / "shortt" grids of tests/test_gpu_parity.py: five decades of interval lengths up to t = 1e5, and intervals down to 1e-6
    (the first step comes out of the interval, not of the controller)."""
    t = {"longt": np.array([0.0, 1.0, 1e2, 1e4, 1e5]), "shortt": np.array([0.0, 1e-6, 1e-4, 1e-2])}[grid]
    th, y0 = _option_inputs(model, n)
    cols = _cols(model, n)
    r = eng.solve_ode_sens_batch(model, th, y0, n, t, **TIGHT)
    flat, dflat = r.flat.cpu().numpy(), r.dflat.cpu().numpy()
    assert not r.status.cpu().numpy().any() and np.isfinite(dflat).all()
    for b in (0, 2):
        ref_f, ref_d = _exact(model, n, th[b], y0, t, cols)
        fb, se = pm.band_error(flat[b], ref_f), _sens_err(dflat[b][:, cols], ref_d)
        print(f"FIG {grid} {model} {n} b={b}: flat_band={fb:.3e} sens_err={se:.3e}")
        assert fb < 0.1
        assert se < SENS_RTOL


@pytest.mark.parametrize("model,n", OPTION_SIZES)
def test_nonzero_start_time(eng, model, n):
    """Autonomous system: only differences of the grid matter, for the tangents as for the states."""
    th, y0 = _option_inputs(model, n)
    t = np.array([0.0, 0.5, 4.0, 60.0])
    a = eng.solve_ode_sens_batch(model, th, y0, n, t)
    b = eng.solve_ode_sens_batch(model, th, y0, n, t + 10.0)
    assert not a.status.cpu().numpy().any() and not b.status.cpu().numpy().any()
    np.testing.assert_allclose(b.flat.cpu().numpy(), a.flat.cpu().numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b.dflat.cpu().numpy(), a.dflat.cpu().numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("model,n", OPTION_SIZES)
def test_forced_first_step_is_honoured(eng, model, n):
    """h0 = 10 on a first interval of 20: the first attempt is a step of 10, which no replica can accept at 1e-9 with rates up to 5 --
    every replica rejects at least once, and the controller recovers to the same accuracy."""
    th, y0 = _option_inputs(model, n)
    t = np.array([0.0, 20.0, 60.0, 960.0])
    cols = _cols(model, n)
    r = eng.solve_ode_sens_batch(model, th, y0, n, t, h0=10.0, **TIGHT)
    free = eng.solve_ode_sens_batch(model, th, y0, n, t, **TIGHT)
    assert not r.status.cpu().numpy().any()
    assert (r.n_steps.cpu().numpy()[:, 1] >= 1).all()
    assert not np.array_equal(r.n_steps.cpu().numpy(), free.n_steps.cpu().numpy())         # the option reached the kernel
    flat, dflat = r.flat.cpu().numpy(), r.dflat.cpu().numpy()
    assert np.isfinite(dflat).all()
    for b in (0, 2):
        ref_f, ref_d = _exact(model, n, th[b], y0, t, cols)
        assert pm.band_error(flat[b], ref_f) < 0.1
        assert _sens_err(dflat[b][:, cols], ref_d) < SENS_RTOL


@pytest.mark.parametrize("model,n", OPTION_SIZES)
def test_step_limit_flags_every_replica_and_leaves_no_trace(eng, model, n):
    """max_steps = 5 on the 14-point grid (13 intervals): PK_ST_MAXSTEPS on every replica, the rows written at t0 finite and zero, NaN
    at the last time point in the columns of every chunk, and the next default call unaffected, bit for bit."""
    from phoskintime_amd._capi import ST_MAXSTEPS
    mid = pm.MODEL_IDS[model]
    th, y0 = _option_inputs(model, n)
    t = pm.TIME_POINTS
    T = t.size
    before = eng.solve_ode_sens_batch(model, th, y0, n, t)
    cut = eng.solve_ode_sens_batch(model, th, y0, n, t, max_steps=5)
    after = eng.solve_ode_sens_batch(model, th, y0, n, t)
    assert not before.status.cpu().numpy().any()
    assert ((cut.status.cpu().numpy() & ST_MAXSTEPS) != 0).all()
    d = cut.dflat.cpu().numpy()
    at_t0 = [T - 5] + [T - 5 + T + j * T for j in range(n)]                      # P(t0) and the sites at t0
    at_end = [T - 6, T - 5 + T - 1] + [T - 5 + T + j * T + T - 1 for j in range(n)]      # R, P and the sites at the last time point
    assert np.all(d[:, at_t0, :] == 0.0)
    assert np.isnan(d[:, at_end, :]).all()
    assert np.isnan(cut.flat.cpu().numpy()[:, at_end]).all()
    assert np.array_equal(after.dflat.cpu().numpy(), before.dflat.cpu().numpy()) and np.array_equal(after.flat.cpu().numpy(), before.flat.cpu().numpy())
    assert np.array_equal(after.status.cpu().numpy(), before.status.cpu().numpy()) and np.array_equal(after.n_steps.cpu().numpy(), before.n_steps.cpu().numpy())
