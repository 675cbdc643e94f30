"""Wave pacing of the parked one-wave LRP12 distmod kernels (csrc/pk_dist_fast.hpp, PK_DIST_SCHED) only tells the SIMD's arbiter which wave
to prefer: it changes no arithmetic, so every policy must reproduce `off` bit for bit -- the int64 views of sol (or flat), metric, status and
n_steps, zero differing bit patterns.  The traced build of the benchmark's kernel (PK_DIST_TRACE=1) is held to the same, and its records
to what a timeline needs.

PK_DIST_SCHED and PK_DIST_TRACE are read once per process, so each setting runs in a fresh child process.  `off` runs first and writes
every output as .npy; the children of the other settings run side by side, write theirs, and also count the bit patterns in which each
of their arrays differs from the file `off` wrote (the trajectories are 110-220 MB per case: only `off` keeps them on disk, the others
keep the small arrays, which the tests compare themselves, and the counts)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
POLICIES = ("lead", "level", "lead+level")
# name -> (n_sites, B, what)
CASES = {
    "n30": (30, 50000, "sol+sum"),          # smallest grid beyond one round (3 072 resident waves x 16 replicas = 49 152): leaders and a second round of 53 waves
    "n30_row": (30, 48, "sol+sum"),         # three workgroups: the single-round path
    "n18": (18, 50000, "sol+sum"),          # 4 x 5 resident
    "n38": (38, 50000, "sol+sum"),          # 8 x 5 resident
    "n32": (32, 50000, "sol+sum"),          # 4 x 8 shadowed
    "n30_nan": (30, 50000, "nan"),          # one replica with a NaN in theta: the non-finite exit, with a priority set
    "n30_budget": (30, 50000, "budget"),    # max_steps = 5: the budget exit and the NaN rows
    "n30_flat": (30, 50000, "flat"),        # DistFlatOnly
    "n30_any": (30, 4096, "any"),           # DistAny through a metric of the full class
}
ARRAYS = ("sol", "flat", "metric", "status", "n_steps")

_CHILD = r"""
import json, sys
from pathlib import Path
import numpy as np
root, out, ref, trace = sys.argv[1], Path(sys.argv[2]), sys.argv[3], sys.argv[4] == "1"
sys.path[:0] = [root, root + "/tests"]
import torch
import test_gpu_dist_fast_sched as t
from oracle import protein_models as pm
from phoskintime_amd import batch
ctx = batch.get_context()
diff = {}
for name in ([k for k in t.CASES if k == "n30"] if trace else t.CASES):
    n, B, what = t.CASES[name]
    theta = np.random.default_rng(4100 + n).uniform(0.0, 20.0, (B, pm.n_params(pm.DIST, n)))
    kw = dict(kernel="group", metric="total_signal", want_flat=False)
    if what == "nan":
        theta[B // 2 + 3, 4 + 7] = np.nan
    elif what == "budget":
        kw["max_steps"] = 5
    elif what == "flat":
        kw = dict(kernel="group", want_flat=True, want_sol=False)
    elif what == "any":
        kw["metric"] = "variance"
    rec = None
    if trace:
        nblk = (B + 15) // 16
        rec = torch.zeros((nblk, 4), dtype=torch.int64, device="cuda")
        ctx.check(ctx.lib.pk_dist_trace_set(ctx.handle, rec.data_ptr(), nblk))
    res = batch.solve_ode_batch(pm.DIST, theta, np.ones(n + 2), n, pm.TIME_POINTS, **kw)
    torch.cuda.synchronize()
    if trace:
        ctx.check(ctx.lib.pk_dist_trace_set(ctx.handle, None, 0))
        np.save(out / (name + "_records.npy"), rec.cpu().numpy())
    for arr in t.ARRAYS:
        x = getattr(res, arr)
        if x is None:
            continue
        x = x.cpu().numpy()
        big = arr in ("sol", "flat")
        if ref == "-" or not big:
            np.save(out / (name + "_" + arr + ".npy"), x)
        if ref != "-":
            y = np.load(Path(ref) / (name + "_" + arr + ".npy"))
            v = (lambda a: a.view(np.int64) if a.dtype == np.float64 else a)
            diff[name + "_" + arr] = int(np.count_nonzero(v(x) != v(y))) if x.shape == y.shape else -1
(out / "diff.json").write_text(json.dumps(diff))
print("done")
"""


def _spawn(out, ref, env, trace=False):
    out.mkdir()
    return subprocess.Popen([sys.executable, "-c", _CHILD, str(ROOT), str(out), str(ref) if ref else "-", "1" if trace else "0"],
                            env={**{k: v for k, v in os.environ.items() if k not in ("PK_DIST_SCHED", "PK_DIST_TRACE")}, **env},
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _wait(p, what):
    log, _ = p.communicate(timeout=600)
    assert p.returncode == 0 and "done" in log, what + ":\n" + log[-4000:]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    base = tmp_path_factory.mktemp("sched")
    _wait(_spawn(base / "off", None, {"PK_DIST_SCHED": "off"}), "off")
    kids = {p: _spawn(base / p, base / "off", {"PK_DIST_SCHED": p}) for p in POLICIES}
    kids["trace"] = _spawn(base / "trace", base / "off", {"PK_DIST_TRACE": "1"}, trace=True)
    for name, p in kids.items():
        _wait(p, name)
    return base


def _bits(x):
    return x.view(np.int64) if x.dtype == np.float64 else x


@pytest.mark.gpu
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case", list(CASES))
def test_policy_has_the_bits_of_off(runs, case, policy):
    what = CASES[case][2]
    diff = json.loads((runs / policy / "diff.json").read_text())
    seen = 0
    for arr in ARRAYS:
        ref = runs / "off" / f"{case}_{arr}.npy"
        if not ref.exists():
            continue
        seen += 1
        assert diff[f"{case}_{arr}"] == 0, (case, policy, arr, diff[f"{case}_{arr}"])
        if arr not in ("sol", "flat"):
            a, b = np.load(ref), np.load(runs / policy / f"{case}_{arr}.npy")
            assert a.shape == b.shape and np.count_nonzero(_bits(a) != _bits(b)) == 0, (case, policy, arr)
    assert seen == (3 if what == "flat" else 4), (case, seen)


@pytest.mark.gpu
def test_cases_reach_the_paths_they_name(runs):
    """What `off` itself computed: healthy batches, the one NaN replica flagged non-finite with NaN rows, every replica out of budget."""
    off = runs / "off"
    for case in ("n30", "n30_row", "n18", "n38", "n32", "n30_any"):
        assert not np.load(off / f"{case}_status.npy").any() and np.isfinite(np.load(off / f"{case}_metric.npy")).all(), case
    st = np.load(off / "n30_nan_status.npy")
    bad = CASES["n30_nan"][1] // 2 + 3
    assert st[bad] == 1 and np.count_nonzero(st) == 1
    assert np.isnan(np.load(off / "n30_nan_sol.npy", mmap_mode="r")[bad, 1:]).all()
    st = np.load(off / "n30_budget_status.npy")
    assert (st == 2).all() and np.load(off / "n30_budget_n_steps.npy").sum(axis=1).max() == 5


@pytest.mark.gpu
def test_traced_kernel_records_and_bits(runs):
    n, B, _ = CASES["n30"]
    diff = json.loads((runs / "trace" / "diff.json").read_text())
    assert diff and all(v == 0 for v in diff.values()), diff
    rec = np.load(runs / "trace" / "n30_records.npy")
    nblk = (B + 15) // 16
    assert rec.shape == (nblk, 4)
    t_entry, t_exit = rec[:, 0], rec[:, 1]
    w = rec[:, 2:].copy().view(np.uint32).reshape(nblk, 4)            # block, hw_id, xcc_id, iterations
    assert (t_exit > t_entry).all()
    assert np.array_equal(np.sort(w[:, 0]), np.arange(nblk))
    simd = np.unique((w[:, 2].astype(np.int64) & 0xF) << 12 | (w[:, 1].astype(np.int64) >> 4) & 0xFFF)      # XCC | SE, SH, CU, SIMD
    assert 1 <= simd.size <= 1024, simd.size
    steps = np.load(runs / "trace" / "n30_n_steps.npy").sum(axis=1)
    per_wave = np.array([steps[16 * b:16 * b + 16].max() for b in range(nblk)])
    assert np.array_equal(w[:, 3], per_wave)                        # a wave runs as long as its slowest replica steps


@pytest.mark.gpu
def test_unknown_policy_is_rejected_before_a_launch():
    script = ("import sys; sys.path.insert(0, sys.argv[1])\nimport numpy as np\nfrom phoskintime_amd import batch\n"
              "from phoskintime_amd._capi import PhoskinError\n"
              "try:\n    batch.solve_ode_batch(0, np.ones((4, 64)), np.ones(32), 30, [0.0, 1.0], kernel='group')\n"
              "except PhoskinError as e:\n    print('rejected:', e)\n")
    r = subprocess.run([sys.executable, "-c", script, str(ROOT)], env={**os.environ, "PK_DIST_SCHED": "fastest"}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rejected:" in r.stdout and all(w in r.stdout for w in ("off", "lead", "level", "lead+level")), r.stdout + r.stderr[-2000:]


def test_policy_names_parse(built_lib):
    """Host side, no GPU: the values PK_DIST_SCHED takes, and that anything else is refused with the valid ones named."""
    parse = lambda s: built_lib.pk_dist_sched_parse(s.encode())
    names = built_lib.pk_dist_sched_names().decode()
    assert [w.strip() for w in names.split(",")] == ["off", "lead", "level", "lead+level"]
    off, lead, level, both = (parse(w) for w in ("off", "lead", "level", "lead+level"))
    assert off == 0 and lead > 0 and level > 0 and lead != level and both == lead | level and parse("level+lead") == both
    for bad in ("", "fastest", "lead+", "+level", "lead+lead", "off+lead", "LEAD", "lead + level", "1"):
        assert parse(bad) == -1, bad
    assert built_lib.pk_dist_sched_parse(None) == -1
