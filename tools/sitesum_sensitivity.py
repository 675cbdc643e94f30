"""Dev tool (CPU): how far a rounding-sized change of the site sum moves the LRP12 trajectories of the distributive model.
Runs the numpy port of oracle/lrp8_dist.c kept in tests/test_gpu_dist_fast_sitesum.py on the benchmark's parameter distribution
(n = 30, theta ~ U(0, 20), y0 = 1, the 14-point grid, rtol 1e-6 / atol 1e-8), once as it is and once with every sum of the port
multiplied by 1 + eps * N(0, 1), and prints the largest band difference |dy| / (1e-8 + 1e-6 |y|) and the step-count differences.
usage: sitesum_sensitivity.py [replicas = 24]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import test_gpu_dist_fast_sitesum as ts  # noqa: E402

n, B = 30, int(sys.argv[1]) if len(sys.argv) > 1 else 24
theta = np.random.default_rng(20260515).uniform(0.0, 20.0, (B, 4 + 2 * n))
y0 = np.ones(n + 2)
base = [ts._lrp12_with_h0(th, n, y0, ts.T) for th in theta]
rng = np.random.default_rng(1)
exact = ts._seq
for eps in (1e-15, 1e-13, 1e-11):
    ts._seq = lambda x: exact(x) * (1.0 + eps * rng.standard_normal())
    pert = [ts._lrp12_with_h0(th, n, y0, ts.T) for th in theta]
    ts._seq = exact
    band = [float(np.max(np.abs(a[0] - b[0]) / (1e-8 + 1e-6 * np.abs(a[0])))) for a, b in zip(base, pert)]
    print("eps %.0e: band difference max %.3e median %.3e; replicas with another step count: %d of %d"
          % (eps, max(band), float(np.median(band)), sum(a[2] != b[2] for a, b in zip(base, pert)), B))
