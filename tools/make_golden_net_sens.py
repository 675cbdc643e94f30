"""Write tests/golden/net_sens_m{0,1,2,4}_small.npz: the exact forward-sensitivity references of tests/net_sens_reference.py
(the oracle's tangent ODE under LSODA at 1e-12) for candidates 0..2 of the four small network fixtures, one column per parameter kind,
with the reference's own tolerance-halving self-consistency (the same integration at 1e-10).  CPU only; one process per candidate.

    python tools/make_golden_net_sens.py [jobs]
"""
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import net_sens_reference as ref  # noqa: E402


def one(job):
    name, k, tol = job
    g, net, X = ref.fixture(name)
    cols, _ = ref.columns_one_per_kind(net)
    Y, dY = ref.tangent_reference(net, X[k], cols, g["t_eval"], y0=g["y0"], rtol=tol, atol=tol)
    return name, k, tol, Y, dY


def main():
    jobs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    work = [(name, k, tol) for name in ref.NAMES for k in range(ref.N_CAND) for tol in (1e-12, 1e-10)]
    with ProcessPoolExecutor(max_workers=jobs) as ex:
        res = {(n, k, tol): (Y, dY) for n, k, tol, Y, dY in ex.map(one, work)}
    for name in ref.NAMES:
        g, net, X = ref.fixture(name)
        cols, names = ref.columns_one_per_kind(net)
        Y = np.stack([res[(name, k, 1e-12)][0] for k in range(ref.N_CAND)])
        dY = np.stack([res[(name, k, 1e-12)][1] for k in range(ref.N_CAND)])
        dY10 = np.stack([res[(name, k, 1e-10)][1] for k in range(ref.N_CAND)])
        self_err = np.abs(dY - dY10).max(axis=(1, 2))
        out = ROOT / "tests" / "golden" / (name.replace("network_", "net_sens_") + ".npz")
        np.savez_compressed(out, cols=cols, names=np.array(names), X=X, t=g["t_eval"], y0=g["y0"], Y=Y, dY=dY, self_err=self_err)
        rel = self_err / np.abs(dY).max(axis=(1, 2))
        print(f"{name}: max |dY(1e-12) - dY(1e-10)| / max|column| = {rel.max():.2e}  (per column, worst candidate: "
              + ", ".join(f"{n}={v:.1e}" for n, v in zip(names, rel.max(axis=0))) + ")", flush=True)


if __name__ == "__main__":
    main()
