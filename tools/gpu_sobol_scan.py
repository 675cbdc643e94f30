"""Time of the three phases of the temporal Sobol' analysis -- design, simulate + measure, indices -- one JSON line per shape (dev tool,
run on an MI355X under a timeout; not a test, and bench.py does not call it).

  python tools/gpu_sobol_scan.py [netlarge_m0] [small] [--repeats R] [--samples N] [--resamples R] [--cpu-row-seconds S]

netlarge_m0 : tests/golden/netlarge_m0.npz (N = 100, S = 552), the reference's problem (vary=None: every c_k plus E_i of every TF),
              n_samples 128, 100 resamples, the reference's time grid (T = 7); fused measurement (order-3 method, LDS kernel)
small       : tests/golden/network_m0_small.npz, same settings

The phases are those of ``temporal_gsa_batch``, restated here so that each can stand between two HIP events on the current stream, after
one warm-up launch of each on the full shape:
  design    : ``sobol.sample_device`` + the scatter into copies of the packed vector (the host's Sobol' draw is outside the events; its
              wall time is reported separately)
  simulate  : ``simulate_measure_batch(want_pred=True)`` + the zeroing of flagged rows / non-finite entries
  indices   : ``sobol.indices_device`` (column statistics, sums, spread)
Reported: the median of R runs (default 5) per phase in ms, min and max; rows / s of the simulate phase; the bytes the index kernels must
read -- Y once for the column statistics plus ceil((R + 1) / 8) times for the sums, and the per-resample workspace once -- against the
time; and, only when ``--cpu-row-seconds`` gives a figure for ONE CPU ``simulate_and_measure`` row, that figure x N_prot x N (D + 2) rows
as the reference's cost, labelled an extrapolation (the project's records hold no such figure for a network row)."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from phoskintime_amd.global_model import NetworkEngine  # noqa: E402
from phoskintime_amd.global_model.simulate import measure_tolerances  # noqa: E402
from phoskintime_amd.sensitivity import sobol  # noqa: E402

TIMES = np.array([0.0, 5.0, 15.0, 30.0, 60.0, 90.0, 120.0])
SLOTS = 8                                                    # kSlots of csrc/pk_sobol.hip


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def leg(case, g, k, n_samples, n_res, repeats, cpu_row_s):
    eng = NetworkEngine.from_npz(g)
    center = eng.pack_params(*(g[n][k] for n in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i")), float(g["tf_scale"][k]))
    vidx = np.concatenate([np.arange(eng.n_K), eng.n_K + 4 * eng.N + eng.total_sites + np.unique(g["TF_indices"])]).astype(np.int64)
    problem = {"num_vars": int(vidx.size), "bounds": [[0.5 * v, 1.5 * v] for v in center[vidx]]}
    D, T = int(vidx.size), TIMES.size
    tol = measure_tolerances(eng)
    lists, ld = eng.make_index_lists(TIMES, TIMES, [], [])
    counts = torch.as_tensor(sobol.resample_counts(n_samples, n_res, 0), device="cuda") if n_res else None
    cd, vd = torch.as_tensor(center, device="cuda"), torch.as_tensor(vidx, device="cuda")
    host = {}

    def design():
        t0 = time.perf_counter()
        Xv, h = sobol.sample_device(problem, n_samples, seed=0)
        host["draw_s"] = time.perf_counter() - t0
        Xd = cd.repeat(Xv.shape[0], 1)
        Xd[:, vd] = Xv
        return Xd, h

    def simulate(Xd):
        out = eng.simulate_measure_batch(lists, Xd, TIMES, max_steps=5000 * T, eps=1e-12, want_pred=True, method="rosw", kernel="lds", **tol)
        if out is None:
            raise RuntimeError("refused: " + (eng.ctx.lib.pk_last_error(eng.ctx.handle) or b"").decode())
        _, pred, status, nst, _ = out
        pred = torch.nan_to_num(torch.where((status != 0)[:, None], torch.zeros_like(pred), pred), nan=0.0, posinf=0.0, neginf=0.0)
        return pred, status, nst

    Xd, h = design(); pred, status, nst = simulate(Xd); sobol.indices_device(h, pred, counts)      # warm-up: code objects, scratch arena, allocator
    torch.cuda.synchronize()
    ms = {"design": [], "simulate": [], "indices": []}
    for _ in range(repeats):
        (Xd, h), dt = _events(design); ms["design"].append(dt)
        (pred, status, nst), dt = _events(lambda: simulate(Xd)); ms["simulate"].append(dt)
        _, dt = _events(lambda: sobol.indices_device(h, pred, counts)); ms["indices"].append(dt)
    B, M = int(pred.shape[0]), int(pred.shape[1])
    y_bytes = 8 * B * M
    passes = -(-(n_res + 1) // SLOTS)
    read = y_bytes * (1 + passes) + 2 * 8 * n_res * D * M
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(case=case, N_prot=eng.N, S=eng.S, D=D, T=T, n_samples=n_samples, resamples=n_res, rows=B, M=M, tol=tol,
               median_ms={k: round(v, 3) for k, v in med.items()}, min_ms={k: round(min(v), 3) for k, v in ms.items()},
               max_ms={k: round(max(v), 3) for k, v in ms.items()}, host_draw_ms=round(1e3 * host["draw_s"], 2),
               rows_per_s=round(B / (1e-3 * med["simulate"]), 1), flagged=int((status != 0).sum()),
               mean_steps=[round(float(v), 2) for v in nst.double().mean(dim=0).cpu()],
               indices_bytes_read=int(read), indices_Y_bytes=int(y_bytes), indices_Y_passes=1 + passes,
               indices_GBps=round(read / (1e-3 * med["indices"]) / 1e9, 1))
    if cpu_row_s is not None:
        res["cpu_extrapolation_s"] = round(cpu_row_s * eng.N * B, 1)
        res["cpu_extrapolation_note"] = f"{cpu_row_s} s per CPU row (given on the command line) x N_prot x rows: an extrapolation, not a measurement"
    print(json.dumps(res), flush=True)
    eng.free_loss(lists)
    eng.close()


def main(argv):
    repeats, n_samples, n_res, cpu_row_s, cases = 5, 128, 100, None, []
    it = iter(argv)
    for a in it:
        if a == "--repeats":
            repeats = int(next(it))
        elif a == "--samples":
            n_samples = int(next(it))
        elif a == "--resamples":
            n_res = int(next(it))
        elif a == "--cpu-row-seconds":
            cpu_row_s = float(next(it))
        else:
            cases.append(a)
    for case in cases or ["netlarge_m0", "small"]:
        name, k = ("netlarge_m0", 0) if case == "netlarge_m0" else ("network_m0_small", 1)
        leg(case, np.load(ROOT / "tests" / "golden" / f"{name}.npz"), k, n_samples, n_res, repeats, cpu_row_s)


if __name__ == "__main__":
    main(sys.argv[1:])
