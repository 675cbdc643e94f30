"""Where one generation of ``GlobalODEBatch.search`` spends its time (recorded, not gated; not a test).

Workload: ``netlarge_m0`` (N = 100, S = 552) with bench.py's config-5 loss data, bounds of +- 1 around the raw fixture candidate,
pop = 8192 from a Latin hypercube, rtol = atol = 1e-8.  What is timed is ``search.search`` itself, through its ``timer`` hook: a device
event where the launches of each phase have been queued -- evaluate (``evaluate_device`` on the offspring, unchanged by the search: the
baseline), rank, associate, survive, mate, and "torch" (concatenation, ideal / nadir reductions, the survivors' gather).  ``rank`` reads 4 bytes per front
on the host, so its figure includes those round trips.  One untimed warm-up generation (it also loads every code object and ramps the
clock through a full evaluation), then ``--gens`` timed ones; every generation is printed, the table holds their medians and ranges.

Where pymoo is installed its reference-direction survival (non-dominated sorting with ``n_stop_if_ranked``, normalisation, association,
niching) is timed on the host on the last two populations concatenated (2 pop rows, a merged population's size) for comparison; otherwise the output says that no host comparison was
possible.

    python tools/moo_generation_split.py [--pop 8192] [--gens 3] [--out build]              # measure: writes moo_generation_split.{json,md}
    python tools/moo_generation_split.py --design build/moo_generation_split.json           # no GPU: put the table into DESIGN.md 5.14
"""
import argparse
import json
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
PHASES = ("evaluate", "rank", "associate", "survive", "mate", "torch")
BEGIN, END = "<!-- moo-generation-split:begin -->", "<!-- moo-generation-split:end -->"


def problem():
    from phoskintime_amd.global_model import NetworkEngine
    from phoskintime_amd.global_model.optproblem import GlobalODEBatch
    g = np.load(ROOT / "tests" / "golden" / "netlarge_m0.npz")
    eng = NetworkEngine.from_npz(g)
    base = eng.pack_params(*(g[k][0] for k in ("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i", "tf_scale")))
    tn = g["t_eval"]
    rng = np.random.default_rng(20260515 + 4)
    lists, ld = eng.make_index_lists(tn, tn, tn[tn >= 4.0], tn)
    eng.free_loss(lists)
    for k in ("obs_prot", "obs_rna", "obs_pho"):
        ld[k] = np.abs(1.0 + 0.05 * rng.standard_normal(ld[k].size))
    defaults = dict(zip(("c_k", "A_i", "B_i", "C_i", "D_i", "Dp_i", "E_i"),
                        np.split(base[:-1], np.cumsum([eng.n_K, eng.N, eng.N, eng.N, eng.N, eng.total_sites]))))
    defaults["tf_scale"] = float(base[-1])
    raw0 = np.log(np.expm1(np.maximum(base, 1e-12)))
    return GlobalODEBatch(eng, None, ld, defaults, {"protein": 1.0, "rna": 1.0, "phospho": 1.0, "prior": 0.01}, tn, xl=raw0 - 1.0, xu=raw0 + 1.0,
                          rtol=1e-8, atol=1e-8)


def measure(pop, gens, seed):
    import torch
    from phoskintime_amd.global_model import search
    prob = problem()
    dev = torch.device("cuda", prob.eng.ctx.device)
    st = torch.cuda.current_stream(dev)
    marks, walls, last = [], [time.perf_counter()], {}           # marks: one list of (phase, event) per generation

    def timer(phase):
        if phase == "start":
            marks.append([])
        if marks:                                                 # the ticks of the start population come before the first "start"
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(st)
            marks[-1].append((phase, ev))

    def callback(gen, state):                                     # search has just read the generation's scalars: the stream is idle
        torch.cuda.synchronize(dev)
        walls.append(time.perf_counter())
        last.update(best_sum=float(state["F"].sum(dim=1).min().item()), prev=last.get("F"), F=state["F"])
        if gen == 0:
            walls[:] = [time.perf_counter()]

    res = search.search(prob, pop, gens + 1, seed, callback=callback, timer=timer)
    rows = []
    for g, (m, h) in enumerate(zip(marks, res.history[1:]), start=1):
        row = dict(gen=g, warmup=g == 1, **{p: 0.0 for p in PHASES}, wall=1e3 * (walls[g] - walls[g - 1]), fronts=h["fronts"], front0=h["front0"])
        for (_, e0), (phase, e1) in zip(m[:-1], m[1:]):
            row[phase] += e0.elapsed_time(e1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    # for the host comparison: the last two populations concatenated -- 2 pop rows, the size a host-side survival is handed per generation
    host = host_comparison(torch.cat([last["prev"], last["F"]], dim=0).cpu().numpy(), res.ref_dirs, pop)
    prob.close()
    return dict(workload=f"netlarge_m0 (N = {prob.eng.N}, S = {prob.eng.S}, n_var = {prob.n_var}), pop = {pop}, merged rows = {2 * pop}, "
                         f"H = {res.ref_dirs.shape[0]}, rtol = atol = 1e-8, bounds +- 1 around the raw fixture candidate",
                device=torch.cuda.get_device_properties(dev).gcnArchName.split(":")[0], generations=rows, host=host, best_sum=last.get("best_sum"))


def host_comparison(F, dirs, pop):
    try:
        import pymoo  # noqa: F401
    except ImportError:
        return dict(available=False, note="pymoo is not installed: no host comparison was possible")
    try:
        from pymoo.algorithms.moo.nsga3 import ReferenceDirectionSurvival
        from pymoo.core.population import Population
        from pymoo.core.problem import Problem
        surv = ReferenceDirectionSurvival(dirs)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            surv.do(Problem(n_var=1, n_obj=F.shape[1]), Population.new(F=F.copy()), n_survive=pop)
            times.append(1e3 * (time.perf_counter() - t0))
        return dict(available=True, survival_ms=times)
    except Exception as e:          # an API of another pymoo version: say so, the device figures stand on their own
        return dict(available=False, note=f"pymoo is installed but its survival could not be timed: {e!r}")


def table(res):
    timed = [r for r in res["generations"] if not r["warmup"]]
    med = {p: float(np.median([r[p] for r in timed])) for p in PHASES + ("wall",)}
    rng = {p: (min(r[p] for r in timed), max(r[p] for r in timed)) for p in PHASES + ("wall",)}
    new = sum(med[p] for p in ("rank", "associate", "survive", "mate"))
    out = [f"Measured on an {'MI355X (gfx950)' if res['device'] == 'gfx950' else res['device']}: {res['workload']}; {len(timed)} generations after one warm-up, device events, median (min .. max) ms.",
           "", "| phase | ms per generation | share of evaluate |", "|---|---|---|"]
    for p in PHASES:
        out.append(f"| {p} | {med[p]:.3f} ({rng[p][0]:.3f} .. {rng[p][1]:.3f}) | {med[p] / med['evaluate']:.4f} |")
    out.append(f"| rank + associate + survive + mate | {new:.3f} | {new / med['evaluate']:.4f} |")
    out.append(f"| host wall clock of the generation | {med['wall']:.3f} ({rng['wall'][0]:.3f} .. {rng['wall'][1]:.3f}) | |")
    out.append("")
    out.append("Fronts peeled per generation (one launch and one 4-byte read each): " + ", ".join(str(r["fronts"]) for r in timed) +
               "; rows of front 0 among the survivors: " + ", ".join(str(r["front0"]) for r in timed) + ".")
    h = res["host"]
    out.append("Host comparison: " + ("pymoo's ReferenceDirectionSurvival on the same merged F took " +
                                      " / ".join(f"{t:.1f}" for t in h["survival_ms"]) + " ms." if h.get("available") else h["note"] + "."))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=8192)
    ap.add_argument("--gens", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="build")
    ap.add_argument("--design", default=None, help="a moo_generation_split.json: write its table into DESIGN.md (no GPU needed)")
    a = ap.parse_args()
    if a.design:
        md = table(json.loads(Path(a.design).read_text()))
        p = ROOT / "DESIGN.md"
        txt = p.read_text()
        if BEGIN not in txt or END not in txt:
            raise SystemExit("DESIGN.md has no generation-split markers")
        p.write_text(re.sub(re.escape(BEGIN) + r".*?" + re.escape(END), lambda m: BEGIN + "\n" + md + "\n" + END, txt, flags=re.S))
        print(md)
        return
    res = measure(a.pop, a.gens, a.seed)
    out = Path(a.out); out.mkdir(parents=True, exist_ok=True)
    (out / "moo_generation_split.json").write_text(json.dumps(res, indent=1))
    md = table(res)
    (out / "moo_generation_split.md").write_text(md + "\n")
    print(md)


if __name__ == "__main__":
    main()
