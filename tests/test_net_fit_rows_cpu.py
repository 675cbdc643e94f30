"""CPU: the least-squares form of the network objective that pk_network_fit_batch minimises (csrc/pk_net_fit.hpp) -- residual scales, prior
rows and their derivative, cost = 1/2 obj_w . F, and the packed-entry map of the normal-equations kernel -- compiled with csrc/pk_lm.hpp
under g++ into a stand-alone program (its own main, nothing loaded into Python), held to long-double numpy, and built and run once more
under the address and undefined-behaviour sanitizers.

``test_half_r2_and_half_w_F_differ_by_the_unfitted_prior``: on the stored exact Y / dY of ``network_m0_small`` the residual rows formed
with the program's scales give 1/2 |r|^2 = 1/2 obj_w . F - 1/2 (sum obj_w) lambda_prior (sum over UNFITTED prior entries d^2) / (5 N),
F from ``net_objgrad_reference.chain``.  Bound: every term of either side is a product of at most 6 factors (obj_w, norm, lambda, w and the
squared difference; the square root and its square: 2 u) summed over n_obs + 5 N terms: (n_obs + 5 N + 12) 2^-53 sum |terms|."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import net_objgrad_reference as og

CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"
LD = np.longdouble
U = 2.0 ** -53

# one request per input line, one %.17g answer (or several) per output line
MAIN = r"""
#include <cstdio>
#include <cstring>
#include "pk_lm.hpp"
#include "pk_net_fit.hpp"
using namespace pk;
int main() {
  char op[16];
  while (std::scanf("%15s", op) == 1) {
    if (!std::strcmp(op, "scale")) {
      double a, b, c, d;
      if (std::scanf("%lf %lf %lf %lf", &a, &b, &c, &d) != 4) return 2;
      std::printf("%.17g\n", nf_obs_scale(a, b, c, d));
    } else if (!std::strcmp(op, "prior")) {            // obj_w[3] lam N raw x d -> scale row drow
      double w[3], lam, x, d; int N, raw;
      if (std::scanf("%lf %lf %lf %lf %d %d %lf %lf", &w[0], &w[1], &w[2], &lam, &N, &raw, &x, &d) != 8) return 2;
      const double sp = nf_prior_scale(w, lam, N);
      std::printf("%.17g %.17g %.17g\n", sp, nf_prior_row(sp, raw ? nf_softplus(x) : x, d), nf_prior_drow(sp, d, raw ? nf_softplus_prime(x) : 1.0));
    } else if (!std::strcmp(op, "cost")) {
      double F[3], w[3];
      if (std::scanf("%lf %lf %lf %lf %lf %lf", &F[0], &F[1], &F[2], &w[0], &w[1], &w[2]) != 6) return 2;
      std::printf("%.17g\n", nf_cost(F, w));
    } else if (!std::strcmp(op, "col")) {
      int c, nK, N, s;
      if (std::scanf("%d %d %d %d", &c, &nK, &N, &s) != 4) return 2;
      std::printf("%d\n", nf_prior_col(c, nK, N, s) ? 1 : 0);
    } else if (!std::strcmp(op, "entries")) {          // K -> every (i, j) of the packed entries, in order
      int K;
      if (std::scanf("%d", &K) != 1) return 2;
      std::printf("%zu", nf_entries(K));
      for (size_t e = 0; e < nf_entries(K); ++e) { int i, j; nf_entry(K, e, &i, &j); std::printf(" %d %d", i, j); if (lm_tri(K + 1, i, j) != e) return 3; }
      std::printf("\n");
    } else return 4;
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("pk_net_fit")
    (d / "main.cpp").write_text(MAIN)
    (d / "only.cpp").write_text('#include "pk_net_fit.hpp"\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{CSRC}", str(d / "only.cpp")], check=True)      # stands alone: no HIP header
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", f"-I{CSRC}", str(d / "main.cpp"), "-o", str(d / "rows")], check=True)
    return d


def ask(exe, lines):
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return [[float(v) for v in ln.split()] for ln in r.stdout.splitlines()]


def requests(rng):
    """Request lines with the long-double answers they must meet and the units in the last place each may be off by."""
    lines, want, ulps = [], [], []
    for _ in range(40):
        a, b, c, d = rng.uniform(0.0, 3.0), 1.0 / rng.uniform(1.0, 300.0), rng.uniform(0.0, 2.0), rng.uniform(0.5, 2.0)
        lines.append(f"scale {a!r} {b!r} {c!r} {d!r}")
        want.append([np.sqrt(LD(a) * LD(b) * LD(c) * LD(d))]); ulps.append(4)                # three products, one root: 3.5 u
    for k in range(40):
        w = [float(v) for v in rng.uniform(0.0, 2.0, 3)]; lam = rng.uniform(0.0, 1.0); N = int(rng.integers(1, 200)); raw = k % 2
        x = rng.uniform(-3.0, 25.0) if raw else rng.uniform(0.01, 5.0); d = rng.uniform(0.01, 5.0)
        lines.append(f"prior {w[0]!r} {w[1]!r} {w[2]!r} {lam!r} {N} {raw} {x!r} {d!r}")
        sp = np.sqrt((LD(w[0]) + LD(w[1]) + LD(w[2])) * LD(lam) / LD(5 * N))
        p = (LD(x) if x > 20.0 else np.log1p(np.exp(LD(x)))) if raw else LD(x)
        dsoft = (LD(1) if x > 20.0 else LD(1) / (LD(1) + np.exp(-LD(x)))) if raw else LD(1)
        # the row carries (p - d): its absolute error is 2 u (|p| + |d|) from softplus and the difference; stated in units of the row
        row = sp * ((p - LD(d)) / (LD(d) + LD(1e-6)))
        cancel = float((abs(p) + abs(LD(d))) / max(abs(p - LD(d)), LD(1e-300)))
        want.append([sp, row, sp / (LD(d) + LD(1e-6)) * dsoft]); ulps.append([5, 8 + 4 * cancel, 12])
    for _ in range(40):
        F, w = rng.uniform(0.0, 50.0, 3), rng.uniform(0.0, 2.0, 3)
        lines.append("cost " + " ".join(repr(float(v)) for v in (*F, *w)))
        want.append([LD(0.5) * (LD(w[0]) * LD(F[0]) + LD(w[1]) * LD(F[1]) + LD(w[2]) * LD(F[2]))]); ulps.append(5)
    return lines, want, ulps


def check_requests(exe):
    lines, want, ulps = requests(np.random.default_rng(11))
    got = ask(exe, lines)
    assert len(got) == len(want)
    for ln, g, w, u in zip(lines, got, want, ulps):
        for q, (gv, wv) in enumerate(zip(g, w)):
            uu = u[q] if isinstance(u, list) else u
            assert abs(LD(gv) - wv) <= uu * U * max(abs(wv), LD(1e-300)), (ln, q, gv, float(wv))
    # the cost is the twin's expression bit for bit: each operation rounded once, no fused multiply-add
    from phoskintime_amd.global_model.polish import cost_of
    for ln, g in zip(lines, got):
        if ln.startswith("cost"):
            v = [float(s) for s in ln.split()[1:]]
            assert g[0] == float(cost_of(np.array(v[:3]), v[3:]))
    # prior columns: A, B, C, D, E carry one, c_k, Dp and tf_scale do not
    nK, N, sites = 3, 6, 8
    cols = list(range(nK + 5 * N + sites + 1))
    got = ask(exe, [f"col {c} {nK} {N} {sites}" for c in cols])
    want = [int(nK <= c < nK + 4 * N or nK + 4 * N + sites <= c < nK + 5 * N + sites) for c in cols]
    assert [int(g[0]) for g in got] == want and sum(want) == 5 * N
    # the packed entries of [J | r]^T [J | r]: every (i, j), i >= j, but (K, K), by columns; K = 23 is the first triangle beyond 256 entries
    for K in (1, 2, 8, 23):
        g = ask(exe, [f"entries {K}"])[0]
        n, pairs = int(g[0]), [(int(a), int(b)) for a, b in zip(g[1::2], g[2::2])]
        assert n == (K + 1) * (K + 2) // 2 - 1 == len(pairs)
        assert pairs == [(i, j) for j in range(K + 1) for i in range(j, K + 1)][:-1]
    assert 22 * 23 // 2 <= 256 < 23 * 24 // 2


def test_scales_prior_rows_cost_and_entry_map(workdir):
    check_requests(workdir / "rows")


def test_the_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(workdir):
    """The same program as a plain executable with nothing preloaded."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *san, f"-I{CSRC}", "-c", str(workdir / "main.cpp"), "-o",
                    str(workdir / "main_san.o")], check=True)
    link = subprocess.run(["g++", *san, str(workdir / "main_san.o"), "-o", str(workdir / "rows_san")], capture_output=True, text=True)
    if link.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + link.stderr.strip().splitlines()[-1])
    check_requests(workdir / "rows_san")


@pytest.mark.parametrize("obj_w", [(1.0, 1.0, 1.0), (0.3, 0.0, 2.5)])
def test_half_r2_and_half_w_F_differ_by_the_unfitted_prior(workdir, obj_w):
    s = og.fixture_data("network_m0_small")
    net, ld, x, dflt, cols = s["net"], s["ld"], s["X"][0], s["defaults"], s["gold"]["cols"]
    r = og.chain(net, s["gold"]["Y"][0], s["gold"]["dY"][0], ld, 0, x, dflt, og.LAM, cols)
    nK, N, sites = net.n_K, net.N, net.total_sites
    norm = [1.0 / max(1e-6, float(np.sum(ld[k]))) for k in ("w_prot", "w_rna", "w_pho")]
    w = np.concatenate([ld["w_prot"], ld["w_rna"], ld["w_pho"]]); obs = np.concatenate([ld["obs_prot"], ld["obs_rna"], ld["obs_pho"]])
    mod = np.repeat([0, 1, 2], [ld["w_prot"].size, ld["w_rna"].size, ld["w_pho"].size])
    scl = np.array([g[0] for g in ask(workdir / "rows", [f"scale {obj_w[m]!r} {norm[m]!r} {og.LAM[m]!r} {float(wi)!r}" for m, wi in zip(mod, w)])])
    has = [c for c in cols if nK <= c < nK + 4 * N or nK + 4 * N + sites <= c < nK + 5 * N + sites]
    assert 0 < len(has) < len(cols)                                   # the stored columns hold entries with and without a prior term
    pri = ask(workdir / "rows", [f"prior {obj_w[0]!r} {obj_w[1]!r} {obj_w[2]!r} {og.LAM[3]!r} {N} 0 {float(x[c])!r} {float(dflt[c])!r}" for c in has])
    rows = np.concatenate([LD(scl) * (LD(r["pred"]) - LD(obs)), LD(np.array([p[1] for p in pri]))])
    half_r2 = LD(0.5) * np.sum(rows * rows)
    half_wF = LD(0.5) * np.sum(LD(np.array(obj_w)) * LD(r["F"]))
    unfit = [q for lo, hi in ((nK, nK + 4 * N), (nK + 4 * N + sites, nK + 5 * N + sites)) for q in range(lo, hi) if q not in has]
    const = LD(0.5) * LD(sum(obj_w)) * LD(og.LAM[3]) * np.sum(((LD(x[unfit]) - LD(dflt[unfit])) / (LD(dflt[unfit]) + LD(1e-6))) ** 2) / LD(5 * N)
    bound = (rows.size + 5 * N + 12) * U * float(half_r2 + const)       # every term is positive: sum |terms| is the value
    assert const > 0 and abs(half_wF - half_r2 - const) <= bound, (float(half_wF), float(half_r2), float(const), bound)
