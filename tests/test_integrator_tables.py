"""CPU known-answer tests for the integrator coefficient tables compiled into the kernels.

Every table in csrc/ was typed in from the literature or derived offline; these tests re-derive / re-verify them in multi-precision
arithmetic (mpmath) and compare with the literals parsed out of the HIP sources, so a typo in a constant cannot survive:
  * RODAS4 (Hairer-Wanner)      : the 8 Rosenbrock order-4 conditions            (tools/check_rodas4.py)
  * ROS34PW2 (Rang-Angermann)   : the 8 order-3 W-method conditions, stiff accuracy, R(inf) = 0   (tools/check_ros34pw2.py)
  * RODAS4 resolvent weights    : re-derived from the stage table                 (tools/rodas4_resolvent.py)
  * LRP8 weights                : order 7 / embedded order 6 conditions solved afresh, A-stability on the imaginary axis (tools/restricted_pade.py)
  * ARK4(3)6L[2]SA (Kennedy-Carpenter) : the rationals of tools/check_ark436.py, every additive order condition to order 4 (embedded: 3),
                                  stiff accuracy and L-stability of the implicit tableau, one copy of the table under csrc/
"""
import importlib.util
import re
import sys
from pathlib import Path

import mpmath as mp
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "phoskintime_amd" / "csrc"


def _load(name):
    spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _literals(text, name):
    """Numbers of `constexpr double NAME... = {a, b, ...}` or `NAME = value` in a source file."""
    m = re.search(name + r"\s*(?:\[\d*\])?\s*=\s*\{([^}]*)\}", text)
    if m:
        return [mp.mpf(x.strip()) for x in m.group(1).split(",") if x.strip()]
    m = re.search(r"\b" + name + r"\s*=\s*([-+0-9.eE]+)", text)
    assert m, name
    return [mp.mpf(m.group(1))]


def _literals_2d(text, name):
    """Rows of `NAME[r][c] = {{a, b, ...}, {...}, ...};` in a source file (the one-dimensional reader stops at the first closing brace)."""
    m = re.search(r"\b" + name + r"\s*\[\d+\]\s*\[\d+\]\s*=\s*\{((?:\s*\{[^{}]*\}\s*,?)+)\s*\}\s*;", text)
    assert m, name
    return [[mp.mpf(x.strip()) for x in row.split(",") if x.strip()] for row in re.findall(r"\{([^{}]*)\}", m.group(1))]


def test_ark436_table_matches_source_and_order_conditions():
    """ARK4(3)6L[2]SA as compiled into csrc/pk_network_solve_ark.hpp (AE, DI = a^I - a^E, B, EB = b - bhat, GAM) against the rationals of
    tools/check_ark436.py; its additive order conditions (order 4, embedded order 3, every coupling between the two tableaus), stiff
    accuracy and L-stability of the implicit tableau, re-run in mpmath; and one copy of the table under csrc/."""
    mp.mp.dps = 50
    chk = _load("check_ark436")
    src = (CSRC / "pk_network_solve_ark.hpp").read_text()
    ns = src[src.index("namespace ark436 {"):src.index("}  // namespace ark436")]
    fr = lambda x: mp.mpf(x.numerator) / mp.mpf(x.denominator)
    AI = [[fr(x) for x in r] for r in chk.AI]; AE = [[fr(x) for x in r] for r in chk.AE]
    b = [fr(x) for x in chk.b]; bh = [fr(x) for x in chk.bh]; c = [fr(x) for x in chk.c]
    close = lambda lit, exact, what: abs(lit - exact) <= mp.mpf("1e-16") * abs(exact) or pytest.fail("%s: %s against %s" % (what, lit, exact))
    # ---- the literals
    assert _literals(ns, "GAM")[0] == fr(chk.g) == mp.mpf(1) / 4
    sAE, sDI, sB, sEB = _literals_2d(ns, "AE"), _literals_2d(ns, "DI"), _literals(ns, r"\bB"), _literals(ns, "EB")
    assert [len(r) for r in sAE] == [5] * 5 and [len(r) for r in sDI] == [5] * 5 and len(sB) == 6 and len(sEB) == 6
    for i in range(5):                                   # rows i = 2 .. 6 of the tableaus, columns 1 .. 5
        for j in range(5):
            if j > i:                                    # the arrays hold the strictly lower triangle
                assert sAE[i][j] == 0 and sDI[i][j] == 0 and AE[i + 1][j] == 0
                continue
            close(sAE[i][j], AE[i + 1][j], "AE[%d][%d]" % (i, j))
            close(sDI[i][j], AI[i + 1][j] - AE[i + 1][j], "DI[%d][%d]" % (i, j))
    for j in range(6):
        close(sB[j], b[j], "B[%d]" % j)
        close(sEB[j], b[j] - bh[j], "EB[%d]" % j)
    assert all(AE[i][5] == 0 for i in range(6)) and all(AI[i][i] == fr(chk.g) for i in range(1, 6))      # what the 5 x 5 arrays leave out: gamma on the diagonal
    # ---- the conditions
    mv = lambda A, v: [sum(A[i][j] * v[j] for j in range(6)) for i in range(6)]
    dot = lambda u, v: sum(x * y for x, y in zip(u, v))
    c2, c3 = [x * x for x in c], [x ** 3 for x in c]
    tabs = (AI, AE)
    tol = mp.mpf("1e-24")                                # the explicit entries are 13-digit rational approximations: residuals <= 3e-26

    def residuals(w, order):
        r = [dot(w, [1] * 6) - 1, dot(w, c) - mp.mpf(1) / 2, dot(w, c2) - mp.mpf(1) / 3] + [dot(w, mv(A, c)) - mp.mpf(1) / 6 for A in tabs]
        if order == 4:
            r += [dot(w, c3) - mp.mpf(1) / 4]
            r += [dot(w, [ci * x for ci, x in zip(c, mv(A, c))]) - mp.mpf(1) / 8 for A in tabs] + [dot(w, mv(A, c2)) - mp.mpf(1) / 12 for A in tabs]
            r += [dot(w, mv(A1, mv(A2, c))) - mp.mpf(1) / 24 for A1 in tabs for A2 in tabs]
        return r

    for A in tabs:
        assert max(abs(sum(A[i]) - c[i]) for i in range(6)) < tol
    assert len(residuals(b, 4)) == 14 and max(abs(v) for v in residuals(b, 4)) < tol
    assert max(abs(v) for v in residuals(bh, 3)) < tol
    assert max(abs(v) for v in residuals(bh, 4)[5:]) > mp.mpf("1e-4")                                   # embedded: order 3 only
    # ---- implicit tableau: first stage explicit, stiffly accurate, L-stable
    assert all(x == 0 for x in AI[0]) and AI[5] == b
    R = lambda z: 1 + z * dot(b, list(mp.lu_solve(mp.eye(6) - z * mp.matrix(AI), mp.matrix([1] * 6))))
    assert abs(R(mp.mpf("0.01")) - mp.e ** mp.mpf("0.01")) < mp.mpf("1e-10") and abs(R(mp.mpf("-1e15"))) < mp.mpf("1e-12")
    assert all(abs(R(mp.mpc(0, y))) <= 1 + mp.mpf("1e-30") for y in (0.1, 1, 3, 10, 100, 1e4))
    # ---- one copy: no other file of csrc/ spells an entry of the table out, and the pair kernels read this namespace
    entries = set(re.findall(r"\d\.\d{10,}", ns))
    assert len(entries) >= 30
    for f in sorted(CSRC.glob("*.h*")):
        text = f.read_text()
        assert text.count("namespace ark436 {") == (1 if f.name == "pk_network_solve_ark.hpp" else 0), f.name
        if f.name != "pk_network_solve_ark.hpp":
            assert not [t for t in entries if t in text], f.name
    assert "using namespace ark436;" in (CSRC / "pk_network_solve_arkp.hpp").read_text()


def test_rodas4_table_satisfies_order_conditions_and_matches_source():
    mp.mp.dps = 50
    src = (CSRC / "pk_solve_kernel.hpp").read_text()
    chk = _load("check_rodas4")
    res = chk.conds(chk.b)
    assert max(abs(v) for v in res.values()) < mp.mpf("1e-14")
    emb = chk.conds(chk.bh)
    assert max(abs(emb[k]) for k in ("1", "2", "3a", "3b")) < mp.mpf("1e-14") and abs(emb["4a"]) > 1e-3      # embedded: order 3 only
    for (i, j), v in chk.a.items():
        assert _literals(src, f"A{i}{j}")[0] == mp.mpf(v)
    for (i, j), v in chk.c.items():
        assert _literals(src, f"C{i}{j}")[0] == mp.mpf(v)


def test_rodas4_resolvent_weights_match_source():
    mp.mp.dps = 60
    src = (CSRC / "pk_solve_kernel.hpp").read_text()
    rr = _load("rodas4_resolvent")
    for k in range(6):
        assert abs(_literals(src, f"RB{k + 1}")[0] - rr.beta[k]) < mp.mpf("1e-16")
        if k >= 1:
            assert abs(_literals(src, f"RE{k + 1}")[0] - rr.eps[k]) < mp.mpf("1e-16")
    assert abs(rr.eps[0]) < mp.mpf("1e-30")
    # the resolvent form reproduces exp(z) to order 4 and is L-stable
    z = mp.mpf("0.01")
    R = 1 + sum(rr.beta[k] * z / (1 - rr.g * z) ** (k + 1) for k in range(6))
    assert abs(R - mp.e ** z) < 10 * z ** 5
    zi = mp.mpf("-1e9")
    assert abs(1 + sum(rr.beta[k] * zi / (1 - rr.g * zi) ** (k + 1) for k in range(6))) < mp.mpf("1e-7")


@pytest.mark.parametrize("name,s_,gam", [("PK_METHOD_LRP8", 8, "0.22"), ("PK_METHOD_LRP12", 12, "0.16")])
def test_lrp_weights_rederived_and_a_stable(name, s_, gam):
    mp.mp.dps = 60
    src = (CSRC / "pk_solve_kernel.hpp").read_text()
    rp = _load("restricted_pade")
    blk = src[src.index("struct ResolventTab<%s>" % name):]
    blk = blk[:blk.index("\n};")]
    g = _literals(blk, "GAM")[0]
    assert g == mp.mpf(gam)
    B = _literals(blk, "B"); E = _literals(blk, "E")
    assert len(B) == s_ and len(E) == s_ and _literals(blk, "NS")[0] == s_ and _literals(blk, "Q")[0] == s_ - 1
    beta = rp.solve_weights(s_, g, s_ - 1)
    bh = rp.solve_weights(s_, g, s_ - 2, extra_zero=(s_,))
    for k in range(s_):
        assert abs(B[k] - beta[k]) < mp.mpf("2e-15") * max(1, abs(beta[k]))
        assert abs(E[k] - (beta[k] - bh[k])) < mp.mpf("2e-15") * max(1, abs(beta[k]))
    # order: R(z) - exp(z) = O(z^s) ; embedded O(z^(s-1))
    z = mp.mpf("0.05")
    assert abs(rp.R(beta, g, z) - mp.e ** z) < 1e-3 * z ** s_ * 100
    assert abs(rp.R(bh, g, z) - mp.e ** z) < 1e-2 * z ** (s_ - 1) * 100
    # L-stability and A-stability (poles sit at 1/gamma > 0; on the imaginary axis |R| <= 1)
    assert abs(rp.R(beta, g, mp.mpf("-1e12"))) < mp.mpf("1e-10") and abs(rp.R(bh, g, mp.mpf("-1e12"))) < mp.mpf("1e-10")
    # LRP8: strictly A-stable.  LRP12: the embedded method strictly, the propagated one up to its own leading error term
    # (|R(iy)|^2 - 1 ~ 2 C_12 y^12 with C_12 > 0 near |y| ~ 1): |R(iy)| <= 1 + 4.5e-9, as the source comment states
    assert rp.a_stable(beta, g, n=1500) <= 1 + (mp.mpf("1e-20") if s_ == 8 else mp.mpf("4.6e-9"))
    assert rp.a_stable(bh, g, n=1500) <= 1 + mp.mpf("1e-20")
    if s_ == 12:
        assert all(abs(rp.R(beta, g, mp.mpc(0, y))) < 1 for y in (2, 3, 5, 10, 100, 1e4))
        assert all(abs(rp.R(beta, g, mp.mpf(-x))) <= 1 for x in (1e-3, 0.1, 1, 3, 10, 100, 1e6))       # the negative real axis
    # the scalar-C oracle carries the same tables
    csrc = (CSRC.parents[1] / "oracle" / "lrp8_dist.c").read_text()
    cb = _literals(csrc, "LB%d" % s_); ce = _literals(csrc, "LE%d" % s_)
    assert [float(x) for x in cb] == [float(x) for x in B] and [float(x) for x in ce] == [float(x) for x in E]


def test_ros34pw2_table_satisfies_w_conditions_and_matches_source():
    mp.mp.dps = 50
    src = (CSRC / "pk_network_solve.hpp").read_text()
    chk = _load("check_ros34pw2")
    assert max(abs(v) for v in chk.conds(chk.b).values()) < mp.mpf("1e-14")
    emb = chk.conds(chk.bh)
    assert max(abs(emb[k]) for k in ("b.1 = 1", "b.A1 = 1/2", "b.G1 = 0")) < mp.mpf("1e-14")
    assert abs(1 - (chk.b * (chk.B ** -1) * chk.one)[0]) < mp.mpf("1e-14")            # R(inf) = 0
    names = {"A21": chk.a[1, 0], "A31": chk.a[2, 0], "A32": chk.a[2, 1], "A41": chk.a[3, 0], "A42": chk.a[3, 1], "A43": chk.a[3, 2],
             "C21": chk.c[1, 0], "C31": chk.c[2, 0], "C32": chk.c[2, 1], "C41": chk.c[3, 0], "C42": chk.c[3, 1], "C43": chk.c[3, 2],
             "E1": chk.m[0] - chk.mh[0], "E2": chk.m[1] - chk.mh[1], "E3": chk.m[2] - chk.mh[2], "E4": chk.m[3] - chk.mh[3], "GAM": chk.g}
    ns = src[src.index("namespace rosw"):src.index("}  // namespace rosw")]
    for k, v in names.items():
        assert abs(_literals(ns, k)[0] - v) < mp.mpf("1e-15") * max(1, abs(v)), k
    assert abs(chk.m[3] - 1) < mp.mpf("1e-15") and all(abs(chk.m[j] - chk.a[3, j]) < mp.mpf("1e-15") for j in range(3))    # y1 = Y4 + U4
