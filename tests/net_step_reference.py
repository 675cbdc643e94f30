"""One-step restatement of the network integrators (net_rosw_solve of csrc/pk_network_solve.hpp and the additive kernels of
csrc/pk_network_solve_ark.hpp / _arkp.hpp / _reg.hpp / _reg2.hpp), shared by tests/test_net_step_reference_cpu.py and
tests/test_gpu_network_steps.py (not a test module).  Plain numpy on the dense S x S system, generic over float64 and numpy.longdouble:
no torch, no library.  It reads like tests/group_reference.py, which does the same for the lane-group kernels.

    rhs             the network right-hand side at the kinase bucket of time tb, from the oracle's formulas (squash, then
                    calculate_synthesis_rate; no merged reciprocal chains), with driver_map
    block_jacobian  the matrix the kernels call A / J_blockdiag: the per-protein diagonal blocks of the Jacobian, analytic, dense S x S.  The
                    mRNA row holds -B_i only (the TF input is never in A); topology 4 takes g_P = 1 / (1 + P)^2 and c_R = C / (1 + R)^2 at y
    sgs_operator    P = (D_g - F) D_g^-1 (D_g - K) of the combinatorial order-3 kernels and of ark2 with EXACT = false (A~ = g I - P)
    rosw_step       one step of ROS34PW2-W:   W U_1 = f(y);  W U_i = f(y + sum_j A_ij U_j) + sum_j C_ij U_j / h,  W = I / (GAM h) - A (or P);
                    y+ = Y_4 + U_4, err = sum_i E_i U_i
    ark_step        one step of the linearly implicit ARK4(3)6L:  r_i = y + h sum_{j<i} [a^E_ij F_j + d_ij G_j],  W Y_i = g r_i,  g = 1 / (GAM h),
                    G_i = g (Y_i - r_i), G_1 = A y (SGS: g y - P y);  y+ = y + h sum_j b_j F_j, err = h sum_j (b_j - bhat_j) F_j
                  each returns (y+, err vector, majorant).  The majorant is the same step evaluated with every addend replaced by its absolute
                  value -- in the right-hand side, in the stage sums, in (Y_i - r_i) -- and with |W^-1| applied in the solves;
                  tau = |majorant|_inf 2^-53 is the unit in which a double-precision evaluation of the step may differ from this one.
    integrate     the free-running loop around a step: stops = output times + bucket edges, a step uses the bucket of its start time, the
                  `last` / half-step rule, step_h0, step_fac with exponent 1/3 (ROSW) or 1/4 (ARK), after_reject, the landing rule.

The tables are the literals of the HIP sources, read with the parser of tests/test_integrator_tables.py (which proves them against
multi-precision derivations) and rounded to double as the compiler rounds them.  With dtype=numpy.longdouble (64-bit mantissa on x86) every
solve is the double-precision LU refined on a long-double residual until the correction stops shrinking."""
from pathlib import Path

import numpy as np
import scipy.linalg as sla

from oracle import network_models as nm
from test_integrator_tables import _literals, _literals_2d

LD = np.longdouble
U = 2.0 ** -53
CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"
ST_NONFINITE, ST_MAXSTEPS, ST_HMIN = 1, 2, 4
#: the library integrates the order-4 method at this factor on the caller's tolerances (pk_network.hip, csrc/pk_env.hpp: ark_tolfac)
ARK_TOLFAC = 0.25


def _tables():
    one = lambda text, name: float(_literals(text, name)[0])
    src = (CSRC / "pk_network_solve.hpp").read_text()
    ns = src[src.index("namespace rosw"):src.index("}  // namespace rosw")]
    c = {k: one(ns, k) for k in ("GAM", "A21", "A31", "A32", "A41", "A42", "A43", "C21", "C31", "C32", "C41", "C42", "C43", "E1", "E2", "E3", "E4")}
    rosw = dict(GAM=c["GAM"], E=[c["E%d" % k] for k in range(1, 5)],
                TA=[[c.get("A%d%d" % (i, j), 0.0) for j in range(1, 4)] for i in range(1, 5)],
                TC=[[c.get("C%d%d" % (i, j), 0.0) for j in range(1, 4)] for i in range(1, 5)])
    src = (CSRC / "pk_network_solve_ark.hpp").read_text()
    ns = src[src.index("namespace ark436"):src.index("}  // namespace ark436")]
    ark = dict(GAM=one(ns, "GAM"), AE=[[float(x) for x in r] for r in _literals_2d(ns, "AE")], DI=[[float(x) for x in r] for r in _literals_2d(ns, "DI")],
               B=[float(x) for x in _literals(ns, r"\bB")], EB=[float(x) for x in _literals(ns, "EB")])
    assert np.shape(ark["AE"]) == np.shape(ark["DI"]) == (5, 5) and len(ark["B"]) == len(ark["EB"]) == 6
    return dict(rosw=rosw, ark=ark)


TAB = _tables()
Q = {"rosw": 3.0, "ark": 4.0}


def _blocks(net):
    """(start, rows) of every protein block."""
    for i in range(net.N):
        ns = int(net.n_sites[i])
        yield i, int(net.offset_y[i]), (1 + (1 << ns)) if net.model == 2 else 2 + ns


def _params(p, D):
    return {k: np.asarray(getattr(p, k), dtype=D) for k in nm.PARAM_KEYS}, D(p.tf_scale)


def _site_rates(net, p, tb, D):
    """(S_all, Kt) at the bucket of tb: S_all = W (K(tb) * c_k), row by row in CSR order."""
    jb = nm.time_bucket(tb, net.kin_grid)
    Kt = np.asarray(net.kin_Kmat[:, jb], dtype=D) * np.asarray(p.c_k, dtype=D)
    S_all = np.zeros(net.total_sites, dtype=D)
    for s in range(net.total_sites):
        acc = D(0)
        for q in range(net.W_indptr[s], net.W_indptr[s + 1]):
            acc = acc + D(net.W_data[q]) * Kt[net.W_indices[q]]
        S_all[s] = acc
    return S_all, Kt


def rhs(net, p, y, tb, dtype=float, absolute=False):
    """f(y) at the bucket of tb.  absolute=True: the same sums with every addend replaced by its magnitude (y is then a majorant of the
    state, TF weights enter by magnitude): the right-hand side's part of the majorant."""
    D = float if dtype is float else LD
    y = np.abs(np.asarray(y, dtype=D)) if absolute else np.asarray(y, dtype=D)
    m = D(1) if absolute else D(-1)                     # the sign of every subtracted term
    q, ts = _params(p, D)
    S_all, Kt = _site_rates(net, p, tb, D)
    one = D(1)
    P_vec = np.zeros(net.N, dtype=D)
    for i, st, rows in _blocks(net):
        d = -1 if net.model == 2 else int(net.driver_map[i])
        if d >= 0:
            P_vec[i] = Kt[d]
        else:
            tot = D(0)
            for k in range(1, rows):                    # P and its sites / every bit-pattern state
                tot = tot + y[st + k]
            P_vec[i] = tot
    dy = np.zeros_like(y)
    for i, st, rows in _blocks(net):
        ss, ns = int(net.offset_s[i]), int(net.n_sites[i])
        acc = D(0)
        for e in range(net.TF_indptr[i], net.TF_indptr[i + 1]):
            w = D(net.TF_data[e])
            acc = acc + (abs(w) if absolute else w) * P_vec[net.TF_indices[e]]
        v = acc / D(net.tf_deg[i])
        if net.model != 4:
            v = v / (one + abs(v))
        u = v / (one + abs(v))                          # calculate_synthesis_rate
        Ai, Bi, Ci, Di, Ei = q["A_i"][i], q["B_i"][i], q["C_i"][i], q["D_i"][i], q["E_i"][i]
        synth = Ai * (one + (ts * u) / (one + u + D(1e-6))) if u >= 0 else Ai / (one + ts * abs(u))
        R = y[st]
        dy[st] = synth + m * Bi * R
        Sr, Dp = S_all[ss:ss + ns], q["Dp_i"][ss:ss + ns]
        if net.model == 0:
            P = y[st + 1]
            sumS, back = D(0), D(0)
            for j in range(ns):
                ps = y[st + 2 + j]
                sumS = sumS + Sr[j]; back = back + Ei * ps
                dy[st + 2 + j] = Sr[j] * P + m * (Ei + Dp[j] + Di) * ps
            dy[st + 1] = Ci * R + m * (Di + sumS) * P + back
        elif net.model == 4:
            P = y[st + 1]
            sum_f, sum_b = D(0), D(0)
            for j in range(ns):
                ps = y[st + 2 + j]
                fwd = (Sr[j] * P) / (one + P); back = Ei * ps
                sum_f = sum_f + fwd; sum_b = sum_b + back
                dy[st + 2 + j] = fwd + m * (Dp[j] + Di) * ps + m * back
            dy[st + 1] = (Ci * R) / (one + R) + m * Di * P + m * sum_f + sum_b
        elif net.model == 1:
            Y = y[st + 1:st + 2 + ns]                   # P0, P1 .. Pns
            dy[st + 1] = Ci * R + m * Di * Y[0] + (m * Sr[0] * Y[0] + Ei * Y[1] if ns else D(0))
            for j in range(ns):
                nxt = j + 1 < ns
                dy[st + 2 + j] = Sr[j] * Y[j] + (Ei * Y[j + 2] if nxt else D(0)) + m * ((Sr[j + 1] if nxt else D(0)) + Ei + Dp[j] + Di) * Y[j + 1]
        else:
            base, nst = st + 1, 1 << ns
            dy[base] = Ci * R + m * Di * y[base]
            for mk in range(nst):
                Pm = y[base + mk]
                for j in range(ns):
                    bit = 1 << j
                    if mk & bit:                        # dephosphorylation into mk ^ bit, degradation
                        dy[base + mk] = dy[base + mk] + m * Ei * Pm + m * (Dp[j] + Di) * Pm
                        dy[base + (mk ^ bit)] = dy[base + (mk ^ bit)] + Ei * Pm
                    else:                               # phosphorylation into mk | bit
                        dy[base + mk] = dy[base + mk] + m * Sr[j] * Pm
                        dy[base + (mk | bit)] = dy[base + (mk | bit)] + Sr[j] * Pm
    return dy


def block_jacobian(net, p, y, tb, dtype=float):
    D = float if dtype is float else LD
    y = np.asarray(y, dtype=D)
    q, _ = _params(p, D)
    S_all, _ = _site_rates(net, p, tb, D)
    one = D(1)
    A = np.zeros((net.S, net.S), dtype=D)
    for i, st, rows in _blocks(net):
        ss, ns = int(net.offset_s[i]), int(net.n_sites[i])
        Bi, Ci, Di, Ei = q["B_i"][i], q["C_i"][i], q["D_i"][i], q["E_i"][i]
        Sr, Dp = S_all[ss:ss + ns], q["Dp_i"][ss:ss + ns]
        A[st, st] = -Bi
        if net.model in (0, 4):
            sat = net.model == 4
            gP = one / ((one + y[st + 1]) * (one + y[st + 1])) if sat else one
            A[st + 1, st] = Ci / ((one + y[st]) * (one + y[st])) if sat else Ci
            sumS = D(0)
            for j in range(ns):
                sumS = sumS + Sr[j] * gP
                A[st + 1, st + 2 + j] = Ei
                A[st + 2 + j, st + 1] = Sr[j] * gP
                A[st + 2 + j, st + 2 + j] = -(Ei + Dp[j] + Di)
            A[st + 1, st + 1] = -(Di + sumS)
        elif net.model == 1:
            A[st + 1, st] = Ci
            A[st + 1, st + 1] = -(Di + (Sr[0] if ns else D(0)))
            for j in range(ns):
                r = st + 2 + j
                A[r, r - 1] = Sr[j]
                A[r - 1, r] = Ei
                A[r, r] = -((Sr[j + 1] if j + 1 < ns else D(0)) + Ei + Dp[j] + Di)
        else:
            base, nst = st + 1, 1 << ns
            A[base, st] = Ci
            for mk in range(nst):
                loss = Di if mk == 0 else D(0)
                for j in range(ns):
                    bit = 1 << j
                    if mk & bit:
                        loss = loss + (Ei + Dp[j] + Di)
                        A[base + (mk ^ bit), base + mk] = Ei
                    else:
                        loss = loss + Sr[j]
                        A[base + (mk | bit), base + mk] = Sr[j]
                A[base + mk, base + mk] = -loss
    return A


def sgs_operator(A_block, g):
    """P = (D_g - F) D_g^-1 (D_g - K): D_g = g I - diag(A), F / K the strictly lower / upper part of A."""
    D = A_block.dtype.type
    Dg = D(g) - np.diag(A_block)
    return (np.diag(Dg) - np.tril(A_block, -1)) @ ((np.diag(Dg) - np.triu(A_block, 1)) / Dg[:, None])


class _Solver:
    """x = W^-1 r.  float: LAPACK's LU.  long double: the double LU, refined on a long-double residual until the correction stops shrinking."""

    def __init__(self, W, blocks):
        self.W = W
        self.ld = W.dtype == LD
        self.blocks = blocks
        self.lu = [sla.lu_factor(W[s:s + n, s:s + n].astype(float)) for s, n in blocks]      # W is block diagonal: LAPACK's row-pivoted LU per block
        self._absinv = None

    def _lu_solve(self, r):
        x = np.empty(r.size)
        for (s, n), lu in zip(self.blocks, self.lu):
            x[s:s + n] = sla.lu_solve(lu, r[s:s + n])
        return x

    def __call__(self, r):
        if not self.ld:
            return self._lu_solve(r)
        x = self._lu_solve(r.astype(float)).astype(LD)
        best = np.inf
        for _ in range(12):
            d = self._lu_solve((r - self.W @ x).astype(float)).astype(LD)
            size = float(np.max(np.abs(d)))
            if not size < best:
                break
            x, best = x + d, size
        return x

    def absinv(self, r):
        if self._absinv is None:
            self._absinv = np.zeros(self.W.shape, dtype=self.W.dtype)
            for s, n in self.blocks:
                self._absinv[s:s + n, s:s + n] = np.abs(np.linalg.inv(self.W[s:s + n, s:s + n].astype(float)))
        return self._absinv @ r


def _operator(net, p, y, tb, hs, gam, operator, D):
    """(g, solve, A-product, |A|-product) of the step's implicit operator: W = g I - A, or P with A~ = g I - P."""
    g = D(1) / (D(hs) * D(gam))
    A = block_jacobian(net, p, y, tb, D)
    eye = np.eye(net.S, dtype=D)
    if operator == "exact":
        W = g * eye - A
    else:
        assert operator == "sgs", operator
        W = sgs_operator(A, g)
        A = g * eye - W
    absA = np.abs(A)
    return g, _Solver(W, [(st, rows) for _, st, rows in _blocks(net)]), (lambda v: A @ v), (lambda v: absA @ v)


def _rosw_stages(f, solve, y, hinv, TA, TC, E):
    Us, Ys = [solve(f(y))], y
    for sg in range(1, 4):
        Ys = y + sum(TA[sg][j] * Us[j] for j in range(sg))
        Us.append(solve(f(Ys) + sum((TC[sg][j] * hinv) * Us[j] for j in range(sg))))
    return Ys + Us[3], sum(E[j] * Us[j] for j in range(4))


def rosw_step(net, p, y, tb, h, operator="exact", dtype=float):
    """(y_new, err_vector, majorant) of one ROS34PW2-W step of size h from y at the bucket of tb."""
    D = float if dtype is float else LD
    t = TAB["rosw"]
    y = np.asarray(y, dtype=D)
    _, solve, _, _ = _operator(net, p, y, tb, h, t["GAM"], operator, D)
    hinv = D(1) / D(h)
    cv = lambda tab, a=False: [[abs(D(x)) if a else D(x) for x in r] for r in tab]
    yn, err = _rosw_stages(lambda v: rhs(net, p, v, tb, D), solve, y, hinv, cv(t["TA"]), cv(t["TC"]), cv([t["E"]])[0])
    maj, _ = _rosw_stages(lambda v: rhs(net, p, v, tb, D, absolute=True), solve.absinv, np.abs(y), hinv, cv(t["TA"], True), cv(t["TC"], True), cv([t["E"]], True)[0])
    return yn, err, maj


def _ark_stages(f, solve, matvec, y, hs, g, gam, AE, DI, B, EB, sign):
    w, v = [hs * f(y)], [hs * matvec(y)]               # w_j = h F_j, v_j = h G_j
    for i in range(5):                                  # stages 2 .. 6
        r = y + sum(AE[i][j] * w[j] + DI[i][j] * v[j] for j in range(i + 1))
        Y = solve(g * r)
        v.append((Y + sign * r) / gam)                  # h G_i = h g (Y_i - r_i)
        w.append(hs * f(Y))
    return y + sum(B[j] * w[j] for j in range(6)), sum(EB[j] * w[j] for j in range(6))


def ark_step(net, p, y, tb, h, operator="exact", dtype=float):
    """(y_new, err_vector, majorant) of one linearly implicit ARK4(3)6L step of size h from y at the bucket of tb."""
    D = float if dtype is float else LD
    t = TAB["ark"]
    y = np.asarray(y, dtype=D)
    g, solve, Av, absAv = _operator(net, p, y, tb, h, t["GAM"], operator, D)
    cv = lambda tab, a=False: [[abs(D(x)) if a else D(x) for x in r] for r in tab]
    gam, hs = D(t["GAM"]), D(h)
    yn, err = _ark_stages(lambda v: rhs(net, p, v, tb, D), solve, Av, y, hs, g, gam, cv(t["AE"]), cv(t["DI"]), cv([t["B"]])[0], cv([t["EB"]])[0], D(-1))
    maj, _ = _ark_stages(lambda v: rhs(net, p, v, tb, D, absolute=True), solve.absinv, absAv, np.abs(y), hs, g, gam, cv(t["AE"], True), cv(t["DI"], True),
                         cv([t["B"]], True)[0], cv([t["EB"]], True)[0], D(1))
    return yn, err, maj


STEP = {"rosw": rosw_step, "ark": ark_step}


def tau(majorant):
    return float(np.max(np.abs(majorant))) * U


def err_norm(y, yn, err, rtol, atol, norm="max"):
    """The kernels' scaled norm of the error estimate: max (NaN-propagating), or ODEPACK's root-mean-square."""
    q = np.abs(err) / (atol + rtol * np.maximum(np.abs(y), np.abs(yn)))
    if np.isnan(q).any():
        return float("nan")
    return float(np.max(q)) if norm == "max" else float(np.sqrt(np.sum(q * q) / q.size))


def step_fac(root, lo=1.0 / 6.0, safety_inv=1.0 / 0.9):
    return max(lo, min(5.0, root * safety_inv))        # csrc/pk_step.hpp


def stops_of(net, t_eval):
    """Landing times (output times + kinase-bucket edges strictly inside the span) and the output row each fills (-1: none)."""
    t_eval = np.asarray(t_eval, float)
    st = [(float(t_eval[k]), k) for k in range(1, t_eval.size)]
    st += [(float(gk), -1) for gk in net.kin_grid if t_eval[0] < gk < t_eval[-1] and not (t_eval[1:] == gk).any()]
    return sorted(st)


def integrate(method, net, p, y0, t_eval, rtol=1e-8, atol=1e-8, h0=0.0, err_norm_="max", operator="exact", max_steps=1000000, dtype=float, trace=None):
    """The free-running loop of the network kernels for one candidate: (Y [T, S], status, (accepted, rejected)); rtol / atol are the
    kernel's own (the library hands the order-4 kernels ARK_TOLFAC times the caller's).  Rows after a failure are NaN.  `trace`: a list
    that receives (t, hs, err) of every step attempted."""
    D = float if dtype is float else LD
    step = STEP[method]
    t_eval = np.asarray(t_eval, float)
    y = np.asarray(y0, dtype=D)
    Y = np.full((t_eval.size, net.S), np.nan)
    Y[0] = y
    nacc = nrej = 0
    status = 0
    tc = float(t_eval[0])
    yf = np.asarray(y, float)
    sc = atol + rtol * np.abs(yf)
    d0, d1 = float(np.max(np.abs(yf) / sc)), float(np.max(np.abs(np.asarray(rhs(net, p, y, tc, D), float)) / sc))
    h = 0.01 * d0 / d1 if (d0 > 1e-5 and d1 > 1e-5) else 1e-6        # step_h0
    if h0 > 0.0:
        h = h0
    if not (h > 0.0):
        h = 1e-6
    after_reject = False
    for te, row in stops_of(net, t_eval):
        tb = tc                                                       # the bucket of the interval's start: no step straddles an edge
        while True:
            if nacc + nrej >= max_steps:
                status |= ST_MAXSTEPS
                break
            last = tc + 1.0001 * h >= te
            hs = te - tc if last else (0.5 * (te - tc) if tc + 2.0 * h > te else h)
            if not (hs > 1e-14 * max(abs(tc), 1e-3)):
                status |= ST_HMIN
                break
            yn, ev, _ = step(net, p, y, tb, hs, operator, D)
            err = err_norm(np.asarray(y, float), np.asarray(yn, float), np.asarray(ev, float), rtol, atol, err_norm_)
            if trace is not None:
                trace.append((tc, hs, err))
            if err != err or err > 1e300:
                nrej += 1
                after_reject = True
                h = 0.1 * hs
                if not np.isfinite(np.asarray(y, float)).all():
                    status |= ST_NONFINITE
                    break
                continue
            hnew = hs / step_fac(err ** (1.0 / Q[method]))
            if err <= 1.0:
                nacc += 1
                y = yn
                tc += hs
                if after_reject:
                    hnew = min(hnew, hs)
                after_reject = False
                if last:
                    tc = te
                    h = max(hnew, h) if hs < h else hnew                # keep the untruncated proposal
                    break
                h = hnew
            else:
                nrej += 1
                after_reject = True
                h = hnew
        if status:
            break
        if row >= 0:
            Y[row] = y
    return Y, status, (nacc, nrej)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU matrix
GOLDEN = Path(__file__).resolve().parent / "golden"
B = 5
COMPARED = (0, 2, 4)
#: forced grid: rtol = atol = TOL with h0 = 1e9 makes every kernel take one step per stop.  Worst error norm of the restatement's own steps
#: over every network of NETWORKS, the candidates COMPARED and both methods (order-4 at ARK_TOLFAC * TOL, as the library runs it):
#: see FORCED_WORST, measured and asserted <= 0.5 by tests/test_net_step_reference_cpu.py
TOL = 16.0
#: worst error norm of the restatement's own forced-grid steps (both methods, every operator a route uses, every network, the candidates
#: COMPARED), measured and asserted by tests/test_net_step_reference_cpu.py: 0.0033 (the premise asks for <= 0.5)
FORCED_WORST = 0.004
#: (method, operator) -> worst |y64 - yld|_inf / tau of one step evaluated in double against long double, over the same steps, rounded up to a
#: power of two (measured 0.40, 0.43, 0.30, 0.14)
R64 = {("rosw", "exact"): 0.5, ("ark", "exact"): 0.5, ("rosw", "sgs"): 0.5, ("ark", "sgs"): 0.25}
H0 = 1e9
#: (tag, topology, N, total_sites, max_sites, seed) of the synthetic networks; n_K = 6 kinases (3 of them driver-mapped proteins), 2 N TF edges
#: the seeds are the first (in steps of 10) whose network reaches its site cap and has a protein without sites (case() asserts both)
_SEED = {(0, 4): 64, (0, 6): 6, (0, 8): 208, (1, 4): 104, (1, 6): 116, (1, 8): 208, (4, 4): 414, (4, 6): 486, (4, 8): 508}
SYNTHETIC = tuple(("m%d_c%d" % (m, c), m, n, s, c, _SEED[m, c]) for m in (0, 1, 4) for c, n, s in ((4, 5, 11), (6, 6, 17), (8, 7, 24))) + (
    ("m2_c2", 2, 6, 8, 2, 202), ("m2_c3", 2, 6, 11, 3, 223), ("m2_c4", 2, 5, 9, 4, 214), ("m0_wide", 0, 70, 150, 4, 4))
GOLDEN_SMALL = tuple("network_m%d_small" % m for m in (0, 1, 2, 4))


def _as_network(desc):
    n_sites = np.asarray(desc["n_sites"])
    model = int(desc["model"])
    blk = (1 + (1 << n_sites.astype(np.int64))) if model == 2 else 2 + n_sites
    return nm.Network(model=model, N=n_sites.size, n_K=np.asarray(desc["kin_Kmat"]).shape[0], total_sites=int(n_sites.sum()), S=int(blk.sum()),
                      n_states=(1 << n_sites.astype(np.int64)) if model == 2 else None,
                      **{k: np.asarray(desc[k]) for k in ("offset_y", "offset_s", "n_sites", "W_indptr", "W_indices", "W_data", "TF_indptr", "TF_indices",
                                                          "TF_data", "tf_deg", "driver_map", "kin_grid", "kin_Kmat")})


def params_of(net, x):
    """Params of one physical candidate row [c_k | A | B | C | D | Dp | E | tf_scale]."""
    cuts = np.cumsum([net.n_K, net.N, net.N, net.N, net.N, net.total_sites, net.N])
    return nm.Params(*np.split(np.asarray(x, float)[:-1], cuts[:-1]), float(x[-1]))


def case(tag):
    """(desc for NetworkEngine(**desc), Network, X [B, n_var], y0 [B, S], t_eval) of one network of the matrix.  Candidates:
    synthetic.random_candidates(spread = 0.5); y0: the default start times U(0.5, 1.5) per candidate and state; t_eval: the kinase-bucket
    edges up to t = 16 plus interior points, so that every stop is an output row."""
    from phoskintime_amd.global_model import synthetic
    if tag in GOLDEN_SMALL:
        g = np.load(GOLDEN / (tag + ".npz"))
        net = nm.Network.from_npz(g)
        desc = {k: np.asarray(g[k]) for k in ("offset_y", "offset_s", "n_sites", "W_indptr", "W_indices", "W_data", "TF_indptr", "TF_indices", "TF_data",
                                              "tf_deg", "driver_map", "kin_grid", "kin_Kmat")}
        desc["model"] = net.model
        seed = 900 + net.model
    else:
        _, model, N, sites, cap, seed = next(s for s in SYNTHETIC if s[0] == tag)
        desc = synthetic.make_network(N=N, total_sites=sites, n_K=6, n_tf_edges=2 * N, model=model, seed=seed, max_sites=cap)
        net = _as_network(desc)
        assert int(net.n_sites.max()) == cap, tag
    # every sum a kernel takes is at most 64 terms long; a protein without sites and a driver-mapped one are present
    assert max(int(np.diff(net.TF_indptr).max()), (1 << int(net.n_sites.max())) if net.model == 2 else int(net.n_sites.max())) <= 64
    assert (net.n_sites == 0).any() and (net.driver_map >= 0).any(), tag
    X =synthetic.random_candidates(desc, B, seed=seed, spread=0.5)
    rng = np.random.default_rng(seed)
    y0 = nm.default_y0(net)[None, :] * rng.uniform(0.5, 1.5, (B, net.S))
    return desc, net, X, y0, forced_times(net)


def forced_times(net):
    grid = np.asarray(net.kin_grid, float)
    edges = grid[grid <= 16.0]
    mids = [0.5 * (a + b) for a, b in zip(edges[:-1], edges[1:]) if b - a >= 0.5]
    t = np.unique(np.concatenate([edges, mids]))
    return t[:15]


def step_reference(method, operator, net, p, rows, t, k, dtype=LD):
    """(y_ref, tau) of output row k: one step of t[k] - t[k-1] from row k - 1 of `rows` (a solver's own output), at the bucket of t[k-1]."""
    yn, _, maj = STEP[method](net, p, rows[k - 1], t[k - 1], t[k] - t[k - 1], operator, dtype)
    return yn, tau(maj)
