"""Step-for-step restatement of the lane-group integrator (solve_kernel of csrc/pk_solve_kernel.hpp), shared by
tests/test_group_reference_cpu.py and tests/test_gpu_group_matrix.py (not a test module).  Plain numpy on the dense S x S system: no torch,
no library.  Every implicit stage is a dense solve with W = g I - J (numpy.linalg.solve: LAPACK's row-pivoted LU), which shares no
elimination order with the device's arrow, cyclic-reduction or Gauss-Jordan solvers.

    one_step    the update of one step of size hs, as the kernel writes it:
                  LRP12 / LRP8 / RODAS4, resolvent form   z_1 = W^-1 f(y) / GAM, z_{k+1} = gW W^-1 z_k, gW = 1 / (GAM hs);
                                                          y+ = y + sum B_k z_k, err = sum E_k z_k
                  RODAS4, classical form                  the six stages u_1 .. u_6 with A_ij, C_ij / hs; err = u_6
                  BDF1 (fewer than two rows of history)   p = y + hs f(y), (I / hs - J) d = f(p) - (p - y) / hs, y+ = p + d, err = d / 2
                  BDF2, w = hs / h_{n-1}                  a1, a2, beta, the quadratic predictor p and ecoef of the kernel's comments;
                                                          (I / (beta hs) - J) d = f(p) - (p - a1 y + a2 y_{n-1}) / (beta hs), err = ecoef d
                  RK4                                     one sub-step
                with the majorant of the update: the element-wise sum of the magnitudes of the terms it adds.  tau = |majorant|_inf 2^-53
                is the unit in which a double-precision evaluation of the same update may differ from this one.
    integrate   the free-running loop around it: first step, truncation to the output times, the controller with its clamps, the
                rejection rules, BDF2's step-ratio limit, RK4's sub-step count.

J and b come from oracle/protein_models.py; the tables are the literals of the HIP source, read with the parser of
tests/test_integrator_tables.py (which proves them against multi-precision derivations) and rounded to double as the compiler rounds them.
With dtype=numpy.longdouble (64-bit mantissa on x86) every solve is the double-precision LU refined four times on a long-double residual."""
from pathlib import Path

import numpy as np
import scipy.linalg as sla

from oracle import protein_models as pm
from test_integrator_tables import _literals

LD = np.longdouble
U = 2.0 ** -53
CSRC = Path(__file__).resolve().parents[1] / "phoskintime_amd" / "csrc"
ST_NONFINITE, ST_MAXSTEPS, ST_HMIN = 1, 2, 4
RESOLVENT = ("lrp12", "lrp8", "rodas4")
#: (method, form) of every one-step update the lane-group kernel has
UPDATES = (("lrp12", "resolvent"), ("lrp8", "resolvent"), ("rodas4", "resolvent"), ("rodas4", "stage"), ("bdf2", "resolvent"), ("rk4", "resolvent"))


def _tables():
    src = (CSRC / "pk_solve_kernel.hpp").read_text()
    one = lambda text, name: float(_literals(text, name)[0])
    tab = {}
    for key, name in (("lrp8", "PK_METHOD_LRP8"), ("lrp12", "PK_METHOD_LRP12")):
        blk = src[src.index("struct ResolventTab<%s>" % name):]
        blk = blk[:blk.index("\n};")]
        tab[key] = dict(GAM=one(blk, "GAM"), Q=one(blk, "Q"), B=[float(x) for x in _literals(blk, "B")], E=[float(x) for x in _literals(blk, "E")])
        assert len(tab[key]["B"]) == len(tab[key]["E"]) == int(one(blk, "NS"))
    r4 = src[src.index("namespace r4 {"):src.index("}  // namespace r4")]
    tab["rodas4"] = dict(GAM=one(r4, "GAM"), Q=4.0, B=[one(r4, "RB%d" % k) for k in range(1, 7)], E=[0.0] + [one(r4, "RE%d" % k) for k in range(2, 7)])
    tab["stage"] = {"%s%d%d" % (c, i, j): one(r4, "%s%d%d" % (c, i, j)) for c, top in (("A", 5), ("C", 6)) for i in range(2, top + 1) for j in range(1, i)}
    return tab


TAB = _tables()


def system(model, theta, n):
    """(J, b) of dy/dt = J y + b in double, as the oracle states them."""
    th = np.asarray(theta, float)
    J = pm.jacobian_analytic(model, th, n)
    return J, pm.rhs(model, np.zeros(J.shape[0]), 0.0, th, n)


class _Solver:
    """x = W^-1 r for W = g I - J.  float: numpy.linalg.solve.  long double: double LU + four refinement passes on a long-double residual."""

    def __init__(self, J, g, dtype):
        self.dtype = dtype
        self.W = g * np.eye(J.shape[0], dtype=dtype) - J.astype(dtype)
        self.lu = None if dtype is float else sla.lu_factor(self.W.astype(float))

    def __call__(self, r):
        if self.dtype is float:
            return np.linalg.solve(self.W, r)
        x = sla.lu_solve(self.lu, r.astype(float)).astype(LD)
        for _ in range(4):
            x = x + sla.lu_solve(self.lu, (r - self.W @ x).astype(float)).astype(LD)
        return x


def _step(method, form, J, b, y, hs, history, dtype):
    D = dtype
    J_, b_ = J.astype(D), b.astype(D)
    y = np.asarray(y, dtype=D)
    hs = D(hs)
    one = D(1)
    f = lambda v: J_ @ v + b_
    if method == "rk4":
        k1 = f(y); k2 = f(y + D(0.5) * hs * k1); k3 = f(y + D(0.5) * hs * k2); k4 = f(y + hs * k3)
        w = hs / D(6)
        return y + w * ((k1 + k4) + D(2) * (k2 + k3)), np.zeros_like(y), np.abs(y) + w * (np.abs(k1) + np.abs(k4) + D(2) * (np.abs(k2) + np.abs(k3)))
    if method in RESOLVENT:
        hinv = one / hs
        if form == "resolvent" or method != "rodas4":
            t = TAB[method]
            gam_inv = one / D(t["GAM"])
            gW = hinv * gam_inv
            solve = _Solver(J, gW, D)
            z = solve(f(y)) * gam_inv
            yn = y + D(t["B"][0]) * z
            maj = np.abs(y) + abs(t["B"][0]) * np.abs(z)
            err = np.zeros_like(y)
            for k in range(1, len(t["B"])):
                z = solve(z) * gW
                yn = yn + D(t["B"][k]) * z
                err = err + D(t["E"][k]) * z
                maj = maj + abs(t["B"][k]) * np.abs(z)
            return yn, err, maj
        c = {k: D(v) for k, v in TAB["stage"].items()}
        solve = _Solver(J, hinv / D(TAB["rodas4"]["GAM"]), D)
        u1 = solve(f(y))
        u2 = solve(f(y + c["A21"] * u1) + c["C21"] * hinv * u1)
        u3 = solve(f(y + (c["A31"] * u1 + c["A32"] * u2)) + hinv * (c["C31"] * u1 + c["C32"] * u2))
        u4 = solve(f(y + (c["A41"] * u1 + c["A42"] * u2 + c["A43"] * u3)) + hinv * (c["C41"] * u1 + c["C42"] * u2 + c["C43"] * u3))
        yn = y + (c["A51"] * u1 + c["A52"] * u2 + c["A53"] * u3 + c["A54"] * u4)
        u5 = solve(f(yn) + hinv * (c["C51"] * u1 + c["C52"] * u2 + c["C53"] * u3 + c["C54"] * u4))
        yn = yn + u5
        u6 = solve(f(yn) + hinv * (c["C61"] * u1 + c["C62"] * u2 + c["C63"] * u3 + c["C64"] * u4 + c["C65"] * u5))
        maj = (np.abs(y) + abs(c["A51"]) * np.abs(u1) + abs(c["A52"]) * np.abs(u2) + abs(c["A53"]) * np.abs(u3) + abs(c["A54"]) * np.abs(u4)
               + np.abs(u5) + np.abs(u6))
        return yn + u6, u6, maj
    assert method == "bdf2", method
    if history is None or len(history) < 2:
        g = one / hs
        solve = _Solver(J, g, D)
        fy = f(y)
        p = y + hs * fy
        d = solve(f(p) - g * (p - y))
        return p + d, D(0.5) * d, np.abs(y) + hs * np.abs(fy) + np.abs(d)
    (ym1, hm1), (ym2, hm2) = history[0], history[1]
    ym1, ym2, hm1, hm2 = np.asarray(ym1, dtype=D), np.asarray(ym2, dtype=D), D(hm1), D(hm2)
    w = hs / hm1
    a1 = (one + w) * (one + w) / (one + D(2) * w)
    a2 = w * w / (one + D(2) * w)
    beta = (one + w) / (one + D(2) * w)
    d1 = (y - ym1) / hm1
    d2 = (ym1 - ym2) / hm2
    dd = (d1 - d2) / (hm1 + hm2)
    p = y + hs * d1 + hs * (hs + hm1) * dd
    g = one / (beta * hs)
    solve = _Solver(J, g, D)
    d = solve(f(p) - g * (p - a1 * y + a2 * ym1))
    ecoef = beta * hs / (hs + hm1 + hm2 - beta * hs)
    return p + d, ecoef * d, np.abs(y) + np.abs(hs * d1) + np.abs(hs * (hs + hm1) * dd) + np.abs(d)


def one_step(method, form, model, theta, n, y, hs, history=None, dtype=float, sys=None):
    """(y_next, err_vector, majorant) of one step of size hs from y.  `history` (BDF2 only): [(y_{n-1}, h_{n-1}), (y_{n-2}, h_{n-2})], most
    recent first; with fewer than two entries the step is the BDF1 start-up, as in the kernel.  `sys`: system(model, theta, n), to spare
    forming it again."""
    J, b = sys if sys is not None else system(model, theta, n)
    return _step(method, form, J, b, y, hs, history, float if dtype is float else LD)


def tau(majorant):
    return float(np.max(np.abs(majorant))) * U


def err_norm(y, yn, err, rtol, atol):
    """The kernel's scaled max-norm of the error estimate (NaN-propagating)."""
    sc = rtol * np.maximum(np.abs(y), np.abs(yn)) + atol
    q = np.abs(err) / sc
    return float("nan") if np.isnan(q).any() else float(np.max(q))


def step_fac(root, lo=1.0 / 6.0, safety_inv=1.0 / 0.9):
    return max(lo, min(5.0, root * safety_inv))        # csrc/pk_step.hpp


def root_q(err, Q, root=np.float32):
    """err^(1/Q) as the kernel takes it (single precision log2 / exp2) or in double."""
    e = min(max(err, 1e-30), 1e30)
    if root is np.float32:
        return float(np.exp2(np.log2(np.float32(e)) * np.float32(1.0 / Q)))
    return float(e ** (1.0 / Q))


def integrate(method, form, model, theta, n, y0, t, rtol=1e-6, atol=1e-8, h0=0.0, rk4_h=1e-3, max_steps=100000, root=np.float32, dtype=float, trace=None):
    """The free-running loop of solve_kernel for one replica: (sol [T, S], status, (accepted, rejected)).  Rows after a failure are NaN.
    `trace`: a list that receives (hs, err) of every adaptive step attempted."""
    J, b = system(model, theta, n)
    D = float if dtype is float else LD
    t = np.asarray(t, float)
    T = t.size
    y = np.asarray(y0, dtype=D)
    sol = np.full((T, y.size), np.nan)
    sol[0] = y
    nacc = nrej = 0
    status = 0
    if T < 2:
        return sol, status, (0, 0)
    if method == "rk4":
        tc = t[0]
        for k in range(1, T):
            span = t[k] - tc
            nsub = max(int(np.ceil(span / rk4_h)), 1)
            if nacc + nsub > max_steps:
                return sol, status | ST_MAXSTEPS, (nacc, nrej)
            h = span / nsub
            for _ in range(nsub):
                y = _step("rk4", form, J, b, y, h, None, D)[0]
            nacc += nsub
            tc = t[k]
            if not np.isfinite(y).all():
                return sol, status | ST_NONFINITE, (nacc, nrej)
            sol[k] = y
        return sol, status, (nacc, nrej)
    fy = J @ np.asarray(y, float) + b
    sc = rtol * np.abs(np.asarray(y, float)) + atol
    d0, d1 = float(np.max(np.abs(np.asarray(y, float)) / sc)), float(np.max(np.abs(fy) / sc))
    h = 0.01 * d0 / d1 if (d0 > 1e-5 and d1 > 1e-5) else 1e-6        # step_h0
    if h0 > 0.0:
        h = h0
    if not (h > 0.0):
        h = 1e-6
    tc, k, te = t[0], 1, t[1]
    bdf = method == "bdf2"
    after_reject = False
    hist = []                                                         # BDF2: (y_{n-1}, h_{n-1}), (y_{n-2}, h_{n-2})
    nhist = 0
    while True:
        if nacc + nrej >= max_steps:
            status |= ST_MAXSTEPS
            break
        if bdf and nhist >= 1:
            h = min(h, 2.0 * hist[0][1])
        last = tc + 1.0001 * h >= te
        hs = te - tc if last else (0.5 * (te - tc) if tc + 2.0 * h > te else h)
        if not (hs > 1e-14 * max(abs(tc), 1e-3)):
            status |= ST_HMIN
            break
        yn, ev, _ = _step(method, form, J, b, y, hs, hist if nhist >= 2 else None, D)
        err = err_norm(np.asarray(y, float), np.asarray(yn, float), np.asarray(ev, float), rtol, atol)
        if trace is not None:
            trace.append((hs, err))
        if err != err or err > 1e300:
            nrej += 1
            after_reject = True
            h = 0.1 * hs
            if not np.isfinite(np.asarray(y, float)).all():
                status |= ST_NONFINITE
                break
            continue
        if bdf:
            fac = step_fac(np.sqrt(err) if nhist < 2 else np.cbrt(err), 0.5)
        else:
            fac = step_fac(root_q(err, TAB[method]["Q"], root))
        hnew = hs / fac
        if err <= 1.0:
            nacc += 1
            if bdf:
                hist = [(y, hs)] + hist[:1]
                nhist = min(nhist + 1, 2)
            y = yn
            tc += hs
            if after_reject and not bdf:
                hnew = min(hnew, hs)
            after_reject = False
            if last:
                tc = te
                sol[k] = y
                k += 1
                h = max(hnew, h) if hs < h else hnew                  # keep the untruncated proposal
                if k >= T:
                    break
                te = t[k]
            else:
                h = hnew
        else:
            nrej += 1
            after_reject = True
            h = hnew
    return sol, status, (nacc, nrej)


# ------------------------------------------------------------------------------------------------ the inputs of the two GPU matrices
#: free-running runs: the tolerances tests/test_gpu_parity.py gives each method, and its limit on the band error against the closed form
FREE = {("lrp12", "resolvent"): ({}, 0.1), ("lrp8", "resolvent"): (dict(rtol=1e-7, atol=1e-9), 0.1),
        ("rodas4", "resolvent"): (dict(rtol=1e-7, atol=1e-9), 0.1), ("rodas4", "stage"): (dict(rtol=1e-7, atol=1e-9), 0.1),
        ("bdf2", "resolvent"): (dict(rtol=1e-9, atol=1e-11, max_steps=2000000), 5.0)}
#: largest difference in accepted or rejected steps between integrate with a single-precision and with a double-precision root, over every
#: size of SIZES and the replicas COMPARED (tests/test_group_reference_cpu.py measures and asserts it).  BDF2 takes sqrt / cbrt in double.
ROOT_SPREAD = {"lrp12": 1, "lrp8": 0, "rodas4": 0, "bdf2": 0}
B = 37
COMPARED = (0, 18, 36)
SPACINGS = (0.02, 0.03, 0.05, 0.04, 0.07, 0.1, 0.15, 0.2, 0.35, 0.6, 1.0)
BDF2_C = (0.05, 0.08, 0.06, 0.1, 0.15, 0.12, 0.2, 0.3)
#: (model, lane-group width) -> n_sites: both sides of every width and the minimum
SIZES = {(pm.DIST, 8): (1, 6), (pm.DIST, 16): (7, 14), (pm.DIST, 32): (15, 30), (pm.DIST, 64): (31, 62),
         (pm.SUCC, 8): (1, 6), (pm.SUCC, 16): (7, 14), (pm.SUCC, 32): (15, 30), (pm.SUCC, 64): (31, 62),
         (pm.RAND, 8): (1, 2), (pm.RAND, 16): (3,), (pm.RAND, 32): (4,), (pm.RAND, 64): (5,)}


def case(model, n, batch=B):
    """(theta [37, P], y0 [37, S]) of one size: replicas 0-17 from U(0, 20), 18-36 log-uniform on [1e-3, 20]; y0 from U(0.2, 2) per replica.
    Another `batch` keeps the proportions (18 in 37 uniform, the rest log-uniform) and is a draw of its own."""
    rng = np.random.default_rng(20261020 + 1000 * model + n)
    P, S = pm.n_params(model, n), pm.n_states(model, n)
    lin = 18 * batch // B
    theta = np.empty((batch, P))
    theta[:lin] = rng.uniform(0.0, 20.0, (lin, P))
    theta[lin:] = np.exp(rng.uniform(np.log(1e-3), np.log(20.0), (batch - lin, P)))
    return theta, rng.uniform(0.2, 2.0, (batch, S))


def compared(batch=B):
    """The replicas every comparison is made on: first, middle, last (COMPARED at 37)."""
    return (0, batch // 2, batch - 1)


def forced(method, model, theta, n):
    """(t, solver options) of the forced grid, on which the kernel takes exactly one step per interval: h0 twice the largest spacing and
    rtol = atol = 1.  The implicit one-step methods take SPACINGS; BDF2 and RK4 take c / max_b |J_b|_inf, c from BDF2_C (step ratios below
    2, and inside RK4's stability region), RK4 with rk4_h = 0.125 / max_b |J_b|_inf: 1 to 3 sub-steps per interval, none on a tie of ceil."""
    opts = dict(rtol=1.0, atol=1.0)
    if method in ("bdf2", "rk4"):
        norm = max(np.abs(pm.jacobian_analytic(model, th, n)).sum(axis=1).max() for th in theta)
        dt = np.array(BDF2_C) / norm
        if method == "rk4":
            opts["rk4_h"] = 0.125 / norm
    else:
        dt = np.array(SPACINGS)
    opts["h0"] = 2.0 * float(dt.max())
    return np.concatenate(([0.0], np.cumsum(dt))), opts


def rk4_substeps(t, rk4_h):
    return [max(int(np.ceil((t[k] - t[k - 1]) / rk4_h)), 1) for k in range(1, len(t))]


def interval_reference(method, form, sys, rows, t, k, rk4_h=None, dtype=LD):
    """(y_ref, tau) of output row k restarted from the rows before it (`rows` [T, S]: a solver's own output): one step of t[k] - t[k-1],
    BDF2 with rows k-2 and k-3 as history once three rows exist, RK4 as its chain of sub-steps (tau summed over them)."""
    hs = t[k] - t[k - 1]
    if method == "rk4":
        nsub = max(int(np.ceil(hs / rk4_h)), 1)
        y, tt = rows[k - 1], 0.0
        for _ in range(nsub):
            y, _, maj = one_step("rk4", form, None, None, None, y, hs / nsub, dtype=dtype, sys=sys)
            tt += tau(maj)
        return y, tt
    hist = None
    if method == "bdf2" and k >= 3:
        hist = [(rows[k - 2], t[k - 1] - t[k - 2]), (rows[k - 3], t[k - 2] - t[k - 3])]
    y, _, maj = one_step(method, form, None, None, None, rows[k - 1], hs, history=hist, dtype=dtype, sys=sys)
    return y, tau(maj)


# ------------------------------------------------------------------------------------------------ the randmod and wide-chain kernels
#: the three groups of environment switches (read once per process: one child process each in tests/test_gpu_rand_matrix.py)
ENV_TWIN = {"PK_WIDE_RAND_EXACT": "2", "PK_RAND_LEVEL6": "1"}
ENV_ROWS = {"PK_RAND_PARITY56": "0", "PK_RAND_ROWS": "1"}
ENV_DEV = {"PK_RAND_PARITY56": "1", "PK_RAND_PARITY6_TB": "16", "PK_RAND_PARITY8_GRID": "512"}
ENV_GROUPS = ({}, ENV_TWIN, ENV_ROWS, ENV_DEV)
ALL3 = ("lrp12", "lrp8", "rodas4")


class Kernel:
    """One kernel instantiation outside the lane-group family, and what selects it: `env` (one of ENV_GROUPS) and `kernel` (the
    solver option, None for "auto"), at batch size B; `plan` is the ProteinKernel protein_plan answers with, `L` the longest accumulation
    of its linear solve (tests/test_gpu_rand_matrix.py says where each one is read)."""

    def __init__(self, name, model, n, methods, plan, L, env=None, kernel=None, batch=B):
        self.name, self.model, self.n, self.methods, self.plan, self.L = name, model, n, methods, plan, L
        self.env, self.kernel, self.B = ENV_GROUPS[0] if env is None else env, kernel, batch

    @property
    def S(self):
        return pm.n_states(self.model, self.n)

    def __repr__(self):
        return "%s n=%d" % (self.name, self.n)


def _chain_L(model, n):
    """distmod: the arrow solve sums the n site rows and the two pivots (S terms); succmod: parallel cyclic reduction adds two terms to
    a row at each of its ceil(log2 S) levels."""
    S = n + 2
    return S if model == pm.DIST else 2 * int(np.ceil(np.log2(S))) + 1


#: wide_chain_kernel: the first size past the lane groups, both sides of the launcher's change from 128 to 256 threads (S = 128 | 129), and
#: the smallest size at which a thread strides over two rows (S = 257 > 256 threads); wide_chain_fits holds up to n = 1276
CHAIN_SIZES = (63, 126, 127, 255)
KERNELS = tuple(
    [Kernel("rand_fast_kernel<%d>" % n, pm.RAND, n, ALL3, "RandFast", 2 ** n) for n in (1, 2)]
    + [Kernel("rand_fast_kernel<%d>" % n, pm.RAND, n, ALL3, "RandFast", 2 ** n, env=ENV_ROWS) for n in (3, 4, 6)]
    + [Kernel("rand_fastr_kernel<%d,%d>" % (n, rpl), pm.RAND, n, ALL3, "RandFast", 2 ** n) for n, rpl in ((3, 2), (4, 4), (5, 2))]
    + [Kernel("tpr_rand_kernel<%d>" % n, pm.RAND, n, ("lrp12",), "Tpr", 2 ** n, kernel="tpr") for n in (1, 2, 3)]
    + [Kernel("rand_parity_kernel<6,8>", pm.RAND, 6, ("lrp12",), "RandParity", 32),
       Kernel("rand_parity_kernel<7,16>", pm.RAND, 7, ("lrp12",), "RandParity", 64),
       Kernel("rand_parity_kernel<7,8>", pm.RAND, 7, ("lrp12",), "RandParity", 64, batch=1024),
       Kernel("rand_parity_kernel<8,16,16>", pm.RAND, 8, ("lrp12",), "RandParity", 128),
       Kernel("rand_parity_kernel<5,4>", pm.RAND, 5, ("lrp12",), "RandParity", 16, env=ENV_DEV),
       Kernel("rand_parity_kernel<6,16>", pm.RAND, 6, ("lrp12",), "RandParity", 32, env=ENV_DEV),
       Kernel("rand_parity_kernel<8,16,32>", pm.RAND, 8, ("lrp12",), "RandParity", 128, env=ENV_DEV),
       Kernel("rand_level_kernel<6>", pm.RAND, 6, ("lrp12",), "RandLevel", 20, env=ENV_TWIN),
       Kernel("rand_level_kernel<8>", pm.RAND, 8, ("lrp12",), "RandLevel", 70, env=ENV_TWIN),
       Kernel("rand_dense_kernel<7>", pm.RAND, 7, ("lrp12",), "RandDense", 128, env=ENV_TWIN)]
    + [Kernel("wide_chain_kernel<%s>" % ("M_DIST" if model == pm.DIST else "M_SUCC"), model, n, ("lrp12",), "WideChain", _chain_L(model, n))
       for model in (pm.DIST, pm.SUCC) for n in CHAIN_SIZES])
#: every (model, n, batch, method) the table integrates, once
KERNEL_CASES = tuple(dict.fromkeys((k.model, k.n, k.B, m) for k in KERNELS for m in k.methods))
#: the double-precision restatement's own |y64 - yld|_inf / tau on the forced grid of each of those cases, worst over the compared
#: replicas and every row, rounded up to one decimal (tests/test_group_reference_cpu.py measures it and holds it below this figure);
#: L x this is where a ratio of tests/test_gpu_rand_matrix.py becomes a finding
KERNEL_R64 = {(pm.RAND, 1, B): (0.6, 1.3, 2.0), (pm.RAND, 2, B): (0.9, 1.2, 2.3), (pm.RAND, 3, B): (2.6, 1.6, 1.8), (pm.RAND, 4, B): (1.5, 2.3, 2.6),
              (pm.RAND, 5, B): (1.3, 1.3, 2.7), (pm.RAND, 6, B): (2.2, 1.6, 2.7), (pm.RAND, 7, B): (2.2,), (pm.RAND, 7, 1024): (2.2,),
              (pm.RAND, 8, B): (2.3,), (pm.DIST, 63, B): (2.6,), (pm.DIST, 126, B): (1.9,), (pm.DIST, 127, B): (2.3,), (pm.DIST, 255, B): (2.6,),
              (pm.SUCC, 63, B): (0.6,), (pm.SUCC, 126, B): (0.9,), (pm.SUCC, 127, B): (1.3,), (pm.SUCC, 255, B): (0.7,)}
KERNEL_R64 = {(model, n, batch, m): r for (model, n, batch), rs in KERNEL_R64.items() for m, r in zip(ALL3, rs)}
#: the same figure for the text of tpr_rand_kernel<1> (a 2 x 2 Gauss-Jordan inverse and FMA dot products) evaluated in correctly rounded
#: double on the CPU, where tests/test_group_reference_cpu.py measures 1.11: the elimination order of that kernel, not LAPACK's
TPR1_TEXT_R64 = 1.2
#: runs whose step counts the controller's clamps set (tests/test_gpu_rand_matrix.py, b): GROWTH has err ~ 0, so every step from h0 up to
#: the grid's spacings grows by the growth clamp's factor 6; SHRINK starts three decades above what its tolerances accept, so its first
#: 9 to 14 steps are rejected at the shrink clamp's factor 5 and the steps after them go through the after-reject rule
GROWTH = dict(rtol=1.0, atol=1.0, h0=1e-13)
SHRINK = dict(rtol=1e-12, atol=1e-14, h0=1e7)
SHRINK_T = np.array([0.0, 1e6, 2e6])
#: largest difference in (accepted, rejected) steps of the SHRINK run between a single- and a double-precision root, over KERNEL_CASES' LRP12
#: cases and the compared replicas (tests/test_group_reference_cpu.py); GROWTH has none: its root is the clamped 1e-30^(1/11) in both
SHRINK_SPREAD = (2, 1)
