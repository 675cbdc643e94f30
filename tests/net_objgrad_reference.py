"""A plain-loop reference for the network objective and its gradient, independent of the kernel (helper, no tests).

``chain`` maps a trajectory ``Y [T, S]``, its tangents ``dY [T, S, K]``, the loss data, the loss mode, the physical candidate, the prior
centre and the lambdas to ``(pred, dpred, sums, dsums, F, dF)``: what ``pk_network_simulate_objective_grad_batch`` forms inside the
integrator.  ``np_point_loss_dpred`` / ``np_fold_tangent`` restate the two scalar derivatives of csrc/pk_network_loss_grad.hpp.

Every result comes with ``mag``: the sum of the absolute values of the elementary products that enter it, and ``n``: the number of terms,
so that a caller can bound the rounding difference between two evaluations of the same formula by (n + OPS) 2^-53 mag.  OPS counts the
operations (and libm ulps) of one term:

    pred   a, c: <= cnt - 1 additions each, one division                                      -> OPS_PRED  = 2 cnt + 1 (cnt <= 2^ns)
    dpred  da: <= cnt - 1 additions; p (1), p dc (1), the difference (1), / c_m (1),
           softplus' (1; applied to dY here, to dpred in the kernel: one more rounding)       -> OPS_DPRED = cnt + 6
    rho'   diff (1) and <= 8 operations; log x 2 (1 ulp each), tanh (2 ulp), sqrt (0.5)       -> OPS_RHO   = 16
    sums   w rho: OPS_RHO + 1 per term, then the running sum                                  -> OPS_SUMS  = OPS_RHO + 1
    dsums  w rho' (OPS_RHO + 1) times dpred (OPS_DPRED), one product, the running sum         -> OPS_DSUMS = OPS_RHO + OPS_DPRED + 2
    F      sums, times norm, times lambda, plus the prior (5 N terms of 3 operations, one division, one product)   -> OPS_SUMS + 8
    dF     dsums, times norm, times lambda, plus d prior (6 operations), times softplus'      -> OPS_DSUMS + 10

Mode 2 subtracts two logarithms; where they nearly cancel the relative error of the difference is unbounded, so its ``mag`` carries the
first-order effect of 2 (|log(diff + eps)| + |log(obs + eps)|) on x = (log - log) / 0.5 through d rho / dx and d rho' / dx.  Mode 5 adds
two terms of either sign; its ``mag`` is the sum of their absolute values."""
import math

import numpy as np

EPS = 1e-9
U = 2.0 ** -53
OPS_RHO = 16
CNT_MAX = 8            # the largest number of states behind one observable on the fixtures the tests use is asserted against this


def np_point_loss_dpred(mode, obs, pred):
    """(d rho / d pred, mag) of oracle.network_models.pointwise_loss(mode, obs - pred, obs, pred)."""
    diff = obs - pred
    if mode == 0:
        v = -(diff + diff)
        return v, abs(v)
    if mode == 1:
        v = -diff if abs(diff) <= 0.5 else -math.copysign(0.5, diff)
        return v, abs(v)
    if mode == 2:
        sh, oe = diff + EPS, obs + EPS
        if not sh > 0.0 or not oe > 0.0:
            return float("nan"), float("nan")
        ls, lo = math.log(sh), math.log(oe)
        x = 2.0 * (ls - lo)
        r = math.sqrt(1.0 + x * x)
        v = -0.5 * x / (r * sh)
        return v, abs(v) + 0.5 / (r ** 3 * sh) * 2.0 * (abs(ls) + abs(lo))
    if mode == 3:
        v = -math.copysign(1.0, diff) if abs(diff) > 20.0 else -math.tanh(diff)
        return v, abs(v)
    if mode == 4:
        v = -2.0 * diff / (1.0 + diff * diff)
        return v, abs(v)
    if mode == 5:
        q = abs(pred) + 1e-6
        t1, t2 = 2.0 * diff / q, (np.sign(pred) * diff * diff) / (q * q)
        return -t1 - t2, abs(t1) + abs(t2)
    if mode == 6:
        q = 1.0 + diff * diff
        v = -2.0 * diff / (q * q)
        return v, abs(v)
    v = -diff / math.sqrt(diff * diff + 1e-6)
    return v, abs(v)


def np_point_loss(mode, obs, pred):
    """(rho, mag): the value by the formulas of the oracle's pointwise_loss, with mode 2's conditioning term in mag."""
    diff = obs - pred
    if mode == 2:
        sh, oe = diff + EPS, obs + EPS
        if not sh > 0.0 or not oe > 0.0:
            return float("nan"), float("nan")
        ls, lo = math.log(sh), math.log(oe)
        x = 2.0 * (ls - lo)
        r = math.sqrt(1.0 + x * x)
        v = 0.25 * (r - 1.0)
        return v, abs(v) + 0.25 * abs(x) / r * 2.0 * (abs(ls) + abs(lo))
    if mode == 0:
        v = diff * diff
    elif mode == 1:
        v = 0.5 * diff * diff if abs(diff) <= 0.5 else 0.5 * (abs(diff) - 0.25)
    elif mode == 3:
        v = abs(diff) - 0.69314718056 if abs(diff) > 20.0 else math.log(math.cosh(diff))
    elif mode == 4:
        v = math.log(1.0 + diff * diff)
    elif mode == 5:
        v = diff * diff / (abs(pred) + 1e-6)
    elif mode == 6:
        v = diff * diff / (diff * diff + 1.0)
    else:
        v = math.sqrt(diff * diff + 1e-6) - 1e-3
    # modes 3 and 4 take the logarithm of a number >= 1 that carries its own rounding: an absolute error of a few 2^-53 whatever the value
    # (0.25 x OPS_RHO of them); mode 7 and the saturated branch of mode 3 subtract a constant
    return v, abs(v) + (0.69314718056 if mode == 3 and abs(diff) > 20.0 else 0.25 if mode in (3, 4) else 0.0) + (1e-3 if mode == 7 else 0.0)


def np_fold_tangent(a, c, da, dc):
    """(dp, mag) of p = max(a, eps) / max(c, eps) along (da, dc); the derivative through an active floor is 0."""
    cm = c if c > EPS else EPS
    p = (a if a > EPS else EPS) / cm
    t1 = da / cm if a > EPS else 0.0 * da
    t2 = p * dc / cm if c > EPS else 0.0 * dc
    return t1 - t2, np.abs(t1) + np.abs(t2)


def entries(net, ld):
    """[(modality, state indices, time index, baseline index, obs, w)] in the caller's (protein | rna | phospho) order."""
    oy, ns, comb = net.offset_y, net.n_sites, net.model == 2
    out = []
    for i, t, o, w in zip(ld["p_prot"], ld["t_prot"], ld["obs_prot"], ld["w_prot"]):
        cnt = (1 << int(ns[i])) if comb else 1 + int(ns[i])
        out.append((0, [int(oy[i]) + 1 + m for m in range(cnt)], int(t), int(ld["prot_base_idx"]), float(o), float(w)))
    for i, t, o, w in zip(ld["p_rna"], ld["t_rna"], ld["obs_rna"], ld["w_rna"]):
        out.append((1, [int(oy[i])], int(t), int(ld["rna_base_idx"]), float(o), float(w)))
    for i, j, t, o, w in zip(ld["p_pho"], ld["s_pho"], ld["t_pho"], ld["obs_pho"], ld["w_pho"]):
        idx = [int(oy[i]) + 1 + m for m in range(1 << int(ns[i])) if (m >> int(j)) & 1] if comb else [int(oy[i]) + 2 + int(j)]
        out.append((2, idx, int(t), int(ld["pho_base_idx"]), float(o), float(w)))
    return out


def chain(net, Y, dY, ld, mode, x, defaults, lambdas, cols, scl=None):
    """dict(pred [n], dpred [n, K], sums [3], dsums [3, K], F [3], dF [3, K], floors: number of active floors, and ``mag`` / ``n``: dicts
    with the same keys, see the module docstring).  ``x`` physical; ``lambdas`` = (protein, rna, phospho, prior); ``defaults`` may be
    None; ``cols`` [K]: the columns' indices into x; ``scl`` [K]: softplus'(raw) where dY is a derivative with respect to raw entries
    (it multiplies the prior term; dY carries it already).  The sums run in time-bucketed list order per modality -- entries sorted by
    time index, stable -- which is the order the loss handle keeps them in."""
    K = dY.shape[2]
    scl = np.ones(K) if scl is None else np.asarray(scl, float)
    ent = entries(net, ld)
    n = len(ent)
    pred, dpred = np.empty(n), np.empty((n, K))
    mpred, mdpred = np.empty(n), np.empty((n, K))
    sums, dsums, msums, mdsums = np.zeros(3), np.zeros((3, K)), np.zeros(3), np.zeros((3, K))
    cnt_terms = np.zeros(3, int)
    floors = 0
    order = sorted(range(n), key=lambda k: (ent[k][0], ent[k][2]))              # stable: list order inside a time bucket
    for k in order:
        m, idx, t, tb, obs, w = ent[k]
        assert len(idx) <= CNT_MAX
        a = 0.0; c = 0.0; da = np.zeros(K); dc = np.zeros(K); mda = np.zeros(K)
        for s in idx:
            a += Y[t, s]; c += Y[tb, s]; da = da + dY[t, s]; dc = dc + dY[tb, s]; mda = mda + np.abs(dY[t, s])
        floors += int(not a > EPS) + int(not c > EPS)
        cm = c if c > EPS else EPS
        p = (a if a > EPS else EPS) / cm
        dp, _ = np_fold_tangent(a, c, da, dc)
        mdp = (mda / cm if a > EPS else 0.0 * mda) + (np.abs(p * dc) / cm if c > EPS else 0.0 * dc)
        pred[k], dpred[k], mpred[k], mdpred[k] = p, dp, abs(p), mdp
        rho, mrho = np_point_loss(mode, obs, p)
        g, mg = np_point_loss_dpred(mode, obs, p)
        sums[m] += w * rho; msums[m] += w * mrho
        dsums[m] += (w * g) * dp; mdsums[m] += (w * mg) * mdp
        cnt_terms[m] += 1
    nK, N, sites = net.n_K, net.N, net.total_sites
    groups = [(nK, nK + 4 * N), (nK + 4 * N + sites, nK + 5 * N + sites)]      # A, B, C, D contiguous, then E
    prior = 0.0; dprior = np.zeros(K)
    lam = [float(v) for v in lambdas]
    if defaults is not None:
        acc = 0.0
        for lo, hi in groups:
            for q in range(lo, hi):
                d = (x[q] - defaults[q]) / (defaults[q] + 1e-6)
                acc += d * d
        prior = lam[3] * (acc / (5 * N))
        for q, col in enumerate(cols):
            if any(lo <= col < hi for lo, hi in groups):
                dprior[q] = lam[3] * 2.0 * (x[col] - defaults[col]) / (defaults[col] + 1e-6) ** 2 / (5 * N)
    norm = [1.0 / max(1e-6, float(np.sum(ld[k]))) for k in ("w_prot", "w_rna", "w_pho")]
    F, dF, mF, mdF = np.empty(3), np.empty((3, K)), np.empty(3), np.empty((3, K))
    for m in range(3):
        F[m] = sums[m] * norm[m] * lam[m] + prior
        mF[m] = msums[m] * norm[m] * abs(lam[m]) + abs(prior)
        dF[m] = dsums[m] * norm[m] * lam[m] + dprior * scl
        mdF[m] = mdsums[m] * norm[m] * abs(lam[m]) + np.abs(dprior * scl)
    nt = {"pred": 0, "dpred": 0, "sums": cnt_terms, "dsums": cnt_terms[:, None], "F": cnt_terms + 5 * N, "dF": cnt_terms[:, None]}
    return dict(pred=pred, dpred=dpred, sums=sums, dsums=dsums, F=F, dF=dF, floors=floors, n=nt,
                mag=dict(pred=mpred, dpred=mdpred, sums=msums, dsums=mdsums, F=mF, dF=mdF))


OPS = {"pred": 2 * CNT_MAX + 1, "dpred": CNT_MAX + 6, "sums": OPS_RHO + 1, "dsums": OPS_RHO + CNT_MAX + 6 + 2, "F": OPS_RHO + 1 + 8,
       "dF": OPS_RHO + CNT_MAX + 6 + 2 + 10}


def bound(res, key):
    """(n + OPS) 2^-53 mag for output ``key`` of a ``chain`` result."""
    return (res["n"][key] + OPS[key]) * U * res["mag"][key]


def softplus_prime(raw):
    raw = np.asarray(raw, float)
    return np.where(raw > 20.0, 1.0, 1.0 / (1.0 + np.exp(-raw)))


def oracle_ld(ld, net):
    """The loss data with the ``prot_map`` column oracle.network_models.loss_function indexes."""
    ns = np.asarray(net.n_sites)
    return dict(ld, prot_map=np.stack([np.asarray(net.offset_y), (1 << ns) if net.model == 2 else ns], axis=1))


LAM = (1.0, 0.5, 2.0, 0.7)
LAMD = dict(protein=1.0, rna=0.5, phospho=2.0, prior=0.7)
_CACHE = {}


def fixture_data(name):
    """Fixture ``name`` with its stored exact reference, the loss data the objective-gradient tests share (observations: candidate 0's
    reference predictions times exp(0.2 N(0, 1)), seed 3) and the prior centre (1.1 x candidate 0), made once."""
    import net_sens_reference as ref
    if name not in _CACHE:
        g, net, X = ref.fixture(name)
        gold = ref.load_golden(name)
        r0 = chain(net, gold["Y"][0], gold["dY"][0], loss_data(net, gold["t"]), 0, X[0], None, LAM, gold["cols"])
        ld = loss_data(net, gold["t"], seed=3, pred0=r0["pred"])
        assert ld["rna_base_idx"] > 0 and ld["prot_base_idx"] == 0 and ld["pho_base_idx"] == 0 and ld["t_rna"].min() >= ld["rna_base_idx"]
        _CACHE[name] = dict(g=g, net=net, X=X, gold=gold, ld=ld, ldo=oracle_ld(ld, net), defaults=X[0] * 1.1)
    return _CACHE[name]


def loss_data(net, t, seed=3, pred0=None):
    """Every protein / site at every time, rna from t = 4 on (rna_base_idx > 0), as tests/test_gpu_network_fused_rosw.py::_loss_data lays
    them out; weights U(0.5, 2); observations: ``pred0`` (the list-order predictions of a reference candidate) times exp(0.2 N(0, 1)),
    or |1 + 0.2 N(0, 1)| without it."""
    t = np.asarray(t, float)
    bidx = lambda t0: int(np.argmin(np.abs(t - float(t0))))
    ip = np.arange(t.size, dtype=np.int32); ir = np.where(t >= 4.0)[0].astype(np.int32)
    N, ns = net.N, np.asarray(net.n_sites)
    pp = np.asarray([i for i in range(N) for _ in range(int(ns[i]))], np.int32)
    ss = np.asarray([j for i in range(N) for j in range(int(ns[i]))], np.int32)
    ld = dict(p_prot=np.repeat(np.arange(N, dtype=np.int32), ip.size), t_prot=np.tile(ip, N),
              p_rna=np.repeat(np.arange(N, dtype=np.int32), ir.size), t_rna=np.tile(ir, N),
              p_pho=np.repeat(pp, ip.size), s_pho=np.repeat(ss, ip.size), t_pho=np.tile(ip, pp.size),
              prot_base_idx=bidx(0.0), rna_base_idx=bidx(4.0), pho_base_idx=bidx(0.0))
    rng = np.random.default_rng(seed)
    sizes = [ld["p_prot"].size, ld["p_rna"].size, ld["p_pho"].size]
    noise = [rng.standard_normal(s) for s in sizes]
    w = [rng.uniform(0.5, 2.0, s) for s in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)])
    for q, k in enumerate(("prot", "rna", "pho")):
        ld["obs_" + k] = (np.abs(1.0 + 0.2 * noise[q]) if pred0 is None else pred0[off[q]:off[q + 1]] * np.exp(0.2 * noise[q]))
        ld["w_" + k] = w[q]
    return ld
