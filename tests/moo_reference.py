"""Numpy restatement of the many-objective bookkeeping (include/phoskin.h, the pk_moo_* block), written from the definitions there and
independent of the device code: dominance with ranks by peeling and by the chain rule, association in ``np.longdouble``, the sequential
niching loop (NOT the closed form the device evaluates; ``survive_closed`` restates that form for the CPU comparison of the two), the
counter-based random numbers in ``uint64``, tournament, bounded SBX and bounded polynomial mutation."""
import numpy as np

LD = np.longdouble
GOLD = np.uint64(0x9E3779B97F4A7C15)


# ---------------------------------------------------------------- dominance and ranks

def dominance(F):
    """D[a, b] = row a dominates row b.  A non-finite row dominates nothing and is dominated by every all-finite row."""
    F = np.asarray(F, float)
    fin = np.isfinite(F).all(axis=1)
    G = np.where(fin[:, None], F, 0.0)
    le = np.ones((F.shape[0],) * 2, bool)
    lt = np.zeros((F.shape[0],) * 2, bool)
    for m in range(F.shape[1]):                                 # one objective at a time: a P x P bool array, not P x P x M
        le &= G[:, None, m] <= G[None, :, m]
        lt |= G[:, None, m] < G[None, :, m]
    D = le & lt & fin[:, None] & fin[None, :]
    D |= fin[:, None] & ~fin[None, :]
    return D


def rank_peel(F, stop_at=0, D=None):
    """(rank [P] int32, n_fronts): front after front; with ``stop_at`` > 0 stop after the first front with which >= stop_at rows are
    ranked, the rest get rank = n_fronts.  ``D``: ``dominance(F)`` where the caller already holds it."""
    D = dominance(F) if D is None else D
    P = D.shape[0]
    rank = np.full(P, -1, np.int32)
    left = D.sum(axis=0)                                        # dominators of each row among the rows not yet peeled
    front = 0
    while (rank < 0).any() and (stop_at == 0 or (rank >= 0).sum() < stop_at):
        cur = (rank < 0) & (left == 0)
        assert cur.any()
        rank[cur] = front
        left -= D[cur].sum(axis=0)                              # the peeled rows dominate nobody any more
        front += 1
    rank[rank < 0] = front
    return rank, front


def rank_chain(F):
    """rank = 0 where nothing dominates the row, else 1 + max rank of its dominators (memoised depth in the dominance order)."""
    D = dominance(F)
    P = D.shape[0]
    rank = np.full(P, -1, np.int64)
    order = np.argsort(D.sum(axis=0), kind="stable")           # fewer dominators first: a dominator of b has strictly fewer than b
    for b in order:
        dom = np.nonzero(D[:, b])[0]
        assert (rank[dom] >= 0).all()
        rank[b] = 0 if dom.size == 0 else 1 + rank[dom].max()
    return rank.astype(np.int32)


# ---------------------------------------------------------------- association

def associate(F, ideal, nadir, dirs):
    """(niche [P] int32, dist [P] float64, all distances [P, H] longdouble).  Non-finite rows: niche -1, dist +inf."""
    F = np.asarray(F, float)
    fin = np.isfinite(F).all(axis=1)
    den = np.maximum(LD(1) * np.asarray(nadir, LD) - np.asarray(ideal, LD), LD(1e-12))
    f = (np.where(fin[:, None], F, 0.0).astype(LD) - np.asarray(ideal, LD)) / den
    w = np.asarray(dirs, LD)
    s = (f @ w.T) / (w * w).sum(axis=1)                         # [P, H]
    r = f[:, None, :] - s[:, :, None] * w[None, :, :]
    d = np.sqrt((r * r).sum(axis=2))
    niche = d.argmin(axis=1).astype(np.int32)                   # first minimum = lowest h
    dist = d[np.arange(F.shape[0]), niche].astype(np.float64)
    niche[~fin] = -1
    dist[~fin] = np.inf
    return niche, dist, d


# ---------------------------------------------------------------- survival

def _split(rank, K):
    """Rows of the whole fronts that fit, and the rows of the first front that does not."""
    rank = np.asarray(rank)
    taken = np.zeros(rank.size, bool)
    l = 0
    while True:
        cur = rank == l
        if taken.sum() + cur.sum() > K:
            return taken, cur
        taken |= cur
        if taken.sum() == rank.size or (rank > l).sum() == 0:
            return taken, np.zeros(rank.size, bool)
        l += 1


def survive_loop(rank, niche, dist, H, K):
    """Ascending indices of the K survivors by the sequential niching loop.  Within a niche rows go by (dist, index), a NaN dist last."""
    rank, niche, dist = np.asarray(rank), np.asarray(niche), np.asarray(dist)
    if K == 0:
        return np.zeros(0, np.int32)
    taken, last = _split(rank, K)
    rho = np.bincount(niche[taken & (niche >= 0)], minlength=H)
    left = [sorted(np.nonzero(last & (niche == j))[0], key=lambda i: (np.isnan(dist[i]), dist[i], i)) for j in range(H)]
    need = K - int(taken.sum())
    while need > 0 and any(left):
        j = min((j for j in range(H) if left[j]), key=lambda j: (rho[j], j))
        taken[left[j].pop(0)] = True
        rho[j] += 1
        need -= 1
    for i in np.nonzero(last & (niche < 0))[0][:need]:
        taken[i] = True
    out = np.nonzero(taken)[0].astype(np.int32)
    assert out.size == K
    return out


def survive_closed(rank, niche, dist, H, K):
    """The same survivors by the closed form (water level L, quotas c_j)."""
    rank, niche, dist = np.asarray(rank), np.asarray(niche), np.asarray(dist)
    if K == 0:
        return np.zeros(0, np.int32)
    taken, last = _split(rank, K)
    rho = np.bincount(niche[taken & (niche >= 0)], minlength=H)
    a = np.bincount(niche[last & (niche >= 0)], minlength=H)
    rest = K - int(taken.sum())
    kn = min(rest, int(a.sum()))
    S = lambda L: int(np.minimum(a, np.maximum(0, L - rho)).sum())
    L = 0
    while L < rank.size and S(L + 1) <= kn:
        L += 1
    c = np.minimum(a, np.maximum(0, L - rho))
    rem = kn - int(c.sum())
    for j in range(H):
        if rem > 0 and rho[j] <= L and c[j] < a[j]:
            c[j] += 1
            rem -= 1
    assert rem == 0
    for j in np.nonzero(c)[0]:
        rows = sorted(np.nonzero(last & (niche == j))[0], key=lambda i: (np.isnan(dist[i]), dist[i], i))
        taken[rows[:c[j]]] = True
    for i in np.nonzero(last & (niche < 0))[0][:rest - kn]:
        taken[i] = True
    out = np.nonzero(taken)[0].astype(np.int32)
    assert out.size == K
    return out


# ---------------------------------------------------------------- random numbers

def _mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform(seed, gen, stream, row, var, P, n_var):
    """u(stream, row, var) in [0, 1); ``row`` / ``var`` may be arrays (broadcast).  All arithmetic mod 2^64."""
    with np.errstate(over="ignore"):
        row = np.asarray(row).astype(np.uint64)
        var = np.asarray(var).astype(np.uint64)
        ctr = np.uint64(1) + ((np.uint64(gen) * np.uint64(8) + np.uint64(stream)) * np.uint64(P) + row) * np.uint64(n_var) + var
        z = _mix(np.uint64(seed) + GOLD * ctr)
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ---------------------------------------------------------------- mating

def tournament(rank, niche, dist, seed, gen, n_var):
    P = len(rank)
    c = np.arange(P)
    a = np.minimum(P - 1, np.floor(uniform(seed, gen, 0, c, 0, P, n_var) * P).astype(np.int64))
    b = np.minimum(P - 1, np.floor(uniform(seed, gen, 1, c, 0, P, n_var) * P).astype(np.int64))
    rank, niche, dist = np.asarray(rank), np.asarray(niche), np.asarray(dist)
    b_wins = (rank[b] < rank[a]) | ((rank[b] == rank[a]) & (niche[a] == niche[b]) & (dist[b] < dist[a]))
    return np.where(b_wins, b, a).astype(np.int32)


def _betaq(u, beta, e):
    alpha = 2.0 - beta ** (-e)
    return (u * alpha) ** (1.0 / e) if u <= 1.0 / alpha else (1.0 / (2.0 - u * alpha)) ** (1.0 / e)


def mate(X, rank, niche, dist, xl, xu, seed, gen, pc, eta_c, pm, eta_m):
    """(Xc [P, n_var], parents [P]) -- scalar loops, one branch per line of the definition."""
    X = np.asarray(X, float)
    P, n = X.shape
    par = tournament(rank, niche, dist, seed, gen, n)
    Xc = np.empty_like(X)
    vs = np.arange(n)[None, :]
    U = {s: uniform(seed, gen, s, np.arange(P)[:, None], vs, P, n) for s in (3, 4, 5, 6, 7)}      # [row, var]; rows = pairs for 3 .. 5
    for q in range((P + 1) // 2):
        c0, c1 = 2 * q, 2 * q + 1
        two = c1 < P
        x0 = X[par[c0]].copy()
        x1 = X[par[c1]].copy() if two else x0.copy()
        if two and uniform(seed, gen, 2, q, 0, P, n) <= pc:
            for v in range(n):
                if U[3][q, v] <= 0.5 and abs(x0[v] - x1[v]) > 1e-14 and xu[v] > xl[v]:
                    y1, y2 = min(x0[v], x1[v]), max(x0[v], x1[v])
                    u = float(U[4][q, v])
                    e = eta_c + 1.0
                    k1 = 0.5 * ((y1 + y2) - _betaq(u, 1.0 + 2.0 * (y1 - xl[v]) / (y2 - y1), e) * (y2 - y1))
                    k2 = 0.5 * ((y1 + y2) + _betaq(u, 1.0 + 2.0 * (xu[v] - y2) / (y2 - y1), e) * (y2 - y1))
                    k1, k2 = min(max(k1, xl[v]), xu[v]), min(max(k2, xl[v]), xu[v])
                    if U[5][q, v] <= 0.5:
                        k1, k2 = k2, k1
                    x0[v], x1[v] = k1, k2
        for c, x in ((c0, x0),) + (((c1, x1),) if two else ()):
            for v in range(n):
                if xu[v] > xl[v] and U[6][c, v] <= pm:
                    u = float(U[7][c, v])
                    w, e = xu[v] - xl[v], eta_m + 1.0
                    d1, d2 = (x[v] - xl[v]) / w, (xu[v] - x[v]) / w
                    if u < 0.5:
                        dq = (2.0 * u + (1.0 - 2.0 * u) * (1.0 - d1) ** e) ** (1.0 / e) - 1.0
                    else:
                        dq = 1.0 - (2.0 * (1.0 - u) + 2.0 * (u - 0.5) * (1.0 - d2) ** e) ** (1.0 / e)
                    x[v] = min(max(x[v] + dq * w, xl[v]), xu[v])
            Xc[c] = x
    return Xc, par
