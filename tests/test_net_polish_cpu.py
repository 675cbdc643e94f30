"""CPU: the host twin of the network fit (``global_model.polish.polish_batch(driver="python")``) with callbacks in place of its two
launches, on a small analytic least-squares problem with a box: 9 protein observations pred_i = exp(M_i . z) of the three fitted entries
z = x[cols] of a 6-entry candidate vector, F = (norm sum w (pred - obs)^2, 0, 0).  Entry 0 of every candidate is held and carries the
row's number, so the callbacks can tell whose trial point they score.

Rows and the reason each must end with:
  0  noisy observations, wide box                                          0  (ftol / xtol)
  1  the same, the box cuts off the minimum in entry z_0                   0, z_0 exactly on its bound
  2  starts ON that bound with the gradient pointing out                   0, z_0 never leaves the bound: every trial has it bit for bit
  3  lb = ub = start in two entries, the third on its lower bound          1  (empty free set), x = x0
  4  lb = ub = start                                                       1  (empty free set), x = x0
  5  the Jacobian callback flags it                                        4, x = clip(x0), status non-zero
  6  every trial of it is flagged                                          2  (damping budget), x = clip(x0), status non-zero
In a second problem the observations are the predictions at the start point, bit for bit: the gradient is exactly 0, reason 1.
With max_iter = 1 row 0 ends with reason 3 one accepted step from its start."""
import numpy as np

from phoskintime_amd.global_model import polish

COLS = np.array([1, 3, 4])
RNG = np.random.default_rng(5)
M = RNG.uniform(-0.6, 0.6, size=(9, 3))
W = RNG.uniform(0.5, 2.0, size=9)
ZT = np.array([0.4, -0.3, 0.8])
OBS = np.exp(M @ ZT) * np.exp(0.05 * RNG.standard_normal(9))
B = 7
LD = dict(w_prot=W, obs_prot=OBS, w_rna=np.zeros(0), obs_rna=np.zeros(0), w_pho=np.zeros(0), obs_pho=np.zeros(0))
LAM = (1.3, 1.0, 1.0, 0.0)
OBJ_W = (0.7, 1.0, 1.0)


def _problem():
    x0 = np.zeros((B, 6))
    x0[:, 0] = np.arange(B)
    x0[:, [2, 5]] = 7.5                                                # held entries: must come back untouched
    x0[:, COLS] = ZT * 0.5 + 0.3
    lb = np.tile(np.array([-5.0, -5.0, -5.0]), (B, 1)); ub = np.tile(np.array([5.0, 5.0, 5.0]), (B, 1))
    ub[1, 0] = 0.2                                                     # the free minimum has z_0 near 0.4
    ub[2, 0] = 0.2; x0[2, 1] = 0.2
    lb[3, :2] = ub[3, :2] = x0[3, COLS[:2]]
    x0[3, COLS[2]] = lb[3, 2] = 1.5                                    # beyond the minimum: the gradient points out of the box
    lb[4] = ub[4] = x0[4, COLS]
    return x0, lb, ub, OBS


def _launches(obs, seen):
    norm = 1.0 / W.sum()

    def pred_of(X):
        return np.exp(X[:, COLS] @ M.T)

    def jac(X):
        p = pred_of(X)
        st = np.where(X[:, 0] == 5, 2, 0).astype(np.int32)
        return p, p[:, :, None] * M[None], st

    def plain(X):
        rows = X[:, 0].astype(int)
        p = pred_of(X)
        F = np.zeros((X.shape[0], 3))
        F[:, 0] = (np.sum(W * (p - obs) ** 2, axis=1) * norm) * LAM[0]
        st = np.zeros(X.shape[0], np.int32)
        if seen["plain"] > 0:
            st[rows == 6] = 2
            F[rows == 6] = 1e12
        seen["plain"] += 1
        seen["trials"].append(X.copy())
        return F, st

    return jac, plain


def _run(max_iter=60, exact=False, **kw):
    x0, lb, ub, obs = _problem()
    ld = LD
    if exact:
        x0 = x0[:1]; lb = lb[0]; ub = ub[0]
        obs = np.exp(x0[:, COLS] @ M.T)[0]
        ld = dict(LD, obs_prot=obs)
    seen = dict(plain=0, trials=[])
    res = polish.polish_batch(None, None, ld, x0, None, COLS, lb=lb, ub=ub, obj_w=OBJ_W, lambdas=LAM, max_iter=max_iter,
                              driver="python", launches=_launches(obs, seen), net_shape=(1, 1, 0), want_g=True, **kw)
    return res, x0, lb, ub, obs, seen


def test_every_row_ends_with_its_reason_and_bound_variables_take_a_zero_step():
    res, x0, lb, ub, obs, seen = _run()
    assert list(res.reason) == [0, 0, 0, 1, 1, 4, 2], res.reason
    held = [0, 2, 5]
    assert np.array_equal(res.x[:, held], x0[:, held])
    z = res.x[:, COLS]
    assert np.all(z >= lb) and np.all(z <= ub)
    # rows 0: the free minimum, gradient of the cost ~ 0 against its scale
    assert np.linalg.norm(res.g[0]) < 1e-6 * max(1.0, res.cost[0])
    assert res.x[1, 1] == ub[1, 0] and res.x[2, 1] == ub[2, 0]         # exactly on the bound
    assert res.cost[1] > res.cost[0] and abs(res.cost[1] - res.cost[2]) <= 1e-8 * res.cost[1]
    # row 2 starts on the bound with the gradient pointing out: every point ever scored for it has the entry on the bound bit for bit
    n2 = 0
    for X in seen["trials"]:
        mine = X[X[:, 0] == 2]
        n2 += mine.shape[0]
        assert np.all(mine[:, 1] == ub[2, 0])
    assert n2 > 3
    assert np.array_equal(res.x[3], x0[3]) and np.array_equal(res.x[4], x0[4])
    assert np.array_equal(res.x[5], x0[5]) and res.status[5] == 2
    assert np.array_equal(res.x[6], x0[6]) and res.status[6] == 2
    assert not res.status[[0, 1, 2, 3, 4]].any()
    # the cost is 1/2 obj_w . F of the returned F
    assert np.array_equal(res.cost, polish.cost_of(res.F, OBJ_W))
    c = res.counters
    assert c["jacobian_phases"] == c["iterations"] == c["host_waits"] - c["trial_rounds"]
    assert c["launches"] == 3 + 3 * c["jacobian_phases"] + 3 * c["trial_rounds"]


def test_a_vanishing_gradient_is_reason_one():
    res, x0, *_ = _run(exact=True)
    assert list(res.reason) == [1] and np.array_equal(res.x, x0) and res.cost[0] == 0.0 and not res.g.any()
    assert res.counters["iterations"] == 1 and res.counters["trial_rounds"] == 0


def test_max_iter_one_and_zero():
    one, x0, lb, ub, _, _ = _run(max_iter=1)
    assert one.reason[0] == 3 and one.counters["iterations"] == 1 and not np.array_equal(one.x[0], x0[0])
    zero, *_ = _run(max_iter=0)
    assert (zero.reason == 3).all() and zero.counters == dict(iterations=0, simulated=B, launches=3, host_waits=0, jacobian_phases=0, trial_rounds=0)
    assert np.array_equal(zero.x[:, COLS], np.minimum(np.maximum(x0[:, COLS], lb), ub)) and one.cost[0] < zero.cost[0]


def test_trial_levels_do_not_change_a_row():
    a, *_ = _run(trial_levels=1)
    b, *_ = _run(trial_levels=3)
    keep = [0, 1, 2, 3, 4, 5]                     # row 6's stub flags by call count, not by point
    assert np.array_equal(a.x[keep], b.x[keep]) and np.array_equal(a.cost[keep], b.cost[keep]) and np.array_equal(a.reason, b.reason)


def test_covariance():
    res, *_ = _run()
    pc = polish.covariance(res.JTJ[0], res.cost[0], 9, 3)
    assert pc.shape == (3, 3) and np.allclose(pc, pc.T) and np.all(np.diag(pc) > 0)
    np.testing.assert_allclose(pc, np.linalg.inv(res.JTJ[0]) * (2.0 * res.cost[0] / 6), rtol=1e-12)
    assert polish.covariance(np.zeros((3, 3)), 1.0, 9, 3) is None
