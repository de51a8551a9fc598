"""Pins the CPU oracle of joint-velocity weights (tests/chain_rest.py):

1. with all-zero weights it returns oracle.chain_batch.ChainOracle's and chain_path.PathCost's
   arrays bit for bit (cost, quadratizations, gains, forward pass, fit);
2. its gradients and Hessians match central differences of its own cost, with the path-oracle
   test's steps and tolerances (tests/test_chain_path_oracle.py: h = 1e-6 and 1e-6 of the largest
   entry for gradients, h = 1e-4 and 1e-5 for Hessians), and the velocity block is exactly
   diag(2·weight) with nothing else in its rows and columns;
3. chain_rest.Rowless through chain_path.fit is ChainOracle.fit bit for bit, so the fixture
   generator's log of line-search margins describes the fit it stores;
4. the weights are read: they change cost and gains; and the fixtures of
   tests/test_gpu_chain_rest.py hold what their generator asserts.
Small shapes (four joints, B = 2, T = 4): the loops are pure Python."""
import json
import os

import numpy as np
import pytest

import chain_path as CP
import chain_rest as CR
from ilqr_amd.chain import coupled_chain_problem, rbd_initial_states
from oracle.chain_batch import ChainOracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, B, T = 4, 2, 4
PW = 50.0
VW, VFW = CR.weights(N, *CR.TASK_W)
ZERO = np.zeros(N)


@pytest.fixture(scope="module")
def case():
    pr = coupled_chain_problem(N)
    f = CP.Dynamics(pr)
    u = np.random.default_rng(3).uniform(-0.5, 0.5, (B, T, N))
    x = CP.rollout(f, rbd_initial_states(B, N, seed0=81), u)
    xt = 0.1 * CP.rollout(f, rbd_initial_states(B, N, seed0=7), 0.5 * u[::-1])
    goal = CP.tool_positions(pr, x[:, -1]).mean(0) + np.array([0.01, -0.02, 0.015])
    return pr, f, x, u, xt, goal


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(bits(a), bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b)


def oracles(pr, goal, mode, vw, vfw):
    """(ChainOracle, RestOracle) of a mode: "joint", "targets" (a goal per trajectory) or "task"."""
    kw = {}
    if mode == "targets":
        kw["targets"] = np.asarray(pr.target) + np.array([[0.1] * N, [-0.2] * N])
    if mode == "task":
        kw["task"] = CR.task_dict(pr, goal)
    return ChainOracle(pr, T, **kw), CR.RestOracle(pr, T, vw, vfw, **kw)


@pytest.mark.parametrize("mode", ["joint", "targets", "task"])
def test_zero_weights_are_chain_oracle(case, mode):
    pr, f, x, u, xt, goal = case
    base, rest = oracles(pr, goal, mode, ZERO, ZERO)
    X, U = x[:, :T].reshape(-1, 2 * N), u.reshape(-1, N)
    assert same(base.l(X, U), rest.l(X, U)) and same(base.lf(x[:, T]), rest.lf(x[:, T]))
    for a, b in zip(base.quad(X, U) + base.fquad(x[:, T]), rest.quad(X, U) + rest.fquad(x[:, T])):
        assert same(a, b)
    (d, K), = base.backward(x, u, [0.01])
    (d2, K2), = rest.backward(x, u, [0.01])
    assert same(d, d2) and same(K, K2)
    prev = np.full(B, np.inf)
    for a, b in zip(base.forward(x, u, d, K, prev), rest.forward(x, u, d, K, prev)):
        assert same(a, b)
    got, want = rest.fit(x, u, max_iter=3), base.fit(x, u, max_iter=3)
    for k in ("x", "u", "cost", "iters", "status"):
        assert same(got[k], want[k]), k


@pytest.mark.parametrize("euclidean", [True, False])
def test_zero_weights_are_path_cost(case, euclidean):
    pr, f, x, u, xt, goal = case
    base = CP.PathCost(pr.chain, N - 1, CP.POINT, CP.WEIGHT, PW, euclidean)
    rest = CR.RestPathCost(pr.chain, N - 1, CP.POINT, CP.WEIGHT, PW, euclidean, ZERO, ZERO)
    path = CP.smooth_path(pr, x, euclidean, seed=1, amp=0.05)
    ta, tb = CP.tiles(x, u, path, f, base), CP.tiles(x, u, path, f, rest)
    for k in ta:
        assert same(ta[k], tb[k]), k
    d, K, _ = CP.backward(x, u, path, f, base)
    z, prev = np.zeros_like(x), np.full(B, np.inf)
    for a, b in zip(CP.forward_pass(x, u, z, d, K, prev, f, path, base), CP.forward_pass(x, u, z, d, K, prev, f, path, rest)):
        assert same(a, b)
    got, want = CP.fit(x, u, f, path, rest, max_iter=2), CP.fit(x, u, f, path, base, max_iter=2)
    for k in ("x", "u", "cost", "iters", "status"):
        assert same(got[k], want[k]), k


def grad_fd(fn, z, h=1e-6):
    g = np.zeros(len(z))
    for i in range(len(z)):
        e = np.zeros(len(z))
        e[i] = h
        g[i] = (fn(z + e) - fn(z - e)) / (2 * h)
    return g


def hess_fd(fn, z, h=1e-4):
    m = len(z)
    H = np.zeros((m, m))
    E = np.eye(m) * h
    for i in range(m):
        for j in range(m):
            H[i, j] = (fn(z + E[i] + E[j]) - fn(z + E[i] - E[j]) - fn(z - E[i] + E[j]) + fn(z - E[i] - E[j])) / (4 * h * h)
    return H


def close(a, b, tol):
    return np.abs(a - b).max() <= tol * np.abs(b).max()


def velocity_block_exact(g, H, X, w):
    """The velocity rows: g = 2w·q̇, H's block diag(2w), nothing else in its rows and columns."""
    assert np.array_equal(g[:, N:], 2 * w * X[:, N:])
    for p in range(len(H)):
        assert np.array_equal(H[p, N:, N:], np.diag(2 * w)) and not H[p, :N, N:].any() and not H[p, N:, :N].any()
        assert np.array_equal(H[p], H[p].T)


@pytest.mark.parametrize("mode", ["joint", "targets", "task"])
def test_quadratization_matches_central_differences(case, mode):
    pr, f, x, u, xt, goal = case
    vw, vfw = CR.weights(N, *(CR.TASK_W if mode == "task" else CR.JOINT_W))
    _, o = oracles(pr, goal, mode, vw, vfw)
    # one point per trajectory, so that a goal per trajectory lines up with the rows
    X, U, XN = x[:, 2], u[:, 2], x[:, T]
    lx, lu, lxx, lux, luu = o.quad(X, U)
    lfx, lfxx = o.fquad(XN)
    assert not lux.any()
    velocity_block_exact(lx, lxx, X, vw)
    velocity_block_exact(lfx, lfxx, XN, vfw)
    for p in range(B):
        fx = lambda z: o.l(np.where(np.arange(B)[:, None] == p, z, X), U)[p]   # noqa: E731
        fu = lambda v: o.l(X, np.where(np.arange(B)[:, None] == p, v, U))[p]   # noqa: E731
        ff = lambda z: o.lf(np.where(np.arange(B)[:, None] == p, z, XN))[p]    # noqa: E731
        assert close(lx[p], grad_fd(fx, X[p]), 1e-6) and close(lu[p], grad_fd(fu, U[p]), 1e-6), p
        assert close(lxx[p], hess_fd(fx, X[p]), 1e-5) and close(luu[p], hess_fd(fu, U[p]), 1e-5), p
        assert close(lfx[p], grad_fd(ff, XN[p]), 1e-6) and close(lfxx[p], hess_fd(ff, XN[p]), 1e-5), p


@pytest.mark.parametrize("euclidean", [True, False])
def test_path_quadratization_matches_central_differences(case, euclidean):
    pr, f, x, u, xt, goal = case
    cost = CR.RestPathCost(pr.chain, N - 1, CP.POINT, CP.WEIGHT, PW, euclidean, VW, VFW)
    path = CP.smooth_path(pr, x, euclidean, seed=1, amp=0.05)
    X, U, rows = x[:, 1:3].reshape(-1, 2 * N), u[:, 1:3].reshape(-1, N), path[:, 1:3].reshape(-1, 3)
    lx, lu, lxx, lux, luu = cost.quad(X, U, rows)
    lfx, lfxx = cost.fquad(x[:, T], path[:, T])
    assert not lux.any()
    velocity_block_exact(lx, lxx, X, VW)
    velocity_block_exact(lfx, lfxx, x[:, T], VFW)
    for p in range(len(X)):
        fx = lambda z: cost.stage(z, U[p], rows[p])  # noqa: E731
        fu = lambda v: cost.stage(X[p], v, rows[p])  # noqa: E731
        assert close(lx[p], grad_fd(fx, X[p]), 1e-6) and close(lu[p], grad_fd(fu, U[p]), 1e-6), p
        assert close(lxx[p], hess_fd(fx, X[p]), 1e-5) and close(luu[p], hess_fd(fu, U[p]), 1e-5), p
    for b in range(B):
        ff = lambda z: cost.final(z, path[b, T])  # noqa: E731
        assert close(lfx[b], grad_fd(ff, x[b, T]), 1e-6) and close(lfxx[b], hess_fd(ff, x[b, T]), 1e-5), b


@pytest.mark.parametrize("mode", ["joint", "task"])
def test_rowless_through_chain_path_is_chain_oracle_fit(case, mode):
    pr, f, x, u, xt, goal = case
    vw, vfw = CR.weights(N, *(CR.TASK_W if mode == "task" else CR.JOINT_W))
    _, o = oracles(pr, goal, mode, vw, vfw)
    xo = o.rollout(x[:, 0], u)   # the oracle's own dynamics (the C step)
    log = []
    got = CP.fit(xo, u, o.dyn, CR.no_path(xo), CR.Rowless(o), max_iter=3, log=log)
    want = o.fit(xo, u, max_iter=3)
    for k in ("x", "u", "cost", "iters", "status"):
        assert same(got[k], want[k]), k
    for k in got["history"]:
        assert same(got["history"][k], want["history"][k]), k
    assert any(k != "gains" for k, _ in log)


def test_weights_and_x_traj_are_read(case):
    pr, f, x, u, xt, goal = case
    vw, vfw = CR.weights(N, *CR.JOINT_W)
    base, rest = oracles(pr, goal, "joint", vw, vfw)
    (d, K), = base.backward(x, u, [0.01])
    (d2, K2), = rest.backward(x, u, [0.01])
    assert np.abs(K - K2).max() > 1e-3 * np.abs(K).max()
    prev = np.full(B, np.inf)
    a = rest.forward(x, u, d2, K2, prev)
    b = rest.forward(x, u, d2, K2, prev, x_traj=xt)
    c = base.forward(x, u, d2, K2, prev)
    assert np.abs(xt[:, :T, N:]).max() > 1e-3
    assert not np.array_equal(a[2], b[2]) and not np.array_equal(a[2], c[2])
    # the running term on x̄ − x_traj, the terminal one on the raw x̄_N
    xb, ub = b[0], b[1]
    qd = xb[:, :T, N:] - xt[:, :T, N:]
    want = sum(base.l(xb[:, t] - xt[:, t], ub[:, t]) for t in range(T)) + base.lf(xb[:, T]) \
        + (vw * qd * qd).sum((1, 2)) + (vfw * xb[:, T, N:] ** 2).sum(1)
    assert np.allclose(b[2], want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("n", [4, 7])
def test_fixtures_hold_their_conditions(n):
    path = os.path.join(GOLD, f"chain{n}c_rest_t16.npz")
    assert os.path.getsize(path) < 256 * 1024
    g = dict(np.load(path, allow_pickle=False))
    meta = json.loads(str(g["meta"]))
    assert g["x"].shape == g["x_traj"].shape == (5, 17, 2 * n) and g["u"].shape == (5, 16, n)
    assert np.array_equal(g["x"][:, 0], rbd_initial_states(5, n, seed0=81))
    assert np.abs(g["x_traj"][:, :, n:]).max() > 1e-3           # its velocity rows are read
    gains = dict(np.load(os.path.join(GOLD, f"chain{n}c_rest_gains_t16.npz"), allow_pickle=False))
    assert os.path.getsize(os.path.join(GOLD, f"chain{n}c_rest_gains_t16.npz")) < 256 * 1024
    for tag, w in (("joint", CR.JOINT_W), ("task", CR.TASK_W), ("path", CR.TASK_W)):
        vw, vfw = CR.weights(n, *w)
        assert np.array_equal(g[f"{tag}_v_weight"], vw) and np.array_equal(g[f"{tag}_vf_weight"], vfw)
        assert len(set(vw)) == len(set(vfw)) == n
        m = meta[tag]
        assert m["margin"] > 1e-9 and m["gain_change"] > 1e-3
        assert gains[f"{tag}_K"].shape == (5, 16, n, 2 * n) and np.isfinite(gains[f"{tag}_K"]).all()
        assert gains[f"{tag}_d"].shape == (5, 16, n) and np.isfinite(gains[f"{tag}_d"]).all()
        assert m["conv_margin"] > 1e-9 and (g[f"{tag}_conv_status"] == 1).all()
        for b, it in enumerate(g[f"{tag}_conv_iters"]):
            assert (g[f"{tag}_conv_trials"][b, :it] >= 1).all()
        assert np.isin(g[f"{tag}_fit_status"], (1, 2)).all() and (g[f"{tag}_fw_trials"] >= 1).all()
        for b, it in enumerate(g[f"{tag}_fit_iters"]):
            assert (g[f"{tag}_cond_trials"][b, :it] >= 1).all() and np.isfinite(g[f"{tag}_fit_cost"][b, :it]).all()
    assert g["path_path"].shape == (5, 17, 3)
