"""Pins the CPU oracle of a tool path (tests/chain_path.py), which restates oracle.closure_fit's
forward pass and fit loop with the step index handed to the cost:

1. on a constant path (every row of trajectory b equal) it IS closure_fit.forward_pass /
   closure_fit.fit run with index-free closures of the same cost: the same bits;
2. its per-step gradient and Hessian, and the terminal ones, match central differences of its
   own cost. Bounds: with steps h the differences carry a truncation error O(h²) times a higher
   derivative and a rounding error ε|ℓ|/h (gradient, h = 1e-6) or ε|ℓ|/h² (Hessian, h = 1e-4):
   about 1e-10 and 1e-8 of |ℓ|, against derivatives no smaller than |ℓ| here — 1e-6 and 1e-5 of
   the largest entry leave two orders;
3. a path that is not constant changes the result (the step index is read), and the fixtures of
   tests/test_gpu_chain_path.py hold what their generator asserts.
Small shapes (four joints, B = 2, T = 4): the loops are pure Python."""
import json
import os

import numpy as np
import pytest

import chain_path as CP
from ilqr_amd.chain import coupled_chain_problem, rbd_initial_states
from oracle import closure_fit

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, B, T = 4, 2, 4
PW = 50.0


@pytest.fixture(scope="module")
def case():
    pr = coupled_chain_problem(N)
    f = CP.Dynamics(pr)
    u = np.random.default_rng(3).uniform(-0.5, 0.5, (B, T, N))
    x = CP.rollout(f, rbd_initial_states(B, N, seed0=81), u)
    return pr, f, x, u


def cost_of(pr, euclidean):
    return CP.PathCost(pr.chain, N - 1, CP.POINT, CP.WEIGHT, PW, euclidean)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.mark.parametrize("euclidean", [True, False])
def test_constant_path_is_closure_fit(case, euclidean):
    pr, f, x, u = case
    cost = cost_of(pr, euclidean)
    c = CP.tool_positions(pr, x[:, -1]) + np.array([[0.01, -0.02, 0.015], [-0.02, 0.01, 0.02]])
    path = np.repeat(c[:, None, :], T + 1, axis=1)
    cc = CP.ConstantClosures(cost, c)
    # the tiles and the gains
    tl = CP.tiles(x, u, path, f, cost)
    tr = closure_fit.derivative_tiles(x, u, f, cc.quad, cc.fquad)
    for k in tl:
        assert np.array_equal(bits(tl[k]), bits(tr[k])), k
    d, K, st = CP.backward(x, u, path, f, cost)
    assert (st == 0).all() and np.isfinite(K).all()
    # one forward pass: accepted from prev = ∞, and a search that has to shrink (prev just below
    # the full step's cost)
    xt = np.zeros_like(x)
    first = CP.forward_pass(x, u, xt, d, K, np.full(B, np.inf), f, path, cost)
    for prev in (np.full(B, np.inf), first[2] * (1.0 - 1e-3)):
        got = CP.forward_pass(x, u, xt, d, K, prev, f, path, cost, max_trials=6)
        want = closure_fit.forward_pass(x, u, xt, d, K, prev, f, cc.immediate_cost, cc.final_cost, max_trials=6)
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b)
    # the fit, with its history
    got = CP.fit(x, u, f, path, cost, max_iter=3)
    want = closure_fit.fit(x, u, f, cc.immediate_cost, cc.final_cost, cc.quad, cc.fquad, max_iter=3)
    for k in ("x", "u", "cost"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["iters"], want["iters"]) and np.array_equal(got["status"], want["status"])
    for k in got["history"]:
        assert np.array_equal(bits(got["history"][k]), bits(want["history"][k])), k


@pytest.mark.parametrize("euclidean", [True, False])
def test_quadratization_matches_central_differences(case, euclidean):
    pr, f, x, u = case
    cost = cost_of(pr, euclidean)
    path = CP.smooth_path(pr, x, euclidean, seed=1, amp=0.05)
    nx = 2 * N
    X, U, rows = x[:, 1:3].reshape(-1, nx), u[:, 1:3].reshape(-1, N), path[:, 1:3].reshape(-1, 3)
    lx, lu, lxx, lux, luu = cost.quad(X, U, rows)
    lfx, lfxx = cost.fquad(x[:, T], path[:, T])
    assert not lux.any() and np.array_equal(lxx, lxx.transpose(0, 2, 1)) and np.array_equal(lfxx, lfxx.transpose(0, 2, 1))
    assert not lx[:, N:].any() and not lxx[:, N:].any() and not lxx[:, :, N:].any()

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

    for p in range(len(X)):
        fx = lambda z: cost.stage(z, U[p], rows[p])  # noqa: E731
        fu = lambda v: cost.stage(X[p], v, rows[p])  # noqa: E731
        assert close(lx[p], grad_fd(fx, X[p]), 1e-6) and close(lu[p], grad_fd(fu, U[p]), 1e-6), p
        assert close(lxx[p], hess_fd(fx, X[p]), 1e-5) and close(luu[p], hess_fd(fu, U[p]), 1e-5), p
    for b in range(B):
        ff = lambda z: cost.final(z, path[b, T])  # noqa: E731
        assert close(lfx[b], grad_fd(ff, x[b, T]), 1e-6) and close(lfxx[b], hess_fd(ff, x[b, T]), 1e-5), b


def test_step_index_is_read(case):
    """Two paths that agree on rows 0 and T and differ in between give different costs and gains."""
    pr, f, x, u = case
    cost = cost_of(pr, True)
    a = CP.smooth_path(pr, x, True, seed=1, amp=0.05)
    b = a.copy()
    b[:, 2] += 0.01
    xt = np.zeros_like(x)
    assert not np.array_equal(CP.total_cost(x, u, xt, a, cost), CP.total_cost(x, u, xt, b, cost))
    assert not np.array_equal(CP.backward(x, u, a, f, cost)[0], CP.backward(x, u, b, f, cost)[0])


@pytest.mark.parametrize("n", [4, 7])
def test_fixtures_hold_their_conditions(n):
    path = os.path.join(GOLD, f"chain{n}c_path_t16.npz")
    assert os.path.getsize(path) < 256 * 1024
    g = dict(np.load(path, allow_pickle=False))
    meta = json.loads(str(g["meta"]))
    assert g["x"].shape == (5, 17, 2 * n) and g["u"].shape == (5, 16, n)
    assert np.array_equal(g["x"][:, 0], rbd_initial_states(5, n, seed0=81))
    assert 10.0 <= meta["path_weight"] <= 100.0 and meta["simple"]["weight"] == 2e3
    for tag in ("euc", "ref"):
        assert g[f"{tag}_path"].shape == (5, 17, 3) and meta[tag]["margin"] > 1e-9
        assert np.isfinite(g[f"{tag}_K"]).all() and np.isfinite(g[f"{tag}_d"]).all()
        assert np.isin(g[f"{tag}_fit_status"], (1, 2)).all() and (g[f"{tag}_fw_trials"] >= 1).all()
        for b, it in enumerate(g[f"{tag}_fit_iters"]):
            assert (g[f"{tag}_cond_trials"][b, :it] >= 1).all() and np.isfinite(g[f"{tag}_fit_cost"][b, :it]).all()
        # the rows differ along every trajectory: a kernel that read one row for all steps shows
        assert (np.abs(np.diff(g[f"{tag}_path"], axis=1)).max(axis=(1, 2)) > 1e-4).all()
