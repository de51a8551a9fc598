"""The CPU oracle of a tool path on the chain family (ilqr_chain_set_task_path) — test-side.

The reference's closures carry no step index, so its fit cannot state a cost whose goal moves
with t. This module restates oracle.closure_fit's forward pass and fit loop with the step's path
row handed to the cost, and builds everything else from oracle/ pieces:

  cost           ℓ_t(x, u) = Σ uₐ² + w_path · Σₖ (πₖ(q) − path[b, t, k])²,   t < T
                 ℓ_f(x_T)  = weight · Σₖ (πₖ(q_T) − path[b, T, k])²
                 π from oracle.cost_functions.point_position (πₖ = pₖ, or p_z for every k in
                 the reference's reading), summed in simple_final_cost's order
  quadratization oracle.dual (ForwardDiff's algorithm) point by point, exact; the stage cost is
                 separable in (q, u) and free of q̇, so ∂²ℓ/∂u∂x = 0 and the velocity rows are 0
  tiles          oracle.closure_fit.derivative_tiles, whose quad sees all B·T points
                 trajectory-major: path[:, :T].reshape(-1, 3) lines up with them
  recursion      oracle.cref.tiles_backward(symmetrize=True)
  dynamics       oracle.rbd.ChainModel (RNEA + RK4, exact Jacobians)

tests/test_chain_path_oracle.py pins it: on a constant path it is closure_fit.forward_pass /
closure_fit.fit with index-free closures of the same cost bit for bit, and its gradients and
Hessians match central differences of its own cost.
"""
from __future__ import annotations

import numpy as np

from oracle import closure_fit, cref
from oracle import cost_functions as OC
from oracle import dual
from oracle import rbd as RBD

POINT = [0.05, 0.02, 0.1]     # the tool point on the last body (the targets suite's)
WEIGHT = 2e3


class Dynamics:
    """oracle.rbd's RK4 step over P points, with its exact Jacobians for derivative_tiles."""

    def __init__(self, pr):
        self.model = RBD.ChainModel(pr.chain, pr.dt)

    def __call__(self, x, u):
        return self.model.step(np.asarray(x, float), np.asarray(u, float))

    def jacobians(self, x, u):
        return self.model.linearize(x, u)


class PathCost:
    """The scalar closures of one trajectory's cost, the step's row an argument."""

    def __init__(self, chain, body, point, weight, path_weight, euclidean):
        self.chain, self.body, self.point = chain, body, [float(v) for v in point]
        self.weight, self.path_weight, self.euclidean = float(weight), float(path_weight), bool(euclidean)
        self.n = chain.n

    def reading(self, x, row):
        ws = OC.point_position(self.chain, self.body, self.point, [x[i] for i in range(self.n)])
        acc = 0.0
        for k in range(3):
            e = (ws[k] if self.euclidean else ws[2]) - float(row[k])
            acc = acc + e * e
        return acc

    def stage(self, x, u, row):
        acc = 0.0
        for k in range(len(u)):
            acc = acc + u[k] * u[k]
        return acc + self.path_weight * self.reading(x, row)

    def final(self, x, row):
        return self.weight * self.reading(x, row)

    # -- over P points, rows (P, 3) ------------------------------------------------------
    def stages(self, X, U, rows):
        return np.array([self.stage(X[p], U[p], rows[p]) for p in range(len(X))], dtype=float)

    def finals(self, X, rows):
        return np.array([self.final(X[p], rows[p]) for p in range(len(X))], dtype=float)

    def quad(self, X, U, rows):
        """closure_fit.dual_quads' five arrays for the stage cost, point p against rows[p]."""
        P, nx = X.shape
        nu, n = U.shape[1], self.n
        lx, lu = np.zeros((P, nx)), np.zeros((P, nu))
        lxx, lux, luu = np.zeros((P, nx, nx)), np.zeros((P, nu, nx)), np.zeros((P, nu, nu))
        for p in range(P):
            x, u, row = X[p], U[p], rows[p]
            of_q = lambda q: self.stage(list(q) + list(x[n:]), u, row)  # noqa: E731
            of_u = lambda v: self.stage(x, v, row)                      # noqa: E731
            lx[p, :n] = dual.gradient(of_q, x[:n])
            lxx[p, :n, :n] = dual.hessian(of_q, x[:n])
            lu[p] = dual.gradient(of_u, u)
            luu[p] = dual.hessian(of_u, u)
        return lx, lu, lxx, lux, luu

    def fquad(self, XN, rows):
        n, nx = self.n, XN.shape[1]
        g, H = np.zeros((len(XN), nx)), np.zeros((len(XN), nx, nx))
        for p in range(len(XN)):
            x, row = XN[p], rows[p]
            of_q = lambda q: self.final(list(q) + list(x[n:]), row)     # noqa: E731
            g[p, :n] = dual.gradient(of_q, x[:n])
            H[p, :n, :n] = dual.hessian(of_q, x[:n])
        return g, H


def tiles(x, u, path, f, cost):
    """The derivative and cost tiles along (x, u) with trajectory b's step t against path[b, t]."""
    T = u.shape[1]
    rows = path[:, :T].reshape(-1, 3)
    return closure_fit.derivative_tiles(x, u, f, lambda xs, us: cost.quad(xs, us, rows),
                                        lambda xN: cost.fquad(xN, path[:, T]))


def backward(x, u, path, f, cost, mu=0.01):
    return cref.tiles_backward(tiles(x, u, path, f, cost), mu=mu, symmetrize=True)


def total_cost(xb, ub, x_traj, path, cost):
    """closure_fit.total_cost with the step index passed on."""
    T = ub.shape[1]
    acc = np.zeros(xb.shape[0])
    for t in range(T):
        acc = acc + cost.stages(xb[:, t] - x_traj[:, t], ub[:, t], path[:, t])
    return acc + cost.finals(xb[:, T], path[:, T])


def forward_pass(x, u, x_traj, d, K, prev_cost, f, path, cost, max_trials=64, alpha0=1.0, shrink=0.5, log=None):
    """closure_fit.forward_pass, statement for statement, the cost reading the step's row.
    log: a list that receives (trial, |prev − cost| / |cost| of the trajectories still searching)."""
    nb, N, nx = x.shape
    T = N - 1
    xo, uo = x.copy(), u.copy()
    cost_out = np.full(nb, np.nan)
    trials = np.zeros(nb, dtype=np.int32)
    done = np.zeros(nb, dtype=bool)
    alpha = np.full(nb, float(alpha0))
    with np.errstate(all="ignore"):
        for trial in range(1, max_trials + 1):
            xb = np.empty_like(x)
            ub = np.empty_like(u)
            xb[:, 0] = x[:, 0]
            for k in range(T):
                dx = xb[:, k] - x[:, k]
                ub[:, k] = (u[:, k] + alpha[:, None] * d[:, k]) + np.einsum("bij,bj->bi", K[:, k], dx)
                xb[:, k + 1] = f(xb[:, k], ub[:, k])
            c = total_cost(xb, ub, x_traj, path, cost)
            if log is not None:
                log.append((trial, np.where(done, np.inf, np.abs(prev_cost - c) / np.abs(c))))
            acc = ~done & ((prev_cost - c) > 0)
            trials = np.where(~done, trial, trials)
            cost_out = np.where(acc | ~done, c, cost_out)
            xo[acc], uo[acc] = xb[acc], ub[acc]
            done |= acc
            if done.all():
                break
            alpha = np.where(done, alpha, alpha * shrink)
    return xo, uo, cost_out, trials, done


def fit(x_init, u_init, f, path, cost, max_iter=100, tol=1e-6, max_trials=64, mu=0.01, alpha0=1.0, shrink=0.5,
        log=None):
    """closure_fit.fit, statement for statement, on the path cost (x_traj = 0: the task costs
    ignore it). log: as forward_pass, plus ("gains", any NaN) per iteration."""
    xi, ui = np.array(x_init, dtype=np.float64), np.array(u_init, dtype=np.float64)
    nb = xi.shape[0]
    xt = np.zeros_like(xi)
    prev = np.full(nb, np.inf)
    status = np.zeros(nb, dtype=np.int32)
    iters = np.zeros(nb, dtype=np.int32)
    hist = {"cost": [], "trials": [], "du2": []}
    for it in range(1, max_iter + 1):
        run = status == 0
        if not run.any():
            break
        d, K, bst = backward(xi, ui, path, f, cost, mu)
        if log is not None:
            log.append(("gains", bool(np.isnan(d).any() or np.isnan(K).any())))
        status = np.where(run & (bst == 4), 4, status)
        run = status == 0
        xn, un, c, ntr, ok = forward_pass(xi, ui, xt, d, K, prev, f, path, cost, max_trials, alpha0, shrink,
                                          log=None if log is None else _running(log, run))
        iters = np.where(run, it, iters)
        bad = run & ~ok
        status = np.where(bad, np.where(np.isnan(c), 4, 3), status)
        acc = run & ok
        prev = np.where(acc, c, prev)
        du2 = ((un - ui) ** 2).sum(axis=(1, 2))
        conv = acc & (du2 <= tol)
        hist["cost"].append(np.where(acc, c, np.nan))
        hist["trials"].append(np.where(run, ntr, 0))
        hist["du2"].append(np.where(run, du2, np.nan))
        status = np.where(conv, 1, status)
        step = acc & ~conv
        xi[step], ui[step] = xn[step], un[step]
    status = np.where(status == 0, 2, status)
    return {"x": xi, "u": ui, "cost": prev, "iters": iters, "status": status,
            "history": {k: np.array(v) for k, v in hist.items()}}


class _running:
    """A forward-pass log that keeps the margins of the running trajectories only."""

    def __init__(self, log, run):
        self.log, self.run = log, run

    def append(self, entry):
        trial, m = entry
        self.log.append((trial, np.where(self.run, m, np.inf)))


# -- the index-free closures of a constant path (every row of trajectory b equal to c[b]) ------
class ConstantClosures:
    """closure_fit's (immediate_cost, final_cost, quad, fquad) of the same cost with the goal
    c (B, 3) baked in: batched over the B trajectories (forward pass) or the B·T points of
    derivative_tiles, trajectory-major."""

    def __init__(self, cost, c):
        self.cost, self.c = cost, np.asarray(c, float)

    def _rows(self, P):
        B = len(self.c)
        assert P % B == 0
        return np.repeat(self.c, P // B, axis=0)

    def immediate_cost(self, X, U):
        return self.cost.stages(X, U, self._rows(len(X)))

    def final_cost(self, X):
        return self.cost.finals(X, self.c)

    def quad(self, X, U):
        return self.cost.quad(X, U, self._rows(len(X)))

    def fquad(self, XN):
        return self.cost.fquad(XN, self.c)


# -- the suite's problems ---------------------------------------------------------------------
def tool_positions(pr, x):
    """The tool point's root-frame position along x (..., nx) → (..., 3)."""
    n = pr.n_joints
    flat = x.reshape(-1, x.shape[-1])
    return np.array([OC.point_position(pr.chain, n - 1, POINT, list(xi[:n])) for xi in flat]).reshape(x.shape[:-1] + (3,))


def rollout(f, x0, u):
    x = np.empty((u.shape[0], u.shape[1] + 1, x0.shape[1]))
    x[:, 0] = x0
    for t in range(u.shape[1]):
        x[:, t + 1] = f(x[:, t], u[:, t])
    return x


def smooth_path(pr, x, euclidean, seed, amp=0.05):
    """A path near the rollout's own tool trajectory: the tool's positions along x (p_z in every
    column for the reference's reading) plus a smooth per-trajectory offset that grows from 0
    at t = 0 to `amp`-sized at T."""
    p = tool_positions(pr, x)
    if not euclidean:
        p = np.repeat(p[..., 2:3], 3, axis=-1)
    B, N, _ = p.shape
    rng = np.random.default_rng(seed)
    a = rng.uniform(-amp, amp, (B, 1, 3))
    ph = rng.uniform(0.0, np.pi, (B, 1, 3))
    s = (np.arange(N) / max(N - 1, 1))[None, :, None]
    return p + a * s * (1.0 + 0.5 * np.sin(2.0 * np.pi * s + ph))
