"""Batched CPU restatement of the chain family's passes — TEST INFRASTRUCTURE ONLY.

The oracle of an ilqr_amd.chain.ChainProblem for a whole batch at once, for tests that run the
oracle at test time on chains of up to seven joints: the per-trajectory oracle (oracle.rbd's
closures through oracle.ilqr_oracle) pays Python once per point and takes tens of seconds there.
Same algorithm, built from pieces that are each pinned elsewhere: oracle.rbd's exact forward-mode
Jacobians over all B·T points in one evaluation, the RK4 step by its C restatement
(cref.chain_dynamics), the costs' exact quadratizations, the C recursion (cref.tiles_backward,
symmetrised S) and closure_fit's forward_pass and fit. tests/test_chain_oracle.py pins it to the
per-trajectory oracle. Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
import anything under oracle/.
"""
from __future__ import annotations

import numpy as np

from . import closure_fit as CF
from . import cref
from . import ilqr_oracle as O


class ChainOracle:
    """backward, forward and fit of one ChainProblem over a batch (x (B, T+1, nx), u (B, T, nu)).
    targets: a joint-space goal per trajectory (B, n); task: the simple-cost dict of
    ChainSolver.set_simple_costs (body, point, final_target, weight, euclidean)."""

    def __init__(self, pr, T, targets=None, task=None):
        from . import rbd
        self.pr, self.T, self.n = pr, T, pr.n_joints
        self.model = rbd.ChainModel(pr.chain, pr.dt)
        self.targets, self.task = targets, task
        model = self.model

        class Dyn:
            def __call__(self, x, u):     # the C restatement of the same RK4 step (rollouts in C, not Python)
                return cref.chain_dynamics(pr, np.asarray(x, float), np.asarray(u, float))

            def jacobians(self, xs, us):
                return model.linearize(xs, us)

        self.dyn = Dyn()
        if task is not None:
            from . import cost_functions as OC
            self._lf1 = OC.simple_final_cost(pr.chain, task["body"], task["point"], task["final_target"],
                                             task["weight"], euclidean=task["euclidean"])

    def _goal(self, rows):
        """θ* for `rows` points: (rows, n); points are trajectory-major with T (or 1) per trajectory."""
        if self.targets is None:
            return np.broadcast_to(np.asarray(self.pr.target, float), (rows, self.n))
        per = rows // len(self.targets)
        return np.repeat(np.asarray(self.targets, float), per, axis=0)

    def l(self, x, u):
        if self.task is not None:
            return (u ** 2).sum(1)
        e = self._goal(len(x)) - x[:, :self.n]
        return (np.asarray(self.pr.q_weight) * e * e).sum(1) + (np.asarray(self.pr.r_weight)[:u.shape[1]] * u * u).sum(1)

    def lf(self, x):
        if self.task is not None:
            return np.array([float(self._lf1(xi)) for xi in x])
        e = self._goal(len(x)) - x[:, :self.n]
        return (np.asarray(self.pr.qf_weight) * e * e).sum(1)

    def quad(self, x, u):
        P, nx = x.shape
        nu, n = u.shape[1], self.n
        lx, lxx = np.zeros((P, nx)), np.zeros((P, nx, nx))
        if self.task is not None:
            rw = np.ones(nu)
        else:
            rw = np.asarray(self.pr.r_weight, float)[:nu]
            lx[:, :n] = -2 * np.asarray(self.pr.q_weight) * (self._goal(P) - x[:, :n])
            lxx[:, :n, :n] = np.diag(2 * np.asarray(self.pr.q_weight, float))
        return lx, 2 * rw * u, lxx, np.zeros((P, nu, nx)), np.broadcast_to(np.diag(2 * rw), (P, nu, nu)).copy()

    def fquad(self, xN):
        P, nx = xN.shape
        n = self.n
        if self.task is not None:
            q = [O.final_cost_quadratization(xi, self._lf1) for xi in xN]
            return np.array([v[1] for v in q], float), np.array([v[2] for v in q], float)
        g, H = np.zeros((P, nx)), np.zeros((P, nx, nx))
        g[:, :n] = -2 * np.asarray(self.pr.qf_weight) * (self._goal(P) - xN[:, :n])
        H[:, :n, :n] = np.diag(2 * np.asarray(self.pr.qf_weight, float))
        return g, H

    def rollout(self, x0, u):
        x = np.empty((u.shape[0], u.shape[1] + 1, x0.shape[1]))
        x[:, 0] = x0
        for t in range(u.shape[1]):
            x[:, t + 1] = self.dyn(x[:, t], u[:, t])
        return x

    def backward(self, x, u, mus):
        """(d, K) at every μ of `mus` from one linearisation."""
        tl = CF.derivative_tiles(x, u, self.dyn, self.quad, self.fquad)
        return [cref.tiles_backward(tl, mu=mu, symmetrize=True)[:2] for mu in mus]

    def forward(self, x, u, d, K, prev, max_trials=64, alpha0=1.0, shrink=0.5):
        return CF.forward_pass(x, u, np.zeros_like(x), d, K, prev, self.dyn, self.l, self.lf, max_trials, alpha0,
                               shrink)

    def fit(self, x, u, **kw):
        return CF.fit(x, u, self.dyn, self.l, self.lf, self.quad, self.fquad, **kw)
