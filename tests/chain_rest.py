"""The CPU oracle of joint-velocity weights on the chain family
(ilqr_chain_set_velocity_weights) — test-side.

While the weights are set every cost mode gains

  ℓ_t(x, u) += Σᵢ v_weightᵢ · q̇ᵢ²          t < T,   q̇ᵢ = x[n + i]
  ℓ_f(x_T)  += Σᵢ vf_weightᵢ · (q̇ᵢ at T)²

with lx[n+i] = 2·v_weightᵢ·q̇ᵢ, lxx[n+i, n+i] = 2·v_weightᵢ, the same with vf_weight at T, and no
position–velocity cross term. The forward pass hands ℓ the difference x̄ − x_traj
(closure_fit.total_cost), so the joint mode's running term reads q̇ − x_traj's velocity rows; the
task modes are run with x_traj = 0, which they ignore on the device.

  RestOracle    oracle.chain_batch.ChainOracle (joint mode, or a task reading) with the four
                formulas added to l, lf, quad and fquad; backward, forward and fit are its own,
                unchanged (closure_fit's).
  RestPathCost  chain_path.PathCost with the same terms: the cost of chain_path.backward,
                forward_pass and fit, unchanged.
  Rowless       a ChainOracle behind chain_path's cost interface (the rows are not read), so
                that chain_path.fit's log of every line-search decision is there for the modes
                without a path too.

tests/test_chain_rest_oracle.py pins them: all-zero weights give ChainOracle's and chain_path's
arrays bit for bit, the derivatives match central differences of the cost, and Rowless through
chain_path.fit is ChainOracle.fit bit for bit.
"""
from __future__ import annotations

import numpy as np

import chain_path as CP
from oracle.chain_batch import ChainOracle


def weights(n, v0, dv, vf0, dvf):
    """Per-joint weights, all distinct: (v0 + dv·i, vf0 + dvf·i), i = 0 … n − 1."""
    i = np.arange(n, dtype=float)
    return v0 + dv * i, vf0 + dvf * i


JOINT_W = (40.0, 10.0, 4000.0, 700.0)   # the joint mode's fixture weights
TASK_W = (0.6, 0.2, 80.0, 14.0)         # the task modes'


class RestOracle(ChainOracle):
    """ChainOracle plus the velocity terms. v_weight, vf_weight: n values each."""

    def __init__(self, pr, T, v_weight, vf_weight, targets=None, task=None):
        super().__init__(pr, T, targets=targets, task=task)
        self.vw, self.vfw = np.asarray(v_weight, float), np.asarray(vf_weight, float)
        assert self.vw.shape == self.vfw.shape == (self.n,)

    def _qd(self, x):
        return x[:, self.n:2 * self.n]

    def l(self, x, u):
        qd = self._qd(x)
        return super().l(x, u) + (self.vw * qd * qd).sum(1)

    def lf(self, x):
        qd = self._qd(x)
        return super().lf(x) + (self.vfw * qd * qd).sum(1)

    def quad(self, x, u):
        lx, lu, lxx, lux, luu = super().quad(x, u)
        n = self.n
        lx, lxx = np.array(lx), np.array(lxx)
        lx[:, n:2 * n] += 2 * self.vw * self._qd(x)
        lxx[:, n:2 * n, n:2 * n] += np.diag(2 * self.vw)
        return lx, lu, lxx, lux, luu

    def fquad(self, xN):
        g, H = super().fquad(xN)
        n = self.n
        g, H = np.array(g), np.array(H)
        g[:, n:2 * n] += 2 * self.vfw * self._qd(xN)
        H[:, n:2 * n, n:2 * n] += np.diag(2 * self.vfw)
        return g, H

    def forward(self, x, u, d, K, prev, x_traj=None, max_trials=64, alpha0=1.0, shrink=0.5):
        """ChainOracle.forward with x_traj handed on (None: zeros)."""
        from oracle import closure_fit as CF
        xt = np.zeros_like(x) if x_traj is None else x_traj
        return CF.forward_pass(x, u, xt, d, K, prev, self.dyn, self.l, self.lf, max_trials, alpha0, shrink)


class RestPathCost(CP.PathCost):
    """chain_path.PathCost plus the velocity terms (its quad and fquad leave the velocity rows 0)."""

    def __init__(self, chain, body, point, weight, path_weight, euclidean, v_weight, vf_weight):
        super().__init__(chain, body, point, weight, path_weight, euclidean)
        self.vw, self.vfw = np.asarray(v_weight, float), np.asarray(vf_weight, float)
        assert self.vw.shape == self.vfw.shape == (self.n,)

    def _term(self, x, w):
        acc = 0.0
        for i in range(self.n):
            acc = acc + w[i] * x[self.n + i] * x[self.n + i]
        return acc

    def stage(self, x, u, row):
        return super().stage(x, u, row) + self._term(x, self.vw)

    def final(self, x, row):
        return super().final(x, row) + self._term(x, self.vfw)

    def quad(self, X, U, rows):
        lx, lu, lxx, lux, luu = super().quad(X, U, rows)
        n = self.n
        lx[:, n:2 * n] += 2 * self.vw * X[:, n:2 * n]
        lxx[:, n:2 * n, n:2 * n] += np.diag(2 * self.vw)
        return lx, lu, lxx, lux, luu

    def fquad(self, XN, rows):
        g, H = super().fquad(XN, rows)
        n = self.n
        g[:, n:2 * n] += 2 * self.vfw * XN[:, n:2 * n]
        H[:, n:2 * n, n:2 * n] += np.diag(2 * self.vfw)
        return g, H


class Rowless:
    """A ChainOracle behind chain_path's cost interface: the rows are not read."""

    def __init__(self, oracle):
        self.o = oracle

    def stages(self, X, U, rows):
        return self.o.l(X, U)

    def finals(self, X, rows):
        return self.o.lf(X)

    def quad(self, X, U, rows):
        return self.o.quad(X, U)

    def fquad(self, XN, rows):
        return self.o.fquad(XN)


def no_path(x):
    """The path argument of chain_path's functions for a Rowless cost."""
    return np.zeros(x.shape[:2] + (3,))


def task_dict(pr, final_target, euclidean=True):
    """ChainSolver.set_simple_costs' arguments for the suite's tool point (chain_path's)."""
    return dict(body=pr.n_joints - 1, point=CP.POINT, final_target=[float(v) for v in final_target],
                weight=CP.WEIGHT, euclidean=euclidean)
