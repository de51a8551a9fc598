"""How far a floating-base fit moves when its Jacobians move by rounding (CPU, no GPU).

The analytic linearisation (ilqr_floating_set_linearization) returns the duals' Jacobians
in another rounding, so a fit from an analytic handle cannot be bit-equal to the closure
oracle's. This module pins the two fit workloads tests/test_gpu_floating_analytic.py
compares with the oracle and measures, on the oracle alone, what a perturbation of A and B
does to them: oracle.closure_fit.fit as it is, and again with the dynamics wrapped in a
callable whose `.jacobians` (honoured by derivative_tiles) returns oracle.jet's plus
entrywise Gaussian noise of relative size NOISE = 1e-12, scaled by each tile's max-abs.

  arm9x60x6      script_batch(9, 60, seed=5) on the 2Dof_arm, max_iter = 6
  coupled5x50x4  the same construction on coupled_floating_model(): 5 trajectories,
                 T = 50, seed 5, max_iter = 4

Measured with noise 1e-14, 1e-13 and 1e-12 and seeds 0, 1, 2: the decisions (iteration
counts, statuses, per-iteration trial counts) never moved and the deviation is linear in
the noise. The largest deviation / noise over the three seeds at 1e-12 (rel = max|a − b| /
max|b|; hist is the per-iteration cost record):

  workload        x        u        cost     hist
  arm9x60x6       1.30e5   2.43e5   6.55e4   4.60e4
  coupled5x50x4   3.47e5   7.99e5   1.39e4   2.48e4

S below is twice that: the sensitivity constants the GPU test's tolerance
max(1e-8, 4·S·ε_J) is built from. (30-iteration fits are no yardstick: on the 33 × 60
workload noise of 1e-12 becomes 1e-6 after 30 iterations.)"""
import functools

import numpy as np
import pytest

from closures import coupled_floating_model, jet_ns, rbd_cost_quads, rbd_floating_arm
from oracle import closure_fit as CF
from oracle import jet

NOISE = 1e-12
SEEDS = (0, 1)
WORKLOADS = {"arm9x60x6": (9, 60, 6), "coupled5x50x4": (5, 50, 4)}   # nb, T, max_iter
# deviation / noise, twice the measurement in the docstring
S = {"arm9x60x6": {"x": 2.6e5, "u": 4.86e5, "cost": 1.31e5, "hist": 9.2e4},
     "coupled5x50x4": {"x": 6.94e5, "u": 1.6e6, "cost": 2.78e4, "hist": 4.96e4}}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def model_of(name):
    """None (the 2Dof_arm) or the coupled mechanism's model dict."""
    return None if name == "arm9x60x6" else coupled_floating_model()


def closures_of(name):
    md = model_of(name)
    return rbd_floating_arm(jet_ns()) if md is None else rbd_floating_arm(jet_ns(), model=md)


@functools.lru_cache(maxsize=None)
def workload(name):
    """(x (nb, T+1, 16), u (nb, T, 8), max_iter): the script's start (rest state, zero
    inputs) plus copies with perturbed velocities, rolled out by the restatement —
    tests/test_gpu_floating.py script_batch's construction on the workload's model."""
    nb, T, max_iter = WORKLOADS[name]
    fj, _, _ = closures_of(name)
    x = np.zeros((nb, T + 1, 16))
    x[:, 0] = np.array([0.0, 0.0, 1.0, 0.5, 0.75, 1.0, 0.0, 0.0] + [0.0] * 8)   # rbd_initial_state()
    x[1:, 0, 8:] = 0.05 * np.random.default_rng(5).standard_normal((nb - 1, 8))
    u = np.zeros((nb, T, 8))
    for t in range(T):
        x[:, t + 1] = fj(x[:, t], u[:, t])
    x.setflags(write=False)
    u.setflags(write=False)
    return x, u, max_iter


@functools.lru_cache(maxsize=None)
def oracle_fit(name):
    """oracle.closure_fit.fit on the workload as it is (shared, not to be written to)."""
    x, u, max_iter = workload(name)
    fj, lj, lfj = closures_of(name)
    return CF.fit(x, u, fj, lj, lfj, *rbd_cost_quads(), max_iter=max_iter, tol=1e-6)


class NoisyJacobians:
    """dynamicsf with oracle.jet's Jacobians plus Gaussian noise of relative size `noise`."""

    def __init__(self, f, noise, seed):
        self.f, self.noise, self.rng = f, noise, np.random.default_rng(seed)

    def __call__(self, x, u):
        return self.f(x, u)

    def jacobians(self, xs, us):
        A, Bm = jet.jacobians(self.f, xs, us)
        out = []
        for M in (np.asarray(A, float), np.asarray(Bm, float)):
            scale = np.abs(M).max(axis=(1, 2), keepdims=True)
            out.append(M + self.noise * scale * self.rng.standard_normal(M.shape))
        return out[0], out[1]


def deviations(o, r):
    return {"x": rel(r["x"], o["x"]), "u": rel(r["u"], o["u"]), "cost": rel(r["cost"], o["cost"]),
            "hist": rel(r["history"]["cost"], o["history"]["cost"])}


def noisy_fit(name, noise, seed):
    x, u, max_iter = workload(name)
    fj, lj, lfj = closures_of(name)
    return CF.fit(x, u, NoisyJacobians(fj, noise, seed), lj, lfj, *rbd_cost_quads(), max_iter=max_iter, tol=1e-6)


def test_script_batch_construction_is_the_gpu_suites():
    """arm9x60x6 is tests/test_gpu_floating.py's script_batch(9, 60, seed=5), bit for bit."""
    from test_gpu_floating import script_batch
    x, u, _ = workload("arm9x60x6")
    xs, us = script_batch(9, 60, seed=5)
    assert np.array_equal(x, xs) and np.array_equal(u, us)


@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_fit_decisions_hold_and_deviation_is_bounded(name):
    o = oracle_fit(name)
    assert not np.isnan(o["history"]["cost"]).any()   # every iteration of every trajectory accepted
    for seed in SEEDS:
        r = noisy_fit(name, NOISE, seed)
        assert r["iters"].tolist() == o["iters"].tolist()
        assert r["status"].tolist() == o["status"].tolist()
        assert r["history"]["trials"].tolist() == o["history"]["trials"].tolist()
        dev = deviations(o, r)
        print(name, "seed", seed, {k: "%.3g" % (v / NOISE) for k, v in dev.items()})
        for k, v in dev.items():
            assert v / NOISE < S[name][k], (name, seed, k, v / NOISE, S[name][k])
