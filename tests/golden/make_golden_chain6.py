"""Fixtures of the six-joint chain (tests/test_gpu_chain6.py, tests/test_chain6_abi.py,
tests/test_gpu_chain6_general.py):

  chain6_t30.npz    rbd_6dof_problem(), gravity zero as the URDF parses, 3 trajectories
  chain6g_t30.npz   rbd_6dof_problem(gravity=True), 2 trajectories
  chain6g_cases_t30.npz   a line-search case (ls_*) and an x_traj case (xt_*) on the gravity
                    fixture's trajectories and gains (kept apart: each file stays under 160 KB)
  chain6c_t24.npz   coupled_6dof_problem() (the general mechanism: no symmetry of the arm's
                    left), 2 trajectories, T = 24
  chain6c_cases_t24.npz   its line-search and x_traj cases

All three targets (chain6, chain6g, chain6c) through make_golden.chain_case (the numpy
oracle: RNEA + RK4, exact Jacobians by
forward-mode AD, the generic oracle passes). The assertions below are conditions on the
cases, so a regenerated fixture cannot hide a fragile one:
  * every Σδu² of every fit history is a factor ≥ 1.25 away from tol,
  * every fit line search takes one trial,
  * the line-search cases take [4, 2] (chain6g) and LS_TRIALS_C (chain6c) trials and every
    accept / reject margin exceeds 1 % of prev_cost.
Prints the oracle's literal-vs-symmetrised spread of the gains (the gain tolerance of the
GPU tests may not be looser than 100× it).

    python tests/golden/make_golden_chain6.py                 # all five files (several minutes of CPU)
    python tests/golden/make_golden_chain6.py chain6g         # one target: chain6, chain6g or chain6c
    python tests/golden/make_golden_chain6.py chain6c_cases   # chain6c_cases_t24 alone, from chain6c_t24
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository and the package on sys.path)
from ilqr_amd.chain import coupled_6dof_problem, rbd_6dof_problem, rbd_initial_states  # noqa: E402
from oracle import ilqr_oracle as O  # noqa: E402
from oracle import rbd as RBD  # noqa: E402

T, FIT_ITERS, TOL = 30, 20, 1e-6
LS_SCALE = [9.0, 2.5]
LS_TRIALS = [4, 2]
# the general mechanism (ilqr_amd.chain.coupled_6dof_problem)
T_C, SEED_C = 24, 81
LS_SCALE_C = [9.0, 2.5]
LS_TRIALS_C = [4, 2]


class Recorder:
    """Wraps the oracle's fit and backward_pass while chain_case runs: keeps every fit
    history and the literal / symmetrised gains of the first backward pass."""

    def __enter__(self):
        self.hists, self.K, self.Ks = [], [], []
        self._fit, self._bw = O.fit, O.backward_pass

        def fit(*a, history=None, **kw):
            if history is not None:
                self.hists.append(history)
            return self._fit(*a, history=history, **kw)

        def backward_pass(*a, **kw):
            r = self._bw(*a, **kw)
            if not self.in_fit:  # chain_case's own pair of calls (fit passes its flags by position)
                (self.Ks if kw.get("symmetrize", False) else self.K).append(r[1])
            return r

        self.in_fit = False

        def fit_guard(*a, **kw):
            self.in_fit = True
            try:
                return fit(*a, **kw)
            finally:
                self.in_fit = False

        O.fit, O.backward_pass = fit_guard, backward_pass
        return self

    def __exit__(self, *exc):
        O.fit, O.backward_pass = self._fit, self._bw


def check_fits(name, rec):
    for b, h in enumerate(rec.hists):
        for e in h:
            r = e["du2"] / TOL
            assert r >= 1.25 or r <= 1.0 / 1.25, (name, b, e)
            assert e["trials"] == 1, (name, b, e)
    du2 = np.array([e["du2"] for h in rec.hists for e in h])
    near = du2[np.argmin(np.abs(np.log(du2 / TOL)))]
    spread = max(np.abs(K - Ks).max() / np.abs(Ks).max() for K, Ks in zip(rec.K, rec.Ks))
    print(f"{name}: du2 closest to tol {near:.3e} (factor {max(near / TOL, TOL / near):.2f}); "
          f"literal-vs-symmetrised gain spread {spread:.2e} (relative)")


def closures(pr):
    model = RBD.ChainModel(pr.chain, pr.dt)
    cost = RBD.ChainCost(pr.target, pr.q_weight, pr.r_weight, pr.qf_weight)
    return RBD.chain_closures(model, cost)


def extend_gravity(name, cases, pr, ls_scale=LS_SCALE, want_trials=LS_TRIALS):
    """The line-search and x_traj cases on the trajectories and gains of fixture `name` (the
    gravity fixture, or the general mechanism's with its own ls_scale / want_trials), in a
    file of their own (`cases`): with them the fixture itself would pass the size limit."""
    g = dict(np.load(os.path.join(HERE, name + ".npz")))
    f, l, lf = closures(pr)
    x, u, d, K = g["x"], g["u"], g["d"], g["K"]
    nb = len(x)
    z = np.zeros_like(x[0])
    total = O.total_cost_generator(z, l, lf)
    ls_prev = np.array([total(x[b], u[b]) for b in range(nb)])
    ls_x, ls_u, ls_cost = np.empty_like(x), np.empty_like(u), np.empty(nb)
    ls_trials = np.empty(nb, dtype=np.int32)
    for b in range(nb):
        st = {}
        ls_x[b], ls_u[b], ls_cost[b] = O.forward_pass(x[b], u[b], z, ls_scale[b] * d[b], K[b], ls_prev[b],
                                                      f, l, lf, max_trials=MG.MAX_TRIALS, stats=st)
        ls_trials[b] = st["trials"]
        for j in range(1, st["trials"] + 1):  # every candidate's margin to prev_cost
            _, _, cj = O.forward_pass(x[b], u[b], z, ls_scale[b] * d[b], K[b], np.inf, f, l, lf,
                                      max_trials=1, alpha0=0.5 ** (j - 1))
            margin = (cj - ls_prev[b]) / ls_prev[b]
            print(f"{name}: ls trajectory {b} trial {j}: cost {cj:.6e} prev {ls_prev[b]:.6e} margin {margin:+.3f}")
            assert (margin < -0.01) if j == st["trials"] else (margin > 0.01), (b, j, margin)
    assert ls_trials.tolist() == want_trials, ls_trials
    xt = 0.1 * x[:, ::-1]
    xt_x, xt_u, xt_cost = np.empty_like(x), np.empty_like(u), np.empty(nb)
    for b in range(nb):
        xt_x[b], xt_u[b], xt_cost[b] = O.forward_pass(x[b], u[b], xt[b], d[b], K[b], np.inf, f, l, lf,
                                                      max_trials=MG.MAX_TRIALS)
    np.savez_compressed(os.path.join(HERE, cases + ".npz"), ls_scale=np.array(ls_scale), ls_prev_cost=ls_prev,
                        ls_trials=ls_trials, ls_x=ls_x, ls_u=ls_u, ls_cost=ls_cost, xt=xt, xt_x=xt_x,
                        xt_u=xt_u, xt_cost=xt_cost)
    print(name, "ls trials", ls_trials.tolist(), "A[6:, :6] max", np.abs(g["A"][..., 6:, :6]).max(),
          "|K| max", np.abs(K).max(), "|x| max", np.abs(x).max())


def main(only=()):
    def want(n):
        return not only or n in only
    if want("chain6"):
        pr = rbd_6dof_problem()
        with Recorder() as rec:
            MG.chain_case("chain6_t30", 6, rbd_initial_states(3, 6, seed0=80), T=T, fit_iters=FIT_ITERS,
                          tol=TOL, pr=pr, robot="6dof_arm")
        check_fits("chain6_t30", rec)
    if want("chain6g"):
        # not seed 80: with gravity its eighth iteration has Σδu² = 1.05e-6 against tol = 1e-6
        pr = rbd_6dof_problem(gravity=True)
        with Recorder() as rec:
            MG.chain_case("chain6g_t30", 6, rbd_initial_states(2, 6, seed0=81), T=T, fit_iters=FIT_ITERS,
                          tol=TOL, pr=pr, robot="6dof_arm+gravity")
        check_fits("chain6g_t30", rec)
        extend_gravity("chain6g_t30", "chain6g_cases_t30", pr)
    if want("chain6c"):
        pr = coupled_6dof_problem()
        with Recorder() as rec:
            MG.chain_case("chain6c_t24", 6, rbd_initial_states(2, 6, seed0=SEED_C), T=T_C, fit_iters=FIT_ITERS,
                          tol=TOL, pr=pr, robot="coupled_6dof")
        check_fits("chain6c_t24", rec)
    if want("chain6c") or want("chain6c_cases"):
        extend_gravity("chain6c_t24", "chain6c_cases_t24", coupled_6dof_problem(), LS_SCALE_C, LS_TRIALS_C)
    for n in ("chain6_t30", "chain6g_t30", "chain6g_cases_t30", "chain6c_t24", "chain6c_cases_t24"):
        p = os.path.join(HERE, n + ".npz")
        if os.path.exists(p):
            assert os.path.getsize(p) < 160 * 1024, (n, os.path.getsize(p))


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
