"""Fixtures of the 4-, 5- and 7-joint chains on the tiles path (tests/test_gpu_chainN.py,
tests/test_chainN_abi.py): ilqr_amd.chain.coupled_chain_problem(n), B = 3 trajectories,
T = 16, from the numpy oracle (oracle/rbd.py, oracle/cost_functions.py). Mirrors
make_golden_chain6.py and make_golden_chain6_task.py. Per joint count n:

  chain{n}c_t16.npz            x, u, A, B, d, K, a forward pass, a fit (make_golden.chain_case)
  chain{n}c_cases_t16.npz      a line-search case (ls_*) and an x_traj case (xt_*) on its
                               trajectories and gains
  chain{n}ctask_euc_t16.npz    the task costs, squared distance of a point on the last body
  chain{n}ctask_ref_t16.npz    the task costs, the reference's reading (p_z against every
                               target component) of an off-axis point on body 2

Three trajectories leave a half-empty wave (two 32-lane groups per workgroup), T = 16 crosses
the tiles kernels' symmetrisation and prefetch periods, seven joints use the forward group's
fifth staging word and four joints the narrow (8 × 4) tiles kernel.

Conditions on the cases, asserted here so that a regenerated fixture cannot hide a fragile one:
  * every fit converges (status 1) within FIT_ITERS = 20 iterations, and every Σδu² of every
    fit history is a factor ≥ 1.25 away from tol;
  * the line-search case of every joint count has a trajectory accepted at trial ≥ 2, and
    every accept / reject margin of it exceeds 1 % of prev_cost;
  * the C restatement (oracle/cref.py) reproduces the counts: the same passes with the RK4
    step evaluated by oracle_chain_dynamics and linearised by its central differences
    (oracle_chain_iterate's rule) give the numpy oracle's iteration counts, per-iteration
    trial counts and line-search trial counts exactly. A count that flips between the two
    oracles could not be demanded of the device.
Each file stays under 256 KB (seven joints: 170 KB; the repository's limit for a committed file is 1 MiB).

    python tests/golden/make_golden_chainN.py          # everything (minutes of CPU)
    python tests/golden/make_golden_chainN.py 7        # one joint count
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository and the package on sys.path)
from make_golden_chain6 import FIT_ITERS, TOL, Recorder, closures  # noqa: E402
from ilqr_amd.chain import coupled_chain_problem, rbd_initial_states  # noqa: E402
from oracle import cost_functions as OC  # noqa: E402
from oracle import cref  # noqa: E402
from oracle import ilqr_oracle as O  # noqa: E402

N_JOINTS = (4, 5, 7)
NB, T = 3, 16
# initial states: rbd_initial_states(NB, n, seed0=SEED[n])
SEED = {4: 81, 5: 81, 7: 81}
# the line-search case: δu scaled per trajectory
LS_SCALE = {4: [9.0, 2.5, 1.0], 5: [9.0, 2.5, 1.0], 7: [9.0, 2.5, 1.0]}
# the task costs: ℓ = Σu², ℓ_f = weight·Σₖ (pₖ − tₖ)² (euc) or weight·Σₖ (p_z − tₖ)² (ref). The
# targets sit within reach of the point (its position at q = 0 is printed beside each case).
TASK = {
    4: dict(euc=dict(seed0=83, simple=dict(body=3, point=[0.05, 0.02, 0.1], final_target=[1.9, 0.9, 1.0],
                                           weight=2e3, euclidean=True)),
            ref=dict(seed0=81, simple=dict(body=2, point=[0.3, -0.2, 0.15], final_target=[0.9, 1.0, 1.1],
                                           weight=2e3, euclidean=False))),
    5: dict(euc=dict(seed0=83, simple=dict(body=4, point=[0.05, 0.02, 0.1], final_target=[2.0, 1.2, 1.3],
                                           weight=2e3, euclidean=True)),
            ref=dict(seed0=81, simple=dict(body=2, point=[0.3, -0.2, 0.15], final_target=[0.9, 1.0, 1.1],
                                           weight=2e3, euclidean=False))),
    # not seed 83 with the target (2.3, 1.5, 1.6): its third trajectory exhausts a line search at
    # its fifth iteration (status 3)
    7: dict(euc=dict(seed0=81, simple=dict(body=6, point=[0.05, 0.02, 0.1], final_target=[2.9, 1.3, 1.3],
                                           weight=2e3, euclidean=True)),
            ref=dict(seed0=81, simple=dict(body=2, point=[0.3, -0.2, 0.15], final_target=[0.9, 1.0, 1.1],
                                           weight=2e3, euclidean=False))),
}
CBE = 6.0554544523933395e-6   # ε^⅓ in fp64: the central-difference step of oracle_chain_iterate


def c_closures(pr, simple=None):
    """The oracle passes' closures on the C restatement: the RK4 step by oracle_chain_dynamics,
    its Jacobians by central differences of that step (h = ε^⅓·max(1, |z_k|), divided by the
    step actually taken); the costs are the numpy oracle's own (exact derivatives)."""
    nx, nu = pr.nx, pr.nu
    _, l, lf = closures(pr)
    if simple is not None:
        a = (pr.chain, simple["body"], simple["point"], simple["final_target"], simple["weight"])
        l = OC.simple_immediate_cost(*a)
        lf = OC.simple_final_cost(*a, euclidean=simple["euclidean"])

    class Dyn:
        def __call__(self, x, u):
            return cref.chain_dynamics(pr, np.asarray(x, float)[None], np.asarray(u, float)[None])[0]

        def jac(self, x, u):
            z = np.concatenate([np.asarray(x, float), np.asarray(u, float)])
            nd = nx + nu
            h = CBE * np.maximum(1.0, np.abs(z))
            Z = np.tile(z, (2 * nd, 1))
            for k in range(nd):
                Z[2 * k, k] = z[k] + h[k]
                Z[2 * k + 1, k] = z[k] - h[k]
            F = cref.chain_dynamics(pr, Z[:, :nx], Z[:, nx:])
            J = np.empty((nx, nd))
            for k in range(nd):
                J[:, k] = (F[2 * k] - F[2 * k + 1]) / (Z[2 * k, k] - Z[2 * k + 1, k])
            return J[:, :nx], J[:, nx:]

    return Dyn(), l, lf


def fit_counts(x, u, f, l, lf):
    """(iterations, status, per-iteration trials) of the oracle's fit for every trajectory."""
    iters, status, trials = [], [], []
    for b in range(len(x)):
        hist = []
        O.fit(x[b], u[b], f, l, lf, max_iter=FIT_ITERS, tol=TOL, max_trials=MG.MAX_TRIALS, history=hist)
        iters.append(len(hist))
        status.append(1 if hist[-1]["du2"] <= TOL else 2)
        trials.append([e["trials"] for e in hist])
    return iters, status, trials


def check_case(name, rec, pr, simple=None):
    """The conditions on a chain_case just written: returns the per-iteration Σδu² and trials."""
    g = dict(np.load(os.path.join(HERE, name + ".npz")))
    assert (g["fit_status"] == 1).all() and (g["fit_iters"] <= FIT_ITERS).all(), (name, g["fit_status"], g["fit_iters"])
    du2 = np.full((NB, FIT_ITERS), np.nan)
    trials = np.zeros((NB, FIT_ITERS), dtype=np.int32)
    for b, h in enumerate(rec.hists):
        du2[b, :len(h)] = [e["du2"] for e in h]
        trials[b, :len(h)] = [e["trials"] for e in h]
        for e in h:
            r = e["du2"] / TOL
            assert r >= 1.25 or r <= 1.0 / 1.25, (name, b, e)
    spread = max(np.abs(K - Ks).max() / np.abs(Ks).max() for K, Ks in zip(rec.K, rec.Ks))
    # the C restatement's counts
    ci, cs, ct = fit_counts(g["x"], g["u"], *c_closures(pr, simple))
    ni = g["fit_iters"].tolist()
    nt = [trials[b, :ni[b]].tolist() for b in range(NB)]
    print(f"{name}: iters {ni} (C {ci}), fit trials {nt} (C {ct}), literal-vs-symmetrised gain spread {spread:.2e}")
    assert ci == ni and cs == g["fit_status"].tolist() and ct == nt, (name, ci, ni, ct, nt)
    return du2, trials, spread


def cases(n, pr):
    """The line-search and x_traj cases on fixture chain{n}c_t16 (make_golden_chain6's
    extend_gravity with three trajectories and the counts taken from the oracle)."""
    name = f"chain{n}c_t{T}"
    g = dict(np.load(os.path.join(HERE, name + ".npz")))
    f, l, lf = closures(pr)
    fc, _, _ = c_closures(pr)
    x, u, d, K = g["x"], g["u"], g["d"], g["K"]
    z = np.zeros_like(x[0])
    total = O.total_cost_generator(z, l, lf)
    ls_prev = np.array([total(x[b], u[b]) for b in range(NB)])
    ls_x, ls_u, ls_cost = np.empty_like(x), np.empty_like(u), np.empty(NB)
    ls_trials = np.empty(NB, dtype=np.int32)
    scale = LS_SCALE[n]
    for b in range(NB):
        st, stc = {}, {}
        ls_x[b], ls_u[b], ls_cost[b] = O.forward_pass(x[b], u[b], z, scale[b] * d[b], K[b], ls_prev[b], f, l, lf,
                                                      max_trials=MG.MAX_TRIALS, stats=st)
        ls_trials[b] = st["trials"]
        O.forward_pass(x[b], u[b], z, scale[b] * d[b], K[b], ls_prev[b], fc, l, lf, max_trials=MG.MAX_TRIALS,
                       stats=stc)
        assert stc["trials"] == st["trials"], (n, b, stc, st)   # the C restatement's count
        for j in range(1, st["trials"] + 1):  # every candidate's margin to prev_cost
            _, _, cj = O.forward_pass(x[b], u[b], z, scale[b] * d[b], K[b], np.inf, f, l, lf, max_trials=1,
                                      alpha0=0.5 ** (j - 1))
            margin = (cj - ls_prev[b]) / ls_prev[b]
            print(f"{name}: ls trajectory {b} trial {j}: cost {cj:.6e} prev {ls_prev[b]:.6e} margin {margin:+.3f}")
            assert (margin < -0.01) if j == st["trials"] else (margin > 0.01), (b, j, margin)
    assert ls_trials.max() >= 2, ls_trials
    xt = 0.1 * x[:, ::-1]
    xt_x, xt_u, xt_cost = np.empty_like(x), np.empty_like(u), np.empty(NB)
    for b in range(NB):
        xt_x[b], xt_u[b], xt_cost[b] = O.forward_pass(x[b], u[b], xt[b], d[b], K[b], np.inf, f, l, lf,
                                                      max_trials=MG.MAX_TRIALS)
    np.savez_compressed(os.path.join(HERE, f"chain{n}c_cases_t{T}.npz"), ls_scale=np.array(scale),
                        ls_prev_cost=ls_prev, ls_trials=ls_trials, ls_x=ls_x, ls_u=ls_u, ls_cost=ls_cost, xt=xt,
                        xt_x=xt_x, xt_u=xt_u, xt_cost=xt_cost)
    print(name, "ls trials", ls_trials.tolist(), f"A[{n}:, :{n}] max", np.abs(g["A"][..., n:, :n]).max(),
          "|K| max", np.abs(K).max(), "|x| max", np.abs(x).max())


def with_conditions(name, du2, trials, spread):
    path = os.path.join(HERE, name + ".npz")
    g = dict(np.load(path))
    g.update(cond_du2=du2, cond_trials=trials, cond_gain_spread=np.array(spread))
    np.savez_compressed(path, **g)


def generate(n):
    pr = coupled_chain_problem(n)
    name = f"chain{n}c_t{T}"
    with Recorder() as rec:
        MG.chain_case(name, n, rbd_initial_states(NB, n, seed0=SEED[n]), T=T, fit_iters=FIT_ITERS, tol=TOL, pr=pr,
                      robot=f"coupled_chain({n})")
    with_conditions(name, *check_case(name, rec, pr))
    cases(n, pr)
    for kind, c in TASK[n].items():
        name = f"chain{n}ctask_{kind}_t{T}"
        s = c["simple"]
        p0 = OC.point_position(pr.chain, s["body"], s["point"], [0.0] * n)
        print(f"{name}: the point at q = 0 is {[round(float(v), 3) for v in p0]}, target {s['final_target']}")
        with Recorder() as rec:
            MG.chain_case(name, n, rbd_initial_states(NB, n, seed0=c["seed0"]), T=T, fit_iters=FIT_ITERS, tol=TOL,
                          pr=pr, robot=f"coupled_chain({n})", simple=s)
        with_conditions(name, *check_case(name, rec, pr, s))
    for f in (f"chain{n}c_t{T}", f"chain{n}c_cases_t{T}", f"chain{n}ctask_euc_t{T}", f"chain{n}ctask_ref_t{T}"):
        size = os.path.getsize(os.path.join(HERE, f + ".npz"))
        print(f"{f}: {size} bytes")
        assert size < 256 * 1024, (f, size)


def main(only=()):
    for n in N_JOINTS:
        if not only or str(n) in only:
            generate(n)


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
