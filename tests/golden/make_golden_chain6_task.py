"""Fixtures of the six-joint chain under cost_functions.jl's task-space costs
(tests/test_gpu_chain6_task.py, tests/test_chain6_task_abi.py): the 6-DoF arm with gravity,
ℓ = Σu², ℓ_f = weight·Σₖ (pₖ − tₖ)² (euclidean) or weight·Σₖ (p_z − tₖ)² (the reference's
reading) of a point fixed on one body.

  chain6task_euc_t30.npz   body 5 (the tool), squared distance, 2 trajectories, T = 30
  chain6task_ref_t24.npz   body 5, the reference's reading, 2 trajectories, T = 24
  chain6task_b2_t24.npz    body 2 with an off-axis point, squared distance, T = 24: joints
                           3-5 do not move the point (zero rows / columns of the terminal tiles)
  chain6ctask_euc_t24.npz  the general mechanism (coupled_6dof_problem), body 5, squared distance
  chain6ctask_ref_t24.npz  the general mechanism, body 2 with an off-axis point, the reference's
                           reading (tests/test_gpu_chain6_general.py)

All through make_golden.chain_case(..., simple=...) (the numpy oracle: RNEA + RK4, exact
Jacobians by forward-mode AD, the costs differentiated by the ForwardDiff restatement). The
conditions of make_golden_chain6.py hold for every case (its check_fits):
  * every Σδu² of every fit history is a factor ≥ 1.25 away from tol,
  * every fit line search takes one trial,
and each file stays under 160 KB. Prints the literal-vs-symmetrised spread of the gains. The
margins and trial counts are also stored in each file (`cond_*`), where the CPU test reads
them back.

    python tests/golden/make_golden_chain6_task.py                      # all (minutes of CPU)
    python tests/golden/make_golden_chain6_task.py chain6task_b2_t24    # one
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository and the package on sys.path)
from make_golden_chain6 import FIT_ITERS, TOL, Recorder, check_fits  # noqa: E402
from ilqr_amd.chain import coupled_6dof_problem, rbd_6dof_problem, rbd_initial_states  # noqa: E402

# The arm's links are about a metre and the tool sits at (5.55, 0.52, 0.10) at q = 0: a
# target near the origin is out of reach and the fit stops at once.
CASES = {
    "chain6task_euc_t30": dict(seed0=81, T=30, simple=dict(
        body=5, point=[0.05, 0.02, 0.1], final_target=[3.9, 3.5, 1.3], weight=2e3, euclidean=True)),
    # not seed 81: at T = 30 its first trajectory ends on Σδu² = 8.66e-7, a factor 1.15 from tol
    "chain6task_ref_t24": dict(seed0=83, T=24, simple=dict(
        body=5, point=[0.05, 0.02, 0.1], final_target=[3.9, 3.5, 1.3], weight=2e3, euclidean=False)),
    "chain6task_b2_t24": dict(seed0=81, T=24, simple=dict(
        body=2, point=[0.3, -0.2, 0.15], final_target=[1.6, 1.2, 0.8], weight=2e3, euclidean=True)),
    # the general mechanism (coupled_6dof_problem: R0 ≠ I in the point's kinematics); its tool
    # sits at (3.30, 0.57, 0.56) at q = 0 and body 2's point at (2.10, 0.11, 0.44)
    # not seed 81: its second trajectory is still moving at max_iter = 20 (status MAX_ITER,
    # cost 6.2e3), twenty iterations of rounding for the iterate tolerance to carry; not seeds
    # 85 or 87 either: a line search inside their fits takes more than one trial (56 trials at
    # seed 85's second iteration, 2 at seed 87's fifth), which check_fits rejects
    "chain6ctask_euc_t24": dict(seed0=83, T=24, general=True, simple=dict(
        body=5, point=[0.05, 0.02, 0.1], final_target=[2.1, 1.4, 1.5], weight=2e3, euclidean=True)),
    "chain6ctask_ref_t24": dict(seed0=81, T=24, general=True, simple=dict(
        body=2, point=[0.3, -0.2, 0.15], final_target=[0.9, 1.0, 1.1], weight=2e3, euclidean=False)),
}


def generate(name, seed0, T, simple, nb=2, general=False):
    pr = coupled_6dof_problem() if general else rbd_6dof_problem(gravity=True)
    with Recorder() as rec:
        MG.chain_case(name, 6, rbd_initial_states(nb, 6, seed0=seed0), T=T, fit_iters=FIT_ITERS, tol=TOL,
                      pr=pr, robot="coupled_6dof" if general else "6dof_arm+gravity", simple=simple)
    check_fits(name, rec)
    # the conditions as data, beside the case they hold for
    path = os.path.join(HERE, name + ".npz")
    g = dict(np.load(path))
    du2 = np.full((nb, FIT_ITERS), np.nan)
    trials = np.zeros((nb, FIT_ITERS), dtype=np.int32)
    for b, h in enumerate(rec.hists):
        du2[b, :len(h)] = [e["du2"] for e in h]
        trials[b, :len(h)] = [e["trials"] for e in h]
    spread = max(np.abs(K - Ks).max() / np.abs(Ks).max() for K, Ks in zip(rec.K, rec.Ks))
    g.update(cond_du2=du2, cond_trials=trials, cond_gain_spread=np.array(spread))
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    assert size < 160 * 1024, (name, size)
    print(f"{name}: {size} bytes, |K| max {np.abs(g['K']).max():.3e}, fit cost "
          f"{[float(c[~np.isnan(c)][-1]) for c in g['fit_cost']]}")


def main(only=()):
    for name, c in CASES.items():
        if not only or name in only:
            generate(name, **c)


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
