"""Fixtures of the per-trajectory goals on the tiles path (tests/test_gpu_chain_targets.py):
ilqr_amd.chain.coupled_chain_problem(n), B = 3 trajectories, T = 16, every trajectory with a
goal of its own (ilqr_chain_set_joint_targets / ilqr_chain_set_task_targets). Trajectory b is
the numpy oracle (oracle/rbd.py, oracle/cost_functions.py) run on that trajectory alone with
its goal: RBD.ChainCost(target_b, …) or OC.simple_final_cost(…, final_target_b, …). Mirrors
make_golden_chainN.py. Per joint count n ∈ {4, 7}:

  chain{n}c_targets_t16.npz      joint-space costs, `targets` (3, n): the problem's target plus
                                 JOINT_OFFSETS[n]
  chain{n}ctask_targets_t16.npz  the squared-distance task cost of make_golden_chainN.TASK[n]["euc"],
                                 `targets` (3, 3): its final_target plus TASK_OFFSETS[n]

Four joints use the narrow tiles kernel and the forward group's shortest stage, seven joints
its fifth staging word and the full register files. Each file holds x, u, the gains d and K, a
forward pass (fw_*) and a fit (fit_*) with its history (fit_cost, cond_du2, cond_trials).

Conditions, asserted here so that a regenerated fixture cannot hide a fragile one:
  * every fit converges (status 1) within FIT_ITERS = 20 iterations, and every Σδu² of every
    fit history is a factor ≥ 1.25 away from tol;
  * the C restatement (oracle/cref.py, make_golden_chainN.c_closures) reproduces every
    iteration count and per-iteration trial count;
  * the three trajectories' iteration counts are not all equal: a goal applied to the wrong
    row shows up in the counts.
Each file stays under 256 KB.

    python tests/golden/make_golden_chain_targets.py            # everything (minutes of CPU)
    python tests/golden/make_golden_chain_targets.py 4 joint    # one joint count, one kind
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the repository and the package on sys.path)
import make_golden_chainN as MGN  # noqa: E402
from make_golden_chain6 import FIT_ITERS, TOL, Recorder  # noqa: E402
from ilqr_amd.chain import coupled_chain_problem, rbd_initial_states  # noqa: E402

N_JOINTS = (4, 7)
NB, T = 3, 16
SEED_JOINT = 81
# joint goals: the problem's target plus these (first n entries)
_ROW1 = (0.35, -0.25, 0.3, -0.4, 0.2, -0.3, 0.25)
_ROW2 = (-0.3, 0.4, -0.2, 0.25, -0.35, 0.2, -0.15)
JOINT_OFFSETS = {
    # row 1 is not _ROW1[:4]: with it the last iteration of that fit has Σδu² = tol / 1.23
    # (with −0.5 for −0.4: tol / 1.37)
    4: ((0.0,) * 4, (0.35, -0.25, 0.3, -0.5), _ROW2[:4]),
    7: ((0.0,) * 7, _ROW1, _ROW2),
}
# task goals: TASK[n]["euc"]'s final_target plus these
TASK_OFFSETS = {
    4: ((0.0, 0.0, 0.0), (-0.4, 0.3, -0.2), (0.2, -0.5, 0.3)),
    # row 2 is not (0.2, −0.5, 0.3): with it the last iteration of that fit has Σδu² = tol / 1.10
    # (with 0.35 for 0.3: tol / 1.87)
    7: ((0.0, 0.0, 0.0), (-0.4, 0.3, -0.2), (0.2, -0.5, 0.35)),
}
KEEP = ("x", "u", "d", "K", "fw_x", "fw_u", "fw_cost", "fit_x", "fit_u", "fit_cost", "fit_iters", "fit_status")


def rows(n, kind):
    """(problem, simple or None, goal) of every trajectory and their initial states."""
    pr = coupled_chain_problem(n)
    if kind == "joint":
        goals = [pr.target + np.array(o) for o in JOINT_OFFSETS[n]]
        return [(dataclasses.replace(pr, target=g), None, g) for g in goals], rbd_initial_states(NB, n, seed0=SEED_JOINT)
    c = MGN.TASK[n]["euc"]
    goals = [np.array(c["simple"]["final_target"]) + np.array(o) for o in TASK_OFFSETS[n]]
    return ([(pr, dict(c["simple"], final_target=[float(v) for v in g]), g) for g in goals],
            rbd_initial_states(NB, n, seed0=c["seed0"]))


def generate(n, kind):
    name = f"chain{n}c_targets_t{T}" if kind == "joint" else f"chain{n}ctask_targets_t{T}"
    cases, x0 = rows(n, kind)
    out = {k: [] for k in KEEP}
    du2 = np.full((NB, FIT_ITERS), np.nan)
    trials = np.zeros((NB, FIT_ITERS), dtype=np.int32)
    for b, (pr, simple, goal) in enumerate(cases):
        tmp = f"_{name}_row{b}"
        with Recorder() as rec:
            MG.chain_case(tmp, n, x0[b:b + 1], T=T, fit_iters=FIT_ITERS, tol=TOL, pr=pr, robot=f"coupled_chain({n})",
                          simple=simple)
        path = os.path.join(HERE, tmp + ".npz")
        g = dict(np.load(path))
        os.remove(path)
        assert g["fit_status"][0] == 1 and g["fit_iters"][0] <= FIT_ITERS, (name, b, g["fit_status"], g["fit_iters"])
        (h,) = rec.hists
        du2[b, :len(h)] = [e["du2"] for e in h]
        trials[b, :len(h)] = [e["trials"] for e in h]
        for e in h:
            r = e["du2"] / TOL
            assert r >= 1.25 or r <= 1.0 / 1.25, (name, b, e)
        # the C restatement's counts, with this trajectory's goal
        ci, cs, ct = MGN.fit_counts(g["x"], g["u"], *MGN.c_closures(pr, simple))
        ni, nt = int(g["fit_iters"][0]), trials[b, :len(h)].tolist()
        print(f"{name} row {b}: goal {np.round(goal, 3).tolist()} iters {ni} (C {ci[0]}), trials {nt} (C {ct[0]})",
              flush=True)
        assert ci == [ni] and cs == [1] and ct == [nt], (name, b, ci, ni, ct, nt)
        for k in KEEP:
            out[k].append(g[k])
    out = {k: np.concatenate(v) for k, v in out.items()}
    iters = out["fit_iters"].tolist()
    assert len(set(iters)) > 1, (name, iters)   # a goal on the wrong row changes a count
    simple0 = cases[0][1]
    meta = {"T": T, "nu": n, "fit_max_iter": FIT_ITERS, "tol": TOL, "robot": f"coupled_chain({n})",
            "simple": None if simple0 is None else {k: v for k, v in simple0.items() if k != "final_target"}}
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, targets=np.stack([c[2] for c in cases]), cond_du2=du2, cond_trials=trials,
                        meta=np.array(json.dumps(meta)), **out)
    size = os.path.getsize(path)
    print(f"{name}: fit iters {iters}, {size} bytes", flush=True)
    assert size < 256 * 1024, (name, size)


def main(only=()):
    for n in N_JOINTS:
        for kind in ("joint", "task"):
            if (not only) or (str(n) in only and (kind in only or not {"joint", "task"} & set(only))):
                generate(n, kind)


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
