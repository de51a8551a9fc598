"""Fixtures of a tool path on the tiles path (tests/test_gpu_chain_path.py):
ilqr_amd.chain.coupled_chain_problem(n), n ∈ {4, 7}, B = 5 trajectories (the last two-trajectory
workgroup half empty), T = 16, the tool point [0.05, 0.02, 0.1] on the last body, weight = 2e3,
path_weight = PATH_WEIGHT, from the CPU oracle of tests/chain_path.py (pinned by
tests/test_chain_path_oracle.py).

  chain{n}c_path_t16.npz   x, u (a rollout of small random torques) and, per task reading
                           r ∈ {"euc", "ref"} (the squared distance; the reference's p_z
                           against every component): r_path (5, 17, 3), a smooth path within
                           AMP of the rollout's own tool trajectory; the gains r_d, r_K at
                           μ = 0.01; one forward pass r_fw_*; a FIT_ITERS-iteration fit
                           r_fit_* with its history (r_fit_cost, r_cond_du2, r_cond_trials)

Conditions, asserted here so that a regenerated fixture cannot hide a fragile one — the seed of
the path's offsets is raised until they hold, and exact trial counts are demanded of the device
only under them:
  * no line search is exhausted and no trajectory ends on NaN;
  * no gain is NaN;
  * every accept-or-reject decision of every line search has |prev_cost − cost| > 1e-9·|cost|.
Each file stays under 256 KB.

    python tests/golden/make_golden_chain_path.py        # both joint counts (a minute of CPU)
    python tests/golden/make_golden_chain_path.py 4
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ilqr.jl_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import chain_path as CP  # noqa: E402
from ilqr_amd.chain import coupled_chain_problem, rbd_initial_states  # noqa: E402

N_JOINTS = (4, 7)
NB, T = 5, 16
PATH_WEIGHT, AMP = 50.0, 0.005
FIT_ITERS, TOL, MU = 6, 1e-6, 0.01
MARGIN = 1e-9
READINGS = {"euc": True, "ref": False}


def inputs(n):
    """x, u of the suite: tests/test_gpu_chain_targets.inputs' rollout, on the CPU model."""
    pr = coupled_chain_problem(n)
    f = CP.Dynamics(pr)
    u = np.random.default_rng(46 + n).uniform(-0.5, 0.5, (NB, T, n))
    return pr, f, CP.rollout(f, rbd_initial_states(NB, n, seed0=81), u), u


def reading(pr, f, x, u, euclidean, seed):
    """One reading's arrays and whether the conditions hold, with its margin."""
    n = pr.n_joints
    cost = CP.PathCost(pr.chain, n - 1, CP.POINT, CP.WEIGHT, PATH_WEIGHT, euclidean)
    path = CP.smooth_path(pr, x, euclidean, seed, amp=AMP)
    d, K, bst = CP.backward(x, u, path, f, cost, MU)
    log = [("gains", bool(np.isnan(d).any() or np.isnan(K).any() or (bst != 0).any()))]
    fw = CP.forward_pass(x, u, np.zeros_like(x), d, K, np.full(NB, np.inf), f, path, cost, log=log)
    r = CP.fit(x, u, f, path, cost, max_iter=FIT_ITERS, tol=TOL, mu=MU, log=log)
    nan_gain = any(v for k, v in log if k == "gains")
    margin = min(float(np.nanmin(m)) for k, m in log if k != "gains")
    ok = (not nan_gain) and bool(fw[4].all()) and bool(np.isin(r["status"], (1, 2)).all()) and margin > MARGIN
    h = r["history"]
    out = dict(path=path, d=d, K=K, fw_x=fw[0], fw_u=fw[1], fw_cost=fw[2], fw_trials=fw[3], fit_x=r["x"], fit_u=r["u"],
               fit_cost=h["cost"].T, fit_iters=r["iters"], fit_status=r["status"], cond_du2=h["du2"].T,
               cond_trials=h["trials"].T.astype(np.int32))
    return ok, margin, out


def generate(n):
    pr, f, x, u = inputs(n)
    arrays, meta = {"x": x, "u": u}, {}
    for tag, euclidean in READINGS.items():
        for seed in range(1, 33):
            ok, margin, out = reading(pr, f, x, u, euclidean, seed)
            print(f"chain{n}c_path {tag} seed {seed}: margin {margin:.2e} iters {out['fit_iters'].tolist()} "
                  f"status {out['fit_status'].tolist()} trials {out['cond_trials'].tolist()} ok {ok}", flush=True)
            if ok:
                break
        assert ok, (n, tag, "no seed in 1..32 meets the conditions")
        arrays.update({f"{tag}_{k}": v for k, v in out.items()})
        meta[tag] = {"seed": seed, "margin": margin}
    meta.update(T=T, nu=n, fit_max_iter=FIT_ITERS, tol=TOL, mu=MU, robot=f"coupled_chain({n})", path_weight=PATH_WEIGHT,
                amp=AMP, simple=dict(body=n - 1, point=CP.POINT, weight=CP.WEIGHT))
    path = os.path.join(HERE, f"chain{n}c_path_t{T}.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(path)
    print(f"chain{n}c_path_t{T}: {size} bytes", flush=True)
    assert size < 256 * 1024, size


if __name__ == "__main__":
    for n in N_JOINTS:
        if len(sys.argv) < 2 or str(n) in sys.argv[1:]:
            generate(n)
