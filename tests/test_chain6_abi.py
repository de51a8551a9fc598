"""The six-joint chain's ABI surface and fixtures, without a GPU: the per-dtype support
query (include/ilqr.h), its export, the problem constructor, and the frozen fixtures of
tests/golden/make_golden_chain6.py against the numpy oracle."""
import os
import re

import numpy as np
import pytest

from ilqr_amd import _lib
from ilqr_amd.chain import ChainProblem, load_robot, rbd_6dof_problem, rbd_initial_states
from oracle import rbd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_chain_supported_dtype_values():
    lib = _lib.load()
    q = lib.ilqr_chain_supported_dtype
    for dt in (_lib.F32, _lib.F64):
        assert q(2, 1, dt) == 1 and q(2, 2, dt) == 1
    assert q(6, 6, _lib.F64) == 1
    assert q(6, 6, _lib.F32) == 0          # fp64 only: the recursion is the f64 MFMA tiles kernel
    assert q(6, 1, _lib.F64) == 0 and q(6, 1, _lib.F32) == 0
    assert q(3, 3, _lib.F64) == 0 and q(2, 3, _lib.F64) == 0 and q(0, 0, _lib.F64) == 0
    assert q(6, 6, 7) == 0 and q(2, 2, 7) == 0 and q(2, 2, -1) == 0   # an invalid dtype
    # the old query keeps its value: "in every dtype"
    assert lib.ilqr_chain_supported(6, 6) == 0
    assert lib.ilqr_chain_supported(2, 2) == 1 and lib.ilqr_chain_supported(2, 1) == 1
    assert lib.ilqr_supported(_lib.PROBLEM_CHAIN, 12, 6) == 0
    assert lib.ilqr_supported(_lib.PROBLEM_CHAIN, 4, 2) == 1


def test_chain_supported_dtype_declared_and_exported():
    with open(os.path.join(ROOT, "include", "ilqr.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+ilqr_chain_supported_dtype\s*\(\s*int\s+n_joints\s*,\s*int\s+nu\s*,\s*int32_t\s+dtype\s*\)\s*;", h)
    assert re.search(r"#define\s+ILQR_ABI_VERSION\s+2\b", h)   # additive: the version stays
    import ctypes as C
    raw = C.CDLL(_lib.load()._name)
    assert hasattr(raw, "ilqr_chain_supported_dtype")


def test_six_joint_problem_shapes():
    with pytest.raises(ValueError):
        ChainProblem(load_robot("6dof_arm"), 3)
    pr = rbd_6dof_problem()
    assert (pr.n_joints, pr.nu, pr.nx, pr.dt) == (6, 6, 12, 0.01)
    assert np.array_equal(pr.target, [0.5, -0.4, 0.3, 0.6, -0.2, 0.4])
    assert (pr.q_weight == 100.0).all() and (pr.r_weight == 10.0).all() and (pr.qf_weight == 1e6).all()
    assert np.array_equal(pr.chain.gravity, np.zeros(3))         # as the URDF parses
    pg = rbd_6dof_problem(gravity=True)
    assert np.array_equal(pg.chain.gravity, [0.0, 0.0, -9.81])
    assert np.array_equal(load_robot("6dof_arm").gravity, np.zeros(3))   # a copy was changed
    s = pg.struct()
    assert (s.n_joints, s.nu) == (6, 6) and list(s.gravity) == [0.0, 0.0, -9.81] and s.target[5] == 0.4


@pytest.mark.parametrize("name,pr,nb,seed0", [("chain6_t30", rbd_6dof_problem(), 3, 80),
                                              ("chain6g_t30", rbd_6dof_problem(gravity=True), 2, 81)])
def test_chain6_fixtures_consistent(name, pr, nb, seed0):
    """Spot-check the frozen six-joint fixtures against the oracle (same seeds)."""
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    assert z["x"].shape == (nb, 31, 12) and z["u"].shape == (nb, 30, 6)
    assert np.allclose(z["x"][:, 0], rbd_initial_states(nb, 6, seed0=seed0), rtol=0, atol=0)
    model = rbd.ChainModel(pr.chain, pr.dt)
    A, B = model.linearize(z["x"][:, 5], z["u"][:, 5])
    assert np.allclose(A, z["A"][:, 5], rtol=0, atol=1e-14) and np.allclose(B, z["B"][:, 5], rtol=0, atol=1e-14)
    assert (z["fit_status"] == 1).all()
    assert z["fit_iters"].tolist() == ([8, 7, 6] if nb == 3 else [7, 5])
    if nb == 2:
        # gravity makes ∂q̈/∂q nonzero from rest: the block a wrong joint rotation shows in
        assert np.abs(z["A"][..., 6:, :6]).max() > 0.05
        c = np.load(os.path.join(GOLD, "chain6g_cases_t30.npz"), allow_pickle=False)
        assert c["ls_trials"].tolist() == [4, 2] and c["ls_scale"].tolist() == [9.0, 2.5]
        assert np.array_equal(c["xt"], 0.1 * z["x"][:, ::-1])
        assert (c["ls_cost"] < c["ls_prev_cost"]).all()
    else:
        assert np.abs(z["A"][:, 0, 6:, :6]).max() == 0.0   # at rest, u = 0, no gravity
