"""The ABI surface and fixtures of the 4-, 5- and 7-joint chains, without a GPU: the support
queries of the new shapes (include/ilqr.h), ilqr_amd.chain.coupled_chain_problem, and the frozen
fixtures of tests/golden/make_golden_chainN.py against the numpy oracle."""
import dataclasses
import os

import numpy as np
import pytest

from ilqr_amd import _lib
from ilqr_amd.chain import (COUPLED7_RPY, RBD_TARGET_JOINTS_6DOF, RBD_TARGET_JOINTS_7DOF, coupled_6dof_problem,
                            coupled_chain_problem, rbd_initial_states)
from ilqr_amd.urdf import rpy_matrix
from oracle import rbd

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NEW = (4, 5, 7)
NB, T = 3, 16
SEED = {4: 81, 5: 81, 7: 81}                       # make_golden_chainN.SEED
TASK_SEED = {4: {"euc": 83, "ref": 81}, 5: {"euc": 83, "ref": 81}, 7: {"euc": 81, "ref": 81}}   # its TASK


def test_chain_supported_new_shapes():
    """(4, 4), (5, 5), (7, 7) iterate in fp64 and not in fp32; three and eight joints, a single
    drive and a partial drive stay refused; the pinned answers keep their values."""
    lib = _lib.load()
    q = lib.ilqr_chain_supported_dtype
    for n in NEW:
        assert q(n, n, _lib.F64) == 1, n
        assert q(n, n, _lib.F32) == 0, n
        assert q(n, n, 7) == 0 and q(n, n, -1) == 0          # an invalid dtype
    for nj, nu in ((3, 3), (8, 8), (7, 1), (4, 2), (9, 9), (4, 1), (5, 4), (7, 6)):
        assert q(nj, nu, _lib.F64) == 0 and q(nj, nu, _lib.F32) == 0, (nj, nu)
    # the pinned old values
    for dt in (_lib.F32, _lib.F64):
        assert q(2, 1, dt) == 1 and q(2, 2, dt) == 1
    assert q(6, 6, _lib.F64) == 1 and q(6, 6, _lib.F32) == 0
    assert q(6, 1, _lib.F64) == 0 and q(2, 3, _lib.F64) == 0 and q(0, 0, _lib.F64) == 0
    # "in every dtype": the old queries answer 0 beyond two joints
    for n in (3, 4, 5, 6, 7, 8):
        assert lib.ilqr_chain_supported(n, n) == 0, n
        assert lib.ilqr_supported(_lib.PROBLEM_CHAIN, 2 * n, n) == 0, n
    assert lib.ilqr_chain_supported(2, 2) == 1 and lib.ilqr_chain_supported(2, 1) == 1
    assert lib.ilqr_supported(_lib.PROBLEM_CHAIN, 4, 2) == 1


def test_coupled_chain_six_is_coupled_6dof():
    """coupled_chain_problem(6) equals coupled_6dof_problem() field by field, with and without gravity."""
    for gravity in (True, False):
        a, b = coupled_chain_problem(6, gravity=gravity), coupled_6dof_problem(gravity=gravity)
        assert [f.name for f in dataclasses.fields(a)] == [f.name for f in dataclasses.fields(b)]
        for f in dataclasses.fields(a):
            if f.name == "chain":
                continue
            va, vb = getattr(a, f.name), getattr(b, f.name)
            assert np.array_equal(va, vb), f.name
        for f in dataclasses.fields(a.chain):
            va, vb = getattr(a.chain, f.name), getattr(b.chain, f.name)
            assert (va == vb) if isinstance(va, (list, float, int)) else np.array_equal(va, vb), f.name
        assert bytes(a.struct()) == bytes(b.struct())


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_coupled_chain_shapes(n):
    """The first n joints take coupled_6dof_problem's constants; the targets are
    RBD_TARGET_JOINTS_6DOF extended by one value."""
    pr, six = coupled_chain_problem(n), coupled_6dof_problem()
    assert (pr.n_joints, pr.nu, pr.nx, pr.dt) == (n, n, 2 * n, 0.01)
    assert RBD_TARGET_JOINTS_7DOF[:6] == RBD_TARGET_JOINTS_6DOF and len(RBD_TARGET_JOINTS_7DOF) == 7
    assert tuple(pr.target) == RBD_TARGET_JOINTS_7DOF[:n]
    assert (pr.q_weight == 100.0).all() and (pr.r_weight == 10.0).all() and (pr.qf_weight == 1e6).all()
    assert np.array_equal(pr.chain.gravity, [0.0, 0.0, -9.81])
    assert np.array_equal(coupled_chain_problem(n, gravity=False).chain.gravity, np.zeros(3))
    m = min(n, 6)
    for name in ("R0", "p", "axis", "mass", "com", "Ic"):
        assert np.array_equal(getattr(pr.chain, name)[:m], getattr(six.chain, name)[:m]), name
    s = pr.struct()
    assert (s.n_joints, s.nu) == (n, n) and s.target[n - 1] == RBD_TARGET_JOINTS_7DOF[n - 1]
    for bad in (3, 8, 2):
        with pytest.raises(ValueError):
            coupled_chain_problem(bad)


def test_coupled_seven_is_not_degenerate():
    """Joint 7 in the sense of test_chain_oracle.py test_coupled_six_is_not_degenerate: on the
    arrays themselves, and in what each symmetrising edit of joint 7 alone does to one oracle
    RK4 step — transposing its R0, taking [a]×·R0 for R0·[a]× (the rotation about the axis
    applied on the other side of the frame: Rot(a, q)·R0 = R0·Rot(R0ᵀa, q)), zeroing its COM,
    dropping its products of inertia — each ≥ 1e-2 of the step's largest entry."""
    pr = coupled_chain_problem(7)
    ch = pr.chain
    i = 6
    assert np.array_equal(ch.R0[i], rpy_matrix(COUPLED7_RPY)) and all(v != 0.0 for v in COUPLED7_RPY)
    assert np.abs(ch.R0[i] - ch.R0[i].T).max() > 0.1                    # R0ᵀ ≠ R0
    assert np.abs(ch.R0[i] @ ch.R0[i].T - np.eye(3)).max() < 1e-15
    assert np.abs(ch.p[i]).min() >= 0.05 and np.abs(ch.com[i]).min() >= 0.03
    assert np.abs(ch.axis[i]).min() > 0.15 and abs(np.linalg.norm(ch.axis[i]) - 1.0) < 1e-15
    assert np.array_equal(ch.Ic[i], ch.Ic[i].T)
    w = np.linalg.eigvalsh(ch.Ic[i])
    assert w[0] > 0 and np.diff(w).min() > 0.1 * w[0] and w[0] + w[1] > w[2]
    assert min(abs(ch.Ic[i][0, 1]), abs(ch.Ic[i][0, 2]), abs(ch.Ic[i][1, 2])) > 1e-3
    assert len(set(ch.mass.tolist())) == 7

    rng = np.random.default_rng(7)
    X = np.concatenate([rng.uniform(-2, 2, (24, 7)), rng.uniform(-1, 1, (24, 7))], axis=1)
    U = rng.uniform(-5, 5, (24, 7))
    base = rbd.ChainModel(ch, 0.01).step(X, U)

    def joint7(name, value):
        a = getattr(ch, name).copy()
        a[i] = value
        return {name: a}

    edits = {"R0 transposed": joint7("R0", ch.R0[i].T),
             "[a]x.R0 for R0.[a]x": joint7("axis", ch.R0[i].T @ ch.axis[i]),
             "COM zeroed": joint7("com", np.zeros(3)),
             "products of inertia dropped": joint7("Ic", np.diag(np.diag(ch.Ic[i])))}
    for what, kw in edits.items():
        moved = rbd.ChainModel(dataclasses.replace(ch, **kw), 0.01).step(X, U)
        r = np.abs(moved - base).max() / np.abs(base).max()
        print(f"joint 7, {what}: one RK4 step moves by {r:.2e} (relative)")
        assert r >= 1e-2, (what, r)


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n", NEW)
def test_chainN_fixtures_consistent(n):
    """Spot-check the frozen fixtures against the oracle (same seeds), and the conditions
    make_golden_chainN.py asserted, read back from the files."""
    pr = coupled_chain_problem(n)
    nx = 2 * n
    z = load(f"chain{n}c_t{T}")
    assert z["x"].shape == (NB, T + 1, nx) and z["u"].shape == (NB, T, n)
    assert z["A"].shape == (NB, T, nx, nx) and z["B"].shape == (NB, T, nx, n) and z["K"].shape == (NB, T, n, nx)
    assert np.array_equal(z["x"][:, 0], rbd_initial_states(NB, n, seed0=SEED[n]))
    model = rbd.ChainModel(pr.chain, pr.dt)
    A, B = model.linearize(z["x"][:, 5], z["u"][:, 5])
    assert np.allclose(A, z["A"][:, 5], rtol=0, atol=1e-14) and np.allclose(B, z["B"][:, 5], rtol=0, atol=1e-14)
    assert np.allclose(model.step(z["x"][:, 5], z["u"][:, 5]), z["x"][:, 6], rtol=0, atol=1e-15)
    assert np.abs(z["A"][..., n:, :n]).max() > 0.05               # ∂q̈/∂q: gravity and coupling
    assert (z["fit_status"] == 1).all() and (z["fit_iters"] <= 20).all() and (z["fit_iters"] >= 2).all()
    for b in range(NB):
        k = int(z["fit_iters"][b])
        du2 = z["cond_du2"][b]
        assert np.isfinite(du2[:k]).all() and np.isnan(du2[k:]).all()
        assert du2[k - 1] <= 1e-6 / 1.25 and (du2[:k - 1] >= 1.25e-6).all()
        assert (z["cond_trials"][b, :k] >= 1).all() and (z["cond_trials"][b, k:] == 0).all()
    c = load(f"chain{n}c_cases_t{T}")
    assert c["ls_trials"].max() >= 2 and (c["ls_trials"] >= 1).all()      # a trial past the first
    assert (c["ls_cost"] < c["ls_prev_cost"]).all()
    assert np.array_equal(c["xt"], 0.1 * z["x"][:, ::-1])
    assert c["ls_x"].shape == z["x"].shape and c["xt_u"].shape == z["u"].shape
    for kind in ("euc", "ref"):
        t = load(f"chain{n}ctask_{kind}_t{T}")
        assert t["x"].shape == (NB, T + 1, nx)
        assert np.array_equal(t["x"][:, 0], rbd_initial_states(NB, n, seed0=TASK_SEED[n][kind]))
        assert (t["fit_status"] == 1).all() and (t["fit_iters"] <= 20).all()
        assert np.allclose(model.step(t["x"][:, 3], t["u"][:, 3]), t["x"][:, 4], rtol=0, atol=1e-15)
    for f in (f"chain{n}c_t{T}", f"chain{n}c_cases_t{T}", f"chain{n}ctask_euc_t{T}", f"chain{n}ctask_ref_t{T}"):
        assert os.path.getsize(os.path.join(GOLD, f + ".npz")) < 256 * 1024, f
