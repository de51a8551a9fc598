"""CPU tests pinning the RBD-family oracle (oracle/rbd.py) and its host plumbing.

RigidBodyDynamics.jl (the reference's dynamics library for
test/RBD_2_link_example) is absent, so the restatement is pinned by known answers:
  * the fixed-base 2Dof_arm.urdf has COMs on the joint origins and isotropic link
    inertias (0.5·I), with zero gravity as the reference parses it
    (RBD_helper_functions.jl:7): M(q) = diag(0.5 + 0.5 + 3·1², 0.5) = diag(4, 0.5)
    for every q and dynamics_bias ≡ 0;
  * on the coupled 6Dof_arm.urdf, M from the recursive Newton-Euler columns equals an
    independent formulation Σ mJ_vᵀJ_v + J_ωᵀ I J_ω, is symmetric positive definite,
    and RNEA(q, q̇, M⁻¹(τ − b)) = τ;
  * the unforced rollout conserves kinetic energy (RK4 error only);
  * the exact (forward-mode) Jacobians match central differences; the cost
    derivatives match oracle.dual (the ForwardDiff restatement).
"""
import os

import numpy as np
import pytest

from ilqr_amd import _lib
from ilqr_amd.chain import (ChainProblem, chain_closures, load_robot, rbd_2dof_problem,
                            rbd_initial_states)
from ilqr_amd.urdf import parse_urdf, rpy_matrix
from oracle import dual
from oracle import rbd as RBD

GOLD = os.path.join(os.path.dirname(__file__), "golden")
REF_URDF = os.path.join(GOLD, "urdf")  # the reference's test/urdf descriptions, stored as fixtures


@pytest.fixture(scope="module")
def arm2():
    return RBD.ChainModel(load_robot("2dof_arm"))


@pytest.fixture(scope="module")
def arm6():
    return RBD.ChainModel(load_robot("6dof_arm"))


def test_two_dof_closed_form(arm2):
    rng = np.random.default_rng(0)
    for _ in range(5):
        q, qd = rng.uniform(-3, 3, 2), rng.uniform(-2, 2, 2)
        assert np.allclose(arm2.mass_matrix_np(q), np.diag([4.0, 0.5]), atol=1e-14)
        assert np.abs(arm2.bias_np(q, qd)).max() < 1e-14


def test_six_dof_mass_matrix_independent_formulation(arm6):
    rng = np.random.default_rng(1)
    for _ in range(5):
        q = rng.uniform(-3, 3, 6)
        M = arm6.mass_matrix_np(q)
        Mj = RBD.mass_matrix_jacobian(arm6.ch, q)
        assert np.abs(M - Mj).max() < 1e-12 * np.abs(Mj).max()
        assert np.abs(M - M.T).max() < 1e-12 * np.abs(M).max()
        assert np.linalg.eigvalsh(M).min() > 0
        # genuinely coupled (unlike the 2-DoF arm)
        assert np.abs(M - np.diag(np.diag(M))).max() > 0.1


def test_six_dof_rnea_inverts_forward_dynamics(arm6):
    rng = np.random.default_rng(2)
    q, qd, tau = rng.uniform(-2, 2, 6), rng.uniform(-1, 1, 6), rng.uniform(-3, 3, 6)
    qdd = np.linalg.solve(arm6.mass_matrix_np(q), tau - arm6.bias_np(q, qd))
    back = arm6.rnea([np.array([v]) for v in q], [np.array([v]) for v in qd],
                     [np.array([v]) for v in qdd])
    assert np.abs(np.array([v[0] for v in back]) - tau).max() < 1e-12


def test_six_dof_energy_conservation(arm6):
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 6)])[None]
    u = np.zeros((1, 6))
    ke = lambda x: 0.5 * x[0, 6:] @ arm6.mass_matrix_np(x[0, :6]) @ x[0, 6:]
    e0 = ke(x)
    for _ in range(100):
        x = arm6.step(x, u)
    assert abs(ke(x) - e0) < 1e-8 * e0


def test_exact_jacobians_match_central_differences(arm6):
    rng = np.random.default_rng(4)
    X, U = rng.uniform(-1, 1, (3, 12)), rng.uniform(-1, 1, (3, 6))
    A, B = arm6.linearize(X, U)
    h = 1e-6
    Afd = np.stack([(arm6.step(X + h * np.eye(12)[k], U) - arm6.step(X - h * np.eye(12)[k], U)) / (2 * h)
                    for k in range(12)], axis=2)
    Bfd = np.stack([(arm6.step(X, U + h * np.eye(6)[k]) - arm6.step(X, U - h * np.eye(6)[k])) / (2 * h)
                    for k in range(6)], axis=2)
    assert np.abs(A - Afd).max() < 1e-8 and np.abs(B - Bfd).max() < 1e-8


def test_cost_derivatives_match_forwarddiff_restatement():
    pr = rbd_2dof_problem(2)
    cost = RBD.ChainCost(pr.target, pr.q_weight, pr.r_weight, pr.qf_weight)
    x, u = np.array([0.3, -0.2, 0.1, 0.05]), np.array([1.5, -0.7])
    _, qv, r, Q, P, R = cost.quad(x, u)
    assert np.allclose(qv, dual.gradient(lambda z: cost.immediate(z, u), x))
    assert np.allclose(r, dual.gradient(lambda z: cost.immediate(x, z), u))
    assert np.allclose(Q, dual.hessian(lambda z: cost.immediate(z, u), x))
    assert np.allclose(R, dual.hessian(lambda z: cost.immediate(x, z), u))
    _, g, H = cost.fquad(x)
    assert np.allclose(g, dual.gradient(cost.final, x)) and np.allclose(H, dual.hessian(cost.final, x))
    # nu = 1: only joint 1's torque is penalised
    c1 = RBD.ChainCost(pr.target, pr.q_weight, pr.r_weight, pr.qf_weight)
    assert c1.immediate(x, u[:1]) == pytest.approx(
        np.sum(pr.q_weight * (pr.target - x[:2]) ** 2) + pr.r_weight[0] * u[0] ** 2)


def test_reference_costs_restated():
    """RBD_helper_functions.jl:85-116 on the joint rows and animate_RBD_2_link.jl:8-10."""
    pr = rbd_2dof_problem(2)
    assert pr.dt == 0.01 and tuple(pr.target) == (1.0, 0.3)
    assert (pr.q_weight == 100.0).all() and (pr.r_weight == 10.0).all() and (pr.qf_weight == 1e6).all()
    dyn, cost, fcost = chain_closures(pr)
    x, u = np.array([0.5, 0.1, 0.0, 0.0]), np.array([1.0, 2.0])
    assert cost(x, u) == pytest.approx(10.0 * (10 * 0.5 ** 2 + 10 * 0.2 ** 2) + (10 * 1 + 10 * 4))
    assert fcost(x) == pytest.approx(1e5 * (10 * 0.5 ** 2 + 10 * 0.2 ** 2))


@pytest.mark.parametrize("name", ["2Dof_arm", "6Dof_arm"])
def test_shipped_robots_match_the_reference_urdfs(name):
    a, b = parse_urdf(os.path.join(REF_URDF, name + ".urdf")), load_robot(name.lower())
    for f in ("R0", "p", "axis", "mass", "com", "Ic"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_urdf_conventions():
    assert np.allclose(rpy_matrix([0, 0, np.pi / 2]) @ [1, 0, 0], [0, 1, 0])
    assert np.allclose(rpy_matrix([np.pi / 2, 0, 0]) @ [0, 1, 0], [0, 0, 1])
    ch = load_robot("2dof_arm")
    assert ch.names == ["joint_1", "joint_2"]
    assert np.allclose(ch.axis, [[0, 0, 1], [0, 1, 0]]) and np.allclose(ch.p, [[0.5, 0.5, 0], [1, 0, 0]])
    # the massless tool link of the 6-DoF arm merges into link_6 without changing it
    ch6 = load_robot("6dof_arm")
    assert ch6.n == 6 and np.allclose(ch6.mass, 3.0)


def test_golden_fixtures_consistent(arm2):
    """Spot-check the frozen chain2 fixture against the oracle (same seeds)."""
    z = np.load(os.path.join(GOLD, "chain2_t100.npz"), allow_pickle=False)
    assert np.allclose(z["x"][:, 0], rbd_initial_states(3, 2, seed0=0))
    A, B = arm2.linearize(z["x"][:, 5], z["u"][:, 5])
    assert np.allclose(A, z["A"][:, 5], rtol=0, atol=1e-14) and np.allclose(B, z["B"][:, 5], atol=1e-14)
    # the fixed-base arm is linear: A = block RK4 of a double integrator
    assert np.allclose(A[0, :2, 2:], 0.01 * np.eye(2))


def test_chain_struct_packing():
    pr = rbd_2dof_problem(1)
    s = pr.struct()
    assert (s.n_joints, s.nu, s.dt) == (2, 1, 0.01)
    assert list(s.axis[0]) == [0.0, 0.0, 1.0] and s.mass[1] == 3.0
    assert s.qf_weight[0] == 1e6 and s.target[1] == 0.3
    with pytest.raises(ValueError):
        ChainProblem(load_robot("2dof_arm"), nu=3)


def test_chain_abi_validates_without_gpu():
    """Argument checks of ilqr_chain_create happen before any HIP call."""
    import ctypes as C
    lib = _lib.load()
    s = rbd_2dof_problem(2).struct()
    h = C.c_void_p()
    assert lib.ilqr_chain_create(C.byref(h), 0, C.byref(s), 0, 8, _lib.F32, 0) == _lib.ERR_BAD_DIMS
    assert lib.ilqr_chain_create(C.byref(h), 0, C.byref(s), 10, 8, 7, 0) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_create(C.byref(h), 0, C.byref(s), 10, 8, _lib.F32, 9) == _lib.ERR_BAD_ARG
    s.nu = 3
    assert lib.ilqr_chain_create(C.byref(h), 0, C.byref(s), 10, 8, _lib.F32, 0) == _lib.ERR_BAD_DIMS
    assert lib.ilqr_chain_supported(2, 2) == 1 and lib.ilqr_chain_supported(2, 1) == 1
    assert lib.ilqr_chain_supported(6, 6) == 0
    assert lib.ilqr_supported(_lib.PROBLEM_CHAIN, 4, 2) == 1


# -- the C restatement of the chain family (oracle/ilqr_ref.c, CPU baseline of config 5)
@pytest.mark.parametrize("robot,nu", [("2dof_arm", 2), ("2dof_arm", 1), ("6dof_arm", 6)])
def test_c_chain_dynamics_matches_numpy_oracle(robot, nu):
    """Two restatements of the same published algorithms (RNEA bias, unit-acceleration
    mass-matrix columns, Gaussian elimination, RK4): C vs numpy agree to rounding."""
    import copy
    from oracle import cref
    ch = copy.deepcopy(load_robot(robot))
    pr = ChainProblem(ch, nu, 0.01, np.full(ch.n, 0.3), np.full(ch.n, 2.0), np.full(ch.n, 0.5),
                      np.full(ch.n, 7.0))
    if robot == "6dof_arm":  # exercise gravity too (the reference parses the URDF without it)
        ch.gravity = np.array([0.0, 0.0, -9.81])
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.5, 1.5, (40, 2 * ch.n))
    U = rng.uniform(-2.0, 2.0, (40, nu))
    ref = RBD.ChainModel(ch, 0.01).step(X, U)
    out = cref.chain_dynamics(pr, X, U)
    assert np.abs(out - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_c_chain_iteration_matches_numpy_oracle():
    """One cold-start iteration (C: central differences; numpy: exact Jacobians):
    gains within the differencing error, rollouts and costs of the same gains exactly."""
    from oracle import cref
    from oracle import ilqr_oracle as O
    pr = rbd_2dof_problem(2)
    T, nb = 30, 3
    x0 = rbd_initial_states(nb, 2)
    model = RBD.ChainModel(pr.chain, pr.dt)
    cost = RBD.ChainCost(pr.target, pr.q_weight, pr.r_weight, pr.qf_weight)
    f, l, lf = RBD.chain_closures(model, cost)
    u = np.zeros((nb, T, 2))
    x = np.zeros((nb, T + 1, 4))
    x[:, 0] = x0
    for t in range(T):
        x[:, t + 1] = model.step(x[:, t], u[:, t])
    d, K, xn, un, c, tr = cref.chain_iterate(pr, x, u)
    assert (tr == 1).all()
    for b in range(nb):
        do, Ko = O.backward_pass(x[b], u[b], f, l, lf, symmetrize=True)
        assert np.abs(K[b] - Ko).max() <= 1e-6 * np.abs(Ko).max()
        assert np.abs(d[b] - do).max() <= 1e-6 * np.abs(do).max()
        xo, uo, co = O.forward_pass(x[b], u[b], np.zeros_like(x[b]), d[b], K[b], np.inf, f, l, lf)
        assert np.abs(xn[b] - xo).max() <= 1e-12 * np.abs(xo).max()
        assert abs(c[b] - co) <= 1e-12 * abs(co)


def test_coupled_chain_is_not_degenerate():
    """The fixture really exercises the coupling terms (CPU-checkable property)."""
    from ilqr_amd.chain import coupled_2dof_problem
    from oracle import rbd
    m = rbd.ChainModel(coupled_2dof_problem(2).chain, 0.01)
    M0, M1 = m.mass_matrix_np(np.array([0.0, 0.0])), m.mass_matrix_np(np.array([0.7, -1.1]))
    assert abs(M0[0, 1]) > 1e-2 and np.abs(M0 - M1).max() > 1e-2
    assert np.abs(m.bias_np(np.array([0.4, 0.9]), np.zeros(2))).max() > 1.0      # gravity
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "chain2c_t40.npz"))
    assert np.abs(g["A"][..., 2:, :2]).max() > 1e-3                                # ∂q̈/∂q


# -- the general six-joint mechanism (ilqr_amd.chain.coupled_6dof_problem) -----------------
@pytest.fixture(scope="module")
def gen6():
    from ilqr_amd.chain import coupled_6dof_problem
    return coupled_6dof_problem()


def test_coupled_six_is_not_degenerate(gen6):
    """Every term that vanishes on the shipped 6-DoF arm is nonzero here, on the arrays
    themselves and in what it does to one RK4 step: each of seven symmetrising edits of the
    mechanism moves ChainModel.step by more than 1e-3 of its largest entry (on the shipped
    arm transposing every R0 moves it by exactly 0)."""
    import dataclasses
    from ilqr_amd.chain import COUPLED6_RPY, RBD_TARGET_JOINTS_6DOF
    ch = gen6.chain
    assert ch.n == 6 and gen6.nu == 6 and tuple(gen6.target) == RBD_TARGET_JOINTS_6DOF
    assert (gen6.q_weight == 100.0).all() and (gen6.r_weight == 10.0).all() and (gen6.qf_weight == 1e6).all()
    assert np.array_equal(ch.gravity, [0.0, 0.0, -9.81])
    assert len(set(COUPLED6_RPY)) == 6
    assert all(sum(v != 0.0 for v in r) >= 2 for r in COUPLED6_RPY[1:]) and any(COUPLED6_RPY[0])
    dominant = []
    for i in range(6):
        assert np.array_equal(ch.R0[i], rpy_matrix(COUPLED6_RPY[i]))
        assert np.abs(ch.R0[i] - ch.R0[i].T).max() > 0.1                    # R0ᵀ ≠ R0
        assert np.abs(ch.R0[i] @ ch.R0[i].T - np.eye(3)).max() < 1e-15
        assert np.abs(ch.p[i]).min() >= 0.05 and np.abs(ch.com[i]).min() >= 0.03
        assert np.abs(ch.axis[i]).min() > 0.15 and abs(np.linalg.norm(ch.axis[i]) - 1.0) < 1e-15
        dominant.append(int(np.abs(ch.axis[i]).argmax()))
        assert np.array_equal(ch.Ic[i], ch.Ic[i].T)
        w = np.linalg.eigvalsh(ch.Ic[i])
        assert w[0] > 0 and np.diff(w).min() > 0.1 * w[0]                    # SPD, distinct moments
        assert w[0] + w[1] > w[2]                                            # a physical body's
        assert min(abs(ch.Ic[i][0, 1]), abs(ch.Ic[i][0, 2]), abs(ch.Ic[i][1, 2])) > 1e-3
    assert set(dominant) == {0, 1, 2} and all(a != b for a, b in zip(dominant, dominant[1:]))
    assert len(set(ch.mass.tolist())) == 6

    rng = np.random.default_rng(7)
    X = np.concatenate([rng.uniform(-2, 2, (24, 6)), rng.uniform(-1, 1, (24, 6))], axis=1)
    U = rng.uniform(-5, 5, (24, 6))
    base = RBD.ChainModel(ch, 0.01).step(X, U)
    p0 = ch.p.copy()
    p0[:, 1:] = 0.0
    ax = ch.axis.copy()
    ax[:, 0] = 0.0
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    edits = {"COMs zeroed": dict(com=np.zeros((6, 3))),
             "products of inertia dropped": dict(Ic=np.array([np.diag(np.diag(I)) for I in ch.Ic])),
             "isotropic inertias": dict(Ic=np.array([np.eye(3) * np.trace(I) / 3.0 for I in ch.Ic])),
             "R0 transposed": dict(R0=np.array([R.T for R in ch.R0])),
             "p's y and z zeroed": dict(p=p0),
             "p's y and z swapped": dict(p=ch.p[:, [0, 2, 1]].copy()),
             "axes' x component removed": dict(axis=ax)}
    for what, kw in edits.items():
        moved = RBD.ChainModel(dataclasses.replace(ch, **kw), 0.01).step(X, U)
        r = np.abs(moved - base).max() / np.abs(base).max()
        print(f"{what}: one RK4 step moves by {r:.2e} (relative)")
        assert r > 1e-3, (what, r)


def test_coupled_six_mass_matrix_independent_formulation(gen6):
    m = RBD.ChainModel(gen6.chain)
    rng = np.random.default_rng(1)
    for _ in range(5):
        q = rng.uniform(-3, 3, 6)
        M = m.mass_matrix_np(q)
        Mj = RBD.mass_matrix_jacobian(gen6.chain, q)
        assert np.abs(M - Mj).max() < 1e-12 * np.abs(Mj).max()
        assert np.abs(M - M.T).max() < 1e-12 * np.abs(M).max()
        assert np.linalg.eigvalsh(M).min() > 0


def test_coupled_six_rnea_inverts_forward_dynamics(gen6):
    m = RBD.ChainModel(gen6.chain)
    rng = np.random.default_rng(2)
    q, qd, tau = rng.uniform(-2, 2, 6), rng.uniform(-1, 1, 6), rng.uniform(-3, 3, 6)
    qdd = np.linalg.solve(m.mass_matrix_np(q), tau - m.bias_np(q, qd))
    back = m.rnea([np.array([v]) for v in q], [np.array([v]) for v in qd], [np.array([v]) for v in qdd])
    assert np.abs(np.array([v[0] for v in back]) - tau).max() < 1e-12


def test_coupled_six_energy_conservation():
    from ilqr_amd.chain import coupled_6dof_problem
    m = RBD.ChainModel(coupled_6dof_problem(gravity=False).chain)
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 6)])[None]
    u = np.zeros((1, 6))
    ke = lambda x: 0.5 * x[0, 6:] @ m.mass_matrix_np(x[0, :6]) @ x[0, 6:]
    e0 = ke(x)
    for _ in range(100):
        x = m.step(x, u)
    assert abs(ke(x) - e0) < 1e-8 * e0


def test_coupled_six_point_kinematics(gen6):
    """oracle.cost_functions.point_position (the recursion tip to root, what the task
    fixtures differentiate) against rbd.world_frames (root to tip, o + R·point)."""
    from oracle import cost_functions as OC
    rng = np.random.default_rng(5)
    worst = 0.0
    for q in rng.uniform(-3, 3, (6, 6)):
        fr = RBD.world_frames(gen6.chain, q)
        for body, pt in ((5, [0.05, 0.02, 0.1]), (2, [0.3, -0.2, 0.15]), (0, [-0.1, 0.25, 0.2])):
            o, _, R = fr[body]
            got = np.array(OC.point_position(gen6.chain, body, pt, [float(v) for v in q]), float)
            worst = max(worst, np.abs(got - (o + R @ np.array(pt))).max())
    print(f"point kinematics: max abs difference {worst:.2e}")
    assert worst < 1e-14


def test_coupled_six_c_restatement(gen6):
    """The C restatement on the general chain: one RK4 step at the tolerance of
    test_c_chain_dynamics_matches_numpy_oracle, and one cold iteration (central differences
    against exact Jacobians) at test_c_chain_iteration_matches_numpy_oracle's."""
    from oracle import cref
    from oracle import ilqr_oracle as O
    pr = gen6
    model = RBD.ChainModel(pr.chain, pr.dt)
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.5, 1.5, (40, 12))
    U = rng.uniform(-2.0, 2.0, (40, 6))
    ref = model.step(X, U)
    out = cref.chain_dynamics(pr, X, U)
    assert np.abs(out - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    cost = RBD.ChainCost(pr.target, pr.q_weight, pr.r_weight, pr.qf_weight)
    f, l, lf = RBD.chain_closures(model, cost)
    T = 8
    u = np.zeros((1, T, 6))
    x = np.zeros((1, T + 1, 12))
    x[:, 0] = rbd_initial_states(1, 6, seed0=81)
    for t in range(T):
        x[:, t + 1] = model.step(x[:, t], u[:, t])
    d, K, xn, un, c, tr = cref.chain_iterate(pr, x, u)
    assert (tr == 1).all()
    do, Ko = O.backward_pass(x[0], u[0], f, l, lf, symmetrize=True)
    assert np.abs(K[0] - Ko).max() <= 1e-6 * np.abs(Ko).max()
    assert np.abs(d[0] - do).max() <= 1e-6 * np.abs(do).max()
    xo, uo, co = O.forward_pass(x[0], u[0], np.zeros_like(x[0]), d[0], K[0], np.inf, f, l, lf)
    assert np.abs(xn[0] - xo).max() <= 1e-12 * np.abs(xo).max()
    assert abs(c[0] - co) <= 1e-12 * abs(co)


def test_coupled_six_fixtures_consistent(gen6):
    """The frozen general-chain fixtures against the oracle and the generators' conditions
    (make_golden_chain6.py chain6c, make_golden_chain6_task.py), read back from the files."""
    import json
    from oracle import cost_functions as OC
    z = np.load(os.path.join(GOLD, "chain6c_t24.npz"), allow_pickle=False)
    assert z["x"].shape == (2, 25, 12) and z["u"].shape == (2, 24, 6)
    assert np.array_equal(z["x"][:, 0], rbd_initial_states(2, 6, seed0=81))
    assert json.loads(str(z["meta"]))["robot"] == "coupled_6dof"
    model = RBD.ChainModel(gen6.chain, gen6.dt)
    A, B = model.linearize(z["x"][:, 5], z["u"][:, 5])
    assert np.allclose(A, z["A"][:, 5], rtol=0, atol=1e-14) and np.allclose(B, z["B"][:, 5], rtol=0, atol=1e-14)
    assert np.abs(z["A"][..., 6:, :6]).max() > 0.05
    assert (z["fit_status"] == 1).all() and z["fit_iters"].tolist() == [7, 10]
    c = np.load(os.path.join(GOLD, "chain6c_cases_t24.npz"), allow_pickle=False)
    assert c["ls_trials"].tolist() == [4, 2] and c["ls_scale"].tolist() == [9.0, 2.5]
    assert np.array_equal(c["xt"], 0.1 * z["x"][:, ::-1])
    assert (c["ls_cost"] < 0.99 * c["ls_prev_cost"]).all()
    for name, seed0, body, euclidean in (("chain6ctask_euc_t24", 83, 5, True), ("chain6ctask_ref_t24", 81, 2, False)):
        path = os.path.join(GOLD, name + ".npz")
        assert os.path.getsize(path) < 160 * 1024
        z = np.load(path, allow_pickle=False)
        meta = json.loads(str(z["meta"]))
        s = meta["simple"]
        assert meta["robot"] == "coupled_6dof" and meta["T"] == 24
        assert (s["body"], s["euclidean"]) == (body, euclidean) and all(v != 0.0 for v in s["point"])
        assert np.array_equal(z["x"][:, 0], rbd_initial_states(2, 6, seed0=seed0))
        for b, n in enumerate(z["fit_iters"]):
            du2, tr = z["cond_du2"][b], z["cond_trials"][b]
            r = du2[:n] / meta["tol"]
            assert ((r >= 1.25) | (r <= 1.0 / 1.25)).all(), (name, b, du2[:n])
            assert (tr[:n] == 1).all() and (tr[n:] == 0).all()
            assert du2[n - 1] <= meta["tol"] and (du2[:n - 1] > meta["tol"]).all()
        assert (z["fit_status"] == 1).all()
        assert float(z["cond_gain_spread"]) < 1e-13
        a = (gen6.chain, s["body"], s["point"], s["final_target"], s["weight"])
        l, lf = OC.simple_immediate_cost(*a), OC.simple_final_cost(*a, euclidean=s["euclidean"])
        x, u = z["fw_x"][1], z["fw_u"][1]
        cost = 0.0
        for t in range(u.shape[0]):
            cost += l(list(x[t]), list(u[t]))
        cost += lf(list(x[-1]))
        assert abs(cost - z["fw_cost"][1]) <= 1e-14 * abs(cost), (name, cost, z["fw_cost"][1])


# -- the batched chain oracle (oracle/chain_batch.py) -----------------------------------------
@pytest.mark.parametrize("case", ["coupled2", "chain4_goal_per_trajectory", "chain4_task"])
def test_batched_chain_oracle_matches_per_trajectory_oracle(case):
    """oracle.chain_batch.ChainOracle (Jacobians of all points at once, rollouts by the C
    restatement, the C recursion, closure_fit's search) against the per-trajectory oracle
    (oracle.rbd's closures through oracle.ilqr_oracle) at μ = 0.05, alpha0 = 0.9, shrink = 0.7:
    gains 1e-11, a searched forward pass and a 3-iteration fit with the same trial counts, iterates
    1e-10 — under the joint-space costs, a goal per trajectory and the task-space costs."""
    from ilqr_amd.chain import coupled_2dof_problem, coupled_chain_problem
    from oracle import cost_functions as OC
    from oracle import ilqr_oracle as O
    from oracle import rbd
    from oracle.chain_batch import ChainOracle
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())  # noqa: E731
    pr = coupled_2dof_problem(2) if case == "coupled2" else coupled_chain_problem(4)
    n, nb, T = pr.n_joints, 2, 8
    targets = task = None
    if case == "chain4_goal_per_trajectory":
        targets = np.asarray(pr.target, float) + np.array([[0.0] * n, [0.35, -0.25, 0.3, -0.4]])
    if case == "chain4_task":
        task = dict(body=n - 1, point=[0.05, 0.02, 0.1], final_target=[1.9, 0.9, 1.0], weight=2e3, euclidean=True)
    orc = ChainOracle(pr, T, targets=targets, task=task)
    rng = np.random.default_rng(5)
    x0 = np.concatenate([rng.uniform(-1, 1, (nb, n)), rng.uniform(-0.5, 0.5, (nb, n))], axis=1)
    u = rng.uniform(-0.5, 0.5, (nb, T, pr.nu))
    x = orc.rollout(x0, u)
    (d, K), = orc.backward(x, u, [0.05])
    pc = orc.l(x[:, :T].reshape(-1, 2 * n), u.reshape(-1, pr.nu)).reshape(nb, T).sum(1) + orc.lf(x[:, T])
    fw = orc.forward(x, u, 6.0 * d, K, pc, max_trials=64, alpha0=0.9, shrink=0.7)
    fit = orc.fit(x, u, max_iter=3, tol=-1.0, mu=0.05, alpha0=0.9, shrink=0.7)
    model = rbd.ChainModel(pr.chain, pr.dt)
    for b in range(nb):
        cost = rbd.ChainCost(pr.target if targets is None else targets[b], pr.q_weight, pr.r_weight, pr.qf_weight)
        f, l, lf = rbd.chain_closures(model, cost)
        if task is not None:
            a = (pr.chain, task["body"], task["point"], task["final_target"], task["weight"])
            l, lf = OC.simple_immediate_cost(*a), OC.simple_final_cost(*a, euclidean=True)
        do, Ko = O.backward_pass(x[b], u[b], f, l, lf, mu=0.05, symmetrize=True)
        assert rel(d[b], do) < 1e-11 and rel(K[b], Ko) < 1e-11, (b, rel(d[b], do), rel(K[b], Ko))
        st = {}
        xo, uo, co = O.forward_pass(x[b], u[b], np.zeros_like(x[b]), 6.0 * d[b], K[b], pc[b], f, l, lf, max_trials=64,
                                    alpha0=0.9, shrink=0.7, stats=st)
        assert fw[3][b] == st["trials"] and rel(fw[1][b], uo) < 1e-10 and abs(fw[2][b] - co) < 1e-10 * abs(co), b
        h = []
        xf, uf = O.fit(x[b], u[b], f, l, lf, max_iter=3, tol=-1.0, max_trials=64, history=h, mu=0.05, symmetrize=True,
                       alpha0=0.9, shrink=0.7)
        assert fit["history"]["trials"][:, b].tolist() == [e["trials"] for e in h], b
        assert rel(fit["u"][b], uf) < 1e-10 and rel(fit["x"][b], xf) < 1e-10, b
    assert (fw[3] > 1).any()     # the forward pass did search
