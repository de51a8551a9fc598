"""RBD problem family (ILQR_PROBLEM_CHAIN): the reference's RigidBodyDynamics.jl
example on a fixed-base serial chain, solved by the ilqr_chain_* kernels.

Reference: test/RBD_2_link_example/RBD_helper_functions.jl (dynamicsf :48-79 —
RK4 of v̇ = M \\ (−dynamics_bias + u); immediate_cost :85-99; final_cost
:105-116), animate_RBD_2_link.jl (Δt = 0.01, target_pose, :8-10) and
test/urdf/2Dof_arm.urdf. BASELINE.json config 5 runs the 2-DoF arm with a fixed
base (nx = 4) in fp32; the reference's floating base (16 states, MRP attitude)
is outside the hot path. The costs keep the reference's joint
rows: Q = 10·diag(jo_cost = 10) → q_weight 100, R = diag(jo_tor_cost = 10) →
r_weight 10, final Q = 1e5·diag(10) → qf_weight 1e6, target θ* = (1.0, 0.3).

`ChainSolver` owns one ilqr_chain_handle; tensors are torch CUDA tensors in the
solver's dtype (float32 or float64), laid out as include/ilqr.h documents.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .solver import FitResult, _ptr, _req, alloc_history
from .urdf import Chain, parse_urdf

ROBOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "robots")

# the reference's RBD example (RBD_helper_functions.jl:85-116, animate_RBD_2_link.jl:8-10)
RBD_DT = 0.01
RBD_TARGET_JOINTS = (1.0, 0.3)          # target_pose[7:8]
RBD_Q_JOINT = 10.0 * 10.0               # jo_cost 10, euclidean_penalty * 10.0
RBD_R_JOINT = 10.0 * 1.0                # jo_tor_cost 10, torque_penalty * 1.0
RBD_QF_JOINT = 10.0 * 100000.0          # jo_cost 10, euclidean_penalty * 100000.0


def load_robot(name: str) -> Chain:
    """A chain description shipped with the package ('2dof_arm', '6dof_arm'; made from
    the reference's test/urdf by tools/make_robots.py) or a path to a URDF file: a serial
    chain of 4 to 7 revolute joints, every joint driven, iterates in fp64."""
    if name.endswith(".urdf"):
        return parse_urdf(name)
    with open(os.path.join(ROBOTS, name + ".json")) as f:
        d = json.load(f)
    return Chain(d["names"], np.array(d["R0"]), np.array(d["p"]), np.array(d["axis"]),
                 np.array(d["mass"]), np.array(d["com"]), np.array(d["Ic"]), np.array(d["gravity"]),
                 float(d.get("base_mass", 0.0)), np.array(d.get("base_com", [0.0] * 3), float),
                 np.array(d.get("base_Ic", np.zeros((3, 3)).tolist()), float))


@dataclass
class ChainProblem:
    """A chain plus the joint-space quadratic costs of the reference's RBD example.
    v_weight / vf_weight (optional, scalars or n_joints values): joint-velocity weights,
    ℓ += Σ v_weightᵢ q̇ᵢ² and ℓ_f += Σ vf_weightᵢ q̇ᵢ² (ChainSolver.set_velocity_weights; four to
    seven joints, fp64). They belong to the problem's joint-space cost (ChainCost, ChainFinalCost):
    ilqr_amd.fit with cost_functions' simple costs on this problem solves those closures' cost,
    without them. None, the default, for both: the reference's cost."""
    chain: Chain
    nu: int
    dt: float = RBD_DT
    target: np.ndarray = None
    q_weight: np.ndarray = None
    r_weight: np.ndarray = None
    qf_weight: np.ndarray = None
    v_weight: np.ndarray = None
    vf_weight: np.ndarray = None

    def __post_init__(self):
        n = self.chain.n
        if self.nu not in (n, 1):
            raise ValueError("nu must be n_joints (every joint driven) or 1 (joint 1 only)")
        def vec(v, default):
            return np.full(n, default, float) if v is None else np.broadcast_to(np.asarray(v, float), (n,)).copy()
        self.target = vec(self.target, 0.0)
        self.q_weight = vec(self.q_weight, 1.0)
        self.r_weight = vec(self.r_weight, 1.0)
        self.qf_weight = vec(self.qf_weight, 1.0)
        if self.v_weight is not None or self.vf_weight is not None:
            self.v_weight, self.vf_weight = vec(self.v_weight, 0.0), vec(self.vf_weight, 0.0)

    @property
    def n_joints(self):
        return self.chain.n

    @property
    def nx(self):
        return 2 * self.chain.n

    def struct(self) -> _lib.ChainStruct:
        ch, n = self.chain, self.chain.n
        if n > _lib.CHAIN_MAX_JOINTS:
            raise ValueError(f"at most {_lib.CHAIN_MAX_JOINTS} joints")
        s = _lib.ChainStruct()
        s.n_joints, s.nu, s.dt = n, self.nu, self.dt
        s.gravity[:] = [float(v) for v in ch.gravity]
        for i in range(n):
            s.joint_rot[i][:] = [float(v) for v in ch.R0[i].reshape(-1)]
            s.joint_pos[i][:] = [float(v) for v in ch.p[i]]
            s.axis[i][:] = [float(v) for v in ch.axis[i]]
            s.mass[i] = float(ch.mass[i])
            s.com[i][:] = [float(v) for v in ch.com[i]]
            s.inertia[i][:] = [float(v) for v in ch.Ic[i].reshape(-1)]
            s.target[i] = float(self.target[i])
            s.q_weight[i] = float(self.q_weight[i])
            s.r_weight[i] = float(self.r_weight[i])
            s.qf_weight[i] = float(self.qf_weight[i])
        return s


def rbd_2dof_problem(nu: int = 2) -> ChainProblem:
    """BASELINE config 5: the reference's RBD example on 2Dof_arm.urdf with a fixed base.
    nu = 2 (every joint driven, the reference's u ∈ R^nv convention) or nu = 1 (joint 1
    only, BASELINE's 'nᵤ=1' row; not reference-pinned)."""
    return ChainProblem(load_robot("2dof_arm"), nu, RBD_DT, RBD_TARGET_JOINTS, RBD_Q_JOINT,
                        RBD_R_JOINT, RBD_QF_JOINT)


def coupled_2dof_problem(nu: int = 2, oblique: bool = False) -> ChainProblem:
    """A non-degenerate 2-joint chain for parity tests (not a reference robot): the
    2Dof_arm's joint layout with the first joint frame tilted, COMs off the joint
    origins, anisotropic inertias with products of inertia, and gravity on. Unlike the
    2Dof_arm (COMs on the joint axes, 0.5·I inertias, zero gravity: constant
    M = diag(4, 0.5), zero bias), M(q) is dense and q-dependent and the bias carries
    Coriolis and gravity terms, so A's q-columns are nonzero.

    oblique=True also turns joint 2's frame about z (R0ᵀ ≠ R0), tilts its axis off the
    principal directions and lifts its origin off the x axis: the rotation order of
    R0·[a]×, the R0·a·aᵀ term and the y, z components of p enter (joint 2's frame, axis
    and p_z are those of tests/closures.py coupled_floating_model; p_y is added)."""
    ch = load_robot("2dof_arm")
    c, s = math.cos(0.3), math.sin(0.3)
    R0, p, axis = ch.R0.copy(), ch.p.copy(), ch.axis.copy()
    R0[0] = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])   # joint 1 tilted about x
    if oblique:
        c, s = math.cos(0.2), math.sin(0.2)
        R0[1] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])   # joint 2 turned about z
        axis[1] = np.array([0.0, 1.0, 0.2]) / math.sqrt(1.04)
        p[1] = np.array([1.0, -0.15, 0.1])
    com = np.array([[0.10, 0.05, 0.20], [0.30, 0.05, -0.15]])
    Ic = np.array([[[0.40, 0.02, 0.01], [0.02, 0.60, 0.03], [0.01, 0.03, 0.30]],
                   [[0.20, 0.01, -0.02], [0.01, 0.35, 0.015], [-0.02, 0.015, 0.25]]])
    chain = Chain(list(ch.names), R0, p, axis, np.array([3.0, 2.0]), com, Ic,
                  np.array([0.0, 0.0, -9.81]))
    return ChainProblem(chain, nu, RBD_DT, RBD_TARGET_JOINTS, RBD_Q_JOINT, RBD_R_JOINT, RBD_QF_JOINT)


RBD_TARGET_JOINTS_6DOF = (0.5, -0.4, 0.3, 0.6, -0.2, 0.4)

# coupled_6dof_problem's constants, written out (no RNG): per joint the frame's
# roll-pitch-yaw, its origin, the (unnormalised) axis, the link's mass and COM, and the
# roll-pitch-yaw of the link's principal axes with the moments diag(0.5, 0.35, 0.2)·scale.
COUPLED6_RPY = ((0.3, 0.0, 0.0), (0.0, -0.25, 0.4), (0.2, 0.15, -0.3), (-0.35, 0.1, 0.0),
                (0.0, 0.3, 0.2), (0.25, -0.2, 0.1))
COUPLED6_P = ((0.4, 0.1, 0.15), (0.8, -0.12, 0.08), (0.7, 0.15, -0.1), (0.6, -0.08, 0.2),
              (0.5, 0.2, 0.05), (0.45, -0.05, -0.12))
COUPLED6_AXIS = ((0.2, -0.3, 0.9), (0.25, 0.9, -0.3), (0.9, 0.2, 0.35), (-0.3, 0.25, 0.9),
                 (0.2, -0.9, 0.3), (0.9, -0.35, 0.2))
COUPLED6_MASS = (4.0, 3.4, 2.8, 2.2, 1.6, 1.0)
COUPLED6_COM = ((0.30, 0.05, -0.10), (0.25, -0.08, 0.06), (0.20, 0.10, 0.04), (0.15, -0.05, -0.07),
                (0.10, 0.04, 0.06), (0.08, -0.03, 0.05))
COUPLED6_INERTIA_RPY = ((0.4, -0.3, 0.5), (-0.5, 0.2, 0.3), (0.3, 0.4, -0.6), (0.6, -0.2, -0.4),
                        (-0.3, -0.5, 0.2), (0.2, 0.6, 0.4))
COUPLED6_MOMENTS = (0.5, 0.35, 0.2)
COUPLED6_INERTIA_SCALE = (1.0, 0.85, 0.7, 0.55, 0.4, 0.25)


def coupled_6dof_problem(gravity: bool = True) -> ChainProblem:
    """A six-joint chain without the 6Dof_arm's symmetries, for parity tests (not a
    reference robot): every joint frame rotated (R0 ≠ R0ᵀ), joint origins with x, y and
    z, oblique axes whose dominant component runs over z, y, x along the chain, distinct
    masses, COMs off the origins in all three components, link inertias with three
    distinct principal moments and all products of inertia nonzero; the 6-DoF arm's
    costs and target. Every term of the recursion and of the task kinematics that
    vanishes on the shipped arm (the COM cross products, ω × Iω, the parallel-axis
    shift, R0·[a]× against [a]×·R0, p's y and z) is nonzero here:
    tests/test_chain_oracle.py test_coupled_six_is_not_degenerate holds it to that."""
    from .urdf import rpy_matrix
    R0 = np.array([rpy_matrix(r) for r in COUPLED6_RPY])
    axis = np.array([np.array(a) / math.sqrt(sum(v * v for v in a)) for a in COUPLED6_AXIS])
    Ic = []
    for r, k in zip(COUPLED6_INERTIA_RPY, COUPLED6_INERTIA_SCALE):
        Rp = rpy_matrix(r)
        I = Rp @ np.diag([k * v for v in COUPLED6_MOMENTS]) @ Rp.T
        Ic.append(0.5 * (I + I.T))
    g = np.array([0.0, 0.0, -9.81]) if gravity else np.zeros(3)
    chain = Chain([f"joint_{i + 1}" for i in range(6)], R0, np.array(COUPLED6_P), axis,
                  np.array(COUPLED6_MASS), np.array(COUPLED6_COM), np.array(Ic), g)
    return ChainProblem(chain, 6, RBD_DT, RBD_TARGET_JOINTS_6DOF, RBD_Q_JOINT, RBD_R_JOINT, RBD_QF_JOINT)


# coupled_chain_problem's seventh joint, written out like the six above (no RNG): a rotated
# frame, an oblique axis, an origin with x, y and z, the COM off the origin, three distinct
# principal moments turned off the link's axes (all products of inertia nonzero).
COUPLED7_RPY = (-0.2, 0.25, -0.35)
COUPLED7_P = (0.4, 0.12, 0.09)
COUPLED7_AXIS = (-0.35, 0.3, 0.9)
COUPLED7_MASS = 0.7
COUPLED7_COM = (0.06, 0.04, -0.05)
COUPLED7_INERTIA_RPY = (-0.4, 0.3, -0.5)
COUPLED7_INERTIA_SCALE = 0.15
# RBD_TARGET_JOINTS_6DOF and one more value
RBD_TARGET_JOINTS_7DOF = RBD_TARGET_JOINTS_6DOF + (-0.3,)


def coupled_chain_problem(n_joints: int, gravity: bool = True) -> ChainProblem:
    """coupled_6dof_problem's mechanism with n_joints ∈ {4, 5, 6, 7} joints, every joint
    driven (not a reference robot): the first n joints take its constants, a seventh has
    constants of its own (COUPLED7_*), the targets are RBD_TARGET_JOINTS_7DOF[:n].
    coupled_chain_problem(6) is coupled_6dof_problem() field by field. No symmetry of the
    shipped arms is left at any count: tests/test_chainN_abi.py holds joint 7 to that."""
    from .urdf import rpy_matrix
    if n_joints not in (4, 5, 6, 7):
        raise ValueError("coupled_chain_problem: n_joints must be 4, 5, 6 or 7")
    n = n_joints
    rpy = (COUPLED6_RPY + (COUPLED7_RPY,))[:n]
    p = (COUPLED6_P + (COUPLED7_P,))[:n]
    ax = (COUPLED6_AXIS + (COUPLED7_AXIS,))[:n]
    mass = (COUPLED6_MASS + (COUPLED7_MASS,))[:n]
    com = (COUPLED6_COM + (COUPLED7_COM,))[:n]
    irpy = (COUPLED6_INERTIA_RPY + (COUPLED7_INERTIA_RPY,))[:n]
    iscale = (COUPLED6_INERTIA_SCALE + (COUPLED7_INERTIA_SCALE,))[:n]
    R0 = np.array([rpy_matrix(r) for r in rpy])
    axis = np.array([np.array(a) / math.sqrt(sum(v * v for v in a)) for a in ax])
    Ic = []
    for r, k in zip(irpy, iscale):
        Rp = rpy_matrix(r)
        I = Rp @ np.diag([k * v for v in COUPLED6_MOMENTS]) @ Rp.T
        Ic.append(0.5 * (I + I.T))
    g = np.array([0.0, 0.0, -9.81]) if gravity else np.zeros(3)
    chain = Chain([f"joint_{i + 1}" for i in range(n)], R0, np.array(p), axis, np.array(mass),
                  np.array(com), np.array(Ic), g)
    return ChainProblem(chain, n, RBD_DT, RBD_TARGET_JOINTS_7DOF[:n], RBD_Q_JOINT, RBD_R_JOINT, RBD_QF_JOINT)


def rbd_6dof_problem(gravity: bool = False) -> ChainProblem:
    """The RBD example's joint-space costs on the shipped 6Dof_arm with a fixed base, every
    joint driven (fp64 iteration kernels). The URDF parses with zero gravity, as the
    reference loads it; gravity=True sets (0, 0, −9.81) on a copy of the chain, which
    makes ∂q̈/∂q nonzero from rest."""
    ch = load_robot("6dof_arm")
    if gravity:
        ch = dataclasses.replace(ch, gravity=np.array([0.0, 0.0, -9.81]))
    return ChainProblem(ch, 6, RBD_DT, RBD_TARGET_JOINTS_6DOF, RBD_Q_JOINT, RBD_R_JOINT, RBD_QF_JOINT)


def rbd_initial_states(batch: int, n_joints: int = 2, seed0: int = 0):
    """x₀[b] = [q ~ U(−1, 1)^n, q̇ = 0] from numpy.random.default_rng(seed0 + b)."""
    x0 = np.zeros((batch, 2 * n_joints))
    for b in range(batch):
        x0[b, :n_joints] = np.random.default_rng(seed0 + b).uniform(-1.0, 1.0, n_joints)
    return x0


# linearization names: "dual" (forward-mode duals, the default), "fd" (central differences)
# and "analytic" (the duals' exact Jacobians from δq̈ = M⁻¹(δτ − δ[ID(q, q̇, q̈)]); chains of
# 4 to 7 joints in float64 only, ilqr_chain_create refuses it elsewhere)
_LIN = {"dual": _lib.LINEARIZE_DUAL, "fd": _lib.LINEARIZE_CENTRAL_FD, "analytic": _lib.LINEARIZE_ANALYTIC}


class ChainSolver:
    """Device-resident batched iLQR for one ChainProblem (one ilqr_chain_handle).
    linearization: "dual", "fd" or, for 4 to 7 joints in float64, "analytic" (as exact as
    "dual", its linearisation about twelve times faster at six joints and faster than "fd")."""

    def __init__(self, problem: ChainProblem, T: int, batch: int, dtype=torch.float64,
                 linearization: str = "dual", device: int = 0):
        self.lib = _lib.load()
        self.p = problem
        self.nj, self.nu, self.nx = problem.n_joints, problem.nu, problem.nx
        self.T, self.batch, self.device = T, batch, device
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("dtype must be torch.float32 or torch.float64")
        self.dtype = dtype
        self.dev = torch.device("cuda", device)
        self._s = problem.struct()
        h = C.c_void_p()
        _lib.check(self.lib.ilqr_chain_create(C.byref(h), device, C.byref(self._s), T, batch,
                                              _lib.F32 if dtype == torch.float32 else _lib.F64,
                                              _LIN[linearization]), "ilqr_chain_create")
        self.h = h
        # the iteration kernels of this shape in the solver's dtype (4 to 7 joints: fp64 only)
        self.iterates = bool(self.lib.ilqr_chain_supported_dtype(
            self.nj, self.nu, _lib.F32 if dtype == torch.float32 else _lib.F64))
        if problem.v_weight is not None:   # the problem's velocity weights (the library refuses 2 joints, fp32)
            try:
                self.set_velocity_weights(problem.v_weight, problem.vf_weight)
            except Exception:
                self.close()
                raise

    def set_dynamics(self, mode: str):
        """The iteration kernels' dynamics evaluator (2-joint chains): "auto" (the closed
        form when its creation check passed), "rnea" (the recursive Newton-Euler, the
        restatement of RigidBodyDynamics.jl's calls) or "closed_form". Four to seven joints run
        the recursion: "auto" and "rnea" mean the same, "closed_form" is unsupported."""
        m = {"auto": _lib.CHAIN_DYN_AUTO, "rnea": _lib.CHAIN_DYN_RNEA,
             "closed_form": _lib.CHAIN_DYN_CLOSED_FORM}[mode]
        _lib.check(self.lib.ilqr_chain_set_dynamics(self.h, m), "ilqr_chain_set_dynamics")

    @property
    def dynamics_mode(self) -> str:
        return {_lib.CHAIN_DYN_RNEA: "rnea", _lib.CHAIN_DYN_CLOSED_FORM: "closed_form"}[
            int(self.lib.ilqr_chain_get_dynamics(self.h))]

    @property
    def closed_form_error(self) -> float:
        """Max relative deviation of the closed form from the recursion at creation."""
        return float(self.lib.ilqr_chain_closed_form_error(self.h))

    def set_simple_costs(self, body, point, final_target, weight, euclidean: bool = False):
        """cost_functions.jl's simple_immediate_cost / simple_final_cost in place of the
        problem's joint-space costs (ilqr_chain_set_simple_costs): ℓ = Σ uᵢ² and
        ℓ_f = weight·Σₖ (p_z − final_targetₖ)² for the point `point` of body `body`
        (0-based link index or the name of the joint that moves it; −1 = the base), or
        the squared distance Σₖ (pₖ − final_targetₖ)² with euclidean=True. A 2-joint
        chain samples the point's closed form at this call; four to seven joints (fp64) compose
        the kinematics on the device at every evaluation (ilqr_chain_set_task_costs)."""
        b = body_index(self.p.chain, body)
        pt = (C.c_double * 3)(*[float(v) for v in np.asarray(point, float).reshape(3)])
        tg = (C.c_double * 3)(*[float(v) for v in np.asarray(final_target, float).reshape(3)])
        mode = _lib.CHAIN_COST_SIMPLE_EUCLIDEAN if euclidean else _lib.CHAIN_COST_SIMPLE
        fn, name = self._cost_entry()
        self._bind()   # the new mode's tiles are enqueued on the handle's stream
        _lib.check(fn(self.h, mode, b, pt, tg, float(weight)), name)

    def _cost_entry(self):
        """The cost-mode entry of this handle: the sampled closed form's for the 2-joint
        family, the on-device kinematics' for the rest."""
        if self.lib.ilqr_chain_supported(self.nj, self.nu):
            return self.lib.ilqr_chain_set_simple_costs, "ilqr_chain_set_simple_costs"
        return self.lib.ilqr_chain_set_task_costs, "ilqr_chain_set_task_costs"

    def set_joint_costs(self):
        """Back to the ChainProblem's joint-space costs."""
        fn, name = self._cost_entry()
        self._bind()
        _lib.check(fn(self.h, _lib.CHAIN_COST_JOINT, 0, None, None, 0.0), name)

    clear_simple_costs = set_joint_costs

    def _set_targets(self, fn, name, targets, width):
        if targets is not None:
            if not isinstance(targets, torch.Tensor):   # a host array: uploaded, then copied by the call
                targets = torch.as_tensor(np.ascontiguousarray(targets), device=self.dev)
            _req(targets, torch.float64, (self.batch, width), "targets")
        self._bind()   # the rows are copied on the handle's stream
        _lib.check(fn(self.h, _ptr(targets)), name)

    def set_joint_targets(self, targets):
        """A joint-space goal θ* per trajectory (ilqr_chain_set_joint_targets; four to seven
        joints, fp64): a float64 CUDA tensor, or a host array, of shape (batch, n_joints), row b
        replacing the problem's `target` for trajectory b while the joint-space costs are in
        effect. The handle keeps a copy (the caller's tensor is free when this returns); a
        further call replaces the rows without allocating; None restores the problem's target."""
        self._set_targets(self.lib.ilqr_chain_set_joint_targets, "ilqr_chain_set_joint_targets", targets, self.nj)

    def set_task_targets(self, targets):
        """A task-space goal per trajectory (ilqr_chain_set_task_targets): shape (batch, 3), row
        b replacing set_simple_costs' final_target for trajectory b in either task reading;
        None restores it. Copy semantics as set_joint_targets."""
        self._set_targets(self.lib.ilqr_chain_set_task_targets, "ilqr_chain_set_task_targets", targets, 3)

    def set_task_path(self, path, weight: float = 0.0):
        """A tool path per trajectory (ilqr_chain_set_task_path; four to seven joints, fp64): a
        float64 CUDA tensor, or a host array, of shape (batch, T + 1, 3). While it is set and a
        task reading of set_simple_costs is in effect, step t < T of trajectory b costs
        Σ uᵢ² + weight·Σₖ (πₖ − path[b, t, k])² (π the reading's point: p, or p_z for every k)
        and row T replaces final_target (and set_task_targets' row b) in ℓ_f. x_traj stays
        ignored by the task costs. None clears the path (weight is then not read). Copy
        semantics as set_joint_targets."""
        if path is not None:
            if not isinstance(path, torch.Tensor):
                path = torch.as_tensor(np.ascontiguousarray(path), device=self.dev)
            _req(path, torch.float64, (self.batch, self.T + 1, 3), "path")
        self._bind()   # the rows are copied, and the cleared mode's tiles enqueued, on the handle's stream
        _lib.check(self.lib.ilqr_chain_set_task_path(self.h, _ptr(path), float(weight)), "ilqr_chain_set_task_path")

    def _weights(self, w, name):
        """A scalar or n_joints values as the C array of a weight vector; None stays None."""
        if w is None:
            return None
        a = np.asarray(w, float)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != self.nj):
            raise ValueError(f"{name}: a scalar or {self.nj} values, got shape {a.shape}")
        return (C.c_double * self.nj)(*[float(v) for v in np.broadcast_to(a, (self.nj,))])

    def set_velocity_weights(self, v_weight, vf_weight):
        """Joint-velocity weights (ilqr_chain_set_velocity_weights; four to seven joints, fp64):
        scalars or n_joints values, None for zeros. While set, every cost mode (joint, both task
        readings, a tool path) adds Σ v_weightᵢ q̇ᵢ² to each step's cost and Σ vf_weightᵢ q̇ᵢ² at
        T to the final cost, q̇ᵢ = x[n_joints + i]; in the joint mode the running term is measured
        on x̄ − x_traj like the position term. (None, None) clears them. They survive changes of
        cost mode, goals and path, and own no device memory."""
        v, vf = self._weights(v_weight, "v_weight"), self._weights(vf_weight, "vf_weight")
        self._bind()   # the Hessian tiles are enqueued on the handle's stream
        _lib.check(self.lib.ilqr_chain_set_velocity_weights(self.h, v, vf), "ilqr_chain_set_velocity_weights",
                   last_error=self.lib.ilqr_chain_last_error)   # a refusal (2 joints, fp32) with the library's sentence

    @property
    def velocity_weights(self):
        """(v_weight, vf_weight) as arrays of n_joints values, or None when not set."""
        v, vf = (C.c_double * self.nj)(), (C.c_double * self.nj)()
        if int(self.lib.ilqr_chain_get_velocity_weights(self.h, v, vf)) != 1:
            return None
        return np.array(v[:]), np.array(vf[:])

    @property
    def target_mode(self) -> frozenset:
        """Which goals are per trajectory: a subset of {"joint", "task", "path"}."""
        m = int(self.lib.ilqr_chain_get_target_mode(self.h))
        return frozenset(k for k, bit in (("joint", _lib.CHAIN_TARGETS_JOINT), ("task", _lib.CHAIN_TARGETS_TASK),
                                          ("path", _lib.CHAIN_TARGETS_PATH))
                         if m & bit)

    def final_cost_quadratization(self, x):
        """final_cost_quadratization (backward_pass.jl:134-153) of the cost in effect at the
        states x (n, nx): (ℓ_f (n,), ∇ℓ_f (n, nx), ∇²ℓ_f (n, nx, nx)) on the device
        (ilqr_chain_final_cost_quadratize: four to seven joints, fp64). With goals per
        trajectory of the mode in effect (a tool path's rows T among them), state s is paired
        with goal s and n must be batch."""
        n = x.shape[0]
        _req(x, torch.float64, (n, self.nx), "x")
        cost = self._new(n, dtype=torch.float64)
        grad = self._new(n, self.nx, dtype=torch.float64)
        hess = self._new(n, self.nx, self.nx, dtype=torch.float64)
        self._bind()
        _lib.check(self.lib.ilqr_chain_final_cost_quadratize(self.h, _ptr(x), n, _ptr(cost), _ptr(grad),
                                                             _ptr(hess)),
                   "ilqr_chain_final_cost_quadratize")
        return cost, grad, hess

    @property
    def cost_mode(self) -> str:
        return {_lib.CHAIN_COST_JOINT: "joint", _lib.CHAIN_COST_SIMPLE: "simple",
                _lib.CHAIN_COST_SIMPLE_EUCLIDEAN: "simple_euclidean"}[
            int(self.lib.ilqr_chain_get_cost_mode(self.h))]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ilqr_chain_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bind(self):
        s = torch.cuda.current_stream(self.dev).cuda_stream
        _lib.check(self.lib.ilqr_chain_set_stream(self.h, C.c_void_p(s)), "ilqr_chain_set_stream")

    def _new(self, *shape, dtype=None):
        return torch.empty(shape, dtype=dtype or self.dtype, device=self.dev)

    def _xu(self, x, u):
        B, T = self.batch, self.T
        _req(x, self.dtype, (B, T + 1, self.nx), "x")
        _req(u, self.dtype, (B, T, self.nu), "u")

    # -- primitives ----------------------------------------------------------------------
    def dynamics(self, x, u):
        """dynamicsf for n independent pairs: x (n, nx), u (n, nu) → (n, nx)."""
        n = x.shape[0]
        _req(x, self.dtype, (n, self.nx), "x")
        _req(u, self.dtype, (n, self.nu), "u")
        out = self._new(n, self.nx)
        self._bind()
        _lib.check(self.lib.ilqr_chain_dynamics(self.h, _ptr(x), _ptr(u), _ptr(out), n),
                   "ilqr_chain_dynamics")
        return out

    def rollout(self, x0, u):
        """x (B, T+1, nx) from x0 (B, nx) under u (B, T, nu) (T dynamics launches)."""
        B, T = u.shape[0], u.shape[1]
        x = self._new(B, T + 1, self.nx)
        x[:, 0] = x0
        for t in range(T):
            x[:, t + 1] = self.dynamics(x[:, t].contiguous(), u[:, t].contiguous())
        return x

    def linearize(self, x, u):
        """(A (B,T,nx,nx), B (B,T,nx,nu)) = linearize_dynamics at every (b, t)."""
        self._xu(x, u)
        A = self._new(self.batch, self.T, self.nx, self.nx)
        Bm = self._new(self.batch, self.T, self.nx, self.nu)
        self._bind()
        _lib.check(self.lib.ilqr_chain_linearize(self.h, _ptr(x), _ptr(u), _ptr(A), _ptr(Bm)),
                   "ilqr_chain_linearize")
        return A, Bm

    def backward(self, x, u, options=None):
        """iLQR.backward_pass → (d (B,T,nu), K (B,T,nu,nx), status (B,)); synchronises."""
        self._xu(x, u)
        d = self._new(self.batch, self.T, self.nu)
        K = self._new(self.batch, self.T, self.nu, self.nx)
        st = self._new(self.batch, dtype=torch.int32)
        o = options or _lib.default_options()
        self._bind()
        _lib.check(self.lib.ilqr_chain_backward(self.h, C.byref(o), _ptr(x), _ptr(u), _ptr(d),
                                                _ptr(K), _ptr(st)),
                   "ilqr_chain_backward", allow=(_lib.ERR_NAN,))
        return d, K, st

    def forward(self, x, u, d, K, prev_cost, x_traj=None, options=None):
        """iLQR.forward_pass → (x̄, ū, new_cost, trials, status); synchronises."""
        self._xu(x, u)
        B, T = self.batch, self.T
        _req(d, self.dtype, (B, T, self.nu), "d")
        _req(K, self.dtype, (B, T, self.nu, self.nx), "K")
        _req(prev_cost, self.dtype, (B,), "prev_cost")
        if x_traj is not None:
            _req(x_traj, self.dtype, (B, T + 1, self.nx), "x_traj")
        xn, un = torch.empty_like(x), torch.empty_like(u)
        cost = self._new(B)
        trials = self._new(B, dtype=torch.int32)
        st = self._new(B, dtype=torch.int32)
        o = options or _lib.default_options()
        self._bind()
        _lib.check(self.lib.ilqr_chain_forward(self.h, C.byref(o), _ptr(x), _ptr(u), _ptr(x_traj),
                                               _ptr(d), _ptr(K), _ptr(prev_cost), _ptr(xn),
                                               _ptr(un), _ptr(cost), _ptr(trials), _ptr(st)),
                   "ilqr_chain_forward", allow=(_lib.ERR_NAN, _lib.ERR_LS_EXHAUSTED))
        return xn, un, cost, trials, st

    def iterate(self, x, u, x_new, u_new, prev_cost, status, new_cost, du2=None, trials=None,
                x_traj=None, options=None):
        """One fit iteration (asynchronous): the bench step of config 5."""
        o = options or _lib.default_options()
        _lib.check(self.lib.ilqr_chain_iterate(self.h, C.byref(o), _ptr(x), _ptr(u), _ptr(x_traj),
                                               _ptr(x_new), _ptr(u_new), _ptr(prev_cost),
                                               _ptr(new_cost), _ptr(du2), _ptr(trials),
                                               _ptr(status)), "ilqr_chain_iterate")

    def fit(self, x_init, u_init, max_iter=100, tol=1e-6, x_traj=None, options=None,
            history: bool = False) -> FitResult:
        """iLQR.fit (forward_pass.jl:148-179) for the whole batch; synchronises. history:
        also return the per-iteration record (ilqr_chain_fit_ex; FitResult.history)."""
        self._xu(x_init, u_init)
        B = self.batch
        xo, uo = torch.empty_like(x_init), torch.empty_like(u_init)
        cost = self._new(B)
        iters = self._new(B, dtype=torch.int32)
        st = self._new(B, dtype=torch.int32)
        o = options or _lib.default_options(max_iter=max_iter, tol=tol)
        self._bind()
        hist, hst = alloc_history(o.max_iter, B, x_init.device) if history else (None, None)
        cs = _lib.check(self.lib.ilqr_chain_fit_ex(self.h, C.byref(o), _ptr(x_init), _ptr(u_init),
                                                   _ptr(x_traj), _ptr(xo), _ptr(uo), _ptr(cost),
                                                   _ptr(iters), _ptr(st),
                                                   C.byref(hst) if hst is not None else None),
                        "ilqr_chain_fit", allow=(_lib.ERR_NAN, _lib.ERR_LS_EXHAUSTED))
        return FitResult(xo, uo, cost, iters, st, cs, hist)


# -- reference-API callables (recognised by ilqr_amd.fit & co.) ---------------------------
class ChainDynamics:
    """dynamicsf(x, u) of a ChainProblem, evaluated on the device (one launch)."""

    def __init__(self, problem: ChainProblem):
        self.problem = problem

    def __call__(self, x, u):
        xt = torch.as_tensor(np.asarray(x, float), device="cuda")[None].contiguous()
        ut = torch.as_tensor(np.asarray(u, float), device="cuda")[None].contiguous()
        s = ChainSolver(self.problem, 1, 1, torch.float64)
        try:
            return s.dynamics(xt, ut)[0].cpu().numpy()
        finally:
            s.close()


class ChainCost:
    """immediate_cost(x, u) = Σ q_weightᵢ(θ*ᵢ − θᵢ)² + Σ r_weightₖ uₖ² (+ Σ v_weightᵢ q̇ᵢ² of a
    problem with velocity weights)."""

    def __init__(self, problem: ChainProblem):
        self.problem = problem

    def __call__(self, x, u):
        p = self.problem
        e = p.target - np.asarray(x[: p.n_joints], float)
        c = float(np.sum(p.q_weight * e * e) + np.sum(p.r_weight[: p.nu] * np.asarray(u, float) ** 2))
        if p.v_weight is not None:
            qd = np.asarray(x[p.n_joints: 2 * p.n_joints], float)
            c += float(np.sum(p.v_weight * qd * qd))
        return c


class ChainFinalCost:
    """final_cost(x) = Σ qf_weightᵢ(θ*ᵢ − θᵢ)² (+ Σ vf_weightᵢ q̇ᵢ² of a problem with velocity
    weights)."""

    def __init__(self, problem: ChainProblem):
        self.problem = problem

    def __call__(self, x):
        p = self.problem
        e = p.target - np.asarray(x[: p.n_joints], float)
        c = float(np.sum(p.qf_weight * e * e))
        if p.vf_weight is not None:
            qd = np.asarray(x[p.n_joints: 2 * p.n_joints], float)
            c += float(np.sum(p.vf_weight * qd * qd))
        return c


def chain_closures(problem: ChainProblem):
    """(dynamicsf, immediate_cost, final_cost) of a ChainProblem."""
    return ChainDynamics(problem), ChainCost(problem), ChainFinalCost(problem)


def body_index(chain: Chain, body) -> int:
    """A body of the chain as ilqr_chain_set_simple_costs numbers it: the link joint i
    moves is body i (RigidBodyDynamics' successor of joint i), −1 the fixed base. Takes
    the index or the joint's name."""
    if isinstance(body, str):
        if body not in chain.names:
            raise ValueError(f"no joint named {body!r} (joints: {chain.names})")
        return chain.names.index(body)
    b = int(body)
    if not -1 <= b < chain.n:
        raise ValueError(f"body {b} outside -1..{chain.n - 1}")
    return b


def chain_problem_of(dynamicsf, immediate_cost, final_cost):
    """The ChainProblem behind a recognised closure triple, else None: the problem's own
    joint-space costs, or cost_functions.jl's simple costs on the problem's chain."""
    if not isinstance(dynamicsf, ChainDynamics):
        return None
    p = dynamicsf.problem
    if (isinstance(immediate_cost, ChainCost) and isinstance(final_cost, ChainFinalCost)
            and p is immediate_cost.problem is final_cost.problem):
        return p
    from .cost_functions import simple_costs_of
    if simple_costs_of(p, immediate_cost, final_cost) is not None:
        return p
    return None
