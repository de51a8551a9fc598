"""cost_functions.jl's task-space costs on the six-joint chain (the 6-DoF arm, fp64) on the
MI355X: ilqr_chain_set_task_costs and ilqr_chain_final_cost_quadratize — the point's
kinematics composed on the device, their analytic first and second derivatives as the
terminal tiles of the wide recursion, and the task cost inside the 32-lane forward group.

Reference: src/cost_functions.jl:5-54 driven by src/backward_pass.jl / src/forward_pass.jl.
Oracle: oracle.cost_functions through oracle.ilqr_oracle (nested forward-mode duals), frozen
in tests/golden/chain6task_*.npz (make_golden_chain6_task.py).
Tolerances (relative to the largest entry): the six-joint suite's own (test_gpu_chain6.py) —
gains 1e-9 (dual) / 1e-6 (central differences), forward 1e-10, fit iterates 1e-8, costs
1e-10 — and 1e-12 for one evaluation of the quadratization."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.chain import ChainDynamics, ChainSolver, rbd_2dof_problem, rbd_6dof_problem, rbd_initial_states

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64
CASES = ["chain6task_euc_t30", "chain6task_ref_t24", "chain6task_b2_t24"]
TOL = {"dual": dict(gain=1e-9, fw=1e-10), "fd": dict(gain=1e-6, fw=1e-6)}
FIT_TOL, COST_TOL, QUAD_TOL = 1e-8, 1e-10, 1e-12


def rel(a, b):
    a = a.double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, float)
    b = b.double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", F64).contiguous()


def inf(nb):
    return torch.full((nb,), float("inf"), dtype=F64, device="cuda")


_loaded = {}


def load(name):
    if name not in _loaded:
        z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        g = {k: z[k] for k in z.files}
        g["meta"] = json.loads(str(g["meta"]))
        _loaded[name] = g
    return _loaded[name]


PR = rbd_6dof_problem(gravity=True)


def set_costs(s, c):
    s.set_simple_costs(c["body"], c["point"], c["final_target"], c["weight"], c["euclidean"])
    assert s.cost_mode == ("simple_euclidean" if c["euclidean"] else "simple")


def solver(g, lin="dual", nb=None):
    n, T = g["u"].shape[:2]
    s = ChainSolver(PR, T, nb or n, dtype=F64, linearization=lin)
    set_costs(s, g["meta"]["simple"])
    return s


# -- 1. the quadratization kernel against nested duals -----------------------------------
def quad_states():
    e, b2 = load("chain6task_euc_t30"), load("chain6task_b2_t24")
    rng = np.random.default_rng(7)
    x = np.concatenate([e["fit_x"][:, -1], b2["fit_x"][:1, -1], np.zeros((1, 12)),
                        np.array([[4.0, -5.0, 7.5, -3.5, 9.0, -8.25, 0.3, -0.2, 0.1, 0.5, -0.4, 0.2]]),
                        np.concatenate([rng.uniform(-2, 2, (3, 6)), rng.uniform(-1, 1, (3, 6))], axis=1)])
    assert x.shape == (8, 12)
    return x


QUAD_COSTS = [dict(body=5, point=[0.05, 0.02, 0.1], final_target=[3.9, 3.5, 1.3], weight=2e3, euclidean=True),
              dict(body=5, point=[0.05, 0.02, 0.1], final_target=[3.9, 3.5, 1.3], weight=2e3, euclidean=False),
              dict(body=2, point=[0.3, -0.2, 0.15], final_target=[1.6, 1.2, 0.8], weight=2e3, euclidean=True),
              dict(body=2, point=[0.3, -0.2, 0.15], final_target=[1.6, 1.2, 0.8], weight=2e3, euclidean=False)]


@pytest.mark.parametrize("k", range(len(QUAD_COSTS)))
def test_final_cost_quadratize_vs_oracle(gpu, k):
    """ilqr_chain_final_cost_quadratize at 8 states (fixture x_N's, q = 0, angles beyond ±π,
    random) against the oracle's final_cost_quadratization of simple_final_cost (nested
    duals): 1e-12 of the largest entry; the Hessian bit-symmetric, its velocity rows and
    columns exactly 0 and, with body = 2, those of joints 3-5 too."""
    from oracle import cost_functions as OC
    from oracle import ilqr_oracle as O
    c = QUAD_COSTS[k]
    x = quad_states()
    lf = OC.simple_final_cost(PR.chain, c["body"], c["point"], c["final_target"], c["weight"],
                              euclidean=c["euclidean"])
    ref = [O.final_cost_quadratization(xi, lf) for xi in x]
    q, qv, Q = (np.array([r[i] for r in ref], dtype=float) for i in range(3))
    s = ChainSolver(PR, 2, 1, dtype=F64)
    set_costs(s, c)
    cost, grad, hess = s.final_cost_quadratization(dev(x))
    torch.cuda.synchronize()
    for i in range(len(x)):
        ec, eg, eh = rel(cost[i], q[i]), rel(grad[i], qv[i]), rel(hess[i], Q[i])
        print(f"quadratize[{k}] state {i}: cost {ec:.3e} grad {eg:.3e} hess {eh:.3e}")
    for i in range(len(x)):
        assert rel(cost[i], q[i]) < QUAD_TOL and rel(grad[i], qv[i]) < QUAD_TOL and rel(hess[i], Q[i]) < QUAD_TOL, i
    assert torch.equal(hess, hess.transpose(1, 2))
    assert bool((hess[:, 6:, :] == 0).all()) and bool((hess[:, :, 6:] == 0).all()) and bool((grad[:, 6:] == 0).all())
    nz = c["body"] + 1
    assert bool((hess[:, nz:6, :] == 0).all()) and bool((hess[:, :, nz:6] == 0).all())
    assert bool((grad[:, nz:6] == 0).all())
    assert float(hess[:, :nz, :nz].abs().min(dim=0).values.max()) > 0   # … and the moved joints' are not
    # outputs are optional
    only = torch.full((len(x),), -1.0, dtype=F64, device="cuda")
    s._bind()
    assert s.lib.ilqr_chain_final_cost_quadratize(s.h, C.c_void_p(dev(x).data_ptr()), len(x),
                                                  C.c_void_p(only.data_ptr()), None, None) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(only, cost)


def test_final_cost_quadratize_joint_mode(gpu):
    """In the joint mode the entry answers the handle's joint-space final cost."""
    x = quad_states()
    s = ChainSolver(PR, 2, 1, dtype=F64)
    cost, grad, hess = s.final_cost_quadratization(dev(x))
    e = PR.target - x[:, :6]
    assert rel(cost, (PR.qf_weight * e * e).sum(1)) < 1e-15
    assert rel(grad[:, :6], -2.0 * PR.qf_weight * e) < 1e-15 and bool((grad[:, 6:] == 0).all())
    Q = np.zeros((12, 12))
    Q[:6, :6] = np.diag(2.0 * PR.qf_weight)
    assert np.array_equal(hess.cpu().numpy(), np.broadcast_to(Q, (len(x), 12, 12)))


# -- 2. known answer ---------------------------------------------------------------------
def test_task_known_answer(gpu):
    """body = −1: the point does not move, so ∇ℓ_f = ∇²ℓ_f = 0 and with ℓ = Σu² the value
    function stays 0: K ≡ 0 exactly and d_t = −2u_t/(2 + μ), μ = 0.01 (H_reg = 2I + μI).
    B = 3, T = 5: the odd batch leaves the last wave half empty."""
    nb, T = 3, 5
    s = ChainSolver(PR, T, nb, dtype=F64)
    s.set_simple_costs(-1, [0.3, 0.2, 0.1], [1.0, 2.0, 3.0], 50.0, True)
    u = dev(np.random.default_rng(46).uniform(-0.5, 0.5, (nb, T, 6)))
    x = s.rollout(dev(rbd_initial_states(nb, 6, seed0=3)), u)
    c, gq, Hq = s.final_cost_quadratization(x[:, -1].contiguous())
    assert bool((gq == 0).all()) and bool((Hq == 0).all())
    assert rel(c, np.full(nb, 50.0 * (0.7 ** 2 + 1.8 ** 2 + 2.9 ** 2))) < 1e-15
    d, K, st = s.backward(x, u)
    assert (st.cpu().numpy() == 0).all()
    assert bool((K == 0).all())
    e = rel(d, -2.0 * u.cpu().numpy() / 2.01)
    print(f"known answer d {e:.3e}")
    assert e < 1e-15, e


# -- 3. fixtures -------------------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
@pytest.mark.parametrize("name", CASES)
def test_task_backward_forward(gpu, name, lin):
    """backward_pass (d, K, statuses 0) and forward_pass with prev_cost = Inf (one trial):
    dual from the fixture's gains, central differences from the device's own."""
    g = load(name)
    t = TOL[lin]
    s = solver(g, lin)
    x, u = dev(g["x"]), dev(g["u"])
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    nb = u.shape[0]
    dd, KK = (dev(g["d"]), dev(g["K"])) if lin == "dual" else (d, K)
    xn, un, c, tr, fst = s.forward(x, u, dd, KK, inf(nb))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"{name}[{lin}] K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e} "
          f"(oracle gain spread {float(g['cond_gain_spread']):.2e})")
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)
    # every lane of a group leaves the same terminal cost: the forward's cost is the sum of the
    # stage costs of its own ū and the quadratization entry's ℓ_f(x̄_N), to rounding
    lf, _, _ = s.final_cost_quadratization(xn[:, -1].contiguous())
    assert rel(c, (un * un).sum((1, 2)) + lf) < 1e-14


@pytest.mark.parametrize("name", CASES)
def test_task_fit(gpu, name):
    """fit: exact iteration counts and statuses, the iterates and the last cost."""
    g = load(name)
    s = solver(g)
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6, history=True)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"{name} fit x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec
    tr = r.history["trials"].cpu().numpy()   # (max_iter, B): the oracle's trial counts
    for b, n in enumerate(g["fit_iters"]):
        assert tr[:n, b].tolist() == g["cond_trials"][b, :n].tolist()


# -- 4. mode switching -------------------------------------------------------------------
def test_task_mode_switching(gpu):
    """task → ILQR_CHAIN_COST_JOINT restores the creation-time tiles: backward and fit on
    chain6g_t30 bit-equal to a fresh handle's. joint → task → task with another target:
    each equal to a fresh handle set once. RNEA / AUTO stay accepted in a task mode."""
    j = np.load(os.path.join(GOLD, "chain6g_t30.npz"), allow_pickle=False)
    g, g2 = load("chain6task_euc_t30"), load("chain6task_ref_t24")
    x, u = dev(j["x"]), dev(j["u"])

    def run(s):
        d, K, st = s.backward(x, u)
        r = s.fit(x, u, max_iter=20, tol=1e-6)
        return d, K, st, r.x, r.u, r.cost, r.iters, r.status

    fresh = ChainSolver(PR, 30, 2, dtype=F64)
    want_joint = run(fresh)
    assert np.array_equal(want_joint[6].cpu().numpy(), j["fit_iters"])
    s = solver(g)
    s.set_dynamics("rnea")
    s.set_dynamics("auto")
    got_task = run(s)
    s.set_joint_costs()
    assert s.cost_mode == "joint"
    for a, b in zip(run(s), want_joint):
        assert torch.equal(a, b)
    set_costs(s, g["meta"]["simple"])
    for a, b in zip(run(s), got_task):
        assert torch.equal(a, b)
    set_costs(s, g2["meta"]["simple"])           # task → task, another mode and weight
    once = ChainSolver(PR, 30, 2, dtype=F64)
    set_costs(once, g2["meta"]["simple"])
    for a, b in zip(run(s), run(once)):
        assert torch.equal(a, b)
    assert not torch.equal(got_task[1], want_joint[1])
    # the old entry restores the joint costs of a six-joint handle too (tiles included)
    assert s.lib.ilqr_chain_set_simple_costs(s.h, _lib.CHAIN_COST_JOINT, 0, None, None, 0.0) == _lib.OK
    assert s.cost_mode == "joint"
    for a, b in zip(run(s), want_joint):
        assert torch.equal(a, b)


# -- 5. batch independence ---------------------------------------------------------------
@pytest.mark.parametrize("nb", [66, 1])
def test_task_batch_independence(gpu, nb):
    """The fixture replicated to B = 66 (33 waves of two trajectories) and B = 1 (half a
    wave) fits to the fixture's iterates and counts."""
    g = load("chain6task_ref_t24")
    idx = np.arange(nb) % g["u"].shape[0] if nb > 1 else np.array([1])
    s = solver(g, nb=nb)
    r = s.fit(dev(g["x"][idx]), dev(g["u"][idx]), max_iter=20, tol=1e-6)
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"][idx])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"][idx])
    ex, eu = rel(r.x, g["fit_x"][idx]), rel(r.u, g["fit_u"][idx])
    print(f"batch {nb} fit x {ex:.3e} u {eu:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    if nb > 1:   # every replica the same bits
        assert torch.equal(r.u[2:], r.u[:-2]) and torch.equal(r.x[2:], r.x[:-2])


# -- 6. ABI edges ------------------------------------------------------------------------
def test_task_abi_edges(gpu):
    lib = _lib.load()
    pt, tg = (C.c_double * 3)(0.05, 0.02, 0.1), (C.c_double * 3)(0.3, 0.5, 0.4)
    nanv = (C.c_double * 3)(0.0, float("nan"), 0.0)
    S, E, J = _lib.CHAIN_COST_SIMPLE, _lib.CHAIN_COST_SIMPLE_EUCLIDEAN, _lib.CHAIN_COST_JOINT
    # 2-joint handles: the same returns as ilqr_chain_set_simple_costs
    for args in [(S, 1, pt, tg, 2e4), (E, 1, pt, tg, 2e4), (S, 2, pt, tg, 1.0), (S, 1, None, tg, 1.0),
                 (7, 1, pt, tg, 1.0), (J, 0, None, None, 0.0)]:
        a, b = ChainSolver(rbd_2dof_problem(2), 4, 2, dtype=F64), ChainSolver(rbd_2dof_problem(2), 4, 2, dtype=F64)
        ra, rb = lib.ilqr_chain_set_task_costs(a.h, *args), lib.ilqr_chain_set_simple_costs(b.h, *args)
        assert ra == rb and a.cost_mode == b.cost_mode, (args, ra, rb)
    a = ChainSolver(rbd_2dof_problem(2), 4, 2, dtype=F64)
    a.set_dynamics("rnea")   # the closed-form requirement is forwarded too
    assert lib.ilqr_chain_set_task_costs(a.h, S, 1, pt, tg, 1.0) == _lib.ERR_UNSUPPORTED
    x2 = torch.zeros((1, 4), dtype=F64, device="cuda")
    assert lib.ilqr_chain_final_cost_quadratize(a.h, C.c_void_p(x2.data_ptr()), 1, None, None,
                                                None) == _lib.ERR_UNSUPPORTED
    # six joints, fp32: does not iterate
    s32 = ChainSolver(PR, 4, 2, dtype=torch.float32)
    assert lib.ilqr_chain_set_task_costs(s32.h, S, 5, pt, tg, 1.0) == _lib.ERR_UNSUPPORTED
    assert s32.cost_mode == "joint"
    assert lib.ilqr_chain_final_cost_quadratize(s32.h, C.c_void_p(x2.data_ptr()), 1, None, None,
                                                None) == _lib.ERR_UNSUPPORTED
    # six joints, fp64
    s = ChainSolver(PR, 4, 2, dtype=F64)
    assert lib.ilqr_chain_set_task_costs(None, S, 5, pt, tg, 1.0) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_set_task_costs(s.h, E, 5, pt, tg, 1.0) == _lib.OK
    assert lib.ilqr_chain_get_cost_mode(s.h) == E
    for args in [(S, 6, pt, tg, 1.0), (S, -2, pt, tg, 1.0), (S, 5, None, tg, 1.0), (S, 5, pt, None, 1.0),
                 (S, 5, nanv, tg, 1.0), (S, 5, pt, tg, float("inf")), (3, 5, pt, tg, 1.0)]:
        assert lib.ilqr_chain_set_task_costs(s.h, *args) == _lib.ERR_BAD_ARG, args
        assert lib.ilqr_chain_get_cost_mode(s.h) == E   # … and the mode is what it was
    assert lib.ilqr_chain_set_task_costs(s.h, S, -1, pt, tg, 1.0) == _lib.OK
    assert lib.ilqr_chain_get_cost_mode(s.h) == S and s.cost_mode == "simple"
    # the old entry on six joints still refuses a task mode, and leaves the mode alone
    assert lib.ilqr_chain_set_simple_costs(s.h, S, 5, pt, tg, 1.0) == _lib.ERR_UNSUPPORTED
    assert lib.ilqr_chain_get_cost_mode(s.h) == S
    assert lib.ilqr_chain_set_dynamics(s.h, _lib.CHAIN_DYN_RNEA) == _lib.OK
    assert lib.ilqr_chain_set_dynamics(s.h, _lib.CHAIN_DYN_CLOSED_FORM) == _lib.ERR_UNSUPPORTED
    assert lib.ilqr_chain_set_task_costs(s.h, J, 0, None, None, 0.0) == _lib.OK
    assert lib.ilqr_chain_get_cost_mode(s.h) == J
    x6 = torch.zeros((1, 12), dtype=F64, device="cuda")
    assert lib.ilqr_chain_final_cost_quadratize(s.h, None, 1, None, None, None) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_final_cost_quadratize(s.h, C.c_void_p(x6.data_ptr()), 0, None, None,
                                                None) == _lib.ERR_BAD_DIMS
    torch.cuda.synchronize()


# -- 7. the rare ends of the line search --------------------------------------------------
@pytest.mark.parametrize("end", ["forward_exhausted", "forward_nan", "iterate_exhausted"])
def test_task_search_ends(gpu, end):
    """An exhausted search and a NaN cost through the task instantiation of the 32-lane
    forward kernels, B = 3, T = 5 (tests/forward_ends.py). Its two x_traj checks are not
    run: ℓ = Σu² ignores x_traj, so a NaN there never reaches the cost."""
    import forward_ends as E
    nb, T = 3, 5
    s = ChainSolver(PR, T, nb, dtype=F64)
    set_costs(s, load("chain6task_euc_t30")["meta"]["simple"])
    u = dev(np.random.default_rng(46).uniform(-0.5, 0.5, (nb, T, 6)))
    x = s.rollout(dev(rbd_initial_states(nb, 6, seed0=3)), u)
    if end.startswith("forward"):
        getattr(E, "check_" + end)(
            lambda x, u, d, K, pc, mt: s.forward(x, u, d, K, pc, options=_lib.default_options(max_trials=mt)), x, u)
    else:
        def iterate(x, u, xn, un, pc, st, nc, du2, tr, xt, o):
            s._bind()
            s.iterate(x, u, xn, un, pc, st, nc, du2=du2, trials=tr, x_traj=xt, options=o)
        E.check_iterate_exhausted(iterate, x, u)


def test_task_x_traj_ignored(gpu):
    """simple_immediate_cost ignores x and x_traj (cost_functions.jl:45-51): the forward with
    an x_traj gives the bits of the forward without."""
    g = load("chain6task_b2_t24")
    s = solver(g)
    x, u, d, K = dev(g["x"]), dev(g["u"]), dev(g["d"]), dev(g["K"])
    a = s.forward(x, u, d, K, inf(2))
    b = s.forward(x, u, d, K, inf(2), x_traj=0.1 * x.flip(1).contiguous())
    for p, q in zip(a, b):
        assert torch.equal(p, q)


# -- 8. the Python mirror -----------------------------------------------------------------
def test_task_api_mirror(gpu):
    """ilqr_amd.fit / backward_pass / forward_pass with ChainDynamics + simple_immediate_cost
    + simple_final_cost on the 6-DoF arm solve on the device; float32 inputs raise the
    fp64 ValueError."""
    import ilqr_amd
    g = load("chain6task_euc_t30")
    c = g["meta"]["simple"]
    a = (PR.chain, c["body"], c["point"], c["final_target"], c["weight"])
    lf = ilqr_amd.simple_final_cost(*a, euclidean=c["euclidean"])
    l = ilqr_amd.simple_immediate_cost(*a)
    dyn = ChainDynamics(PR)
    xo, uo = ilqr_amd.fit(g["x"][0], g["u"][0], dyn, l, lf, max_iter=20, tol=1e-6)
    assert rel(xo, g["fit_x"][0]) < FIT_TOL and rel(uo, g["fit_u"][0]) < FIT_TOL
    d, K = ilqr_amd.backward_pass(g["x"][1], g["u"][1], dyn, l, lf)
    assert rel(K, g["K"][1]) < TOL["dual"]["gain"] and rel(d, g["d"][1]) < TOL["dual"]["gain"]
    xn, un, cost = ilqr_amd.forward_pass(g["x"][1], g["u"][1], None, g["d"][1], g["K"][1], np.inf, dyn, l, lf)
    assert rel(xn, g["fw_x"][1]) < TOL["dual"]["fw"] and rel(cost, g["fw_cost"][1]) < TOL["dual"]["fw"]
    host = sum(l(xn[t], un[t]) for t in range(un.shape[0])) + lf(xn[-1])
    assert abs(cost - host) <= 1e-12 * abs(host)
    x32, u32 = g["x"][0].astype(np.float32), g["u"][0].astype(np.float32)
    with pytest.raises(ValueError, match="fp64"):
        ilqr_amd.fit(x32, u32, dyn, l, lf, max_iter=2, tol=1e-6)
    with pytest.raises(ValueError, match="fp64"):
        ilqr_amd.backward_pass(x32, u32, dyn, l, lf)
