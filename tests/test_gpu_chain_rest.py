"""Joint-velocity weights on the tiles path (4 to 7 joints, fp64) on the MI355X:
ilqr_chain_set_velocity_weights through ChainSolver, the tool-path suite's shapes
(coupled_chain_problem(n), T = 16, B = 5: the last two-trajectory workgroup half empty).

1. against the CPU oracle of tests/chain_rest.py (tests/golden/chain{4,7}c_rest_t16.npz,
   make_golden_chain_rest.py), joint mode, a task reading and a task reading with a path: gains
   under every linearisation, a forward pass (with x_traj in the joint mode), the fit with exact
   iteration and trial counts;
2. five and six joints, whose stage tails differ: a joint-mode forward pass with x_traj and a
   goal per trajectory against the oracle run here;
3. bits: row b of the B = 5 handle is a B = 1 handle; replaced weights are a fresh handle's; a
   cleared handle is one that never had weights (gains: the Hessian tiles are restored);
   joint → task → joint keeps the weights; goal rows and a path before or after the weights;
   all-zero weights against none (values; the forward's outputs as bits);
4. final_cost_quadratization: cost, gradient, Hessian against the oracle, the Hessian exactly
   symmetric, its velocity block exactly diag(2·vf_weight);
5. T = 1, B = 1 in the joint mode with x_traj (the prefetch clamp of the velocity words);
6. create, set weights, fit and destroy three times: the device memory in use stays;
7. refusals, the getter, ChainProblem(v_weight=…) through ilqr_amd.fit;
8. a terminal weight makes the reach end slower than without: the device agrees with the oracle's
   pair of fits.
Tolerances are the task suite's (test_gpu_chain6_task.py), imported."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import chain_path as CP
import chain_rest as CR
import ilqr_amd
from ilqr_amd import _lib
from ilqr_amd.chain import (ChainProblem, ChainSolver, chain_closures, coupled_2dof_problem, coupled_chain_problem,
                            rbd_initial_states)
from test_gpu_chain6_task import COST_TOL, FIT_TOL, QUAD_TOL, TOL, dev, inf, rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64
T, NB = 16, 5
MODES = ("joint", "task", "path")

_loaded, _problem = {}, {}


def fixture(n):
    if n not in _loaded:
        z = np.load(os.path.join(GOLD, f"chain{n}c_rest_t{T}.npz"), allow_pickle=False)
        g = {k: z[k] for k in z.files}
        z = np.load(os.path.join(GOLD, f"chain{n}c_rest_gains_t{T}.npz"), allow_pickle=False)   # m_d, m_K
        g.update({k: z[k] for k in z.files})
        g["meta"] = json.loads(str(g["meta"]))
        _loaded[n] = g
    return _loaded[n]


def problem(n):
    if n not in _problem:
        _problem[n] = coupled_chain_problem(n)
    return _problem[n]


def solver(n, mode, nb=NB, lin="dual", horizon=T, path=None, weights="fixture"):
    """A handle in `mode` as the fixture states it ("fixture": with its weights; None: without)."""
    g = fixture(n) if n in (4, 7) else None
    s = ChainSolver(problem(n), horizon, nb, dtype=F64, linearization=lin)
    if mode != "joint":
        m = g["meta"]["simple"]
        s.set_simple_costs(m["body"], m["point"], m["final_target"], m["weight"], m["euclidean"])
    if mode == "path":
        s.set_task_path(dev(g["path_path"] if path is None else path), g["meta"]["path_weight"])
    if weights == "fixture":
        s.set_velocity_weights(g[f"{mode}_v_weight"], g[f"{mode}_vf_weight"])
    elif weights is not None:
        s.set_velocity_weights(*weights)
    return s


def same(a, b):
    """The same bits (NaN entries of a history included)."""
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def run(s, x, u, x_traj=None, iters=3):
    """Everything the weights reach, as {name: (tensor, batch dimension)}: the gains, a forward pass,
    a fit with its history."""
    nb = x.shape[0]
    d, K, st = s.backward(x, u)
    out = {"d": (d, 0), "K": (K, 0), "bw_status": (st, 0)}
    for k, v in zip(("x", "u", "cost", "trials", "status"), s.forward(x, u, d, K, inf(nb), x_traj=x_traj)):
        out[f"fw_{k}"] = (v, 0)
    r = s.fit(x, u, max_iter=iters, tol=1e-6, x_traj=x_traj, history=True)
    out.update(fit_x=(r.x, 0), fit_u=(r.u, 0), fit_cost=(r.cost, 0), fit_iters=(r.iters, 0), fit_status=(r.status, 0))
    out.update({"hist_" + k: (v, 1) for k, v in r.history.items()})
    return out


def assert_same_run(a, b, what):
    for k, (t, _) in a.items():
        assert same(t, b[k][0]), (what, k)


def xu(n):
    g = fixture(n)
    return dev(g["x"]), dev(g["u"]), dev(g["x_traj"])


# -- 1. against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "analytic", "fd"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 7])
def test_rest_gains_vs_oracle(gpu, n, mode, lin):
    g = fixture(n)
    s = solver(n, mode, lin=lin)
    t = TOL["fd" if lin == "fd" else "dual"]
    d, K, st = s.backward(dev(g["x"]), dev(g["u"]))
    ek, ed = rel(K, g[f"{mode}_K"]), rel(d, g[f"{mode}_d"])
    print(f"rest[{n}, {mode}, {lin}] K {ek:.3e} d {ed:.3e}")
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 7])
def test_rest_forward_fit_vs_oracle(gpu, n, mode):
    g = fixture(n)
    s = solver(n, mode)
    t = TOL["dual"]
    x, u, xt = xu(n)
    xn, un, c, tr, fst = s.forward(x, u, dev(g[f"{mode}_d"]), dev(g[f"{mode}_K"]), inf(NB),
                                   x_traj=xt if mode == "joint" else None)
    ex, eu, ec = rel(xn, g[f"{mode}_fw_x"]), rel(un, g[f"{mode}_fw_u"]), rel(c, g[f"{mode}_fw_cost"])
    print(f"rest[{n}, {mode}] fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert np.array_equal(tr.cpu().numpy(), g[f"{mode}_fw_trials"]) and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"], (ex, eu)
    assert ec < COST_TOL, ec
    r = s.fit(x, u, max_iter=g["meta"][mode]["fit_max_iter"], tol=g["meta"]["tol"], history=True)
    assert r.call_status == _lib.OK
    iters = g[f"{mode}_fit_iters"]
    assert np.array_equal(r.iters.cpu().numpy(), iters), (r.iters, iters)
    assert np.array_equal(r.status.cpu().numpy(), g[f"{mode}_fit_status"])
    ex, eu = rel(r.x, g[f"{mode}_fit_x"]), rel(r.u, g[f"{mode}_fit_u"])
    ec = rel(r.cost, g[f"{mode}_fit_cost"][np.arange(NB), iters - 1])
    print(f"rest[{n}, {mode}] fit x {ex:.3e} u {eu:.3e} cost {ec:.3e} iters {iters.tolist()}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec
    trials = r.history["trials"].cpu().numpy()
    for b, it in enumerate(iters):   # every line search, none left out
        assert trials[:it, b].tolist() == g[f"{mode}_cond_trials"][b, :it].tolist()
    # the fit that stops by convergence (the fixture's tol: every decision on the way holds the margin)
    r = s.fit(x, u, max_iter=g["meta"]["max_iter"], tol=g["meta"][mode]["conv_tol"], history=True)
    assert r.call_status == _lib.OK
    iters = g[f"{mode}_conv_iters"]
    assert np.array_equal(r.iters.cpu().numpy(), iters), (r.iters, iters)
    assert (r.status.cpu().numpy() == _lib.TRAJ_CONVERGED).all() and (g[f"{mode}_conv_status"] == _lib.TRAJ_CONVERGED).all()
    ex, eu, ec = rel(r.x, g[f"{mode}_conv_x"]), rel(r.u, g[f"{mode}_conv_u"]), rel(r.cost, g[f"{mode}_conv_cost"])
    print(f"rest[{n}, {mode}] converging fit x {ex:.3e} u {eu:.3e} cost {ec:.3e} iters {iters.tolist()}")
    assert ex < FIT_TOL and eu < FIT_TOL and ec < COST_TOL, (ex, eu, ec)
    trials = r.history["trials"].cpu().numpy()
    for b, it in enumerate(iters):
        assert trials[:it, b].tolist() == g[f"{mode}_conv_trials"][b, :it].tolist()


# -- 2. five and six joints --------------------------------------------------------------------
def small_case(n, nb, horizon, seed):
    pr = problem(n)
    f = CP.Dynamics(pr)
    rng = np.random.default_rng(seed + n)
    u = rng.uniform(-0.5, 0.5, (nb, horizon, n))
    x = CP.rollout(f, rbd_initial_states(nb, n, seed0=81), u)
    xt = 0.1 * CP.rollout(f, rbd_initial_states(nb, n, seed0=7), rng.uniform(-0.5, 0.5, (nb, horizon, n)))
    goals = np.asarray(pr.target) + rng.uniform(-0.3, 0.3, (nb, n))
    return pr, x, u, xt, goals


def oracle_forward(o, x, u, xt):
    (d, K), = o.backward(x, u, [0.01])
    return (d, K) + tuple(o.forward(x, u, d, K, np.full(len(x), np.inf), x_traj=xt))


@pytest.mark.parametrize("n", [5, 6])
def test_rest_five_six_joints_forward_with_x_traj_and_goal_rows(gpu, n):
    pr, x, u, xt, goals = small_case(n, 3, 6, 46)
    vw, vfw = CR.weights(n, *CR.JOINT_W)
    d, K, xo, uo, co, tro, ok = oracle_forward(CR.RestOracle(pr, 6, vw, vfw, targets=goals), x, u, xt)
    assert ok.all() and np.abs(xt[:, :, n:]).max() > 1e-3
    s = ChainSolver(pr, 6, 3, dtype=F64)
    s.set_joint_targets(dev(goals))
    s.set_velocity_weights(vw, vfw)
    dg, Kg, st = s.backward(dev(x), dev(u))
    ek, ed = rel(Kg, K), rel(dg, d)
    xn, un, c, tr, fst = s.forward(dev(x), dev(u), dev(d), dev(K), inf(3), x_traj=dev(xt))
    ex, eu, ec = rel(xn, xo), rel(un, uo), rel(c, co)
    print(f"rest[{n}] rows + x_traj: K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert (st.cpu().numpy() == 0).all() and np.array_equal(tr.cpu().numpy(), tro) and (fst.cpu().numpy() == 0).all()
    assert ek < TOL["dual"]["gain"] and ed < TOL["dual"]["gain"], (ek, ed)
    assert ex < TOL["dual"]["fw"] and eu < TOL["dual"]["fw"] and ec < COST_TOL, (ex, eu, ec)
    # x_traj's velocity rows are read: without them the cost is another
    c0 = s.forward(dev(x), dev(u), dev(d), dev(K), inf(3))[2]
    assert rel(c0, co) > 1e-6


# -- 3. bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 7])
def test_rest_rows_equal_single_trajectory_handles(gpu, n, mode):
    g = fixture(n)
    x, u, xt = xu(n)
    xt = xt if mode == "joint" else None
    got = run(solver(n, mode, lin="analytic"), x, u, xt)
    costs = []
    for b in range(NB):
        one = solver(n, mode, nb=1, lin="analytic", path=g["path_path"][b:b + 1])
        want = run(one, x[b:b + 1].contiguous(), u[b:b + 1].contiguous(), None if xt is None else xt[b:b + 1].contiguous())
        for k, (t, dim) in got.items():
            assert same(t.select(dim, b), want[k][0].select(dim, 0)), (n, mode, k, b)
        costs.append(want["fw_cost"][0][0].item())
        one.close()
    assert len(set(costs)) == NB, costs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 7])
def test_rest_lifecycle(gpu, n, mode):
    g = fixture(n)
    x, u, xt = xu(n)
    xt = xt if mode == "joint" else None
    w = (g[f"{mode}_v_weight"], g[f"{mode}_vf_weight"])
    other = (w[0] * 1.5, w[1] * 0.5)
    never = run(solver(n, mode, weights=None), x, u, xt)
    want, want_other = run(solver(n, mode), x, u, xt), run(solver(n, mode, weights=other), x, u, xt)
    assert not same(want["K"][0], never["K"][0]) and not same(want["K"][0], want_other["K"][0])
    assert not same(want["fw_cost"][0], never["fw_cost"][0])

    s = solver(n, mode, weights=other)
    s.set_velocity_weights(*w)                                        # replaced
    assert_same_run(run(s, x, u, xt), want, "replaced weights")
    s.set_velocity_weights(None, None)                                # cleared: the Hessian tiles are the mode's
    assert s.velocity_weights is None
    assert_same_run(run(s, x, u, xt), never, "cleared weights")
    s.set_velocity_weights(*w)
    # only one of the two: the other is zeros
    s.set_velocity_weights(w[0], None)
    assert_same_run(run(s, x, u, xt), run(solver(n, mode, weights=(w[0], np.zeros(n))), x, u, xt), "v_weight alone")
    s.set_velocity_weights(*w)
    # through another cost mode and back
    if mode == "joint":
        m = g["meta"]["simple"]
        s.set_simple_costs(m["body"], m["point"], m["final_target"], m["weight"], m["euclidean"])
        assert_same_run(run(s, x, u), run(solver(n, "task", weights=w), x, u), "joint → task keeps the weights")
        s.set_joint_costs()
    else:
        s.set_joint_costs()
        assert_same_run(run(s, x, u), run(solver(n, "joint", weights=w), x, u), "task → joint keeps the weights")
        m = g["meta"]["simple"]
        s.set_simple_costs(m["body"], m["point"], m["final_target"], m["weight"], m["euclidean"])
    assert np.array_equal(s.velocity_weights[0], w[0]) and np.array_equal(s.velocity_weights[1], w[1])
    assert_same_run(run(s, x, u, xt), want, "back in the mode")


@pytest.mark.parametrize("n", [4, 7])
def test_rest_goal_rows_and_path_in_either_order(gpu, n):
    g = fixture(n)
    x, u, xt = xu(n)
    w = (g["task_v_weight"], g["task_vf_weight"])
    rng = np.random.default_rng(5 + n)
    jrows = dev(np.asarray(problem(n).target) + rng.uniform(-0.3, 0.3, (NB, n)))
    trows = dev(g["path_path"][:, T] + rng.uniform(-0.02, 0.02, (NB, 3)))
    path = dev(g["path_path"])
    pw = g["meta"]["path_weight"]
    steps = {"joint rows": ("joint", lambda s: s.set_joint_targets(jrows)),
             "task rows": ("task", lambda s: s.set_task_targets(trows)),
             "path": ("task", lambda s: s.set_task_path(path, pw))}
    plain = {}
    for what, (mode, put) in steps.items():
        runs = []
        for order in ("weights first", "weights last"):
            s = solver(n, mode, weights=w if order == "weights first" else None)
            put(s)
            if order == "weights last":
                s.set_velocity_weights(*w)
            runs.append(run(s, x, u, xt if mode == "joint" else None))
        assert_same_run(runs[0], runs[1], what)
        s = solver(n, mode, weights=None)
        put(s)
        plain[what] = run(s, x, u, xt if mode == "joint" else None)
        assert not same(runs[0]["K"][0], plain[what]["K"][0]), what          # … and both are read (a goal: d, not K)
        assert not same(runs[0]["d"][0], run(solver(n, mode, weights=w), x, u, xt if mode == "joint" else None)["d"][0]), what


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 7])
def test_rest_zero_weights_equal_no_weights(gpu, n, mode):
    """2·0·q̇ is −0.0 where q̇ < 0 and may surface as a signed zero in the tiles and the gains:
    those are compared as values; the forward's x̄, ū, cost and trial counts as bits."""
    x, u, xt = xu(n)
    xt = xt if mode == "joint" else None
    a = run(solver(n, mode, weights=(np.zeros(n), np.zeros(n))), x, u, xt)
    b = run(solver(n, mode, weights=None), x, u, xt)
    for k, (t, _) in a.items():
        assert torch.equal(t, b[k][0]) or (t.is_floating_point() and same(t, b[k][0])), k   # NaN history entries: bits
    # the forward pass on the same gains
    d, K = b["d"][0], b["K"][0]
    fa = solver(n, mode, weights=(0.0, 0.0)).forward(x, u, d, K, inf(NB), x_traj=xt)
    fb = solver(n, mode, weights=None).forward(x, u, d, K, inf(NB), x_traj=xt)
    for p, q in zip(fa, fb):
        assert same(p, q)


# -- 4. the quadratization -----------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 7])
def test_rest_final_cost_quadratization(gpu, n, mode):
    g = fixture(n)
    pr = problem(n)
    vw, vfw = g[f"{mode}_v_weight"], g[f"{mode}_vf_weight"]
    s = solver(n, mode)
    # states away from the goal (test_gpu_chain_path.py's reasoning), the rollout's own velocities
    xN = rbd_initial_states(NB, n, seed0=200)
    xN[:, n:] = g["x"][:, -1, n:]
    if mode == "path":
        o = CR.RestPathCost(pr.chain, n - 1, CP.POINT, CP.WEIGHT, g["meta"]["path_weight"], True, vw, vfw)
        rows = g["path_path"][:, T]
        q, (qv, Q) = o.finals(xN, rows), o.fquad(xN, rows)
    else:
        o = CR.RestOracle(pr, T, vw, vfw, **({"task": g["meta"]["simple"]} if mode == "task" else {}))
        q, (qv, Q) = o.lf(xN), o.fquad(xN)
    cost, grad, hess = s.final_cost_quadratization(dev(xN))
    e = rel(cost, q), rel(grad, qv), rel(hess, Q)
    print(f"rest[{n}, {mode}] quadratize: cost {e[0]:.3e} grad {e[1]:.3e} hess {e[2]:.3e}")
    assert max(e) < QUAD_TOL, e
    H = hess.cpu().numpy()
    assert np.array_equal(H, H.transpose(0, 2, 1))
    for b in range(NB):
        assert np.array_equal(H[b, n:, n:], np.diag(2 * vfw))
        assert not H[b, :n, n:].any() and not H[b, n:, :n].any()
    assert np.array_equal(grad.cpu().numpy()[:, n:], 2 * vfw * xN[:, n:])
    s.set_velocity_weights(None, None)
    _, grad0, hess0 = s.final_cost_quadratization(dev(xN))
    assert not hess0[:, n:].any() and not hess0[:, :, n:].any() and not grad0[:, n:].any()


# -- 5. one step, one trajectory -------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_rest_one_step_one_trajectory(gpu, n):
    """T = 1: the prefetch of step t + 1's velocity words is clamped to the only row there is."""
    pr, x, u, xt, _ = small_case(n, 1, 1, 46)
    vw, vfw = CR.weights(n, *CR.JOINT_W)
    d, K, xo, uo, co, tro, ok = oracle_forward(CR.RestOracle(pr, 1, vw, vfw), x, u, xt)
    assert ok.all()
    s = ChainSolver(pr, 1, 1, dtype=F64)
    s.set_velocity_weights(vw, vfw)
    dg, Kg, st = s.backward(dev(x), dev(u))
    ek, ed = rel(Kg, K), rel(dg, d)
    xn, un, c, tr, fst = s.forward(dev(x), dev(u), dev(d), dev(K), inf(1), x_traj=dev(xt))
    ex, eu, ec = rel(xn, xo), rel(un, uo), rel(c, co)
    print(f"rest T=1 [{n}] K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert st.item() == 0 and tr.item() == int(tro[0]) and fst.item() == 0
    assert ek < TOL["dual"]["gain"] and ed < TOL["dual"]["gain"], (ek, ed)
    assert ex < TOL["dual"]["fw"] and eu < TOL["dual"]["fw"] and ec < COST_TOL, (ex, eu, ec)


# -- 6. lifetime -------------------------------------------------------------------------------
def test_rest_handles_give_their_memory_back(gpu):
    """Create, set weights, fit, destroy — three times after a first round that loads what the
    runtime loads once. The device memory in use may end above where it started by no more than
    2 MiB, the runtime's sub-allocator chunk. The bound is deliberately not zero: it is
    test_gpu_handle_lifetime.py's criterion for "returns to where it was", since the runtime may
    keep a chunk of its own; a handle's buffers at this shape are well above it."""
    n = 7
    x, u, xt = xu(n)

    def round_():
        s = solver(n, "joint")
        r = s.fit(x, u, max_iter=2, tol=1e-6, x_traj=xt)
        assert r.call_status == _lib.OK
        s.close()
        torch.cuda.synchronize()

    round_()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        round_()
    free1, _ = torch.cuda.mem_get_info()
    print(f"rest lifetime: in use +{free0 - free1} B after three rounds")
    assert free0 - free1 <= 2 << 20, (free0, free1)


# -- 7. setter, getter, ChainProblem -----------------------------------------------------------
def test_rest_refusals_and_getter(gpu):
    lib = _lib.load()
    one = (C.c_double * 8)(*[1.0] * 8)

    def refused(s):
        for a, b in ((one, one), (one, None), (None, None)):
            assert lib.ilqr_chain_set_velocity_weights(s.h, a, b) == _lib.ERR_UNSUPPORTED
            msg = lib.ilqr_chain_last_error().decode()
            assert "ilqr_chain_set_velocity_weights" in msg and "tiles path" in msg, msg
        assert lib.ilqr_chain_get_velocity_weights(s.h, None, None) == 0 and s.velocity_weights is None
        with pytest.raises(_lib.IlqrError) as e:
            s.set_velocity_weights(1.0, 2.0)
        assert e.value.status == _lib.ERR_UNSUPPORTED

    refused(ChainSolver(coupled_2dof_problem(2), T, 2, dtype=F64))
    refused(ChainSolver(coupled_2dof_problem(2), T, 2, dtype=torch.float32))
    for n in (4, 7):
        refused(ChainSolver(problem(n), T, 2, dtype=torch.float32))
    assert lib.ilqr_chain_set_velocity_weights(None, one, one) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_get_velocity_weights(None, None, None) == -1
    # a ChainProblem with weights on a 2-joint chain: the library's refusal, with its message
    p2 = coupled_2dof_problem(2)
    with pytest.raises(_lib.IlqrError) as e:
        ChainSolver(ChainProblem(p2.chain, 2, p2.dt, p2.target, p2.q_weight, p2.r_weight, p2.qf_weight, v_weight=1.0), T, 2)
    assert e.value.status == _lib.ERR_UNSUPPORTED and "tiles path" in str(e.value)

    n = 4
    g = fixture(n)
    x, u, xt = xu(n)
    w = (g["joint_v_weight"], g["joint_vf_weight"])
    s = solver(n, "joint", weights=None)
    assert s.velocity_weights is None
    bad = w[0].copy()
    for v in (float("nan"), float("inf"), -float("inf")):
        bad[2] = v
        for args in ((bad, w[1]), (w[0], bad), (bad, None)):
            with pytest.raises(_lib.IlqrError) as e:
                s.set_velocity_weights(*args)
            assert e.value.status == _lib.ERR_BAD_ARG
    assert s.velocity_weights is None
    with pytest.raises(ValueError):
        s.set_velocity_weights(np.ones(n + 1), None)
    s.set_velocity_weights(*w)
    before = run(s, x, u, xt)
    with pytest.raises(_lib.IlqrError):
        s.set_velocity_weights(bad, w[1])
    got = s.velocity_weights
    assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])
    assert_same_run(run(s, x, u, xt), before, "a refused call changes nothing")
    # the getter: whichever output is given, scalars broadcast, zeros for a missing vector or when cleared
    v = (C.c_double * n)()
    assert lib.ilqr_chain_get_velocity_weights(s.h, None, v) == 1 and np.array_equal(np.array(v[:]), w[1])
    assert lib.ilqr_chain_get_velocity_weights(s.h, v, None) == 1 and np.array_equal(np.array(v[:]), w[0])
    s.set_velocity_weights(None, 3.0)
    got = s.velocity_weights
    assert np.array_equal(got[0], np.zeros(n)) and np.array_equal(got[1], np.full(n, 3.0))
    s.set_velocity_weights(-1.0, None)                     # negative finite weights are accepted
    assert np.array_equal(s.velocity_weights[0], np.full(n, -1.0))
    s.set_velocity_weights(None, None)
    assert lib.ilqr_chain_get_velocity_weights(s.h, v, None) == 0 and not np.array(v[:]).any()


def test_rest_chain_problem_through_fit(gpu):
    n = 4
    g = fixture(n)
    b = problem(n)
    w = (g["joint_v_weight"], g["joint_vf_weight"])
    pr = ChainProblem(b.chain, b.nu, b.dt, b.target, b.q_weight, b.r_weight, b.qf_weight, v_weight=w[0], vf_weight=w[1])
    s = ChainSolver(pr, T, NB, dtype=F64)
    got = s.velocity_weights
    assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])
    x, u, _ = xu(n)
    want = solver(n, "joint").fit(x, u, max_iter=3, tol=1e-6)
    r = s.fit(x, u, max_iter=3, tol=1e-6)
    assert same(r.x, want.x) and same(r.u, want.u) and same(r.cost, want.cost)
    # the reference API on the problem's closures solves the cost the closures state
    xo, uo = ilqr_amd.fit(g["x"], g["u"], *chain_closures(pr), max_iter=3, tol=1e-6)
    assert np.array_equal(np.asarray(xo), want.x.cpu().numpy()) and np.array_equal(np.asarray(uo), want.u.cpu().numpy())
    xb, ub = ilqr_amd.fit(g["x"], g["u"], *chain_closures(b), max_iter=3, tol=1e-6)
    assert rel(xb, xo) > 1e-3                      # … which is not the problem's without weights
    f, l, lf = chain_closures(pr)
    o = CR.RestOracle(b, T, *w)
    assert np.isclose(l(g["x"][0, 3], g["u"][0, 3]), o.l(g["x"][:1, 3], g["u"][:1, 3])[0], rtol=1e-14)
    assert np.isclose(lf(g["x"][0, T]), o.lf(g["x"][:1, T])[0], rtol=1e-14)
    _, qv, Q = ilqr_amd.final_cost_quadratization(g["x"][0, T], lf)
    gq, HQ = o.fquad(g["x"][:1, T])
    assert np.allclose(np.asarray(qv), gq[0], rtol=1e-14, atol=0) and np.array_equal(np.asarray(Q), HQ[0])
    # cost_functions' simple costs on the problem with weights: their closures state no velocity
    # term, and the fit solves what they state
    from ilqr_amd.chain import ChainDynamics
    from ilqr_amd.cost_functions import simple_final_cost, simple_immediate_cost
    m = g["meta"]["simple"]
    args = (m["body"], m["point"], m["final_target"], m["weight"])
    simple = lambda q: (ChainDynamics(q), simple_immediate_cost(q.chain, *args), simple_final_cost(q.chain, *args))  # noqa: E731
    xs, us = ilqr_amd.fit(g["x"], g["u"], *simple(pr), max_iter=2, tol=1e-6)
    xp, up = ilqr_amd.fit(g["x"], g["u"], *simple(b), max_iter=2, tol=1e-6)
    assert np.array_equal(np.asarray(xs), np.asarray(xp)) and np.array_equal(np.asarray(us), np.asarray(up))
    # a problem without the fields is the problem it was
    assert b.v_weight is None and ChainSolver(b, T, NB, dtype=F64).velocity_weights is None


# -- 8. the reach ends slower ------------------------------------------------------------------
def test_rest_terminal_weight_slows_the_arrival(gpu):
    """Four joints, the task reading, vf = 80 + 14i and v = 0: max |q̇_T| of the fit is below the
    same handle's fit without weights, and the device agrees with the oracle's pair of fits at
    FIT_TOL. Each fit runs for the iterations whose every line-search decision holds the fixture
    generator's margin in the oracle (chain_path.fit's log), so that a decision taken otherwise on
    the device cannot stand behind a difference."""
    n = 4
    g = fixture(n)
    pr = problem(n)
    x, u = g["x"], g["u"]
    vfw = CR.weights(n, *CR.TASK_W)[1]
    s = solver(n, "task", weights=None)
    speed = {}
    for tag, w in (("plain", None), ("rest", (np.zeros(n), vfw))):
        s.set_velocity_weights(*(w or (None, None)))
        o = CR.RestOracle(pr, T, *(w or (np.zeros(n), np.zeros(n))), task=g["meta"]["simple"])
        log, per_iter = [], []
        CP.fit(x, u, o.dyn, CR.no_path(x), CR.Rowless(o), max_iter=6, tol=1e-6, log=log)
        for k, m in log:
            if k == "gains":
                per_iter.append(np.inf)
            else:
                per_iter[-1] = min(per_iter[-1], float(np.nanmin(m)))
        iters = next((i for i, m in enumerate(per_iter) if not m > 1e-9), len(per_iter))
        assert iters >= 2, per_iter
        want = o.fit(x, u, max_iter=iters, tol=1e-6)
        r = s.fit(dev(x), dev(u), max_iter=iters, tol=1e-6)
        ex, eu = rel(r.x, want["x"]), rel(r.u, want["u"])
        speed[tag] = (np.abs(want["x"][:, T, n:]).max(), r.x[:, T, n:].abs().max().item())
        print(f"rest arrival [{tag}] {iters} iterations: x {ex:.3e} u {eu:.3e} max|q̇_T| oracle {speed[tag][0]:.4f} "
              f"device {speed[tag][1]:.4f}")
        assert np.array_equal(r.iters.cpu().numpy(), want["iters"])
        assert ex < FIT_TOL and eu < FIT_TOL, (tag, ex, eu)
    assert speed["rest"][0] < speed["plain"][0] and speed["rest"][1] < speed["plain"][1], speed
