"""A tool path on the tiles path (4 to 7 joints, fp64) on the MI355X: ilqr_chain_set_task_path
through ChainSolver, the targets suite's shapes (coupled_chain_problem(n), n = 4 and 7, T = 16,
B = 5: the last two-trajectory workgroup half empty; the tool point [0.05, 0.02, 0.1] on the
last body, weight = 2e3).

1. against the CPU oracle of tests/chain_path.py (tests/golden/chain{4,7}c_path_t16.npz,
   make_golden_chain_path.py), both task readings: gains under every linearisation, a forward
   pass, the fit with exact iteration and trial counts;
2. bits: row b of the B = 5 handle is a B = 1 handle given path b; a replaced path is a fresh
   handle's; a cleared path is a handle that never had one (lxx restored); task → joint → task
   keeps the path;
3. the path's row T wins over set_task_targets' rows, which return when the path is cleared;
4. final_cost_quadratization pairs state s with path[s, T];
5. a NaN in one trajectory's row ends that trajectory alone;
6. T = 1, B = 1 (the prefetch clamp) against the oracle;
7. create, set a path, fit and destroy three times: the device memory in use stays where it was;
8. refusals.
Tolerances are the task suite's (test_gpu_chain6_task.py), imported; every comparison of 2, 3
and 5 is of bits."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import chain_path as CP
from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver, coupled_2dof_problem, coupled_chain_problem, rbd_initial_states
from test_gpu_chain6_task import COST_TOL, FIT_TOL, QUAD_TOL, TOL, dev, inf, rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64
T, NB = 16, 5
PW = 50.0
FIT_ITERS = 6
GOALS = np.array([[1.9, 0.9, 1.0], [1.5, 1.2, 0.8], [2.1, 0.4, 1.3]])
READINGS = {"euc": True, "ref": False}

_loaded, _problem, _inputs = {}, {}, {}


def fixture(n):
    if n not in _loaded:
        z = np.load(os.path.join(GOLD, f"chain{n}c_path_t{T}.npz"), allow_pickle=False)
        g = {k: z[k] for k in z.files}
        g["meta"] = json.loads(str(g["meta"]))
        _loaded[n] = g
    return _loaded[n]


def problem(n):
    if n not in _problem:
        _problem[n] = coupled_chain_problem(n)
    return _problem[n]


def task_solver(n, euclidean, nb=NB, lin="dual", horizon=T, goal=(9.0, -9.0, 9.0)):
    """A handle in a task mode whose own final_target is nowhere near any path: row T has to arrive."""
    s = ChainSolver(problem(n), horizon, nb, dtype=F64, linearization=lin)
    s.set_simple_costs(n - 1, CP.POINT, [float(v) for v in goal], CP.WEIGHT, euclidean)
    return s


def same(a, b):
    """The same bits (NaN entries of a history included)."""
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def inputs(n):
    """x, u of five trajectories (the fixture's) and paths to go with them: the fixture's two and
    a third, far from both."""
    if n not in _inputs:
        g = fixture(n)
        rng = np.random.default_rng(7 + n)
        s = np.linspace(0.0, 1.0, T + 1)[None, :, None]
        far = g["euc_path"] + 0.03 * s * GOALS[[0, 1, 2, 1, 0]][:, None, :] + 0.002 * rng.standard_normal((NB, T + 1, 3))
        _inputs[n] = (dev(g["x"]), dev(g["u"]), {"a": g["euc_path"], "b": g["ref_path"], "far": far})
    return _inputs[n]


def run(s, x, u):
    """Everything a path reaches, as {name: (tensor, batch dimension)}: the gains, a forward pass, a
    fit with its history."""
    nb = x.shape[0]
    d, K, st = s.backward(x, u)
    out = {"d": (d, 0), "K": (K, 0), "bw_status": (st, 0)}
    for k, v in zip(("x", "u", "cost", "trials", "status"), s.forward(x, u, d, K, inf(nb))):
        out[f"fw_{k}"] = (v, 0)
    r = s.fit(x, u, max_iter=FIT_ITERS, tol=1e-6, history=True)
    out.update(fit_x=(r.x, 0), fit_u=(r.u, 0), fit_cost=(r.cost, 0), fit_iters=(r.iters, 0), fit_status=(r.status, 0))
    out.update({"hist_" + k: (v, 1) for k, v in r.history.items()})
    return out


def assert_same_run(a, b, what):
    for k, (t, _) in a.items():
        assert same(t, b[k][0]), (what, k)


# -- 1. against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "analytic", "fd"])
@pytest.mark.parametrize("tag", ["euc", "ref"])
@pytest.mark.parametrize("n", [4, 7])
def test_path_gains_vs_oracle(gpu, n, tag, lin):
    g = fixture(n)
    s = task_solver(n, READINGS[tag], lin=lin)
    s.set_task_path(dev(g[f"{tag}_path"]), g["meta"]["path_weight"])
    assert s.target_mode == {"path"}
    t = TOL["fd" if lin == "fd" else "dual"]
    d, K, st = s.backward(dev(g["x"]), dev(g["u"]))
    ek, ed = rel(K, g[f"{tag}_K"]), rel(d, g[f"{tag}_d"])
    print(f"path[{n}, {tag}, {lin}] K {ek:.3e} d {ed:.3e}")
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)


@pytest.mark.parametrize("tag", ["euc", "ref"])
@pytest.mark.parametrize("n", [4, 7])
def test_path_forward_fit_vs_oracle(gpu, n, tag):
    g = fixture(n)
    s = task_solver(n, READINGS[tag])
    s.set_task_path(g[f"{tag}_path"], g["meta"]["path_weight"])       # a host array
    t = TOL["dual"]
    x, u = dev(g["x"]), dev(g["u"])
    xn, un, c, tr, fst = s.forward(x, u, dev(g[f"{tag}_d"]), dev(g[f"{tag}_K"]), inf(NB))
    ex, eu, ec = rel(xn, g[f"{tag}_fw_x"]), rel(un, g[f"{tag}_fw_u"]), rel(c, g[f"{tag}_fw_cost"])
    print(f"path[{n}, {tag}] fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert np.array_equal(tr.cpu().numpy(), g[f"{tag}_fw_trials"]) and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"], (ex, eu)
    assert ec < COST_TOL, ec
    r = s.fit(x, u, max_iter=g["meta"]["fit_max_iter"], tol=g["meta"]["tol"], history=True)
    assert r.call_status == _lib.OK
    iters = g[f"{tag}_fit_iters"]
    assert np.array_equal(r.iters.cpu().numpy(), iters), (r.iters, iters)
    assert np.array_equal(r.status.cpu().numpy(), g[f"{tag}_fit_status"])
    ex, eu = rel(r.x, g[f"{tag}_fit_x"]), rel(r.u, g[f"{tag}_fit_u"])
    ec = rel(r.cost, g[f"{tag}_fit_cost"][np.arange(NB), iters - 1])
    print(f"path[{n}, {tag}] fit x {ex:.3e} u {eu:.3e} cost {ec:.3e} iters {iters.tolist()}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec
    trials = r.history["trials"].cpu().numpy()
    for b, it in enumerate(iters):
        assert trials[:it, b].tolist() == g[f"{tag}_cond_trials"][b, :it].tolist()


# -- 2. bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("euclidean", [True, False])
@pytest.mark.parametrize("n", [4, 7])
def test_path_rows_equal_single_trajectory_handles(gpu, n, euclidean):
    x, u, P = inputs(n)
    path = P["far"]
    s = task_solver(n, euclidean, lin="analytic" if euclidean else "fd")
    s.set_task_path(dev(path), PW)
    got = run(s, x, u)
    costs = []
    for b in range(NB):
        one = task_solver(n, euclidean, nb=1, lin="analytic" if euclidean else "fd")
        one.set_task_path(dev(path[b:b + 1]), PW)
        want = run(one, x[b:b + 1].contiguous(), u[b:b + 1].contiguous())
        for k, (t, dim) in got.items():
            assert same(t.select(dim, b), want[k][0].select(dim, 0)), (n, euclidean, k, b)
        costs.append(want["fw_cost"][0][0].item())
        one.close()
    assert len(set(costs)) == NB, costs          # five problems: the comparison is not vacuous


@pytest.mark.parametrize("n", [4, 7])
def test_path_lifecycle(gpu, n):
    x, u, P = inputs(n)
    never = run(task_solver(n, True), x, u)

    def fresh(path, w=PW):
        s = task_solver(n, True)
        s.set_task_path(dev(path), w)
        return run(s, x, u)

    want_a, want_far = fresh(P["a"]), fresh(P["far"])
    assert not same(want_a["K"][0], never["K"][0]) and not same(want_a["K"][0], want_far["K"][0])
    assert not same(fresh(P["a"], 10.0)["K"][0], want_a["K"][0])      # the weight is read

    s = task_solver(n, True)
    assert s.target_mode == frozenset()
    mine = dev(P["a"])
    s.set_task_path(mine, PW)
    mine.zero_()                       # the handle has its copy: the caller's tensor is free
    torch.cuda.synchronize()
    assert s.target_mode == {"path"}
    assert_same_run(run(s, x, u), want_a, "first path, caller's tensor zeroed")
    s.set_task_path(dev(P["far"]), PW)                                 # replaced between fits
    assert_same_run(run(s, x, u), want_far, "replaced path")
    s.set_task_path(dev(P["a"]), 10.0)                                 # … and with another weight
    assert_same_run(run(s, x, u), fresh(P["a"], 10.0), "replaced weight")
    s.set_task_path(None)                                              # cleared: lxx is the mode's again
    assert s.target_mode == frozenset()
    assert_same_run(run(s, x, u), never, "cleared path")
    # task → joint → task with the path kept
    joint = run(ChainSolver(problem(n), T, NB, dtype=F64), x, u)
    s.set_task_path(dev(P["far"]), PW)
    first = run(s, x, u)
    s.set_joint_costs()
    assert s.target_mode == {"path"} and s.cost_mode == "joint"
    assert_same_run(run(s, x, u), joint, "joint mode under a path")    # inert, and lxx the joint mode's
    s.set_simple_costs(n - 1, CP.POINT, [9.0, -9.0, 9.0], CP.WEIGHT, True)
    assert s.target_mode == {"path"}
    assert_same_run(first, want_far, "path before the joint mode")
    assert_same_run(run(s, x, u), want_far, "path after the joint mode")
    # a path set in the joint mode applies from the next task mode on
    t = ChainSolver(problem(n), T, NB, dtype=F64)
    t.set_task_path(dev(P["a"]), PW)
    assert_same_run(run(t, x, u), joint, "a path set in the joint mode")
    t.set_simple_costs(n - 1, CP.POINT, [9.0, -9.0, 9.0], CP.WEIGHT, True)
    assert_same_run(run(t, x, u), want_a, "… then a task mode")
    # shape and dtype are checked as every tensor argument is
    with pytest.raises(AssertionError):
        s.set_task_path(dev(P["a"][:4]), PW)
    with pytest.raises(AssertionError):
        s.set_task_path(dev(P["a"][:, :T]), PW)
    with pytest.raises(TypeError):
        s.set_task_path(dev(P["a"]).float(), PW)
    with pytest.raises(TypeError):
        s.set_task_path(torch.as_tensor(P["a"]), PW)   # a host tensor


# -- 3. the path and the rows of set_task_targets ------------------------------------------
@pytest.mark.parametrize("n", [4, 7])
def test_path_row_T_wins_over_task_targets(gpu, n):
    x, u, P = inputs(n)
    rows = GOALS[[0, 1, 2, 1, 0]]
    only_rows = task_solver(n, True)
    only_rows.set_task_targets(dev(rows))
    want_rows = run(only_rows, x, u)
    only_path = task_solver(n, True)
    only_path.set_task_path(dev(P["a"]), PW)
    want_path = run(only_path, x, u)
    assert not same(want_rows["fw_cost"][0], want_path["fw_cost"][0])
    for order in ("rows first", "path first"):
        s = task_solver(n, True)
        if order == "rows first":
            s.set_task_targets(dev(rows))
            s.set_task_path(dev(P["a"]), PW)
        else:
            s.set_task_path(dev(P["a"]), PW)
            s.set_task_targets(dev(rows))
        assert s.target_mode == {"task", "path"}
        assert_same_run(run(s, x, u), want_path, order)
        s.set_task_path(None)
        assert s.target_mode == {"task"}
        assert_same_run(run(s, x, u), want_rows, order + ", path cleared")


# -- 4. the quadratization -----------------------------------------------------------------
@pytest.mark.parametrize("tag", ["euc", "ref"])
@pytest.mark.parametrize("n", [4, 7])
def test_path_final_cost_quadratization(gpu, n, tag):
    from oracle import cost_functions as OC
    from oracle import ilqr_oracle as O
    g = fixture(n)
    path = g[f"{tag}_path"]
    s = task_solver(n, READINGS[tag])
    s.set_task_path(dev(path), PW)
    # States away from the path's end. The kinematics carry the point to a few ε·|p|, so the
    # error e = π − row, and with it ∇ℓ_f = 2w Σ eₖ∇πₖ, is known to ε·|p| / |e| of its size:
    # QUAD_TOL presumes |e| of the order of |p|, as at the task suite's states. At the fit's own
    # terminal states the tool sits within millimetres of row T of a two-metre arm and three of
    # the sixteen digits are gone before the kernel has rounded anything.
    xN = rbd_initial_states(NB, n, seed0=200)
    xN[:, n:] = g["x"][:, -1, n:]
    cost, grad, hess = s.final_cost_quadratization(dev(xN))
    for b in range(NB):
        lf = OC.simple_final_cost(problem(n).chain, n - 1, CP.POINT, path[b, T].tolist(), CP.WEIGHT, euclidean=READINGS[tag])
        q, qv, Q = (np.asarray(v, float) for v in O.final_cost_quadratization(xN[b], lf))
        e = rel(cost[b], q), rel(grad[b], qv), rel(hess[b], Q)
        print(f"path[{n}, {tag}] quadratize state {b}: cost {e[0]:.3e} grad {e[1]:.3e} hess {e[2]:.3e}")
        assert max(e) < QUAD_TOL, (b, e)
    for m in (4, 6):
        with pytest.raises(_lib.IlqrError) as e:
            s.final_cost_quadratization(torch.zeros((m, 2 * n), dtype=F64, device="cuda"))
        assert e.value.status == _lib.ERR_BAD_DIMS
    s.set_task_path(None)              # … and without a path any n again
    s.final_cost_quadratization(torch.zeros((6, 2 * n), dtype=F64, device="cuda"))
    torch.cuda.synchronize()


# -- 5. isolation ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 7])
def test_path_nan_row_ends_its_trajectory_alone(gpu, n):
    x, u, P = inputs(n)
    path = P["a"].copy()

    def fit(p):
        s = task_solver(n, True)
        s.set_task_path(dev(p), PW)
        return s.fit(x, u, max_iter=FIT_ITERS, tol=1e-6, history=True)

    clean = fit(path)
    path[3, 7, 1] = np.nan
    r = fit(path)
    assert r.call_status == _lib.ERR_NAN
    assert r.status[3].item() == _lib.TRAJ_NAN
    keep = [0, 1, 2, 4]
    assert (r.status[keep] != _lib.TRAJ_NAN).all()
    for a, b in ((r.x, clean.x), (r.u, clean.u), (r.cost, clean.cost), (r.iters, clean.iters), (r.status, clean.status)):
        assert same(a[keep], b[keep])
    for k in r.history:
        assert same(r.history[k][:, keep], clean.history[k][:, keep]), k


# -- 6. one step, one trajectory -------------------------------------------------------------
@pytest.mark.parametrize("euclidean", [True, False])
@pytest.mark.parametrize("n", [4, 7])
def test_path_one_step_one_trajectory(gpu, n, euclidean):
    """T = 1: the prefetch of step t + 1 is clamped to the only row pair there is."""
    pr = problem(n)
    f = CP.Dynamics(pr)
    u = np.random.default_rng(46 + n).uniform(-0.5, 0.5, (1, 1, n))
    x = CP.rollout(f, rbd_initial_states(1, n, seed0=81), u)
    path = CP.smooth_path(pr, x, euclidean, seed=1, amp=0.005)
    cost = CP.PathCost(pr.chain, n - 1, CP.POINT, CP.WEIGHT, PW, euclidean)
    d, K, bst = CP.backward(x, u, path, f, cost)
    xo, uo, co, tro, ok = CP.forward_pass(x, u, np.zeros_like(x), d, K, np.full(1, np.inf), f, path, cost)
    assert (bst == 0).all() and ok.all()
    s = task_solver(n, euclidean, nb=1, horizon=1)
    s.set_task_path(dev(path), PW)
    dg, Kg, st = s.backward(dev(x), dev(u))
    ek, ed = rel(Kg, K), rel(dg, d)
    xn, un, c, tr, fst = s.forward(dev(x), dev(u), dev(d), dev(K), inf(1))
    ex, eu, ec = rel(xn, xo), rel(un, uo), rel(c, co)
    print(f"path T=1 [{n}, {euclidean}] K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert st.item() == 0 and tr.item() == int(tro[0]) and fst.item() == 0
    assert ek < TOL["dual"]["gain"] and ed < TOL["dual"]["gain"], (ek, ed)
    assert ex < TOL["dual"]["fw"] and eu < TOL["dual"]["fw"] and ec < COST_TOL, (ex, eu, ec)


# -- 7. lifetime -------------------------------------------------------------------------------
def test_path_handles_give_their_memory_back(gpu):
    """Create, set a path, fit, destroy — three times after a first round that loads what the
    runtime loads once. The device memory in use may end above where it started by no more than
    2 MiB, the runtime's sub-allocator chunk (test_gpu_handle_lifetime.py's criterion)."""
    n = 7
    x, u, P = inputs(n)
    path = dev(P["a"])

    def round_():
        s = task_solver(n, True)
        s.set_task_path(path, PW)
        r = s.fit(x, u, max_iter=2, tol=1e-6)
        assert r.call_status == _lib.OK
        s.close()
        torch.cuda.synchronize()

    round_()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(3):
        round_()
    free1, _ = torch.cuda.mem_get_info()
    print(f"path lifetime: in use +{free0 - free1} B after three rounds")
    assert free0 - free1 <= 2 << 20, (free0, free1)


# -- 8. refusals -------------------------------------------------------------------------------
def test_path_refusals(gpu):
    lib = _lib.load()

    def refused(s):
        path = torch.zeros((s.batch, T + 1, 3), dtype=F64, device="cuda")
        for p in (C.c_void_p(path.data_ptr()), None):
            assert lib.ilqr_chain_set_task_path(s.h, p, 1.0) == _lib.ERR_UNSUPPORTED
            msg = lib.ilqr_chain_last_error().decode()
            assert "ilqr_chain_set_task_path" in msg and "tiles path" in msg, msg
        assert lib.ilqr_chain_get_target_mode(s.h) == 0

    refused(ChainSolver(coupled_2dof_problem(2), T, 2, dtype=F64))
    refused(ChainSolver(coupled_2dof_problem(2), T, 2, dtype=torch.float32))
    for n in (4, 7):
        refused(ChainSolver(problem(n), T, 2, dtype=torch.float32))
    # a non-finite weight leaves the handle as it was: no path, and a path that is set stays
    n = 4
    x, u, P = inputs(n)
    s = task_solver(n, True)
    for w in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.IlqrError) as e:
            s.set_task_path(dev(P["a"]), w)
        assert e.value.status == _lib.ERR_BAD_ARG
    assert s.target_mode == frozenset()
    s.set_task_path(dev(P["a"]), PW)
    before = run(s, x, u)
    with pytest.raises(_lib.IlqrError):
        s.set_task_path(dev(P["far"]), float("nan"))
    assert s.target_mode == {"path"}
    assert_same_run(run(s, x, u), before, "a refused call changes nothing")
