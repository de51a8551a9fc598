"""A goal per trajectory on the tiles path (4 to 7 joints, fp64) on the MI355X:
ilqr_chain_set_joint_targets / ilqr_chain_set_task_targets through ChainSolver, T = 16.

1. against the numpy oracle run on every trajectory alone with its own goal
   (tests/golden/chain{4,7}c_targets_t16.npz, chain{4,7}ctask_targets_t16.npz;
   make_golden_chain_targets.py);
2. against shared-goal handles, bit for bit: row b of a handle with goals [0, 1, 2, 1, 0]
   equals row b of the handle created with goal g(b) for all five trajectories;
3. a uniform override (every row the handle's own goal) is the shared path, bit for bit;
4. lifecycle: clearing, cost-mode switches, the caller's tensor, goals replaced between fits;
5. a NaN row ends its trajectory alone;
6. refusals.
Tolerances are the six-joint suites' (test_gpu_chain6.py, test_gpu_chain6_task.py); every
comparison of 2 to 5 is of bits."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver, coupled_2dof_problem, coupled_chain_problem, rbd_initial_states
from test_gpu_chain6 import COST_TOL, FIT_TOL, TOL, dev, inf, rel
from test_gpu_chain6_task import QUAD_TOL
from test_gpu_chain6_task import TOL as TASK_TOL

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64
T = 16
MODES = ["joint", "simple", "euclidean"]
# the linearisation each mode of 2 and 3 runs under: the goal is independent of it, every one is run
LIN = {"joint": "dual", "simple": "analytic", "euclidean": "fd"}
ROWS = [0, 1, 2, 1, 0]          # B = 5: the last workgroup (two trajectories) half empty
JOINT_OFFSETS = np.array([[0.0] * 7, [0.35, -0.25, 0.3, -0.4, 0.2, -0.3, 0.25], [-0.3, 0.4, -0.2, 0.25, -0.35, 0.2, -0.15]])
TASK_GOALS = np.array([[1.9, 0.9, 1.0], [1.5, 1.2, 0.8], [2.1, 0.4, 1.3]])
FIT_ITERS = 6

_loaded, _problem, _inputs = {}, {}, {}


def load(name):
    if name not in _loaded:
        z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        g = {k: z[k] for k in z.files}
        g["meta"] = json.loads(str(g["meta"]))
        _loaded[name] = g
    return _loaded[name]


def fixture(n, kind):
    return load(f"chain{n}c_targets_t{T}" if kind == "joint" else f"chain{n}ctask_targets_t{T}")


def problem(n):
    if n not in _problem:
        _problem[n] = coupled_chain_problem(n)
    return _problem[n]


def task_costs(n, goal, euclidean):
    return dict(body=n - 1, point=[0.05, 0.02, 0.1], final_target=[float(v) for v in goal], weight=2e3,
                euclidean=euclidean)


def set_costs(s, c):
    s.set_simple_costs(c["body"], c["point"], c["final_target"], c["weight"], c["euclidean"])


def same(a, b):
    """The same bits (NaN entries of a history included)."""
    if a.is_floating_point():
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def inputs(n, nb=5):
    """x, u, x_traj of nb trajectories of the n-joint mechanism: a rollout of small random torques."""
    if (n, nb) not in _inputs:
        s = ChainSolver(problem(n), T, nb, dtype=F64)
        u = dev(np.random.default_rng(46 + n).uniform(-0.5, 0.5, (nb, T, n)))
        x = s.rollout(dev(rbd_initial_states(nb, n, seed0=81)), u)
        s.close()
        _inputs[n, nb] = (x, u, (0.1 * x.flip(1)).contiguous())
    return _inputs[n, nb]


def goals(n, mode):
    return problem(n).target + JOINT_OFFSETS[:, :n] if mode == "joint" else TASK_GOALS


def shared_solver(n, mode, goal, nb=5, lin=None):
    """A handle of the shared-goal path with `goal` for every trajectory."""
    pr = dataclasses.replace(problem(n), target=goal) if mode == "joint" else problem(n)
    s = ChainSolver(pr, T, nb, dtype=F64, linearization=lin or LIN[mode])
    if mode != "joint":
        set_costs(s, task_costs(n, goal, mode == "euclidean"))
    return s


def rows_solver(n, mode, rows, nb=5, lin=None):
    """A handle whose own goal is goals(n, mode)[0] and whose trajectories get `rows`."""
    s = shared_solver(n, mode, goals(n, mode)[0], nb, lin)
    (s.set_joint_targets if mode == "joint" else s.set_task_targets)(dev(rows))
    return s


def run(s, n, nb=5):
    """Everything a goal reaches, as {name: (tensor, batch dimension)}: the gains, a forward pass
    without and one with x_traj, a fit with its history."""
    x, u, xt = inputs(n, nb)
    d, K, st = s.backward(x, u)
    out = {"d": (d, 0), "K": (K, 0), "bw_status": (st, 0)}
    for tag, kw in (("fw", {}), ("fwxt", dict(x_traj=xt))):
        for k, v in zip(("x", "u", "cost", "trials", "status"), s.forward(x, u, d, K, inf(nb), **kw)):
            out[f"{tag}_{k}"] = (v, 0)
    r = s.fit(x, u, max_iter=FIT_ITERS, tol=1e-6, x_traj=xt if s.cost_mode == "joint" else None, history=True)
    out.update(fit_x=(r.x, 0), fit_u=(r.u, 0), fit_cost=(r.cost, 0), fit_iters=(r.iters, 0), fit_status=(r.status, 0))
    out.update({"hist_" + k: (v, 1) for k, v in r.history.items()})
    return out


def assert_rows_equal(got, want, b_got, b_want, what):
    for k, (t, dim) in got.items():
        assert same(t.select(dim, b_got), want[k][0].select(dim, b_want)), (what, k, b_got, b_want)


# -- 1. against the oracle -----------------------------------------------------------------
def oracle_solver(n, kind, lin="dual"):
    g = fixture(n, kind)
    s = ChainSolver(problem(n), T, 3, dtype=F64, linearization=lin)
    if kind == "joint":
        s.set_joint_targets(dev(g["targets"]))
        assert s.target_mode == {"joint"}
    else:
        # the handle's own final_target is none of the rows': every row has to arrive
        set_costs(s, dict(g["meta"]["simple"], final_target=[9.0, -9.0, 9.0]))
        s.set_task_targets(dev(g["targets"]))
        assert s.target_mode == {"task"}
    return g, s


@pytest.mark.parametrize("lin", ["dual", "analytic", "fd"])
@pytest.mark.parametrize("kind", ["joint", "task"])
@pytest.mark.parametrize("n", [4, 7])
def test_targets_gains_vs_oracle(gpu, n, kind, lin):
    """backward_pass of every trajectory against the oracle's with that trajectory's goal: the
    dual tolerance under "dual" and "analytic", the central-difference one under "fd"."""
    g, s = oracle_solver(n, kind, lin)
    t = (TOL if kind == "joint" else TASK_TOL)["fd" if lin == "fd" else "dual"]
    d, K, st = s.backward(dev(g["x"]), dev(g["u"]))
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    print(f"targets[{n}, {kind}, {lin}] K {ek:.3e} d {ed:.3e}")
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)


@pytest.mark.parametrize("kind", ["joint", "task"])
@pytest.mark.parametrize("n", [4, 7])
def test_targets_forward_fit_vs_oracle(gpu, n, kind):
    """The forward pass from the fixture's gains, the fit (iterates at FIT_TOL, exact iteration
    counts, statuses and per-iteration trial counts) and, for the task cost, its quadratization at
    the fixture's terminal states against nested duals with each state's own goal."""
    g, s = oracle_solver(n, kind)
    t = (TOL if kind == "joint" else TASK_TOL)["dual"]
    x, u = dev(g["x"]), dev(g["u"])
    xn, un, c, tr, fst = s.forward(x, u, dev(g["d"]), dev(g["K"]), inf(3))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"targets[{n}, {kind}] fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)
    r = s.fit(x, u, max_iter=20, tol=1e-6, history=True)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    ec = rel(r.cost, g["fit_cost"][np.arange(3), g["fit_iters"] - 1])
    print(f"targets[{n}, {kind}] fit x {ex:.3e} u {eu:.3e} cost {ec:.3e} iters {g['fit_iters'].tolist()}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec
    trials = r.history["trials"].cpu().numpy()
    for b, it in enumerate(g["fit_iters"]):
        assert trials[:it, b].tolist() == g["cond_trials"][b, :it].tolist()
    if kind == "task":
        from oracle import cost_functions as OC
        from oracle import ilqr_oracle as O
        c = g["meta"]["simple"]
        xN = g["fit_x"][:, -1]
        cost, grad, hess = s.final_cost_quadratization(dev(xN))
        for b in range(3):
            lf = OC.simple_final_cost(problem(n).chain, c["body"], c["point"], g["targets"][b].tolist(), c["weight"],
                                      euclidean=c["euclidean"])
            q, qv, Q = (np.asarray(v, float) for v in O.final_cost_quadratization(xN[b], lf))
            e = rel(cost[b], q), rel(grad[b], qv), rel(hess[b], Q)
            print(f"targets[{n}] quadratize state {b}: cost {e[0]:.3e} grad {e[1]:.3e} hess {e[2]:.3e}")
            assert max(e) < QUAD_TOL, (b, e)


# -- 2. against single-goal handles, bit for bit -------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_targets_equal_shared_goal_handles(gpu, n, mode):
    G = goals(n, mode)
    got = run(rows_solver(n, mode, G[ROWS]), n)
    want = [run(shared_solver(n, mode, G[k]), n) for k in range(3)]
    for b, k in enumerate(ROWS):
        assert_rows_equal(got, want[k], b, b, (n, mode))
    # … and the three goals are three problems: the comparison is not vacuous
    costs = [want[k]["fit_cost"][0][0].item() for k in range(3)]
    assert len(set(costs)) == 3, costs
    # (d, not K: the joint-space Hessians, and with them the feedback gains, do not depend on θ*)
    assert not same(want[0]["d"][0], want[1]["d"][0]) and not same(want[1]["fw_cost"][0], want[2]["fw_cost"][0])


# -- 3. a uniform override is the shared path ------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_targets_uniform_is_shared_path(gpu, n, mode):
    g0 = goals(n, mode)[0]
    s = rows_solver(n, mode, np.tile(g0, (5, 1)))
    assert s.target_mode == {"joint" if mode == "joint" else "task"}
    plain = shared_solver(n, mode, g0)
    assert plain.target_mode == frozenset()
    got, want = run(s, n), run(plain, n)
    for k, (t, _) in got.items():
        assert same(t, want[k][0]), (n, mode, k)


# -- 4. lifecycle ------------------------------------------------------------------------------
def assert_same_run(a, b, what):
    for k, (t, _) in a.items():
        assert same(t, b[k][0]), (what, k)


@pytest.mark.parametrize("n", [4, 7])
def test_targets_lifecycle(gpu, n):
    GJ, GT = goals(n, "joint"), goals(n, "euclidean")
    rows_j, rows_t = GJ[ROWS], GT[ROWS]
    fresh_joint = run(shared_solver(n, "joint", GJ[0], lin="dual"), n)
    fresh_task = run(shared_solver(n, "euclidean", GT[0], lin="dual"), n)
    want_j = run(rows_solver(n, "joint", rows_j, lin="dual"), n)
    want_t = run(rows_solver(n, "euclidean", rows_t, lin="dual"), n)
    assert not same(want_j["d"][0], fresh_joint["d"][0]) and not same(want_t["d"][0], fresh_task["d"][0])

    s = shared_solver(n, "joint", GJ[0], lin="dual")
    assert s.target_mode == frozenset()
    mine = dev(rows_j)
    s.set_joint_targets(mine)
    mine.zero_()                       # the handle has its copy: the caller's tensor is free
    torch.cuda.synchronize()
    assert s.target_mode == {"joint"}
    assert_same_run(run(s, n), want_j, "joint rows, caller's tensor zeroed")
    # a task mode neither applies nor drops the joint rows
    set_costs(s, task_costs(n, GT[0], True))
    assert s.target_mode == {"joint"} and s.cost_mode == "simple_euclidean"
    assert_same_run(run(s, n), fresh_task, "task mode under joint rows")
    s.set_task_targets(rows_t)         # a host array
    assert s.target_mode == {"joint", "task"}
    assert_same_run(run(s, n), want_t, "task rows")
    s.set_joint_costs()                # … and back: the joint rows are still there, the task rows idle
    assert s.target_mode == {"joint", "task"} and s.cost_mode == "joint"
    assert_same_run(run(s, n), want_j, "joint rows after a task mode")
    s.set_joint_targets(None)
    assert s.target_mode == {"task"}
    assert_same_run(run(s, n), fresh_joint, "joint rows cleared")
    set_costs(s, task_costs(n, GT[0], True))
    assert_same_run(run(s, n), want_t, "task rows after the joint mode")
    s.set_task_targets(None)
    assert s.target_mode == frozenset()
    assert_same_run(run(s, n), fresh_task, "task rows cleared")
    # new goals before each fit (the MPC use): each fit equals a fresh handle's
    s.set_joint_costs()
    other = GJ[[2, 0, 1, 0, 2]]
    s.set_joint_targets(dev(rows_j))
    first = run(s, n)
    s.set_joint_targets(dev(other))
    second = run(s, n)
    assert_same_run(first, want_j, "first goals")
    assert_same_run(second, run(rows_solver(n, "joint", other, lin="dual"), n), "replaced goals")
    # shape and dtype are checked as every tensor argument is
    with pytest.raises(AssertionError):
        s.set_joint_targets(dev(rows_j[:4]))
    with pytest.raises(AssertionError):
        s.set_task_targets(dev(rows_j))
    with pytest.raises(TypeError):
        s.set_joint_targets(dev(rows_j).float())
    with pytest.raises(ValueError):
        s.set_joint_targets(dev(np.tile(rows_j, (1, 2)))[:, :n])
    with pytest.raises(TypeError):
        s.set_task_targets(torch.as_tensor(rows_t))   # a host tensor


# -- 5. isolation ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["joint", "euclidean"])
@pytest.mark.parametrize("n", [4, 7])
def test_targets_nan_row_ends_its_trajectory_alone(gpu, n, mode):
    rows = goals(n, mode)[ROWS].copy()
    x, u, _ = inputs(n)
    clean = rows_solver(n, mode, rows).fit(x, u, max_iter=FIT_ITERS, tol=1e-6, history=True)
    rows[3, 1] = np.nan
    r = rows_solver(n, mode, rows).fit(x, u, max_iter=FIT_ITERS, tol=1e-6, history=True)
    assert r.call_status == _lib.ERR_NAN
    assert r.status[3].item() == _lib.TRAJ_NAN
    keep = [0, 1, 2, 4]
    assert (r.status[keep] != _lib.TRAJ_NAN).all()
    for a, b in ((r.x, clean.x), (r.u, clean.u), (r.cost, clean.cost), (r.iters, clean.iters), (r.status, clean.status)):
        assert same(a[keep], b[keep])
    for k in r.history:
        assert same(r.history[k][:, keep], clean.history[k][:, keep]), k


# -- 6. refusals -------------------------------------------------------------------------------
def test_targets_refusals(gpu):
    lib = _lib.load()

    def refused(s, width):
        rows = torch.zeros((s.batch, width), dtype=F64, device="cuda")
        for fn in (lib.ilqr_chain_set_joint_targets, lib.ilqr_chain_set_task_targets):
            for p in (C.c_void_p(rows.data_ptr()), None):
                assert fn(s.h, p) == _lib.ERR_UNSUPPORTED
                assert lib.ilqr_chain_last_error().decode()
        assert lib.ilqr_chain_get_target_mode(s.h) == 0

    refused(ChainSolver(coupled_2dof_problem(2), T, 2, dtype=F64), 2)
    refused(ChainSolver(coupled_2dof_problem(2), T, 2, dtype=torch.float32), 2)
    for n in (4, 5, 6, 7):
        refused(ChainSolver(problem(n), T, 2, dtype=torch.float32), n)
    # the quadratization under an override pairs state s with row s: n == batch
    n = 4
    s = rows_solver(n, "euclidean", TASK_GOALS[ROWS])
    x = inputs(n)[0][:, -1].contiguous()
    s.final_cost_quadratization(x)
    for m in (4, 6):
        xm = torch.zeros((m, 2 * n), dtype=F64, device="cuda")
        with pytest.raises(_lib.IlqrError) as e:
            s.final_cost_quadratization(xm)
        assert e.value.status == _lib.ERR_BAD_DIMS
    s.set_joint_costs()                # the task rows idle: the joint final cost at any n
    s.final_cost_quadratization(torch.zeros((6, 2 * n), dtype=F64, device="cuda"))
    s.set_joint_targets(dev(goals(n, "joint")[ROWS]))
    with pytest.raises(_lib.IlqrError) as e:
        s.final_cost_quadratization(torch.zeros((6, 2 * n), dtype=F64, device="cuda"))
    assert e.value.status == _lib.ERR_BAD_DIMS
    cost, grad, _ = s.final_cost_quadratization(x)
    pr = problem(n)
    err = goals(n, "joint")[ROWS] - x[:, :n].cpu().numpy()
    assert rel(cost, (pr.qf_weight * err * err).sum(1)) < 1e-15 and rel(grad[:, :n], -2.0 * pr.qf_weight * err) < 1e-15
    torch.cuda.synchronize()
