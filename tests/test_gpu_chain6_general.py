"""Every six-joint chain kernel on a mechanism with no symmetries
(ilqr_amd.chain.coupled_6dof_problem), on the MI355X.

The shipped 6-DoF arm has R0 = I, COMs on the joint origins, 0.5·I inertias, axes ±y / ±z
and joint origins along x: the COM cross products, ω × Iω, the inertia off-diagonals, the
order of R0·[a]×, the row-or-column reading of R0 and the y, z components of p are zero or
trivially right in every test on it (transposing every R0 of the arm changes one RK4 step
by exactly 0). Here each of them moves a step by ≥ 1e-2 of its largest entry
(tests/test_chain_oracle.py test_coupled_six_is_not_degenerate), ≥ 1e9 × the rollout
tolerance, so a kernel that gets one of them wrong fails at once.

Fixtures: tests/golden/make_golden_chain6.py chain6c (chain6c_t24, chain6c_cases_t24) and
make_golden_chain6_task.py (chain6ctask_euc_t24, chain6ctask_ref_t24): the numpy oracle's
output, B = 2, T = 24. Tolerances: the six-joint suite's own (test_gpu_chain6.py TOL,
FIT_TOL, COST_TOL; test_gpu_chain6_task.py QUAD_TOL), imported, not restated. Every test
prints its measured errors; profiles/chain6_general/ keeps a run's.
"""
import json
import os

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver, coupled_6dof_problem, rbd_initial_states
from test_gpu_chain6 import COST_TOL, FIT_TOL, TOL, chain_fit_replay, dev, inf, rel
from test_gpu_chain6_task import QUAD_TOL
from test_gpu_chain6_task import TOL as TASK_TOL

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64
PR = coupled_6dof_problem()
TASK_CASES = ["chain6ctask_euc_t24", "chain6ctask_ref_t24"]

_loaded = {}


def load(name):
    if name not in _loaded:
        z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        g = {k: z[k] for k in z.files}
        g["meta"] = json.loads(str(g["meta"])) if "meta" in g else None
        _loaded[name] = g
    return _loaded[name]


@pytest.fixture(scope="module")
def gc():
    g = dict(load("chain6c_t24"))
    g.update({k: v for k, v in load("chain6c_cases_t24").items() if k != "meta"})
    return g


@pytest.fixture(scope="module")
def model():
    from oracle import rbd
    return rbd.ChainModel(PR.chain, PR.dt)


def solver(g, lin="dual", nb=None, simple=None):
    n, T = g["u"].shape[:2]
    s = ChainSolver(PR, T, nb or n, dtype=F64, linearization=lin)
    assert s.iterates
    if simple is not None:
        set_costs(s, simple)
    return s


def set_costs(s, c):
    s.set_simple_costs(c["body"], c["point"], c["final_target"], c["weight"], c["euclidean"])
    assert s.cost_mode == ("simple_euclidean" if c["euclidean"] else "simple")


def zero_gains(nb, T):
    return (torch.zeros((nb, T, 6), dtype=F64, device="cuda"),
            torch.zeros((nb, T, 6, 12), dtype=F64, device="cuda"))


# -- a. the dynamics kernel ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_general_dynamics(gpu, model, dtype):
    """One RK4 step (the scalar rnea on every joint's R0, p, axis, COM and full inertia) at
    24 random states, q ∈ ±2, q̇ ∈ ±1, u ∈ ±5, against the oracle computed here; all rows,
    and the velocity rows against their own size (test_chain6_dynamics' bounds)."""
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-2, 2, (24, 6)), rng.uniform(-1, 1, (24, 6))], axis=1)
    u = rng.uniform(-5, 5, (24, 6))
    ref = model.step(x, u)
    s = ChainSolver(PR, 1, 1, dtype=dtype)
    assert s.iterates == (dtype == torch.float64)
    xn = s.dynamics(dev(x, dtype), dev(u, dtype))
    e, ev = rel(xn, ref), rel(xn[:, 6:], ref[:, 6:])
    print(f"general dynamics[{dtype}] x {e:.3e} velocity rows {ev:.3e}")
    tol = 1e-12 if dtype == torch.float64 else 5e-5
    assert e < tol and ev < tol, (e, ev)


# -- b. ragged linearisation --------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
def test_general_linearize_ragged(gpu, model, lin):
    """chain_linearize_tiles_kernel, 5 × 3 points × 18 directions = 270 lanes (a partial
    second workgroup) at random states against the oracle's exact forward-mode Jacobians;
    ∂q̈/∂q (largest entry 0.187 beside A's unit diagonal) against its own size.

    The block's bound: 1e-9 with dual numbers (test_chain6_linearize_ragged's). With central
    differences the suite has no number of the block's own, so FD_BLOCK_TOL = 1e-8 follows
    the project's rule, at most 100 × the oracle's own spread: the C restatement's central
    differences (its step h = ε^⅓·max(1, |z_k|), divided by the step taken) differ from the
    exact Jacobian in this block, at these 15 points, by 1.22e-10 of the block's largest
    entry (measured on the CPU; recomputed below and held to the rule). Device: 1.13e-10."""
    nb, T = 5, 3
    rng = np.random.default_rng(61)
    x = np.concatenate([rng.uniform(-2, 2, (nb, T + 1, 6)), rng.uniform(-1, 1, (nb, T + 1, 6))], axis=2)
    u = rng.uniform(-5, 5, (nb, T, 6))
    Ar, Br = model.linearize(x[:, :T].reshape(-1, 12), u.reshape(-1, 6))
    s = ChainSolver(PR, T, nb, dtype=F64, linearization=lin)
    A, B = s.linearize(dev(x), dev(u))
    A, B = A.reshape(-1, 12, 12), B.reshape(-1, 12, 6)
    ea, eb, eq = rel(A, Ar), rel(B, Br), rel(A[:, 6:, :6], Ar[:, 6:, :6])
    print(f"general linearize_ragged[{lin}] A {ea:.3e} B {eb:.3e} A[6:, :6] {eq:.3e} "
          f"(|A[6:, :6]| max {np.abs(Ar[:, 6:, :6]).max():.3f})")
    assert ea < TOL[lin]["AB"] and eb < TOL[lin]["AB"], (ea, eb)
    if lin == "dual":
        assert eq < 1e-9, eq   # test_chain6_linearize_ragged's bound for the block
    else:
        spread = c_central_difference_block_spread(x[:, :T].reshape(-1, 12), u.reshape(-1, 6), Ar)
        print(f"general linearize_ragged[fd] the C restatement's exact-vs-central-difference spread of "
              f"A[6:, :6] {spread:.3e}")
        assert FD_BLOCK_TOL <= 100.0 * spread, spread   # the bound stays within the rule
        assert eq < FD_BLOCK_TOL, eq


FD_BLOCK_TOL = 1e-8


def c_central_difference_block_spread(X, U, A_exact):
    """The oracle's own spread for the fd column: A[6:, :6] by central differences of the C
    restatement's RK4 step (oracle_chain_iterate's rule: h = ε^⅓·max(1, |z_k|), divided by
    the step actually taken) against the exact block, relative to its largest entry."""
    from oracle import cref
    cbe = 6.0554544523933395e-6   # ε^⅓, fp64
    Z = np.concatenate([X, U], axis=1)
    blk = np.empty((len(Z), 6, 6))
    for k in range(6):
        h = cbe * np.maximum(1.0, np.abs(Z[:, k]))
        zp, zm = Z.copy(), Z.copy()
        zp[:, k], zm[:, k] = Z[:, k] + h, Z[:, k] - h
        fp, fm = cref.chain_dynamics(PR, zp[:, :12], zp[:, 12:]), cref.chain_dynamics(PR, zm[:, :12], zm[:, 12:])
        blk[:, :, k] = ((fp - fm) / (zp[:, k] - zm[:, k])[:, None])[:, 6:]
    return rel(blk, A_exact[:, 6:, :6])


# -- c. fixture parity --------------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
def test_general_linearize_backward_forward(gpu, gc, lin):
    """linearize_dynamics, backward_pass (d, K, statuses 0) and forward_pass with
    prev_cost = Inf (one trial): dual from the fixture's gains, fd from the device's own."""
    g, t = gc, TOL[lin]
    s = solver(g, lin)
    x, u = dev(g["x"]), dev(g["u"])
    A, B = s.linearize(x, u)
    ea, eb = rel(A, g["A"]), rel(B, g["B"])
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    nb = u.shape[0]
    dd, KK = (dev(g["d"]), dev(g["K"])) if lin == "dual" else (d, K)
    xn, un, c, tr, fst = s.forward(x, u, dd, KK, inf(nb))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"chain6c[{lin}] A {ea:.3e} B {eb:.3e} K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ea < t["AB"] and eb < t["AB"], (ea, eb)
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)


# -- d. rollout ---------------------------------------------------------------------------
def test_general_rollout(gpu, gc):
    """The 32-lane forward group with δu = K = 0 (rnea_cv on the LDS constants) is the
    fixture's x, and ilqr_chain_dynamics stepped T times (the scalar rnea): two evaluators
    of a mechanism on which they can differ."""
    g = gc
    s = solver(g)
    x, u = dev(g["x"]), dev(g["u"])
    nb, T = u.shape[:2]
    x_in = x.clone()
    x_in[:, 1:] = 0.0     # not the rollout: the output is the kernel's own
    xn, un, c, tr, st = s.forward(x_in, u, *zero_gains(nb, T), inf(nb))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    assert torch.equal(un, u)
    step = s.rollout(x[:, 0].contiguous(), u)
    e, es, ev = rel(xn, g["x"]), rel(xn, step), rel(xn[..., 6:], step[..., 6:])
    print(f"general rollout vs fixture {e:.3e} vs dynamics {es:.3e} (velocity rows {ev:.3e})")
    assert e < 1e-11, e     # test_chain6_rollout's bound against the fixture
    assert es < TOL["dual"]["roll"] and ev < TOL["dual"]["roll"], (es, ev)


# -- e. line search and x_traj ------------------------------------------------------------
def test_general_line_search_and_x_traj(gpu, gc):
    """δu scaled by the fixture's ls_scale with prev_cost = the cost of (x, u): the oracle's
    trial counts (4 beside 2), the accepted iterate and its cost; then x_traj in the line
    search's objective."""
    g = gc
    s = solver(g)
    x, u, K = dev(g["x"]), dev(g["u"]), dev(g["K"])
    d = dev(g["d"] * g["ls_scale"][:, None, None])
    xn, un, c, tr, st = s.forward(x, u, d, K, dev(g["ls_prev_cost"]))
    assert tr.cpu().numpy().tolist() == g["ls_trials"].tolist() == [4, 2]
    assert (st.cpu().numpy() == 0).all()
    t = TOL["dual"]["fw"]
    ex, eu, ec = rel(xn, g["ls_x"]), rel(un, g["ls_u"]), rel(c, g["ls_cost"])
    print(f"general line search x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < t and eu < t and ec < t, (ex, eu, ec)
    xn, un, c, tr, st = s.forward(x, u, dev(g["d"]), K, inf(2), x_traj=dev(g["xt"]))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    ex, eu, ec = rel(xn, g["xt_x"]), rel(un, g["xt_u"]), rel(c, g["xt_cost"])
    print(f"general x_traj x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < t and eu < t and ec < t, (ex, eu, ec)
    assert rel(c, g["fw_cost"]) > 1e3 * t   # the target moved the cost


# -- f. fit -------------------------------------------------------------------------------
def test_general_fit(gpu, gc):
    """fit: the oracle's iteration counts and statuses, the iterates and the last cost."""
    g = gc
    s = solver(g)
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"chain6c fit iters {r.iters.tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec


@pytest.mark.parametrize("max_iter,tol", [(20, 1e-6), (3, -1.0)])
def test_general_fit_equals_iterate_replay(gpu, gc, max_iter, tol):
    """The fit is its iterations: x, u, cost, iteration counts, statuses and call status
    equal an ilqr_chain_iterate replay bit for bit."""
    g = gc
    s = solver(g)
    x0, u0 = dev(g["x"]), dev(g["u"])
    ref = chain_fit_replay(s, x0, u0, max_iter, tol, None)
    r = s.fit(x0.clone(), u0.clone(), max_iter=max_iter, tol=tol)
    got = (r.x, r.u, r.cost, r.iters, r.status, r.call_status)
    assert got[5] == ref[5]
    for a, b in zip(got[:4], ref[:4]):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(got[4], ref[4])
    if max_iter == 20:
        assert np.array_equal(ref[3].cpu().numpy(), g["fit_iters"])
    else:
        assert ref[3].cpu().numpy().tolist() == [3, 3] and (ref[4].cpu().numpy() == _lib.TRAJ_MAX_ITER).all()


# -- g. batch independence ----------------------------------------------------------------
def _forward_and_iterate(s, x, u, d, K):
    nb = x.shape[0]
    fw = s.forward(x, u, d, K, inf(nb))
    xn, un = torch.empty_like(x), torch.empty_like(u)
    nc = torch.empty((nb,), dtype=F64, device="cuda")
    du2 = torch.empty((nb,), dtype=F64, device="cuda")
    tr = torch.empty((nb,), dtype=torch.int32, device="cuda")
    st = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    s._bind()
    s.iterate(x, u, xn, un, None, st, nc, du2=du2, trials=tr, options=_lib.default_options(tol=-1.0))
    torch.cuda.synchronize()
    return list(fw) + [xn, un, nc, du2, tr, st]


def test_general_batch_independence(gpu, gc):
    """The fixture's two trajectories tiled to B = 66 (33 waves of two 32-lane groups, a
    partial workgroup; the wide tiles kernel's raw-buffer loads) and each alone at B = 1
    (half a wave): forward_pass from the fixture's gains and one iterate give every copy
    the bits of the B = 2 run."""
    g = gc
    x2, u2, d2, K2 = dev(g["x"]), dev(g["u"]), dev(g["d"]), dev(g["K"])
    want = _forward_and_iterate(solver(g), x2, u2, d2, K2)
    assert (want[3].cpu().numpy() == 1).all() and (want[4].cpu().numpy() == 0).all()     # forward
    assert (want[9].cpu().numpy() == 1).all() and (want[10].cpu().numpy() == 0).all()    # iterate
    e = rel(want[0], g["fw_x"])
    assert e < TOL["dual"]["fw"], e
    reps = 33
    tile = lambda a: a.repeat(reps, *([1] * (a.dim() - 1)))  # noqa: E731
    got = _forward_and_iterate(solver(g, nb=66), tile(x2), tile(u2), tile(d2), tile(K2))
    for a, b in zip(got, want):
        assert torch.equal(a, tile(b))
    for k in (0, 1):
        one = lambda a: a[k:k + 1].contiguous()  # noqa: E731
        got = _forward_and_iterate(solver(g, nb=1), one(x2), one(u2), one(d2), one(K2))
        for a, b in zip(got, want):
            assert torch.equal(a, b[k:k + 1])


# -- h. task costs ------------------------------------------------------------------------
def quad_states():
    e, r = load("chain6ctask_euc_t24"), load("chain6ctask_ref_t24")
    rng = np.random.default_rng(7)
    x = np.concatenate([e["fit_x"][:, -1], r["fit_x"][:1, -1], np.zeros((1, 12)),
                        np.array([[4.0, -5.0, 7.5, -3.5, 9.0, -8.25, 0.3, -0.2, 0.1, 0.5, -0.4, 0.2]]),
                        np.concatenate([rng.uniform(-2, 2, (3, 6)), rng.uniform(-1, 1, (3, 6))], axis=1)])
    assert x.shape == (8, 12)
    return x


QUAD_COSTS = [dict(body=5, point=[0.05, 0.02, 0.1], final_target=[2.1, 1.4, 1.5], weight=2e3, euclidean=True),
              dict(body=5, point=[0.05, 0.02, 0.1], final_target=[2.1, 1.4, 1.5], weight=2e3, euclidean=False),
              dict(body=2, point=[0.3, -0.2, 0.15], final_target=[0.9, 1.0, 1.1], weight=2e3, euclidean=True),
              dict(body=2, point=[0.3, -0.2, 0.15], final_target=[0.9, 1.0, 1.1], weight=2e3, euclidean=False)]


@pytest.mark.parametrize("k", range(len(QUAD_COSTS)))
def test_general_final_cost_quadratize(gpu, k):
    """chain_point_fk and chain_task_quad6 with R0 ≠ I and oblique axes: ℓ_f, ∇ℓ_f, ∇²ℓ_f at 8
    states (fixture x_N's, q = 0, angles beyond ±π, random) against nested duals; the Hessian
    bit-symmetric, velocity rows and columns exactly 0, and those of the joints past the body."""
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
    errs = [(rel(cost[i], q[i]), rel(grad[i], qv[i]), rel(hess[i], Q[i])) for i in range(len(x))]
    for i, (ec, eg, eh) in enumerate(errs):
        print(f"general quadratize[{k}] state {i}: cost {ec:.3e} grad {eg:.3e} hess {eh:.3e}")
    for i, e in enumerate(errs):
        assert max(e) < QUAD_TOL, (i, e)
    assert torch.equal(hess, hess.transpose(1, 2))
    assert bool((hess[:, 6:, :] == 0).all()) and bool((hess[:, :, 6:] == 0).all()) and bool((grad[:, 6:] == 0).all())
    nz = c["body"] + 1
    assert bool((hess[:, nz:6, :] == 0).all()) and bool((hess[:, :, nz:6] == 0).all())
    assert bool((grad[:, nz:6] == 0).all())
    assert float(hess[:, :nz, :nz].abs().min(dim=0).values.max()) > 0   # … and the moved joints' are not


def test_general_task_base_body(gpu):
    """body = −1: the point does not move — gradient and Hessian exactly zero and the cost the
    constant weight·|point − target|²."""
    s = ChainSolver(PR, 2, 1, dtype=F64)
    s.set_simple_costs(-1, [0.3, 0.2, 0.1], [1.0, 2.0, 3.0], 50.0, True)
    c, gq, Hq = s.final_cost_quadratization(dev(quad_states()))
    assert bool((gq == 0).all()) and bool((Hq == 0).all())
    e = rel(c, np.full(8, 50.0 * (0.7 ** 2 + 1.8 ** 2 + 2.9 ** 2)))
    print(f"general base body cost {e:.3e}")
    assert e < QUAD_TOL, e   # one evaluation's bound: the sum's order is the kernel's own
    assert torch.equal(c, c[:1].expand(8))   # … and the same bits at every state


@pytest.mark.parametrize("lin", ["dual", "fd"])
@pytest.mark.parametrize("name", TASK_CASES)
def test_general_task_backward_forward(gpu, name, lin):
    """backward_pass and forward_pass under the task costs (the terminal tiles and the 32-lane
    group's task instantiation): dual from the fixture's gains, fd from the device's own."""
    g, t = load(name), TASK_TOL[lin]
    s = solver(g, lin, simple=g["meta"]["simple"])
    x, u = dev(g["x"]), dev(g["u"])
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    dd, KK = (dev(g["d"]), dev(g["K"])) if lin == "dual" else (d, K)
    xn, un, c, tr, fst = s.forward(x, u, dd, KK, inf(2))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"{name}[{lin}] K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e} "
          f"(oracle gain spread {float(g['cond_gain_spread']):.2e})")
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)


@pytest.mark.parametrize("name", TASK_CASES)
def test_general_task_fit(gpu, name):
    g = load(name)
    s = solver(g, simple=g["meta"]["simple"])
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"{name} fit iters {r.iters.tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec


def test_general_task_mode_switching(gpu, gc):
    """task → joint restores the creation-time tiles, joint → task sets them again: backward
    and fit bit-equal to a fresh handle's in either mode."""
    g = load("chain6ctask_euc_t24")
    x, u = dev(gc["x"]), dev(gc["u"])

    def run(s):
        d, K, st = s.backward(x, u)
        r = s.fit(x, u, max_iter=20, tol=1e-6)
        return d, K, st, r.x, r.u, r.cost, r.iters, r.status

    want_joint = run(solver(gc))
    assert np.array_equal(want_joint[6].cpu().numpy(), gc["fit_iters"])
    want_task = run(solver(gc, simple=g["meta"]["simple"]))
    s = solver(gc, simple=g["meta"]["simple"])
    s.set_joint_costs()
    assert s.cost_mode == "joint"
    for a, b in zip(run(s), want_joint):
        assert torch.equal(a, b)
    set_costs(s, g["meta"]["simple"])
    for a, b in zip(run(s), want_task):
        assert torch.equal(a, b)
    assert not torch.equal(want_task[1], want_joint[1])


# -- i. one cold iteration at batch against the C restatement ------------------------------
def test_general_batch66_iteration_vs_c_oracle(gpu):
    """B = 66, T = 12, central differences, one fit iteration from cold against the C
    restatement on the general chain (test_chain6_batch128_iteration_vs_c_oracle's check)."""
    from oracle import cref
    B, T = 66, 12
    s = ChainSolver(PR, T, B, dtype=F64, linearization="fd")
    u = torch.zeros((B, T, 6), dtype=F64, device="cuda")
    x = s.rollout(dev(rbd_initial_states(B, 6)), u)
    xn, un = torch.empty_like(x), torch.empty_like(u)
    pc = torch.empty((B,), dtype=F64, device="cuda")
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    tr = torch.empty((B,), dtype=torch.int32, device="cuda")
    s._bind()
    s.iterate(x, u, xn, un, None, st, pc, trials=tr, options=_lib.default_options(tol=-1.0))
    torch.cuda.synchronize()
    d, K, xo, uo, co, tro = cref.chain_iterate(PR, x.cpu().numpy(), u.cpu().numpy())
    assert (st.cpu().numpy() == 0).all()
    assert np.array_equal(tr.cpu().numpy(), tro)
    t = TOL["fd"]
    eu, ex, ec = rel(un, uo), rel(xn, xo), rel(pc, co)
    print(f"general batch66 fd iteration trials {sorted(set(tro.tolist()))} u {eu:.3e} x {ex:.3e} cost {ec:.3e}")
    assert eu < t["fw"] and ex < t["fw"] and ec < t["fw"], (eu, ex, ec)


# -- j. the large-argument branch of the 32-lane group --------------------------------------
def test_general_rollout_large_angle(gpu, gc, model):
    """chain_xdot_cv32's in-line |angle| > 1e5 branch: B = 3, T = 4, trajectory b with joint
    (0, 2, 5)[b]'s initial angle 2e5 + its fixture value, so the lane that takes the branch
    is a different lane of the DPP row each time. The forward with δu = K = 0 row by row
    against the dynamics kernel stepped and against the oracle: angle rows and velocity
    rows each against their own largest entry, at the suite's rollout tolerance."""
    nb, T = 3, 4
    joints = (0, 2, 5)
    x0 = gc["x"][[0, 1, 0], 0].copy()
    for b, j in enumerate(joints):
        x0[b, j] += 2e5
    rng = np.random.default_rng(9)
    u = rng.uniform(-5, 5, (nb, T, 6))
    ref = np.empty((nb, T + 1, 12))
    ref[:, 0] = x0
    for t in range(T):
        ref[:, t + 1] = model.step(ref[:, t], u[:, t])
    s = ChainSolver(PR, T, nb, dtype=F64)
    ud = dev(u)
    step = s.rollout(dev(x0), ud)
    x_in = torch.zeros((nb, T + 1, 12), dtype=F64, device="cuda")
    x_in[:, 0] = dev(x0)
    xn, un, c, tr, st = s.forward(x_in, ud, *zero_gains(nb, T), inf(nb))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    assert float(np.abs(ref[:, 1:, 6:]).max()) > 0.1    # the state moved
    tol = TOL["dual"]["roll"]
    errs = []
    for b, j in enumerate(joints):
        rows = {"big angle": [j], "other angles": [i for i in range(6) if i != j], "velocities": list(range(6, 12))}
        e = {}
        for what, other in (("dynamics", step), ("oracle", ref)):
            for name, idx in rows.items():
                e[what, name] = rel(xn[b][:, idx], other[b][:, idx])
        print(f"large angle, joint {j}: " + ", ".join(f"vs {w} {n} {v:.3e}" for (w, n), v in e.items()))
        errs.append(e)
    for b, e in enumerate(errs):
        assert max(e.values()) < tol, (b, e)
