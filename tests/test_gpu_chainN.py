"""Chains of 4, 5 and 7 joints on the tiles path (ilqr_amd.chain.coupled_chain_problem(n),
nx = 2n, nu = n, fp64) on the MI355X: every chain entry point, both linearisations, the
joint-space and the task-space costs, at the joint counts beside six.

What each count reaches that six joints do not: seven joints the fifth staging word of the
32-lane forward group (133 step inputs), its eighth role (the odd DPP row's lane 12) and the
wide tiles kernel at 14 × 7; four joints the narrow (8 × 4) tiles kernel, a two-word stage and
an odd row with one role; five joints a three-word stage and the wide kernel at 10 × 5.

Fixtures: tests/golden/make_golden_chainN.py (chain{n}c_t16 + chain{n}c_cases_t16,
chain{n}ctask_euc_t16, chain{n}ctask_ref_t16): the numpy oracle's output, B = 3 (a half-empty
last wave: two 32-lane groups per workgroup), T = 16. Tolerances: the six-joint suite's own
(test_gpu_chain6.py TOL, FIT_TOL, COST_TOL; test_gpu_chain6_task.py QUAD_TOL), imported, not
restated. Every test prints its measured errors; profiles/chain_n/ keeps a run's.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver, chain_closures, coupled_chain_problem
from test_gpu_chain6 import COST_TOL, FIT_TOL, TOL, chain_fit_replay, dev, inf, rel
from test_gpu_chain6_task import QUAD_TOL
from test_gpu_chain6_task import TOL as TASK_TOL

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64
NJ = [4, 5, 7]
T = 16
KINDS = ["euc", "ref"]

_loaded, _problem, _model = {}, {}, {}


def load(name):
    if name not in _loaded:
        z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
        g = {k: z[k] for k in z.files}
        g["meta"] = json.loads(str(g["meta"])) if "meta" in g else None
        _loaded[name] = g
    return _loaded[name]


def problem(n):
    if n not in _problem:
        _problem[n] = coupled_chain_problem(n)
    return _problem[n]


def model(n):
    if n not in _model:
        from oracle import rbd
        _model[n] = rbd.ChainModel(problem(n).chain, problem(n).dt)
    return _model[n]


def joint_fixture(n):
    g = dict(load(f"chain{n}c_t{T}"))
    g.update({k: v for k, v in load(f"chain{n}c_cases_t{T}").items() if k != "meta"})
    return g


def task_fixture(n, kind):
    return load(f"chain{n}ctask_{kind}_t{T}")


def set_costs(s, c):
    s.set_simple_costs(c["body"], c["point"], c["final_target"], c["weight"], c["euclidean"])
    assert s.cost_mode == ("simple_euclidean" if c["euclidean"] else "simple")


def solver(n, g, lin="dual", nb=None, simple=None):
    s = ChainSolver(problem(n), g["u"].shape[1], nb or g["u"].shape[0], dtype=F64, linearization=lin)
    assert s.iterates
    if simple is not None:
        set_costs(s, simple)
    return s


def random_points(n, count, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-2, 2, (count, n)), rng.uniform(-1, 1, (count, n))], axis=1)
    return x, rng.uniform(-5, 5, (count, n))


# -- a. the dynamics kernel ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", NJ)
def test_chainN_dynamics(gpu, n, dtype):
    """One RK4 step (the scalar rnea) at 24 random states, q ∈ ±2, q̇ ∈ ±1, u ∈ ±5, against the
    oracle; all rows, and the velocity rows against their own size (test_general_dynamics'
    bounds). The fp32 handle does not iterate and still answers."""
    x, u = random_points(n, 24, 7)
    ref = model(n).step(x, u)
    s = ChainSolver(problem(n), 1, 1, dtype=dtype)
    assert s.iterates == (dtype == torch.float64)
    xn = s.dynamics(dev(x, dtype), dev(u, dtype))
    e, ev = rel(xn, ref), rel(xn[:, n:], ref[:, n:])
    print(f"chain{n} dynamics[{dtype}] x {e:.3e} velocity rows {ev:.3e}")
    tol = 1e-12 if dtype == torch.float64 else 5e-5
    assert e < tol and ev < tol, (e, ev)


# -- b. ragged linearisation --------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
@pytest.mark.parametrize("n", NJ)
def test_chainN_linearize_ragged(gpu, n, lin):
    """chain_linearize_tiles_kernel, 5 × 3 points × 3n directions (180, 225, 315 lanes: a
    partial workgroup, points straddling waves) at random states against the oracle's exact
    forward-mode Jacobians; with dual numbers ∂q̈/∂q against its own size
    (test_chain6_linearize_ragged's bound for the block)."""
    nb, Tr = 5, 3
    nx = 2 * n
    rng = np.random.default_rng(61)
    x = np.concatenate([rng.uniform(-2, 2, (nb, Tr + 1, n)), rng.uniform(-1, 1, (nb, Tr + 1, n))], axis=2)
    u = rng.uniform(-5, 5, (nb, Tr, n))
    Ar, Br = model(n).linearize(x[:, :Tr].reshape(-1, nx), u.reshape(-1, n))
    s = ChainSolver(problem(n), Tr, nb, dtype=F64, linearization=lin)
    A, B = s.linearize(dev(x), dev(u))
    A, B = A.reshape(-1, nx, nx), B.reshape(-1, nx, n)
    ea, eb, eq = rel(A, Ar), rel(B, Br), rel(A[:, n:, :n], Ar[:, n:, :n])
    print(f"chain{n} linearize_ragged[{lin}] A {ea:.3e} B {eb:.3e} A[{n}:, :{n}] {eq:.3e} "
          f"(|A[{n}:, :{n}]| max {np.abs(Ar[:, n:, :n]).max():.3f})")
    assert ea < TOL[lin]["AB"] and eb < TOL[lin]["AB"], (ea, eb)
    if lin == "dual":
        assert eq < 1e-9, eq


# -- c. fixture parity: linearisation, backward gains, forward ------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
@pytest.mark.parametrize("n", NJ)
def test_chainN_linearize_backward_forward(gpu, n, lin):
    """linearize_dynamics, backward_pass (d, K, statuses 0: the narrow tiles kernel for four
    joints, the wide one for five and seven) and forward_pass with prev_cost = Inf (one trial):
    dual from the fixture's gains, fd from the device's own."""
    g, t = joint_fixture(n), TOL[lin]
    s = solver(n, g, lin)
    x, u = dev(g["x"]), dev(g["u"])
    A, B = s.linearize(x, u)
    ea, eb = rel(A, g["A"]), rel(B, g["B"])
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    nb = u.shape[0]
    dd, KK = (dev(g["d"]), dev(g["K"])) if lin == "dual" else (d, K)
    xn, un, c, tr, fst = s.forward(x, u, dd, KK, inf(nb))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"chain{n}c[{lin}] A {ea:.3e} B {eb:.3e} K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e} "
          f"(oracle gain spread {float(g['cond_gain_spread']):.2e})")
    assert ea < t["AB"] and eb < t["AB"], (ea, eb)
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)


# -- d. rollout: the 32-lane group against the scalar pass ----------------------------------
@pytest.mark.parametrize("n", NJ)
def test_chainN_rollout(gpu, n):
    """The 32-lane forward group with δu = K = 0 (rnea_cv on the LDS constants, NJ + 1 roles) is
    the fixture's x, and ilqr_chain_dynamics stepped T times (the scalar rnea)."""
    g = joint_fixture(n)
    s = solver(n, g)
    x, u = dev(g["x"]), dev(g["u"])
    nb = u.shape[0]
    x_in = x.clone()
    x_in[:, 1:] = 0.0     # not the rollout: the output is the kernel's own
    zd = torch.zeros((nb, T, n), dtype=F64, device="cuda")
    zK = torch.zeros((nb, T, n, 2 * n), dtype=F64, device="cuda")
    xn, un, c, tr, st = s.forward(x_in, u, zd, zK, inf(nb))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    assert torch.equal(un, u)
    step = s.rollout(x[:, 0].contiguous(), u)
    e, es, ev = rel(xn, g["x"]), rel(xn, step), rel(xn[..., n:], step[..., n:])
    print(f"chain{n} rollout vs fixture {e:.3e} vs dynamics {es:.3e} (velocity rows {ev:.3e})")
    assert e < 1e-11, e     # test_chain6_rollout's bound against the fixture
    assert es < TOL["dual"]["roll"] and ev < TOL["dual"]["roll"], (es, ev)


# -- e. line search and x_traj ------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_chainN_line_search_and_x_traj(gpu, n):
    """δu scaled by the fixture's ls_scale with prev_cost = the cost of (x, u): the oracle's
    trial counts (one of them past the first), the accepted iterate and its cost; then x_traj
    in the line search's objective."""
    g = joint_fixture(n)
    s = solver(n, g)
    x, u, K = dev(g["x"]), dev(g["u"]), dev(g["K"])
    nb = u.shape[0]
    d = dev(g["d"] * g["ls_scale"][:, None, None])
    xn, un, c, tr, st = s.forward(x, u, d, K, dev(g["ls_prev_cost"]))
    assert g["ls_trials"].max() >= 2
    assert tr.cpu().numpy().tolist() == g["ls_trials"].tolist(), (tr, g["ls_trials"])
    assert (st.cpu().numpy() == 0).all()
    t = TOL["dual"]["fw"]
    ex, eu, ec = rel(xn, g["ls_x"]), rel(un, g["ls_u"]), rel(c, g["ls_cost"])
    print(f"chain{n} line search trials {g['ls_trials'].tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < t and eu < t and ec < t, (ex, eu, ec)
    xn, un, c, tr, st = s.forward(x, u, dev(g["d"]), K, inf(nb), x_traj=dev(g["xt"]))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    ex, eu, ec = rel(xn, g["xt_x"]), rel(un, g["xt_u"]), rel(c, g["xt_cost"])
    print(f"chain{n} x_traj x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < t and eu < t and ec < t, (ex, eu, ec)
    assert rel(c, g["fw_cost"]) > 1e3 * t   # the target moved the cost


# -- f. one iterate -----------------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_chainN_iterate(gpu, n):
    """ilqr_chain_iterate from cold (prev_cost null = Inf): the fixture's forward pass — the
    backward gains and the accepted iterate in one call — with Σδu² and one trial."""
    g = joint_fixture(n)
    s = solver(n, g)
    x, u = dev(g["x"]), dev(g["u"])
    nb = u.shape[0]
    xn, un = torch.empty_like(x), torch.empty_like(u)
    nc = torch.empty((nb,), dtype=F64, device="cuda")
    du2 = torch.empty((nb,), dtype=F64, device="cuda")
    tr = torch.empty((nb,), dtype=torch.int32, device="cuda")
    st = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    s._bind()
    s.iterate(x, u, xn, un, None, st, nc, du2=du2, trials=tr, options=_lib.default_options(tol=-1.0))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (tr.cpu().numpy() == 1).all()
    t = TOL["dual"]["fw"]
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(nc, g["fw_cost"])
    e2 = rel(du2, ((g["fw_u"] - g["u"]) ** 2).sum(axis=(1, 2)))
    print(f"chain{n} iterate x {ex:.3e} u {eu:.3e} cost {ec:.3e} du2 {e2:.3e}")
    assert ex < t and eu < t and ec < t and e2 < t, (ex, eu, ec, e2)


# -- g. fit -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_chainN_fit(gpu, n):
    """fit: the oracle's iteration counts and statuses, the iterates and the last cost."""
    g = joint_fixture(n)
    s = solver(n, g)
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"chain{n}c fit iters {r.iters.tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec


@pytest.mark.parametrize("max_iter,tol", [(20, 1e-6), (3, -1.0)])
@pytest.mark.parametrize("n", NJ)
def test_chainN_fit_equals_iterate_replay(gpu, n, max_iter, tol):
    """The fit is its iterations: x, u, cost, iteration counts, statuses and call status
    equal an ilqr_chain_iterate replay bit for bit."""
    g = joint_fixture(n)
    s = solver(n, g)
    x0, u0 = dev(g["x"]), dev(g["u"])
    nb = x0.shape[0]
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
        assert ref[3].cpu().numpy().tolist() == [3] * nb and (ref[4].cpu().numpy() == _lib.TRAJ_MAX_ITER).all()


# -- h. task costs ------------------------------------------------------------------------
def quad_states(n):
    e, r = task_fixture(n, "euc"), task_fixture(n, "ref")
    big = np.array([4.0, -5.0, 7.5, -3.5, 9.0, -8.25, 6.5])[:n]          # angles beyond ±π
    vel = np.array([0.3, -0.2, 0.1, 0.5, -0.4, 0.2, -0.1])[:n]
    x = np.concatenate([e["fit_x"][:2, -1], r["fit_x"][:1, -1], np.zeros((1, 2 * n)),
                        np.concatenate([big, vel])[None], random_points(n, 3, 7)[0]])
    assert x.shape == (8, 2 * n)
    return x


def quad_costs(n):
    return [task_fixture(n, "euc")["meta"]["simple"], dict(task_fixture(n, "euc")["meta"]["simple"], euclidean=False),
            task_fixture(n, "ref")["meta"]["simple"], dict(task_fixture(n, "ref")["meta"]["simple"], euclidean=True)]


@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("n", NJ)
def test_chainN_final_cost_quadratize(gpu, n, k):
    """chain_point_fk and chain_task_quad_fk: ℓ_f, ∇ℓ_f, ∇²ℓ_f at 8 states (fixture x_N's, q = 0,
    angles beyond ±π, random) against the oracle's nested duals, for the tool and for body 2 in
    both readings; the Hessian bit-symmetric, velocity rows and columns exactly 0, and those of
    the joints past the body."""
    from oracle import cost_functions as OC
    from oracle import ilqr_oracle as O
    c = quad_costs(n)[k]
    x = quad_states(n)
    lf = OC.simple_final_cost(problem(n).chain, c["body"], c["point"], c["final_target"], c["weight"],
                              euclidean=c["euclidean"])
    ref = [O.final_cost_quadratization(xi, lf) for xi in x]
    q, qv, Q = (np.array([r[i] for r in ref], dtype=float) for i in range(3))
    s = ChainSolver(problem(n), 2, 1, dtype=F64)
    set_costs(s, c)
    cost, grad, hess = s.final_cost_quadratization(dev(x))
    torch.cuda.synchronize()
    errs = [(rel(cost[i], q[i]), rel(grad[i], qv[i]), rel(hess[i], Q[i])) for i in range(len(x))]
    for i, (ec, eg, eh) in enumerate(errs):
        print(f"chain{n} quadratize[{k}] state {i}: cost {ec:.3e} grad {eg:.3e} hess {eh:.3e}")
    for i, e in enumerate(errs):
        assert max(e) < QUAD_TOL, (i, e)
    assert torch.equal(hess, hess.transpose(1, 2))
    assert bool((hess[:, n:, :] == 0).all()) and bool((hess[:, :, n:] == 0).all()) and bool((grad[:, n:] == 0).all())
    nz = c["body"] + 1
    assert bool((hess[:, nz:n, :] == 0).all()) and bool((hess[:, :, nz:n] == 0).all())
    assert bool((grad[:, nz:n] == 0).all())
    assert float(hess[:, :nz, :nz].abs().min(dim=0).values.max()) > 0   # … and the moved joints' are not


@pytest.mark.parametrize("lin", ["dual", "fd"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NJ)
def test_chainN_task_backward_forward(gpu, n, kind, lin):
    """backward_pass and forward_pass under the task costs (the terminal tiles and the 32-lane
    group's task instantiation): dual from the fixture's gains, fd from the device's own."""
    g, t = task_fixture(n, kind), TASK_TOL[lin]
    s = solver(n, g, lin, simple=g["meta"]["simple"])
    x, u = dev(g["x"]), dev(g["u"])
    nb = u.shape[0]
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    dd, KK = (dev(g["d"]), dev(g["K"])) if lin == "dual" else (d, K)
    xn, un, c, tr, fst = s.forward(x, u, dd, KK, inf(nb))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"chain{n}ctask_{kind}[{lin}] K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e} "
          f"(oracle gain spread {float(g['cond_gain_spread']):.2e})")
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NJ)
def test_chainN_task_fit(gpu, n, kind):
    """A fit under the task costs: the oracle's iteration counts and statuses, the iterates and
    the last cost."""
    g = task_fixture(n, kind)
    s = solver(n, g, simple=g["meta"]["simple"])
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"chain{n}ctask_{kind} fit iters {r.iters.tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec


@pytest.mark.parametrize("n", NJ)
def test_chainN_task_mode_switching(gpu, n):
    """task → joint restores the creation-time tiles, joint → task sets them again: backward
    and fit bit-equal to a fresh handle's in either mode."""
    gc, g = joint_fixture(n), task_fixture(n, "euc")
    x, u = dev(gc["x"]), dev(gc["u"])

    def run(s):
        d, K, st = s.backward(x, u)
        r = s.fit(x, u, max_iter=20, tol=1e-6)
        return d, K, st, r.x, r.u, r.cost, r.iters, r.status

    want_joint = run(solver(n, gc))
    assert np.array_equal(want_joint[6].cpu().numpy(), gc["fit_iters"])
    want_task = run(solver(n, gc, simple=g["meta"]["simple"]))
    s = solver(n, gc, simple=g["meta"]["simple"])
    s.set_joint_costs()
    assert s.cost_mode == "joint"
    for a, b in zip(run(s), want_joint):
        assert torch.equal(a, b)
    set_costs(s, g["meta"]["simple"])
    for a, b in zip(run(s), want_task):
        assert torch.equal(a, b)
    assert not torch.equal(want_task[1], want_joint[1])


# -- i. the ABI edges of the new counts -----------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_chainN_what_stays_closed(gpu, n):
    """An fp32 handle refuses fit and still rolls out; set_simple_costs and CLOSED_FORM are
    refused; body index n is BAD_ARG (and n − 1, the last body, is taken)."""
    g, pr = joint_fixture(n), problem(n)
    nb = g["u"].shape[0]
    s32 = ChainSolver(pr, T, nb, dtype=torch.float32)
    assert not s32.iterates
    x, u = dev(g["x"], torch.float32), dev(g["u"], torch.float32)
    xo, uo = torch.empty_like(x), torch.empty_like(u)
    s32._bind()
    o = _lib.default_options(max_iter=2)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert s32.lib.ilqr_chain_fit(s32.h, C.byref(o), p(x), p(u), None, p(xo), p(uo), None, None,
                                  None) == _lib.ERR_UNSUPPORTED
    tgt = (C.c_double * 3)(0.1, 0.2, 0.3)
    assert s32.lib.ilqr_chain_set_task_costs(s32.h, _lib.CHAIN_COST_SIMPLE, 0, tgt, tgt, 1.0) == _lib.ERR_UNSUPPORTED
    xn = s32.dynamics(x[:, 0].contiguous(), u[:, 0].contiguous())   # … and still rolls out
    e = rel(xn, g["x"][:, 1])
    print(f"chain{n} fp32 dynamics {e:.3e}")
    assert e < 5e-5, e
    s = solver(n, g)
    lib = s.lib
    assert lib.ilqr_chain_set_simple_costs(s.h, _lib.CHAIN_COST_SIMPLE, n - 1, tgt, tgt, 1.0) == _lib.ERR_UNSUPPORTED
    assert s.cost_mode == "joint"
    assert lib.ilqr_chain_set_dynamics(s.h, _lib.CHAIN_DYN_CLOSED_FORM) == _lib.ERR_UNSUPPORTED
    s.set_dynamics("rnea")
    assert s.dynamics_mode == "rnea"
    s.set_dynamics("auto")
    assert s.dynamics_mode == "rnea"
    assert s.closed_form_error == 0.0   # "not used"
    assert lib.ilqr_chain_set_task_costs(s.h, _lib.CHAIN_COST_SIMPLE, n, tgt, tgt, 1.0) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_set_task_costs(s.h, _lib.CHAIN_COST_SIMPLE, -2, tgt, tgt, 1.0) == _lib.ERR_BAD_ARG
    assert s.cost_mode == "joint"
    s._bind()
    assert lib.ilqr_chain_set_task_costs(s.h, _lib.CHAIN_COST_SIMPLE, n - 1, tgt, tgt, 1.0) == _lib.OK
    assert s.cost_mode == "simple"


# -- j. the API mirror ----------------------------------------------------------------------
def test_chain7_api_mirror(gpu):
    """ilqr_amd.fit through chain_closures(coupled_chain_problem(7)): float64 inputs solve,
    float32 inputs raise the ValueError that names fp64."""
    import ilqr_amd
    g = joint_fixture(7)
    dyn, cost, fcost = chain_closures(problem(7))
    xo, uo = ilqr_amd.fit(g["x"][0], g["u"][0], dyn, cost, fcost, max_iter=20, tol=1e-6)
    assert uo.dtype == np.float64
    ex, eu = rel(xo, g["fit_x"][0]), rel(uo, g["fit_u"][0])
    print(f"chain7 api fit x {ex:.3e} u {eu:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    x32, u32 = g["x"][0].astype(np.float32), g["u"][0].astype(np.float32)
    with pytest.raises(ValueError, match="fp64"):
        ilqr_amd.fit(x32, u32, dyn, cost, fcost, max_iter=2, tol=1e-6)
