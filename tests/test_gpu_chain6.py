"""The six-joint chain (the 6-DoF arm, nx = 12, nu = 6, fp64) on the MI355X: the
linearisation written as tiles, the wide tiles recursion, the 32-lane forward group, and
the 2-joint family's entry points and semantics on top of them.

Fixtures: tests/golden/make_golden_chain6.py (chain6_t30: gravity zero as the URDF parses;
chain6g_t30 + chain6g_cases_t30: gravity on, with a line-search case and an x_traj case).
Tolerances: the 2-joint family's fp64 rows (tests/test_gpu_chain.py TOL)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver, chain_closures, rbd_6dof_problem, rbd_initial_states

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
F64 = torch.float64

TOL = {  # linearisation → tolerances (fp64)
    "dual": dict(roll=1e-12, AB=1e-11, gain=1e-9, fw=1e-10),
    "fd": dict(roll=1e-12, AB=1e-7, gain=1e-6, fw=1e-6),
}
FIT_TOL, COST_TOL = 1e-8, 1e-10


def rel(a, b):
    a = a.double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, float)
    b = b.double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def g6():
    return load("chain6_t30")


@pytest.fixture(scope="module")
def g6g():
    g = load("chain6g_t30")
    g.update(load("chain6g_cases_t30"))
    return g


def fixture_of(name, g6, g6g):
    return (g6, rbd_6dof_problem()) if name == "chain6" else (g6g, rbd_6dof_problem(gravity=True))


def solver(g, pr, lin="dual", nb=None):
    n, T = g["u"].shape[:2]
    return ChainSolver(pr, T, nb or n, dtype=F64, linearization=lin)


def inf(nb):
    return torch.full((nb,), float("inf"), dtype=F64, device="cuda")


# -- 1. ragged linearisation ------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
def test_chain6_linearize_ragged(gpu, lin):
    """One lane per (b, t, direction): 5 × 3 points × 18 directions = 270 lanes, a partial
    second workgroup and points straddling waves, at random states with gravity on, vs
    the oracle's exact forward-mode Jacobians."""
    from oracle import rbd
    pr = rbd_6dof_problem(gravity=True)
    nb, T = 5, 3
    rng = np.random.default_rng(61)
    x = np.concatenate([rng.uniform(-2, 2, (nb, T + 1, 6)), rng.uniform(-1, 1, (nb, T + 1, 6))], axis=2)
    u = rng.uniform(-5, 5, (nb, T, 6))
    Ar, Br = rbd.ChainModel(pr.chain, pr.dt).linearize(x[:, :T].reshape(-1, 12), u.reshape(-1, 6))
    s = ChainSolver(pr, T, nb, dtype=F64, linearization=lin)
    assert s.iterates
    A, B = s.linearize(dev(x), dev(u))
    A, B = A.reshape(-1, 12, 12), B.reshape(-1, 12, 6)
    ea, eb = rel(A, Ar), rel(B, Br)
    print(f"linearize_ragged[{lin}] A {ea:.3e} B {eb:.3e}")
    assert ea < TOL[lin]["AB"] and eb < TOL[lin]["AB"], (ea, eb)
    if lin == "dual":
        # ∂q̈/∂q (entries ~0.1 beside A's unit diagonal) against its own size
        eq = rel(A[:, 6:, :6], Ar[:, 6:, :6])
        print(f"linearize_ragged[dual] A[6:, :6] {eq:.3e}")
        assert eq < 1e-9, eq


# -- 2. fixture parity ------------------------------------------------------------------
@pytest.mark.parametrize("lin", ["dual", "fd"])
@pytest.mark.parametrize("name", ["chain6", "chain6g"])
def test_chain6_linearize_backward_forward(gpu, g6, g6g, name, lin):
    """linearize_dynamics, backward_pass (d, K, statuses 0) and forward_pass from the
    fixture's gains with prev_cost = Inf (one trial), at the linearisation's column."""
    g, pr = fixture_of(name, g6, g6g)
    t = TOL[lin]
    s = solver(g, pr, lin)
    x, u = dev(g["x"]), dev(g["u"])
    A, B = s.linearize(x, u)
    ea, eb = rel(A, g["A"]), rel(B, g["B"])
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    nb = u.shape[0]
    # dual: the forward from the fixture's gains; fd: from the device's own (fd) gains
    dd, KK = (dev(g["d"]), dev(g["K"])) if lin == "dual" else (d, K)
    xn, un, c, tr, fst = s.forward(x, u, dd, KK, inf(nb))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"{name}[{lin}] A {ea:.3e} B {eb:.3e} K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ea < t["AB"] and eb < t["AB"], (ea, eb)
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)


@pytest.mark.parametrize("name", ["chain6", "chain6g"])
def test_chain6_fit(gpu, g6, g6g, name):
    """fit (forward_pass.jl:148-179): exact iteration counts and statuses, the iterates
    and the last cost."""
    g, pr = fixture_of(name, g6, g6g)
    s = solver(g, pr)
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"{name} fit x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec


# -- 3. rollout -------------------------------------------------------------------------
def test_chain6_rollout(gpu, g6g):
    """forward with δu = K = 0 and prev_cost = Inf is the plain rollout: the gravity
    fixture's x, and ilqr_chain_dynamics applied step by step (the scalar pass)."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    s = solver(g, pr)
    x, u = dev(g["x"]), dev(g["u"])
    nb, T = u.shape[:2]
    # start from a trajectory that is NOT the rollout, so the output is the kernel's own
    x_in = x.clone()
    x_in[:, 1:] = 0.0
    xn, un, c, tr, st = s.forward(x_in, u, torch.zeros_like(u), torch.zeros((nb, T, 6, 12), dtype=F64, device="cuda"),
                                  inf(nb))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    assert torch.equal(un, u)
    e = rel(xn, g["x"])
    step = s.rollout(x[:, 0].contiguous(), u)
    es = rel(xn, step)
    print(f"rollout vs fixture {e:.3e} vs dynamics {es:.3e}")
    assert e < 1e-11, e
    assert es < TOL["dual"]["roll"], es


# -- 4. line search ---------------------------------------------------------------------
def test_chain6_line_search(gpu, g6g):
    """δu scaled by (9, 2.5) with prev_cost = the cost of (x, u): trajectory 0 accepts its
    fourth trial beside trajectory 1's second. With max_trials = 3 trajectory 0 is
    exhausted: it returns its inputs bit for bit, the call ILQR_ERR_LS_EXHAUSTED, and
    trajectory 1 is what it was."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    s = solver(g, pr)
    x, u, K = dev(g["x"]), dev(g["u"]), dev(g["K"])
    d = dev(g["d"] * g["ls_scale"][:, None, None])
    pc = dev(g["ls_prev_cost"])
    xn, un, c, tr, st = s.forward(x, u, d, K, pc)
    assert tr.cpu().numpy().tolist() == g["ls_trials"].tolist() == [4, 2]
    assert (st.cpu().numpy() == 0).all()
    t = TOL["dual"]["fw"]
    ex, eu, ec = rel(xn, g["ls_x"]), rel(un, g["ls_u"]), rel(c, g["ls_cost"])
    print(f"line search x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < t and eu < t and ec < t, (ex, eu, ec)
    o = _lib.default_options(max_trials=3)
    s._bind()
    x2, u2 = torch.empty_like(x), torch.empty_like(u)
    c2 = torch.empty((2,), dtype=F64, device="cuda")
    tr2 = torch.empty((2,), dtype=torch.int32, device="cuda")
    st2 = torch.empty((2,), dtype=torch.int32, device="cuda")
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    cs = s.lib.ilqr_chain_forward(s.h, C.byref(o), p(x), p(u), None, p(d), p(K), p(pc), p(x2), p(u2), p(c2),
                                  p(tr2), p(st2))
    assert cs == _lib.ERR_LS_EXHAUSTED
    assert st2.cpu().numpy().tolist() == [_lib.TRAJ_LS_EXHAUSTED, _lib.TRAJ_OK]
    assert tr2.cpu().numpy().tolist() == [3, 2]
    assert torch.equal(x2[0], x[0]) and torch.equal(u2[0], u[0])
    assert torch.equal(x2[1], xn[1]) and torch.equal(u2[1], un[1]) and torch.equal(c2[1], c[1])


# -- 5. x_traj --------------------------------------------------------------------------
def test_chain6_x_traj(gpu, g6g):
    """x_traj enters the line search's objective only (forward_pass.jl:187-190)."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    s = solver(g, pr)
    nb = g["u"].shape[0]
    xn, un, c, tr, st = s.forward(dev(g["x"]), dev(g["u"]), dev(g["d"]), dev(g["K"]), inf(nb), x_traj=dev(g["xt"]))
    assert (tr.cpu().numpy() == 1).all() and (st.cpu().numpy() == 0).all()
    t = TOL["dual"]["fw"]
    ex, eu, ec = rel(xn, g["xt_x"]), rel(un, g["xt_u"]), rel(c, g["xt_cost"])
    print(f"x_traj x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < t and eu < t and ec < t, (ex, eu, ec)
    assert rel(c, g["fw_cost"]) > 1e3 * t   # the target moved the cost, far beyond the tolerance


# -- 6. both load paths of the tiles kernel ----------------------------------------------
def test_chain6_backward_both_tile_loads(gpu, g6g):
    """nb = 66 takes the wide tiles kernel's raw-buffer loads (≥ 64), nb = 2 its per-element
    loads; nx = 12, nu = 6 leave padded rows and columns to the out-of-range offsets.
    Every copy of the two trajectories is bit-equal to the nb = 2 run, with μ = 0 too."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    nb = 66
    reps = nb // 2
    x2, u2 = dev(g["x"]), dev(g["u"])
    x66, u66 = x2.repeat(reps, 1, 1), u2.repeat(reps, 1, 1)
    s2, s66 = solver(g, pr), solver(g, pr, nb=nb)
    d2, K2, st2 = s2.backward(x2, u2)
    d66, K66, st66 = s66.backward(x66, u66)
    assert (st2.cpu().numpy() == 0).all() and (st66.cpu().numpy() == 0).all()
    ek, ed = rel(K66[:2], g["K"]), rel(d66[:2], g["d"])
    print(f"tiles nb=66 K {ek:.3e} d {ed:.3e}")
    assert ek < TOL["dual"]["gain"] and ed < TOL["dual"]["gain"], (ek, ed)
    assert torch.equal(K66, K2.repeat(reps, 1, 1, 1)) and torch.equal(d66, d2.repeat(reps, 1, 1))
    o = _lib.default_options(mu=0.0)
    d2z, K2z, st2z = s2.backward(x2, u2, options=o)
    d66z, K66z, st66z = s66.backward(x66, u66, options=o)
    assert (st2z.cpu().numpy() == 0).all() and (st66z.cpu().numpy() == 0).all()
    assert bool(torch.isfinite(K66z).all()) and bool(torch.isfinite(d66z).all())
    assert torch.equal(K66z, K2z.repeat(reps, 1, 1, 1)) and torch.equal(d66z, d2z.repeat(reps, 1, 1))
    assert not torch.equal(K2z, K2)   # μ entered


# -- 7. masking -------------------------------------------------------------------------
def test_chain6_iterate_masks(gpu, g6g):
    """ilqr_chain_iterate on a batch of 6: a NaN state ends its trajectory ILQR_TRAJ_NAN, a
    trajectory that enters CONVERGED comes out untouched, and the other four are what
    the same call without the two gives, bit for bit."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    nb, SENT = 6, -12345.0
    x, u = dev(g["x"]).repeat(3, 1, 1), dev(g["u"]).repeat(3, 1, 1)
    x[0::2, 0, :6] += torch.arange(3, dtype=F64, device="cuda")[:, None] * 0.01   # six different starts
    s = solver(g, pr, nb=nb)
    x = s.rollout(x[:, 0].contiguous(), u)

    def run(xi, status):
        xn, un = torch.full_like(xi, SENT), torch.full_like(u, SENT)
        nc = torch.full((nb,), SENT, dtype=F64, device="cuda")
        du2 = torch.full((nb,), SENT, dtype=F64, device="cuda")
        tr = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
        st = torch.tensor(status, dtype=torch.int32, device="cuda")
        s._bind()
        s.iterate(xi, u, xn, un, None, st, nc, du2=du2, trials=tr, options=_lib.default_options(tol=-1.0))
        torch.cuda.synchronize()
        return xn, un, nc, du2, tr, st

    ref = run(x, [0] * nb)
    assert (ref[5].cpu().numpy() == 0).all() and (ref[4].cpu().numpy() == 1).all()
    xb = x.clone()
    xb[2, 3, 1] = float("nan")
    got = run(xb, [0, 0, 0, 0, _lib.TRAJ_CONVERGED, 0])
    st = got[5].cpu().numpy().tolist()
    assert st == [0, 0, _lib.TRAJ_NAN, 0, _lib.TRAJ_CONVERGED, 0], st
    for a in got[:4]:   # trajectory 4: x_new, u_new, cost and Σδu² words untouched
        assert bool((a[4] == SENT).all())
    assert got[4][4].item() == -7
    keep = [0, 1, 3, 5]
    for a, b in zip(got[:5], ref[:5]):
        assert torch.equal(a[keep], b[keep])


# -- 8. fit = iterate replay ------------------------------------------------------------
def chain_fit_replay(s, x0, u0, max_iter, tol, max_trials, x_traj=None):
    """fit (forward_pass.jl:148-179) restated as ilqr_chain_iterate calls (the helper of
    tests/test_gpu_chain.py): prev_cost = Inf, each iteration on the still-running
    trajectories, a trajectory that stops keeps the iteration's INPUT, the running ones
    the last accepted iterate and MAX_ITER."""
    nb = x0.shape[0]
    s._bind()
    o = _lib.default_options(max_iter=max_iter, tol=tol, max_trials=max_trials)
    x, u = x0.clone(), u0.clone()
    pc = inf(nb)
    st = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    tr = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    it_out = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    rx, ru = x0.clone(), u0.clone()
    for it in range(1, max_iter + 1):
        run = st == 0
        if not bool(run.any()):
            break
        xn, un = torch.empty_like(x), torch.empty_like(u)
        tr.fill_(-1)
        s.iterate(x, u, xn, un, pc, st, pc, trials=tr, x_traj=x_traj, options=o)
        it_out[run & (tr != -1)] = it   # the forward ran it (a NaN backward stops before)
        stopped = run & (st != 0)
        rx[stopped], ru[stopped] = x[stopped], u[stopped]
        keep = run & (st == 0)
        x = torch.where(keep[:, None, None], xn, x)
        u = torch.where(keep[:, None, None], un, u)
    run = st == 0
    rx[run], ru[run] = x[run], u[run]
    st = torch.where(run, torch.full_like(st, _lib.TRAJ_MAX_ITER), st)
    s_np = st.cpu().numpy()
    cs = _lib.ERR_NAN if (s_np == _lib.TRAJ_NAN).any() else (
        _lib.ERR_LS_EXHAUSTED if (s_np == _lib.TRAJ_LS_EXHAUSTED).any() else _lib.OK)
    return rx, ru, pc, it_out, st, cs


@pytest.mark.parametrize("max_iter,tol,max_trials,inplace", [
    (20, 1e-6, None, False),   # early convergence: the poll stops the loop
    (3, -1.0, 2, False),       # to max_iter, a capped search
    (5, 1e-6, None, True),     # x_out = x_init: no direct output, copies
    (1, -1.0, None, False),
    (0, -1.0, None, False),    # the input is the result
])
def test_chain6_fit_equals_iterate_replay(gpu, g6g, max_iter, tol, max_trials, inplace):
    """chain_fit_t drives the six-joint kernels as it drives the 2-joint ones: x, u, cost,
    iterations, status and call status of the fit equal the replay's, bit for bit."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    s = solver(g, pr)
    x0, u0 = dev(g["x"]), dev(g["u"])
    ref = chain_fit_replay(s, x0, u0, max_iter, tol, max_trials)
    for _ in range(2):   # twice: the re-armed call-status words
        xi, ui = x0.clone(), u0.clone()
        if inplace:
            nb = xi.shape[0]
            cost = torch.empty((nb,), dtype=F64, device="cuda")
            it = torch.empty((nb,), dtype=torch.int32, device="cuda")
            st = torch.empty((nb,), dtype=torch.int32, device="cuda")
            s._bind()
            o = _lib.default_options(max_iter=max_iter, tol=tol, max_trials=max_trials)
            p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            cs = s.lib.ilqr_chain_fit(s.h, C.byref(o), p(xi), p(ui), None, p(xi), p(ui), p(cost), p(it), p(st))
            got = (xi, ui, cost, it, st, cs)
        else:
            r = s.fit(xi, ui, max_iter=max_iter, tol=tol,
                      options=_lib.default_options(max_iter=max_iter, tol=tol, max_trials=max_trials))
            got = (r.x, r.u, r.cost, r.iters, r.status, r.call_status)
        assert got[5] == ref[5]
        for a, b in zip(got[:4], ref[:4]):
            torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
        assert torch.equal(got[4], ref[4])
    if max_iter == 20:
        assert np.array_equal(ref[3].cpu().numpy(), g["fit_iters"])


# -- 9. one cold iteration at batch against the C restatement ----------------------------
def test_chain6_batch128_iteration_vs_c_oracle(gpu):
    """B = 128, T = 20, central differences, gravity on, one fit iteration from cold
    against the C restatement (oracle_chain_iterate: fp64, central differences)."""
    from oracle import cref
    pr = rbd_6dof_problem(gravity=True)
    B, T = 128, 20
    s = ChainSolver(pr, T, B, dtype=F64, linearization="fd")
    u = torch.zeros((B, T, 6), dtype=F64, device="cuda")
    x = s.rollout(dev(rbd_initial_states(B, 6)), u)
    xn, un = torch.empty_like(x), torch.empty_like(u)
    pc = torch.empty((B,), dtype=F64, device="cuda")
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    tr = torch.empty((B,), dtype=torch.int32, device="cuda")
    s._bind()
    s.iterate(x, u, xn, un, None, st, pc, trials=tr, options=_lib.default_options(tol=-1.0))
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and (tr.cpu().numpy() == 1).all()
    d, K, xo, uo, co, tro = cref.chain_iterate(pr, x.cpu().numpy(), u.cpu().numpy())
    assert (tro == 1).all()
    t = TOL["fd"]
    eu, ex, ec = rel(un, uo), rel(xn, xo), rel(pc, co)
    print(f"batch128 fd iteration u {eu:.3e} x {ex:.3e} cost {ec:.3e}")
    assert eu < t["fw"] and ex < t["fw"] and ec < t["fw"], (eu, ex, ec)


# -- 10. API mirror ---------------------------------------------------------------------
def test_chain6_api_mirror(gpu, g6g):
    """ilqr_amd.fit through chain_closures: float64 solves, float32 raises a ValueError
    that names fp64 (no silent promotion, no bare ILQR_ERR_UNSUPPORTED)."""
    import ilqr_amd
    g = g6g
    dyn, cost, fcost = chain_closures(rbd_6dof_problem(gravity=True))
    xo, uo = ilqr_amd.fit(g["x"][0], g["u"][0], dyn, cost, fcost, max_iter=20, tol=1e-6)
    assert uo.dtype == np.float64
    ex, eu = rel(xo, g["fit_x"][0]), rel(uo, g["fit_u"][0])
    print(f"api fit x {ex:.3e} u {eu:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    d, K = ilqr_amd.backward_pass(g["x"][0], g["u"][0], dyn, cost, fcost)
    assert rel(K, g["K"][0]) < TOL["dual"]["gain"] and rel(d, g["d"][0]) < TOL["dual"]["gain"]
    xn, un, c = ilqr_amd.forward_pass(g["x"][0], g["u"][0], None, g["d"][0], g["K"][0], np.inf, dyn, cost, fcost)
    assert rel(xn, g["fw_x"][0]) < TOL["dual"]["fw"] and rel(c, g["fw_cost"][0]) < TOL["dual"]["fw"]
    x32, u32 = g["x"][0].astype(np.float32), g["u"][0].astype(np.float32)
    with pytest.raises(ValueError, match="fp64"):
        ilqr_amd.fit(x32, u32, dyn, cost, fcost, max_iter=2, tol=1e-6)
    with pytest.raises(ValueError, match="fp64"):
        ilqr_amd.backward_pass(x32, u32, dyn, cost, fcost)


def test_chain6_what_stays_closed(gpu, g6g):
    """A six-joint fp32 handle answers dynamics only; six joints run the recursion only."""
    g, pr = g6g, rbd_6dof_problem(gravity=True)
    nb, T = g["u"].shape[:2]
    s32 = ChainSolver(pr, T, nb, dtype=torch.float32)
    assert not s32.iterates
    x, u = dev(g["x"], torch.float32), dev(g["u"], torch.float32)
    xo, uo = torch.empty_like(x), torch.empty_like(u)
    s32._bind()
    o = _lib.default_options(max_iter=2)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert s32.lib.ilqr_chain_fit(s32.h, C.byref(o), p(x), p(u), None, p(xo), p(uo), None, None,
                                  None) == _lib.ERR_UNSUPPORTED
    xn = s32.dynamics(x[:, 0].contiguous(), u[:, 0].contiguous())   # … and still rolls out
    assert rel(xn, g["x"][:, 1]) < 5e-5
    s = solver(g, pr)
    assert s.iterates
    tgt = (C.c_double * 3)(0.1, 0.2, 0.3)
    assert s.lib.ilqr_chain_set_simple_costs(s.h, _lib.CHAIN_COST_SIMPLE, 5, tgt, tgt, 1.0) == _lib.ERR_UNSUPPORTED
    assert s.lib.ilqr_chain_set_dynamics(s.h, _lib.CHAIN_DYN_CLOSED_FORM) == _lib.ERR_UNSUPPORTED
    s.set_dynamics("rnea")
    assert s.dynamics_mode == "rnea"
    s.set_dynamics("auto")
    assert s.dynamics_mode == "rnea"
    assert s.closed_form_error == 0.0   # "not used"


# -- 12. the rare ends of the line search (tests/forward_ends.py) --------------------------
@pytest.mark.parametrize("end", ["forward_exhausted", "forward_nan", "iterate_exhausted", "iterate_nan",
                                 "fit_input_kept"])
def test_chain6_search_ends(gpu, end):
    """An exhausted search and a NaN cost through the 32-lane forward kernels, B = 3, T = 5
    (two trajectories per wave: the last wave half empty): inputs returned bit for bit by
    the 32 lanes' strided copy, trials = max_trials, LS_EXHAUSTED / NAN, and in a fit the
    iteration's input kept."""
    import forward_ends as E
    nb, T = 3, 5
    s = ChainSolver(rbd_6dof_problem(gravity=True), T, nb, dtype=F64)
    rng = np.random.default_rng(46)
    u = dev(rng.uniform(-0.5, 0.5, (nb, T, 6)))
    x = s.rollout(dev(rbd_initial_states(nb, 6, seed0=3)), u)
    if end.startswith("forward"):
        getattr(E, "check_" + end)(
            lambda x, u, d, K, pc, mt: s.forward(x, u, d, K, pc, options=_lib.default_options(max_trials=mt)), x, u)
    elif end.startswith("iterate"):
        def iterate(x, u, xn, un, pc, st, nc, du2, tr, xt, o):
            s._bind()
            s.iterate(x, u, xn, un, pc, st, nc, du2=du2, trials=tr, x_traj=xt, options=o)
        getattr(E, "check_" + end)(iterate, x, u)
    else:
        E.check_fit_input_kept(lambda x, u, xt, mi, tol: s.fit(x, u, max_iter=mi, tol=tol, x_traj=xt), x, u)
