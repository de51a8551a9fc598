"""ILQR_LINEARIZE_ANALYTIC (chain_linearize_analytic_kernel) on the MI355X, for 4, 5, 6 and 7
joints on ilqr_amd.chain.coupled_chain_problem(n): the exact Jacobians from
δq̈ = M⁻¹(δτ − δ[ID(q, q̇, q̈)]), a point's 3n directions on consecutive lanes of one wave
(5, 4, 3, 3 points per wave), the stage's primal exchanged through a wave-private LDS region.

Fixtures: chain{4,5,7}c_t16, chain6c_t24, their _cases and chain{n}ctask_euc (the numpy
oracle's output). Tolerances: the dual mode's (test_gpu_chain6.py TOL["dual"], FIT_TOL,
COST_TOL; the task suite's for the task fit), imported, not restated. Every test prints its
measured errors."""
import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver, rbd_2dof_problem
from test_gpu_chain6 import COST_TOL, FIT_TOL, TOL, chain_fit_replay, dev, inf, rel
from test_gpu_chain6_task import COST_TOL as TASK_COST_TOL
from test_gpu_chain6_task import FIT_TOL as TASK_FIT_TOL
from test_gpu_chainN import load, model, problem, set_costs

pytestmark = pytest.mark.gpu
F64 = torch.float64
NJ = [4, 5, 6, 7]
T_OF = {4: 16, 5: 16, 6: 24, 7: 16}
SENT = -12345.0


def joint_fixture(n):
    g = dict(load(f"chain{n}c_t{T_OF[n]}"))
    g.update({k: v for k, v in load(f"chain{n}c_cases_t{T_OF[n]}").items() if k != "meta"})
    return g


def solver(n, g, lin="analytic", simple=None):
    s = ChainSolver(problem(n), g["u"].shape[1], g["u"].shape[0], dtype=F64, linearization=lin)
    assert s.iterates
    if simple is not None:
        set_costs(s, simple)
    return s


def random_xu(n, nb, Tr, seed=61):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-2, 2, (nb, Tr + 1, n)), rng.uniform(-1, 1, (nb, Tr + 1, n))], axis=2)
    return x, rng.uniform(-5, 5, (nb, Tr, n))


def against_oracle(n, nb, Tr, tag):
    x, u = random_xu(n, nb, Tr)
    Ar, Br = model(n).linearize(x[:, :Tr].reshape(-1, 2 * n), u.reshape(-1, n))
    out = {}
    for lin in ("analytic", "dual"):
        s = ChainSolver(problem(n), Tr, nb, dtype=F64, linearization=lin)
        A, B = s.linearize(dev(x), dev(u))
        out[lin] = A.reshape(-1, 2 * n, 2 * n), B.reshape(-1, 2 * n, n)
        s.close()
    A, B = out["analytic"]
    ea, eb, eq = rel(A, Ar), rel(B, Br), rel(A[:, n:, :n], Ar[:, n:, :n])
    print(f"chain{n} analytic {tag} A {ea:.3e} B {eb:.3e} A[{n}:, :{n}] {eq:.3e}; "
          f"to the device's dual mode A {rel(A, out['dual'][0]):.3e} B {rel(B, out['dual'][1]):.3e}")
    assert ea < TOL["dual"]["AB"] and eb < TOL["dual"]["AB"], (ea, eb)
    assert eq < 1e-9, eq


# -- a. ragged linearisation ----------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_analytic_linearize_ragged(gpu, n):
    """11 × 2 = 22 points: no multiple of the 5, 4 or 3 points of a wave, so the last wave is
    part idle and its lanes past the last point clamp their reads and skip the store."""
    against_oracle(n, 11, 2, "ragged")


# -- b. placement independence --------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_analytic_placement_independent(gpu, n):
    """The same 22 points as (B, T) = (11, 2), (1, 22) and (22, 1): A and B of a point do not
    depend on the wave, the place in the wave or the neighbours it has, bit for bit."""
    xp, up = random_xu(n, 22, 1, seed=62)
    xp, up = xp[:, 0], up[:, 0]
    got = []
    for nb, Tr in ((11, 2), (1, 22), (22, 1)):
        x = np.zeros((nb, Tr + 1, 2 * n))
        x[:, :Tr] = xp.reshape(nb, Tr, 2 * n)
        s = ChainSolver(problem(n), Tr, nb, dtype=F64, linearization="analytic")
        A, B = s.linearize(dev(x), dev(up.reshape(nb, Tr, n)))
        got.append((A.reshape(22, 2 * n, 2 * n).clone(), B.reshape(22, 2 * n, n).clone()))
        s.close()
    assert bool(torch.isfinite(got[0][0]).all()) and float(got[0][1].abs().max()) > 0
    for A, B in got[1:]:
        assert torch.equal(A, got[0][0]) and torch.equal(B, got[0][1])


# -- c. several workgroups, a partial last one ----------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_analytic_linearize_several_workgroups(gpu, n):
    """64 × 9 = 576 points: 29, 36, 48, 48 workgroups of 20, 16, 12, 12 points, the last partial
    (576 = 28·20 + 16) or, at 16 and 12, full — with T = 9 trajectories straddle waves."""
    against_oracle(n, 64, 9, "64x9")


# -- d. fixture parity ----------------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_analytic_linearize_backward_forward(gpu, n):
    """linearize, backward (statuses 0) and forward from the device's own gains (one trial)
    against the fixture, at the dual mode's tolerances."""
    g, t = joint_fixture(n), TOL["dual"]
    s = solver(n, g)
    x, u = dev(g["x"]), dev(g["u"])
    A, B = s.linearize(x, u)
    ea, eb = rel(A, g["A"]), rel(B, g["B"])
    d, K, st = s.backward(x, u)
    ek, ed = rel(K, g["K"]), rel(d, g["d"])
    xn, un, c, tr, fst = s.forward(x, u, d, K, inf(u.shape[0]))
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(c, g["fw_cost"])
    print(f"chain{n}c[analytic] A {ea:.3e} B {eb:.3e} K {ek:.3e} d {ed:.3e} fw x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ea < t["AB"] and eb < t["AB"], (ea, eb)
    assert (st.cpu().numpy() == 0).all()
    assert ek < t["gain"] and ed < t["gain"], (ek, ed)
    assert (tr.cpu().numpy() == 1).all() and (fst.cpu().numpy() == 0).all()
    assert ex < t["fw"] and eu < t["fw"] and ec < t["fw"], (ex, eu, ec)


# -- e. iterate and fit ---------------------------------------------------------------------
def iterate(s, x, u, status, prev_cost=None):
    nb = u.shape[0]
    xn, un = torch.full_like(x, SENT), torch.full_like(u, SENT)
    nc = torch.full((nb,), SENT, dtype=F64, device="cuda")
    du2 = torch.full((nb,), SENT, dtype=F64, device="cuda")
    tr = torch.full((nb,), -7, dtype=torch.int32, device="cuda")
    st = torch.tensor(status, dtype=torch.int32, device="cuda")
    s._bind()
    s.iterate(x, u, xn, un, prev_cost, st, nc, du2=du2, trials=tr, options=_lib.default_options(tol=-1.0))
    torch.cuda.synchronize()
    return xn, un, nc, du2, tr, st


@pytest.mark.parametrize("n", NJ)
def test_analytic_iterate(gpu, n):
    """ilqr_chain_iterate from cold: the fixture's forward pass, Σδu² and one trial."""
    g = joint_fixture(n)
    s = solver(n, g)
    x, u = dev(g["x"]), dev(g["u"])
    xn, un, nc, du2, tr, st = iterate(s, x, u, [0] * u.shape[0])
    assert (st.cpu().numpy() == 0).all() and (tr.cpu().numpy() == 1).all()
    t = TOL["dual"]["fw"]
    ex, eu, ec = rel(xn, g["fw_x"]), rel(un, g["fw_u"]), rel(nc, g["fw_cost"])
    e2 = rel(du2, ((g["fw_u"] - g["u"]) ** 2).sum(axis=(1, 2)))
    print(f"chain{n}[analytic] iterate x {ex:.3e} u {eu:.3e} cost {ec:.3e} du2 {e2:.3e}")
    assert ex < t and eu < t and ec < t and e2 < t, (ex, eu, ec, e2)


@pytest.mark.parametrize("n", NJ)
def test_analytic_fit(gpu, n):
    """fit: the fixture's iteration counts and statuses exactly, the iterates and the last cost;
    and the fit is its iterations — an ilqr_chain_iterate replay, bit for bit."""
    g = joint_fixture(n)
    s = solver(n, g)
    x0, u0 = dev(g["x"]), dev(g["u"])
    r = s.fit(x0.clone(), u0.clone(), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"chain{n}c[analytic] fit iters {r.iters.tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < FIT_TOL and eu < FIT_TOL, (ex, eu)
    assert ec < COST_TOL, ec
    ref = chain_fit_replay(s, x0, u0, 20, 1e-6, None)
    assert r.call_status == ref[5]
    for a, b in zip((r.x, r.u, r.cost, r.iters), ref[:4]):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(r.status, ref[4])


# -- f. task costs --------------------------------------------------------------------------
@pytest.mark.parametrize("n", NJ)
def test_analytic_task_fit(gpu, n):
    """A fit under the task costs (the terminal tiles beside the analytic A and B)."""
    g = load(f"chain{n}ctask_euc_t{T_OF[n]}")
    s = solver(n, g, simple=g["meta"]["simple"])
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=20, tol=1e-6)
    assert r.call_status == _lib.OK
    assert np.array_equal(r.iters.cpu().numpy(), g["fit_iters"]), (r.iters, g["fit_iters"])
    assert np.array_equal(r.status.cpu().numpy(), g["fit_status"])
    ex, eu = rel(r.x, g["fit_x"]), rel(r.u, g["fit_u"])
    last = g["fit_cost"][np.arange(len(g["fit_iters"])), g["fit_iters"] - 1]
    ec = rel(r.cost, last)
    print(f"chain{n}ctask_euc[analytic] fit iters {r.iters.tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < TASK_FIT_TOL and eu < TASK_FIT_TOL, (ex, eu)
    assert ec < TASK_COST_TOL, ec


# -- g, h. trajectories that share a wave ---------------------------------------------------
def three_short(n):
    """Three trajectories of T = 7 steps from the fixture: trajectory 1's points 7..13 share
    a wave with trajectory 0's or 2's at every joint count (waves of 5, 4, 3 points)."""
    g = joint_fixture(n)
    idx = np.arange(3) % g["u"].shape[0]
    x, u = g["x"][idx, :8].copy(), g["u"][idx, :7].copy()
    x[2, :, :n] += 0.01          # three different trajectories at six joints too
    s = ChainSolver(problem(n), 7, 3, dtype=F64, linearization="analytic")
    return s, dev(x), dev(u)


@pytest.mark.parametrize("n", NJ)
def test_analytic_stopped_trajectory(gpu, n):
    """status [0, LS_EXHAUSTED, 0] into iterate: trajectory 1's outputs untouched, 0 and 2
    bit-equal to the all-OK run."""
    s, x, u = three_short(n)
    ref = iterate(s, x, u, [0, 0, 0])
    assert (ref[5].cpu().numpy() == 0).all()
    got = iterate(s, x, u, [0, _lib.TRAJ_LS_EXHAUSTED, 0])
    assert got[5].cpu().numpy().tolist() == [0, _lib.TRAJ_LS_EXHAUSTED, 0]
    for a in got[:4]:
        assert bool((a[1] == SENT).all())
    assert got[4][1].item() == -7
    for a, b in zip(got[:5], ref[:5]):
        assert torch.equal(a[[0, 2]], b[[0, 2]])


@pytest.mark.parametrize("n", NJ)
def test_analytic_nan_trajectory(gpu, n):
    """A NaN in every state of trajectory 1: it ends ILQR_TRAJ_NAN as with dual numbers, and
    nothing leaks to the points of trajectories 0 and 2 that share its waves."""
    s, x, u = three_short(n)
    ref = iterate(s, x, u, [0, 0, 0])
    xb = x.clone()
    xb[1, :, 1] = float("nan")
    got = iterate(s, xb, u, [0, 0, 0])
    assert got[5].cpu().numpy().tolist() == [0, _lib.TRAJ_NAN, 0]
    sd = ChainSolver(problem(n), 7, 3, dtype=F64, linearization="dual")
    assert iterate(sd, xb, u, [0, 0, 0])[5].cpu().numpy().tolist() == [0, _lib.TRAJ_NAN, 0]
    for a, b in zip(got[:5], ref[:5]):
        assert torch.equal(a[[0, 2]], b[[0, 2]])
    A, B = s.linearize(xb, u)
    Ar, Br = s.linearize(x, u)
    assert torch.equal(A[[0, 2]], Ar[[0, 2]]) and torch.equal(B[[0, 2]], Br[[0, 2]])
    assert bool(torch.isnan(A[1]).any())


# -- i. refusals ----------------------------------------------------------------------------
def test_analytic_refusals(gpu):
    with pytest.raises(_lib.IlqrError) as e:
        ChainSolver(rbd_2dof_problem(), 8, 2, dtype=F64, linearization="analytic")
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.IlqrError) as e:
        ChainSolver(problem(6), 8, 2, dtype=torch.float32, linearization="analytic")
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(KeyError):
        ChainSolver(problem(6), 8, 2, dtype=F64, linearization="exact")
