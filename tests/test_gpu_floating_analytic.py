"""GPU tests of the floating-base family's analytic linearisation
(ilqr_floating_set_linearization(h, ILQR_LINEARIZE_ANALYTIC), fb_linearize_analytic_kernel):
the duals' exact Jacobians from δν̇ = M⁻¹(δu − δ[ID(θ, ν, ν̇)]), on the 2Dof_arm and on the
coupled mechanism (tests/closures.py coupled_floating_model, every term non-zero).

The lane map: the primal launch has a lane per point, the tangent launch 21 consecutive lanes
per point (3 and a bit points a wave, 12 and a bit a workgroup); the shapes below are no
multiple of either, put the same points at every place in a wave, and span several
workgroups and, with narrow trial slots, several chunks. Jacobians against oracle.jet at the family's 1e-10; fits against
the closure oracle with exact decisions and the tolerance max(1e-8, 4·S·ε_J) of
tests/test_floating_analytic_stability.py."""
import functools

import numpy as np
import pytest
import torch

from closures import coupled_floating_model, jet_ns, rbd_floating_arm
from ilqr_amd import _lib, api, cache
from ilqr_amd.floating import FloatingDynamics, FloatingSolver, floating_closures, rbd_example_problem
from oracle import jet
from test_floating_analytic_stability import S, oracle_fit, workload
from test_gpu_floating import _problem_of, random_states, rel

pytestmark = pytest.mark.gpu

MECHS = ["2dof_arm", "coupled"]
WORKLOAD_OF = {"2dof_arm": "arm9x60x6", "coupled": "coupled5x50x4"}


@functools.lru_cache(maxsize=None)
def mech(name):
    """(FloatingProblem, the restatement's dynamics) of a mechanism."""
    if name == "2dof_arm":
        return rbd_example_problem(), rbd_floating_arm(jet_ns())[0]
    md = coupled_floating_model()
    return _problem_of(md), rbd_floating_arm(jet_ns(), model=md)[0]


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared workloads are read-only


def points_as(pts_x, pts_u, nb, T):
    """The n = nb·T points laid out as a (nb, T) batch: x (nb, T+1, 16), u (nb, T, 8)."""
    x = np.zeros((nb, T + 1, 16))
    x[:, :T] = pts_x.reshape(nb, T, 16)
    x[:, T] = pts_x[0]
    return x, pts_u.reshape(nb, T, 8).copy()


def linearize(p, x, u, lin):
    s = FloatingSolver(p, u.shape[1], u.shape[0], linearization=lin)
    try:
        assert s.linearization == lin
        A, Bm = s.linearize(cu(x), cu(u))
        torch.cuda.synchronize()
    finally:
        s.close()
    return A.cpu().numpy().reshape(-1, 16, 16), Bm.cpu().numpy().reshape(-1, 16, 8)


@pytest.mark.parametrize("name", MECHS)
def test_ragged_batch_vs_forward_mode(gpu, name, monkeypatch):
    """(B, T) = (5, 5): 25 points are 525 lanes of the tangent launch, no multiple of a wave or
    of a workgroup, and points that straddle both."""
    p, fj = mech(name)
    nb, T = 5, 5
    px, pu = random_states(nb * T, seed=11)
    x, u = points_as(px, pu, nb, T)
    A, Bm = linearize(p, x, u, "analytic")
    Aj, Bj = jet.jacobians(fj, px, pu)
    Ad, Bd = linearize(p, x, u, "dual")
    print(f"{name} 5x5 analytic vs jet A {rel(A, Aj):.3e} B {rel(Bm, Bj):.3e}; "
          f"vs the device's duals A {rel(A, Ad):.3e} B {rel(Bm, Bd):.3e}")
    assert rel(A, Aj) < 1e-10 and rel(Bm, Bj) < 1e-10
    unit = np.zeros((16, 3))
    unit[3:6] = np.eye(3)
    assert all(np.array_equal(a[:, 3:6], unit) for a in A)   # r enters nothing: exactly e_3..e_5
    # four trial slots a trajectory hold 10 of the 25 points' records: three chunks, the same bits
    monkeypatch.setenv("ILQR_FB_CAND", "4")
    Ac, Bc = linearize(p, x, u, "analytic")
    assert np.array_equal(Ac, A) and np.array_equal(Bc, Bm)


@pytest.mark.parametrize("name", MECHS)
def test_placement_does_not_change_the_bits(gpu, name):
    """The same 26 points as (13, 2), (1, 26) and (26, 1): a point's column does not depend
    on where in a wave or a workgroup, or on which trajectory and step, it sits."""
    p, _ = mech(name)
    px, pu = random_states(26, seed=23)
    ref = None
    for nb, T in ((13, 2), (1, 26), (26, 1)):
        got = linearize(p, *points_as(px, pu, nb, T), "analytic")
        if ref is None:
            ref = got
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (nb, T)


@pytest.mark.parametrize("name", MECHS)
def test_several_workgroups_vs_forward_mode(gpu, name):
    """(7, 11): 77 points, 1617 lanes over seven workgroups, angles to ±3, MRP 0.4σ."""
    p, fj = mech(name)
    nb, T = 7, 11
    px, pu = random_states(nb * T, seed=29)
    A, Bm = linearize(p, *points_as(px, pu, nb, T), "analytic")
    Aj, Bj = jet.jacobians(fj, px, pu)
    print(f"{name} 7x11 analytic vs jet A {rel(A, Aj):.3e} B {rel(Bm, Bj):.3e}")
    assert rel(A, Aj) < 1e-10 and rel(Bm, Bj) < 1e-10


def fit_all(s, x, u, max_iter):
    r = s.fit(x, u, max_iter=max_iter, tol=1e-6, history=True)
    return (r.x, r.u, r.cost, r.iters, r.status, r.history["trials"], r.history["cost"])


def same_bits(a, b):
    return all(torch.equal(v, w) or (v.dtype.is_floating_point and
                                     torch.equal(torch.nan_to_num(v, nan=-1.0), torch.nan_to_num(w, nan=-1.0)))
               for v, w in zip(a, b))


@pytest.mark.parametrize("name", MECHS)
def test_mode_switching_on_one_handle(gpu, name):
    """Analytic then dual on one handle: linearize and a 4-iteration fit are bit-equal to a
    fresh dual handle's; the reverse switch to a fresh analytic handle's. The setter's
    refusals on a live handle leave the mode as it was."""
    p, _ = mech(name)
    xw, uw, _ = workload(WORKLOAD_OF[name])
    x, u = cu(xw), cu(uw)
    nb, T = uw.shape[:2]
    fresh = {}
    for lin in ("dual", "analytic"):
        s = FloatingSolver(p, T, nb, linearization=lin)
        try:
            fresh[lin] = (s.linearize(x, u), fit_all(s, x, u, 4))
        finally:
            s.close()
    assert not torch.equal(fresh["dual"][0][0], fresh["analytic"][0][0])   # two roundings
    for first, then in (("analytic", "dual"), ("dual", "analytic")):
        s = FloatingSolver(p, T, nb, linearization=first)
        try:
            a = (s.linearize(x, u), fit_all(s, x, u, 4))
            assert same_bits(a[0], fresh[first][0]) and same_bits(a[1], fresh[first][1])
            s.set_linearization(then)
            assert s.linearization == then
            b = (s.linearize(x, u), fit_all(s, x, u, 4))
            assert same_bits(b[0], fresh[then][0]) and same_bits(b[1], fresh[then][1]), (first, then)
            # refusals: central differences are not this family's, other values are no modes
            assert s.lib.ilqr_floating_set_linearization(s.h, _lib.LINEARIZE_CENTRAL_FD) == _lib.ERR_UNSUPPORTED
            assert b"ilqr_floating_set_linearization" in s.lib.ilqr_floating_last_error()
            for bad in (3, -1, 9):
                assert s.lib.ilqr_floating_set_linearization(s.h, bad) == _lib.ERR_BAD_ARG
            assert s.linearization == then
        finally:
            s.close()


@pytest.mark.parametrize("name", MECHS)
def test_nan_trajectory_stops_alone(gpu, name):
    """A NaN in trajectory 1's x_init: it ends with ILQR_TRAJ_NAN, alone, and every other
    trajectory is bit-equal to the same fit with trajectory 1 replaced by a copy of trajectory 0."""
    p, _ = mech(name)
    xw, uw, _ = workload(WORKLOAD_OF[name])
    nb, T = uw.shape[:2]
    xn, xc = xw.copy(), xw.copy()
    xn[1, 0, 9] = np.nan
    xn[1, 1:] = np.nan
    xc[1] = xw[0]
    uc = uw.copy()
    uc[1] = uw[0]
    s = FloatingSolver(p, T, nb, linearization="analytic")
    try:
        r = s.fit(cu(xn), cu(uw), max_iter=4)
        c = s.fit(cu(xc), cu(uc), max_iter=4)
    finally:
        s.close()
    assert r.call_status == _lib.ERR_NAN
    assert (r.status == _lib.TRAJ_NAN).nonzero().flatten().tolist() == [1]
    keep = [b for b in range(nb) if b != 1]
    assert torch.equal(r.x[keep], c.x[keep]) and torch.equal(r.u[keep], c.u[keep])
    assert torch.equal(r.cost[keep], c.cost[keep]) and torch.equal(r.iters[keep], c.iters[keep])
    assert torch.equal(r.status[keep], c.status[keep])


@pytest.mark.parametrize("name", MECHS)
def test_fit_vs_closure_oracle(gpu, name):
    """arm9x60x6 and coupled5x50x4 from analytic handles against oracle.closure_fit.fit: exact
    iteration counts, statuses and trial history; x, u, cost and the cost history within
    max(1e-8, 4·S·ε_J) — 1e-8 the family's fit tolerance, S the CPU-measured sensitivity of
    the workload to noise in A and B (tests/test_floating_analytic_stability.py), ε_J the rel of
    the device's analytic A and B against oracle.jet on the workload's starting trajectory,
    4 the margin for device rounding being structured, not Gaussian. The formula above 1e-6
    fails outright (a wrong term on the coupled mechanism is orders of magnitude above).

    Measured on an MI355X: ε_J = 3.44e-16 (arm9x60x6) and 5.83e-16 (coupled5x50x4), so
    4·S·ε_J ≤ 6.7e-10 and 3.8e-9 and the tolerance is 1e-8 on every quantity of both workloads;
    the deviations themselves: x 2.0e-13, u 2.0e-13, cost 1.1e-13, history 8.0e-14 (arm) and
    3.8e-13, 4.7e-13, 1.2e-14, 2.7e-14 (coupled)."""
    p, fj = mech(name)
    wl = WORKLOAD_OF[name]
    xw, uw, max_iter = workload(wl)
    nb, T = uw.shape[:2]
    o = oracle_fit(wl)
    x, u = cu(xw), cu(uw)
    s = FloatingSolver(p, T, nb, linearization="analytic")
    try:
        A, Bm = s.linearize(x, u)
        r = s.fit(x, u, max_iter=max_iter, tol=1e-6, history=True)
    finally:
        s.close()
    Aj, Bj = jet.jacobians(fj, xw[:, :T].reshape(-1, 16), uw.reshape(-1, 8))
    eps = max(rel(A.reshape(-1, 16, 16), Aj), rel(Bm.reshape(-1, 16, 8), Bj))
    tol = {k: max(1e-8, 4.0 * S[wl][k] * eps) for k in S[wl]}
    got = {"x": rel(r.x, o["x"]), "u": rel(r.u, o["u"]), "cost": rel(r.cost, o["cost"]),
           "hist": rel(r.history["cost"][:max_iter], o["history"]["cost"])}
    print(f"{wl} eps_J {eps:.3e} tol {tol} measured {got}")
    assert max(tol.values()) <= 1e-6, (eps, tol)
    assert r.iters.tolist() == o["iters"].tolist()
    assert r.status.tolist() == o["status"].tolist()
    assert r.history["trials"][:max_iter].cpu().tolist() == o["history"]["trials"].tolist()
    for k in tol:
        assert got[k] < tol[k], (k, got[k], tol[k])


@pytest.mark.parametrize("name", MECHS)
def test_reference_api_honours_the_mode(gpu, name):
    """ilqr_amd.fit with floating_closures(p, linearization="analytic") is bit-equal to an
    analytic FloatingSolver's fit; a dual and an analytic caller hold a handle each; and
    helpers.linearize_dynamics with an analytic FloatingDynamics is within 1e-10 of jet."""
    from ilqr_amd.helpers import linearize_dynamics
    api.clear_cache()
    p, fj = mech(name)
    xw, uw, _ = workload(WORKLOAD_OF[name])
    nb, T = 2, 30
    x, u = cu(xw[:nb, :T + 1]), cu(uw[:nb, :T])
    try:
        xd, ud = api.fit(x, u, *floating_closures(p), max_iter=4)
        xa, ua = api.fit(x, u, *floating_closures(p, linearization="analytic"), max_iter=4)
        assert cache.size() == 2
        for lin, (xf, uf) in (("dual", (xd, ud)), ("analytic", (xa, ua))):
            s = FloatingSolver(p, T, nb, linearization=lin)
            try:
                r = s.fit(x, u, max_iter=4, tol=1e-6)
            finally:
                s.close()
            assert torch.equal(xf, r.x) and torch.equal(uf, r.u), lin
        da, Ka = api.backward_pass(x, u, *floating_closures(p, linearization="analytic"))
        dd, Kd = api.backward_pass(x, u, *floating_closures(p))
        assert rel(da, dd) < 1e-9 and rel(Ka, Kd) < 1e-9
        px, pu = random_states(6, seed=31)
        AT, BT = linearize_dynamics(px, pu[:5], FloatingDynamics(p, linearization="analytic"))
        AD, _ = linearize_dynamics(px, pu[:5], FloatingDynamics(p))
        Aj, Bj = jet.jacobians(fj, px[:5], pu[:5])
        print(f"{name} linearize_dynamics analytic vs jet A {rel(AT, Aj):.3e} B {rel(BT, Bj):.3e}")
        assert rel(AT, Aj) < 1e-10 and rel(BT, Bj) < 1e-10
        assert rel(AD, Aj) < 1e-10 and not np.array_equal(np.asarray(AT), np.asarray(AD))
    finally:
        api.clear_cache()
