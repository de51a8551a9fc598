"""GPU parity tests of the 2-link arm family (ILQR_PROBLEM_TWO_LINK) through the C ABI.

Reference: test/2_link_example/2_link_helper_functions.jl (dynamics, costs) driven
by src/backward_pass.jl / src/forward_pass.jl. Oracle: oracle.ilqr_oracle.TwoLink
(literal restatement, ForwardDiff restated by oracle.dual), frozen in
tests/golden/twolink_t50.npz (make_golden.py).

Tolerances (fp64): the device evaluates RK4 with FMA contraction, sincos from the
device math library, an LDLᵀ 2×2 solve and the exact step_back rewrite, so it
agrees with the oracle to rounding: rollouts rel 1e-12, gains rel 1e-10, costs rel
1e-12, fit iterates rel 1e-9 (after up to 7 Newton-like iterations), iteration
counts exactly.
"""
import os

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.problems import TwoLinkArm, two_link_closures, two_link_initial_states
from ilqr_amd.solver import Solver
from oracle import ilqr_oracle as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL_ROLL = 1e-12
TOL_GAIN = 1e-10
TOL_COST = 1e-12
TOL_FIT = 1e-9


def rel(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(GOLD, "twolink_t50.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def tl_solver(T, B):
    return Solver(4, 2, T, B, kind=_lib.PROBLEM_TWO_LINK)


def test_tl_rollout(gpu, g):
    """dynamicsf (RK4 functor) rollout from x₀ with u = 0 (animate_2_link.jl:11-16)."""
    nb, T = g["u"].shape[:2]
    s = tl_solver(T, nb)
    x = s.rollout(dev(g["x"][:, 0]), dev(g["u"]))
    assert rel(x, g["x"]) < TOL_ROLL


def test_tl_backward(gpu, g):
    nb, T = g["u"].shape[:2]
    s = tl_solver(T, nb)
    d, K, st = s.backward(dev(g["x"]), dev(g["u"]))
    assert (st.cpu().numpy() == _lib.TRAJ_OK).all()
    for b in range(nb):
        assert rel(d[b], g["d"][b]) < TOL_GAIN, b
        assert rel(K[b], g["K"][b]) < TOL_GAIN, b


def test_tl_forward(gpu, g):
    nb, T = g["u"].shape[:2]
    s = tl_solver(T, nb)
    pc = torch.full((nb,), float("inf"), dtype=torch.float64, device="cuda")
    xn, un, cost, trials, st = s.forward(dev(g["x"]), dev(g["u"]), dev(g["d"]), dev(g["K"]), pc)
    assert (st.cpu().numpy() == _lib.TRAJ_OK).all()
    assert (trials.cpu().numpy() == 1).all()
    assert rel(xn, g["fw_x"]) < TOL_ROLL * 10
    assert rel(un, g["fw_u"]) < TOL_ROLL * 10
    assert rel(cost, g["fw_cost"]) < TOL_COST


def test_tl_forward_line_search_shrinks(gpu, g):
    """prev_cost just above the α=1 cost of a doubled step forces α-halving
    (forward_pass.jl:77-82); the accepted rollout equals the oracle's at that α."""
    nb, T = g["u"].shape[:2]
    x, u = g["x"][:1], g["u"][:1]
    d2 = 6.0 * g["d"][:1]  # overshoot: α = 1 increases the cost
    K = g["K"][:1]
    TL = O.TwoLink
    c0 = O.total_cost_generator(np.zeros_like(x[0]), TL.immediate_cost, TL.final_cost)(x[0], u[0])
    st = {}
    xo, uo, co = O.forward_pass(x[0], u[0], np.zeros_like(x[0]), d2[0], K[0], c0, TL.dynamicsf,
                                TL.immediate_cost, TL.final_cost, max_trials=64, stats=st)
    assert st["trials"] > 1
    s = tl_solver(T, 1)
    xn, un, cost, trials, sts = s.forward(dev(x), dev(u), dev(d2), dev(K),
                                          torch.tensor([c0], dtype=torch.float64, device="cuda"))
    assert int(trials[0]) == st["trials"]
    assert rel(xn[0], xo) < 1e-11 and rel(un[0], uo) < 1e-11
    assert abs(float(cost[0]) - co) / co < TOL_COST


def test_tl_x_traj(gpu, g):
    """x_traj enters only the line-search objective (forward_pass.jl:187-190)."""
    nb, T = g["u"].shape[:2]
    xt = 0.05 * np.random.default_rng(3).standard_normal(g["x"].shape)
    s = tl_solver(T, nb)
    pc = torch.full((nb,), float("inf"), dtype=torch.float64, device="cuda")
    xn, un, cost, _, _ = s.forward(dev(g["x"]), dev(g["u"]), dev(g["d"]), dev(g["K"]), pc,
                                   x_traj=dev(xt))
    TL = O.TwoLink
    for b in range(nb):
        ref = O.total_cost_generator(xt[b], TL.immediate_cost, TL.final_cost)(g["fw_x"][b], g["fw_u"][b])
        assert abs(float(cost[b]) - ref) / ref < 1e-11
    assert rel(xn, g["fw_x"]) < TOL_ROLL * 10  # the rollout itself is unchanged


def test_tl_fit(gpu, g):
    nb, T = g["u"].shape[:2]
    s = tl_solver(T, nb)
    r = s.fit(dev(g["x"]), dev(g["u"]), max_iter=40, tol=1e-6)
    st = r.status.cpu().numpy()
    assert (st == _lib.TRAJ_CONVERGED).all(), st
    assert (r.iters.cpu().numpy() == g["fit_iters"]).all()
    for b in range(nb):
        assert rel(r.x[b], g["fit_x"][b]) < TOL_FIT, b
        assert rel(r.u[b], g["fit_u"][b]) < TOL_FIT, b
        it = int(g["fit_iters"][b])
        assert abs(float(r.cost[b]) - g["fit_cost"][b, it - 1]) / g["fit_cost"][b, it - 1] < 1e-11


def test_tl_api_mirror(gpu, g):
    """iLQR.fit / backward_pass / forward_pass called with the 2-link closures."""
    from ilqr_amd import api
    f, l, lf = two_link_closures()
    d, K = api.backward_pass(g["x"][0], g["u"][0], f, l, lf)
    assert rel(d, g["d"][0]) < TOL_GAIN and rel(K, g["K"][0]) < TOL_GAIN
    xn, un, c = api.forward_pass(g["x"][0], g["u"][0], None, g["d"][0], g["K"][0], np.inf, f, l, lf)
    assert rel(xn, g["fw_x"][0]) < TOL_ROLL * 10 and abs(c - g["fw_cost"][0]) / g["fw_cost"][0] < TOL_COST
    xf, uf = api.fit(g["x"][0], g["u"][0], f, l, lf, max_iter=40, tol=1e-6)
    assert rel(xf, g["fit_x"][0]) < TOL_FIT


def test_tl_config2_batch(gpu):
    """BASELINE config 2: B = 1024 random x₀ (default_rng(b).random(4)), u₀ = 0, T = 50.
    Every trajectory converges with monotone cost; three sampled trajectories match
    the oracle's fit; the device rollout matches the host dynamics."""
    B, T = 1024, 50
    x0 = two_link_initial_states(B)
    s = tl_solver(T, B)
    u0 = torch.zeros((B, T, 2), dtype=torch.float64, device="cuda")
    x = s.rollout(dev(x0), u0)
    f, l, lf = two_link_closures()
    for b in (0, 517):
        assert rel(x[b], O.rollout(x0[b], np.zeros((T, 2)), f)) < TOL_ROLL
    r = s.fit(x, u0, max_iter=100, tol=1e-6)
    st = r.status.cpu().numpy()
    assert (st == _lib.TRAJ_CONVERGED).all(), np.unique(st, return_counts=True)
    xs, us = x.cpu().numpy(), u0.cpu().numpy()
    TL = O.TwoLink
    for b in (0, 517, 1023):
        h = []
        fx, fu = O.fit(xs[b], us[b], TL.dynamicsf, TL.immediate_cost, TL.final_cost, max_iter=100,
                       tol=1e-6, max_trials=64, history=h)
        assert int(r.iters[b]) == len(h), b
        assert rel(r.x[b], fx) < TOL_FIT and rel(r.u[b], fu) < TOL_FIT, b
        assert abs(float(r.cost[b]) - h[-1]["cost"]) / h[-1]["cost"] < 1e-11


def _fit_vs_c_oracle(x, u, max_iter, tol=1e-6):
    """fit_ex on the device against the C restatement's fit (oracle/ilqr_ref.c, symmetrised
    step_back): status and iteration count exactly, the returned iterate at TOL_FIT, the
    cost at 1e-11, and the per-iteration record — every iteration's accepted cost (the
    reference's `Iteration: i  Total Cost: c` line, forward_pass.jl:167) at 1e-11 and its
    line-search trial count exactly."""
    from oracle import cref
    B, T, nu = u.shape
    s = Solver(4, nu, T, B, kind=_lib.PROBLEM_TWO_LINK)
    try:
        r = s.fit(dev(x), dev(u), max_iter=max_iter, tol=tol, history=True)
    finally:
        s.close()
    xo, uo, co, it, st, h = cref.tl_fit(x, u, max_iter=max_iter, tol=tol, symmetrize=True, history=True)
    np.testing.assert_array_equal(r.status.cpu().numpy(), st)
    np.testing.assert_array_equal(r.iters.cpu().numpy(), it)
    assert rel(r.x, xo) < TOL_FIT and rel(r.u, uo) < TOL_FIT, (rel(r.x, xo), rel(r.u, uo))
    assert rel(r.cost, co) < 1e-11
    n = int(it.max())
    hc, ht = r.history["cost"][:n].cpu().numpy(), r.history["trials"][:n].cpu().numpy()
    np.testing.assert_array_equal(ht, h["trials"][:n])
    ran = ht > 0
    assert np.isfinite(hc[ran]).all() and np.isnan(hc[~ran]).all()
    assert float(np.max(np.abs(hc[ran] - h["cost"][:n][ran]) / np.abs(h["cost"][:n][ran]))) < 1e-11
    return r, it, h


def test_tl_animate_workload_vs_c_oracle(gpu):
    """The reference's end-to-end example, animate_2_link.jl:7-25: x₀ = [.1, −.1, 0, 0],
    u₀ = 0, x_init the rollout of u₀, T = 900, tol = 1e-6, max_iter = 10⁶ — fit on the
    device against the C restatement's fit (iteration count, iterates, per-iteration cost
    history), the repaired check of test_iLQR.jl:19 (final_cost(x̄_N) < 0.01), and every
    frame of the animation the reference saved from this run (elbow and tool within
    0.01, under a pixel)."""
    T = 900
    s = tl_solver(T, 1)
    u0 = np.zeros((1, T, 2))
    x = s.rollout(dev(np.array([[0.1, -0.1, 0.0, 0.0]])), dev(u0)).cpu().numpy()
    s.close()
    f, _, _ = two_link_closures()
    assert rel(x[0], O.rollout(np.array([0.1, -0.1, 0.0, 0.0]), u0[0], f)) < TOL_ROLL
    r, it, h = _fit_vs_c_oracle(x, u0, max_iter=10**6)
    assert int(r.status[0]) == _lib.TRAJ_CONVERGED and int(it[0]) >= 3
    th = TwoLinkArm.inverse_kinematics()
    xN = r.x[0, -1].cpu().numpy()
    assert float(np.sum((th - xN[:2]) ** 2)) < 0.01
    # and against the reference's EXECUTED output: the animation this very script saved
    # (figures/iLQR_2_link_quad_4.gif, 91 frames t = 1:10:901; tests/test_reference_gifs.py)
    import test_reference_gifs as G
    z = np.load(G.GOLD, allow_pickle=False)
    de, dt = G.frame_error(r.x[0, ::10, :2].cpu().numpy(), z["quad_4_theta"])
    assert de < G.TOL and dt < G.TOL, (de, dt)


def test_tl_test_iLQR_workload_vs_c_oracle(gpu):
    """test/test_iLQR.jl:8-19 as intended: x_init with every state the random x₀, u_init =
    zeros(100, 2), T = 100, tol = 1e-6 — eight seeded x₀ (default_rng(seed).random(4),
    seeds 0..7) on the device against the C restatement's fit (iteration counts, iterates,
    per-iteration cost history). As written the reference test cannot run: `repeat(x₀,
    101, 1)'` is 1×404, so fit's `@assert N == M + 1` fails, and `max_iter = 1e5` is a
    Float64 that `max_iter::Int64` rejects (the integer 10⁵ is used here). Its check
    final_cost(x̄_N) < 0.01 does NOT hold for this workload: from these x₀ a 1 s horizon
    ends 2.3-8.6 rad² from θ* — the oracle's fit and the device's agree on that, which is
    what is asserted (the check holds for the T = 900 example above)."""
    B, T = 8, 100
    x0 = np.stack([np.random.default_rng(b).random(4) for b in range(B)])
    x = np.repeat(x0[:, None, :], T + 1, axis=1)
    u = np.zeros((B, T, 2))
    r, it, h = _fit_vs_c_oracle(x, u, max_iter=10**5)
    assert (r.status.cpu().numpy() == _lib.TRAJ_CONVERGED).all()
    assert (it >= 8).all()


def test_tl_bad_problem_args(gpu):
    """A TWO_LINK descriptor carrying LQ matrices is rejected (ILQR_ERR_BAD_ARG)."""
    import ctypes as C
    s = tl_solver(10, 2)
    junk = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = _lib.Problem(_lib.PROBLEM_TWO_LINK, 0, junk.data_ptr(), None, None, None, None)
    x = torch.zeros((2, 11, 4), dtype=torch.float64, device="cuda")
    u = torch.zeros((2, 10, 2), dtype=torch.float64, device="cuda")
    d = torch.empty((2, 10, 2), dtype=torch.float64, device="cuda")
    K = torch.empty((2, 10, 2, 4), dtype=torch.float64, device="cuda")
    rc = s.lib.ilqr_backward(s.h, C.byref(p), None, C.c_void_p(x.data_ptr()), C.c_void_p(u.data_ptr()),
                             C.c_void_p(d.data_ptr()), C.c_void_p(K.data_ptr()), None)
    assert rc == _lib.ERR_BAD_ARG


# -- the nu = 1 variant (BASELINE.json configs 1-2: "n_u = 1") -------------------------------
# f₁(x, u) = f(x, [u₁, 0]) on ILQR_PROBLEM_TWO_LINK with nu = 1 (SURVEY.md §0's
# build-defined wrapper: the reference's dynamicsf multiplies inv(M), 2×2, by u,
# 2_link_helper_functions.jl:63-65, so it needs nu = 2). NOT reference-pinned: the
# oracle is the same restatement with the second torque held at 0
# (oracle.ilqr_oracle.TwoLink.dynamicsf_nu1), frozen in tests/golden/twolink_nu1_t50.npz.
@pytest.fixture(scope="module")
def g1():
    z = np.load(os.path.join(GOLD, "twolink_nu1_t50.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def tl1_solver(T, B):
    return Solver(4, 1, T, B, kind=_lib.PROBLEM_TWO_LINK)


def test_tl_nu1_supported(gpu):
    lib = _lib.load()
    assert lib.ilqr_supported(_lib.PROBLEM_TWO_LINK, 4, 1) == 1
    assert lib.ilqr_supported(_lib.PROBLEM_TWO_LINK, 4, 3) == 0


def test_tl_nu1_passes(gpu, g1):
    nb, T = g1["u"].shape[:2]
    s = tl1_solver(T, nb)
    x = s.rollout(dev(g1["x"][:, 0]), dev(g1["u"]))
    assert rel(x, g1["x"]) < TOL_ROLL
    d, K, st = s.backward(dev(g1["x"]), dev(g1["u"]))
    assert (st.cpu().numpy() == _lib.TRAJ_OK).all()
    assert d.shape == (nb, T, 1) and K.shape == (nb, T, 1, 4)
    assert rel(d, g1["d"]) < TOL_GAIN and rel(K, g1["K"]) < TOL_GAIN
    pc = torch.full((nb,), float("inf"), dtype=torch.float64, device="cuda")
    xn, un, cost, trials, st = s.forward(dev(g1["x"]), dev(g1["u"]), dev(g1["d"]), dev(g1["K"]), pc)
    assert (st.cpu().numpy() == _lib.TRAJ_OK).all() and (trials.cpu().numpy() == 1).all()
    assert rel(xn, g1["fw_x"]) < TOL_ROLL * 10 and rel(un, g1["fw_u"]) < TOL_ROLL * 10
    assert rel(cost, g1["fw_cost"]) < TOL_COST


def test_tl_nu1_fit(gpu, g1):
    nb, T = g1["u"].shape[:2]
    s = tl1_solver(T, nb)
    r = s.fit(dev(g1["x"]), dev(g1["u"]), max_iter=40, tol=1e-6)
    assert (r.status.cpu().numpy() == _lib.TRAJ_CONVERGED).all()
    assert (r.iters.cpu().numpy() == g1["fit_iters"]).all()
    assert rel(r.x, g1["fit_x"]) < TOL_FIT and rel(r.u, g1["fit_u"]) < TOL_FIT


def test_tl_nu1_api_mirror(gpu, g1):
    from ilqr_amd import api
    f, l, lf = two_link_closures(nu=1)
    d, K = api.backward_pass(g1["x"][1], g1["u"][1], f, l, lf)
    assert rel(d, g1["d"][1]) < TOL_GAIN and rel(K, g1["K"][1]) < TOL_GAIN
    xf, uf = api.fit(g1["x"][1], g1["u"][1], f, l, lf, max_iter=40, tol=1e-6)
    assert rel(uf, g1["fit_u"][1]) < TOL_FIT
    with pytest.raises(AssertionError):  # a nu = 2 control trajectory for the nu = 1 problem
        api.backward_pass(g1["x"][1], np.zeros((g1["u"].shape[1], 2)), f, l, lf)


def test_tl_nu1_config2_batch(gpu):
    """Config 2 in the nu = 1 shape: B = 1024, T = 50; the fit converges for every
    trajectory and sampled trajectories match the oracle's fit."""
    B, T = 1024, 50
    x0 = two_link_initial_states(B)
    s = tl1_solver(T, B)
    u0 = torch.zeros((B, T, 1), dtype=torch.float64, device="cuda")
    x = s.rollout(dev(x0), u0)
    r = s.fit(x, u0, max_iter=100, tol=1e-6)
    st = r.status.cpu().numpy()
    assert np.isin(st, [_lib.TRAJ_CONVERGED, _lib.TRAJ_LS_EXHAUSTED]).all(), np.unique(st, return_counts=True)
    xs, us = x.cpu().numpy(), u0.cpu().numpy()
    TL = O.TwoLink
    for b in (0, 777):
        if st[b] != _lib.TRAJ_CONVERGED:
            continue
        h = []
        fx, fu = O.fit(xs[b], us[b], TL.dynamicsf_nu1, TL.immediate_cost, TL.final_cost, max_iter=100,
                       tol=1e-6, max_trials=64, history=h)
        assert int(r.iters[b]) == len(h), b
        assert rel(r.u[b], fu) < TOL_FIT, b


# -- the forward's line-search candidate groups and rollout fallback (ilqr_twolink.hip:
# tl_forward_group, rk4_roll) ---------------------------------------------------------------
def _search_case(g, scales):
    """Trajectories of the fixture with δu scaled so the α-halving search needs 1..n
    trials against prev_cost = the cost of the input trajectory."""
    TL = O.TwoLink
    nb = g["u"].shape[0]
    idx = np.arange(len(scales)) % nb
    x, u, K = g["x"][idx], g["u"][idx], g["K"][idx]
    d = g["d"][idx] * np.asarray(scales, dtype=float)[:, None, None]
    pc = np.array([O.total_cost_generator(np.zeros_like(x[i]), TL.immediate_cost, TL.final_cost)(x[i], u[i])
                   for i in range(len(scales))])
    return x, u, d, K, pc


def test_tl_forward_candidates_match_sequential(gpu, g):
    """Four candidates per trajectory side by side (B ≤ 65536) accept the trial the
    sequential search of forward_pass.jl:70-87 accepts: trial counts 1..>4 (rounds past
    the first), rollouts and costs against the oracle."""
    nb, T = g["u"].shape[:2]
    scales = [1, 3, 6, 12, 24, 48, 96, 3, 400]  # trials 1-7 and 9 (tests/golden: 3 trajectories)
    x, u, d, K, pc = _search_case(g, scales)
    s = tl_solver(T, len(scales))
    xn, un, cost, trials, st = s.forward(dev(x), dev(u), dev(d), dev(K), dev(pc))
    assert (st.cpu().numpy() == _lib.TRAJ_OK).all()
    TL = O.TwoLink
    seen = set()
    for i in range(len(scales)):
        so = {}
        xo, uo, co = O.forward_pass(x[i], u[i], np.zeros_like(x[i]), d[i], K[i], pc[i], TL.dynamicsf,
                                    TL.immediate_cost, TL.final_cost, max_trials=64, stats=so)
        assert int(trials[i]) == so["trials"], i
        seen.add(so["trials"])
        assert rel(xn[i], xo) < 1e-11 and rel(un[i], uo) < 1e-11, i
        assert abs(float(cost[i]) - co) / co < TOL_COST, i
    assert max(seen) > 4 and len(seen) >= 4, seen  # first, later and past-the-first-round trials


def test_tl_forward_exhaustion_across_rounds(gpu, g):
    """max_trials = 6 (not a multiple of the 4 candidates): an unreachable prev_cost
    exhausts after trial 6 with the inputs returned; a reachable one accepts."""
    nb, T = g["u"].shape[:2]
    x, u, d, K, pc = _search_case(g, [1, 24])  # the second needs 5 trials
    pc[0] = -1.0  # no rollout has a negative cost
    s = tl_solver(T, 2)
    xn, un, cost, trials, st = s.forward(dev(x), dev(u), dev(d), dev(K), dev(pc), max_trials=6)
    st = st.cpu().numpy()
    assert st[0] == _lib.TRAJ_LS_EXHAUSTED and int(trials[0]) == 6
    assert rel(xn[0], x[0]) == 0.0 and rel(un[0], u[0]) == 0.0
    assert st[1] == _lib.TRAJ_OK and 1 < int(trials[1]) <= 6


def test_tl_forward_wide_batch_equals_grouped(gpu, g):
    """Past B = 65536 the forward runs one lane per trajectory (sequential trials); the
    same trajectories in a small batch (candidate groups) give bit-identical results."""
    nb, T = g["u"].shape[:2]
    scales = [1, 6, 24, 96, 48, 3, 12, 48]
    x, u, d, K, pc = _search_case(g, scales)
    Bw = 65544
    rep = np.arange(Bw) % len(scales)
    sw = tl_solver(T, Bw)
    rw = sw.forward(dev(x[rep]), dev(u[rep]), dev(d[rep]), dev(K[rep]), dev(pc[rep]))
    ss = tl_solver(T, len(scales))
    rs = ss.forward(dev(x), dev(u), dev(d), dev(K), dev(pc))
    for a, b in zip(rw, rs):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        for off in (0, 8 * 1000, Bw - len(scales) - (Bw % len(scales))):
            np.testing.assert_array_equal(a[off:off + len(scales)], b)


def test_tl_rollout_fast_velocity_fallback(gpu):
    """|θ̇₂|·Δt beyond rk4_roll's series range (h > 1/8) redoes the rollout on the
    generic RK4; fast and slow trajectories share waves. Rollouts against the oracle."""
    T = 30
    rng = np.random.default_rng(5)
    x0 = rng.random((64, 4))
    x0[::3, 3] = 40.0 * (rng.random(22) - 0.5) + 30.0  # |θ̇₂| up to 50 rad/s
    x0[1::7, 1] = 1e3 + rng.random(9)                   # large angles (reduction by π/2)
    u = 0.5 * rng.standard_normal((64, T, 2))
    s = tl_solver(T, 64)
    x = s.rollout(dev(x0), dev(u))
    f, _, _ = two_link_closures()
    for b in range(64):
        ref = O.rollout(x0[b], u[b], f)
        assert rel(x[b], ref) < TOL_ROLL * 10, b


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("end", ["forward_exhausted", "forward_nan", "iterate_exhausted", "iterate_nan",
                                 "fit_input_kept"])
def test_tl_search_ends(gpu, nu, end):
    """An exhausted search and a NaN cost (tests/forward_ends.py) through ilqr_forward,
    ilqr_iterate and ilqr_fit of the 2-link family, B = 5, T = 7 (four candidates per
    trajectory: the second wave a quarter full): inputs returned bit for bit, trials =
    max_trials, LS_EXHAUSTED / NAN, and in a fit the iteration's input kept."""
    import forward_ends as E
    nb, T = 5, 7
    s = Solver(4, nu, T, nb, kind=_lib.PROBLEM_TWO_LINK)
    rng = np.random.default_rng(50 + nu)
    x0 = np.concatenate([rng.uniform(-1, 1, (nb, 2)), rng.uniform(-0.5, 0.5, (nb, 2))], axis=1)
    u = dev(rng.uniform(-0.5, 0.5, (nb, T, nu)))
    x = s.rollout(dev(x0), u)
    if end.startswith("forward"):
        getattr(E, "check_" + end)(lambda x, u, d, K, pc, mt: s.forward(x, u, d, K, pc, max_trials=mt), x, u)
    elif end.startswith("iterate"):
        def iterate(x, u, xn, un, pc, st, nc, du2, tr, xt, o):
            s._bind_stream()
            s.iterate(x, u, xn, un, pc, st, du2=du2, trials=tr, x_traj=xt, options=o, new_cost=nc)
        getattr(E, "check_" + end)(iterate, x, u)
    else:
        E.check_fit_input_kept(lambda x, u, xt, mi, tol: s.fit(x, u, x_traj=xt, max_iter=mi, tol=tol), x, u)
