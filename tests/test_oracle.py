"""CPU tests: pin the oracle (CPU restatement of the reference) with known-answer
tests derived from the reference's own tests and algebra, and check the
committed golden vectors and the C restatement against it."""
import json
import os

import numpy as np
import pytest

from ilqr_amd.problems import quadrotor_batch, random_lq_batch
from oracle import cref, dual
from oracle import ilqr_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


# -- AD restatement (ForwardDiff) --------------------------------------------------
def test_dual_ad_matches_analytic_lq_derivatives():
    """ForwardDiff on linear/quadratic closures is exact; so must the restatement be
    (linearize_dynamics :25-40, immediate_cost_quadratization :81-109,
    final_cost_quadratization :134-153)."""
    rng = np.random.default_rng(3)
    n, m = 12, 4
    A, B = rng.standard_normal((n, n)), rng.standard_normal((n, m))
    Q, R, Qf = rng.standard_normal((n, n)), rng.standard_normal((m, m)), rng.standard_normal((n, n))
    f, l, lf = O.lq_closures(A, B, Q, R, Qf)
    x, u = rng.standard_normal(n), rng.standard_normal(m)
    Aad = dual.jacobian(lambda z: f(z, u), x)
    Bad = dual.jacobian(lambda z: f(x, z), u)
    assert np.array_equal(Aad, A) and np.array_equal(Bad, B)
    # strip the analytic shortcut to force the generic AD path
    plain_l = lambda xx, uu: xx @ (Q @ xx) + uu @ (R @ uu)  # noqa: E731
    plain_lf = lambda xx: xx @ (Qf @ xx)  # noqa: E731
    ad = O.immediate_cost_quadratization(x, u, plain_l)
    an = l.quad(x, u)
    for a, b in zip(ad[1:], an[1:]):
        assert rel(a, b) < 1e-14 if np.abs(b).max() > 0 else np.abs(a).max() == 0
    fad = O.final_cost_quadratization(x, plain_lf)
    fan = lf.fquad(x)
    assert rel(fad[1], fan[1]) < 1e-14 and rel(fad[2], fan[2]) < 1e-14


def test_linearisation_of_linear_dynamics_is_exact():
    """Repaired test/test_linearize_dynamics.jl:24-25: for linear f the linearised
    one-step prediction A x + B u equals f(x, u) (the test's 1e-10 bound)."""
    lq, x, u = random_lq_batch(1, 12, 4, 10, seed=5)
    f = lambda xx, uu: lq.A[0] @ xx + lq.B[0] @ uu  # noqa: E731  (no analytic shortcut)
    for t in range(10):
        A, B = O.linearize_dynamics(x[0, t], u[0, t], f)
        pred = A @ x[0, t] + B @ u[0, t]
        assert np.abs(pred - x[0, t + 1]).max() < 1e-10


def test_twolink_constants_and_ik():
    """test/2_link_example/2_link_helper_functions.jl:5-26 constants; values quoted
    in SURVEY.md §8a12 (θ* = (-1.6804522359448377, 1.9714279194962687))."""
    k = json.load(open(os.path.join(GOLD, "twolink_constants.json")))
    assert O.TwoLink.alpha == 0.8333333333333335
    assert O.TwoLink.beta == 0.25000000000000006
    assert abs(O.TwoLink.delta - 1 / 6) < 1e-15
    th = O.TwoLink.inverse_kinematics(O.TwoLink.target_tool_loc)
    assert th[0] == -1.6804522359448377 and th[1] == 1.9714279194962687
    assert th.tolist() == k["theta_star"]
    # forward kinematics of θ* reaches the target tool location
    l1, l2 = O.TwoLink.l1, O.TwoLink.l2
    tip = (l1 * np.cos(th[0]) + l2 * np.cos(th[0] + th[1]), l1 * np.sin(th[0]) + l2 * np.sin(th[0] + th[1]))
    assert np.allclose(tip, O.TwoLink.target_tool_loc, atol=1e-12)


def test_twolink_ad_matches_central_differences():
    TL = O.TwoLink
    rng = np.random.default_rng(1)
    for _ in range(3):
        x, u = rng.random(4), rng.standard_normal(2)
        A, B = O.linearize_dynamics(x, u, TL.dynamicsf)
        e = 1e-6
        Afd = np.stack([(TL.dynamicsf(x + e * np.eye(4)[i], u) - TL.dynamicsf(x - e * np.eye(4)[i], u)) / (2 * e)
                        for i in range(4)], 1)
        Bfd = np.stack([(TL.dynamicsf(x, u + e * np.eye(2)[i]) - TL.dynamicsf(x, u - e * np.eye(2)[i])) / (2 * e)
                        for i in range(2)], 1)
        assert np.abs(A - Afd).max() < 1e-8 and np.abs(B - Bfd).max() < 1e-8


def test_twolink_coriolis_quirk():
    """`for k in length(θ)` (2_link_helper_functions.jl:43) iterates k = 2 only:
    C = ½ θ̇₂ ∂M/∂θ₂ transposed — NOT the physical Coriolis matrix."""
    th, thd = np.array([0.3, 0.7]), np.array([0.5, -1.1])
    C = np.asarray(O.TwoLink.coriolis_matrix(th, thd), dtype=float)
    b, s2 = O.TwoLink.beta, np.sin(0.7)
    exp = np.array([[-b * s2 * thd[1], -0.5 * b * s2 * thd[1]], [-0.5 * b * s2 * thd[1], 0.0]])
    assert np.allclose(C, exp, rtol=0, atol=1e-15)


def test_twolink_fit_decreases_cost_to_a_stationary_point():
    """Repaired test/test_iLQR.jl (broken as written: Float64 max_iter, 1×404
    state matrix): fit from a seeded x₀ with u₀ = 0 terminates by the tol test
    with a monotonically decreasing cost (the @assert at forward_pass.jl:168).
    The test's `final_cost(x̄[end]) < 0.01` does not hold for this oracle at
    T = 100…300 (the running cost dominates); see DESIGN.md §Oracle."""
    TL = O.TwoLink
    T = 100
    x0 = np.random.default_rng(42).random(4)
    x = O.rollout(x0, np.zeros((T, 2)), TL.dynamicsf)
    hist = []
    xf, uf = O.fit(x, np.zeros((T, 2)), TL.dynamicsf, TL.immediate_cost, TL.final_cost,
                   max_iter=200, tol=1e-6, max_trials=60, history=hist)
    c = [h["cost"] for h in hist]
    assert all(b < a for a, b in zip(c, c[1:]))
    assert hist[-1]["du2"] <= 1e-6 and len(hist) < 200
    assert TL.final_cost(xf[-1]) < TL.final_cost(x[-1])


# -- LQ known answers --------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_lq_fit_converges_to_kkt_solution(seed):
    """iLQR's fixed point has δu ≡ 0, i.e. ∇_u J = 0, so fit converges to the exact
    minimiser of the LQ problem independent of μ."""
    lq, x, u = quadrotor_batch(1, T=20, seed0=seed)
    f, l, lf = O.lq_closures(lq.A[0], lq.B[0], lq.Q[0], lq.R[0], lq.Qf[0])
    xf, uf = O.fit(x[0], u[0], f, l, lf, max_iter=50, tol=1e-14, max_trials=60)
    X, U = O.lq_kkt_solution(lq.A[0], lq.B[0], lq.Q[0], lq.R[0], lq.Qf[0], x[0, 0], 20)
    assert rel(uf, U) < 1e-6 and rel(xf, X) < 1e-6


def test_literal_step_back_amplifies_asymmetry():
    """Documents the reference-numerics finding: the literal
    update (backward_pass.jl:270) diverges on the headline instances at T = 100,
    while the symmetrised recursion (identity in exact arithmetic) does not."""
    lq, x, u = quadrotor_batch(1, T=100, seed0=0)
    f, l, lf = O.lq_closures(lq.A[0], lq.B[0], lq.Q[0], lq.R[0], lq.Qf[0])
    d, K = O.backward_pass(x[0], u[0], f, l, lf, symmetrize=True)
    assert np.isfinite(K).all() and np.abs(K).max() < 1e3
    try:
        with np.errstate(all="ignore"):
            dl, Kl = O.backward_pass(x[0], u[0], f, l, lf)
        diverged = not np.isfinite(Kl).all() or rel(Kl, K) > 1e-3
    except (np.linalg.LinAlgError, AssertionError):
        diverged = True
    assert diverged
    # on a short horizon the two agree to rounding
    d20, K20 = O.backward_pass(x[0, :21], u[0, :20], f, l, lf)
    d20s, K20s = O.backward_pass(x[0, :21], u[0, :20], f, l, lf, symmetrize=True)
    assert rel(K20, K20s) < 1e-9


def test_fit_returns_previous_iterate_and_rejects_float_max_iter():
    """forward_pass.jl:171-178: on convergence fit returns the iterate BEFORE the
    update; forward_pass.jl:152: max_iter::Int64 (test_iLQR.jl:4's 1e5 is a TypeError)."""
    lq, x, u = quadrotor_batch(1, T=10, seed0=3)
    f, l, lf = O.lq_closures(lq.A[0], lq.B[0], lq.Q[0], lq.R[0], lq.Qf[0])
    with pytest.raises(TypeError):
        O.fit(x[0], u[0], f, l, lf, max_iter=1e5)
    hist = []
    xf, uf = O.fit(x[0], u[0], f, l, lf, max_iter=50, tol=1e-6, max_trials=60, history=hist)
    # replay: the returned iterate is the input of the last (converging) iteration
    xi, ui, pc = x[0], u[0], np.inf
    for h in hist[:-1]:
        d, K = O.backward_pass(xi, ui, f, l, lf)
        xi, ui, pc = O.forward_pass(xi, ui, np.zeros_like(xi), d, K, pc, f, l, lf)
    assert np.array_equal(xf, xi) and np.array_equal(uf, ui)
    assert hist[-1]["du2"] <= 1e-6 and all(h["du2"] > 1e-6 for h in hist[:-1])


def test_shape_assertions():
    lq, x, u = quadrotor_batch(1, T=5, seed0=0)
    f, l, lf = O.lq_closures(lq.A[0], lq.B[0], lq.Q[0], lq.R[0], lq.Qf[0])
    with pytest.raises(AssertionError):
        O.backward_pass(x[0, :-1], u[0], f, l, lf)   # backward_pass.jl:329


# -- golden vectors and the C restatement --------------------------------------------
def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", ["quad_t16", "quad_t100_sym", "dense_t16", "dense_t64_sym", "dense_xtraj"])
def test_golden_reproduces_and_c_oracle_agrees(name):
    g = _load(name)
    meta = json.loads(str(g["meta"]))
    from ilqr_amd.problems import LQBatch
    lq = LQBatch(g["A"], g["B"], g["Q"], g["R"], g["Qf"])
    sym = meta["symmetrize"]
    xt = g.get("xtraj")
    # numpy oracle reproduces the committed vectors (first trajectory)
    f, l, lf = O.lq_closures(lq.A[0], lq.B[0], lq.Q[0], lq.R[0], lq.Qf[0])
    d, K = O.backward_pass(g["x"][0], g["u"][0], f, l, lf, symmetrize=sym)
    assert rel(K, g["K"][0]) < 1e-12 and rel(d, g["d"][0]) < 1e-12
    # C restatement agrees with the fixtures for the whole batch
    dc, Kc, st = cref.lq_backward(lq, g["x"], g["u"], symmetrize=sym)
    assert (st == 0).all()
    assert rel(Kc, g["K"]) < 1e-9 and rel(dc, g["d"]) < 1e-9
    xn, un, c, tr = cref.lq_forward(lq, g["x"], g["u"], xt, g["d"], g["K"], np.inf)
    assert rel(xn, g["fw_x"]) < 1e-10 and rel(un, g["fw_u"]) < 1e-10
    assert rel(c, g["fw_cost"]) < 1e-11 and np.array_equal(tr, g["fw_trials"])
    xo, uo, co, it, st = cref.lq_fit(lq, g["x"], g["u"], x_traj=xt, max_iter=meta["fit_max_iter"],
                                     tol=meta["tol"], symmetrize=sym)
    assert np.array_equal(it, g["fit_iters"])
    assert rel(uo, g["fit_u"]) < 1e-8 and rel(xo, g["fit_x"]) < 1e-8


def test_golden_twolink_reproduces():
    g = _load("twolink_t50")
    TL = O.TwoLink
    d, K = O.backward_pass(g["x"][0], g["u"][0], TL.dynamicsf, TL.immediate_cost, TL.final_cost)
    assert rel(K, g["K"][0]) < 1e-12 and rel(d, g["d"][0]) < 1e-12


def test_c_oracle_twolink_agrees_with_golden():
    """The C restatement's 2-link path (dual-number AD, oracle/ilqr_ref.c) against
    the Python oracle's frozen fixture: backward, forward and fit."""
    g = _load("twolink_t50")
    d, K, st = cref.tl_backward(g["x"], g["u"])
    assert (st == 0).all() and rel(d, g["d"]) < 1e-12 and rel(K, g["K"]) < 1e-12
    xn, un, c, tr = cref.tl_forward(g["x"], g["u"], None, g["d"], g["K"], np.inf)
    assert (tr == 1).all() and rel(xn, g["fw_x"]) < 1e-13 and rel(un, g["fw_u"]) < 1e-13
    assert rel(c, g["fw_cost"]) < 1e-14
    xo, uo, co, it, st = cref.tl_fit(g["x"], g["u"], max_iter=40)
    assert np.array_equal(it, g["fit_iters"]) and (st == 1).all()
    assert rel(xo, g["fit_x"]) < 1e-12 and rel(uo, g["fit_u"]) < 1e-12


def test_c_oracle_twolink_nu1_agrees_with_golden():
    """The C restatement's nu = 1 variant (f(x, [u₁, 0])) against the Python oracle's
    twolink_nu1_t50 fixture (TwoLink.dynamicsf_nu1): backward, forward and fit."""
    g = _load("twolink_nu1_t50")
    d, K, st = cref.tl_backward(g["x"], g["u"])
    assert d.shape[-1] == 1 and K.shape[-2:] == (1, 4)
    assert (st == 0).all() and rel(d, g["d"]) < 1e-12 and rel(K, g["K"]) < 1e-12
    xn, un, c, tr = cref.tl_forward(g["x"], g["u"], None, g["d"], g["K"], np.inf)
    assert (tr == 1).all() and rel(xn, g["fw_x"]) < 1e-13 and rel(un, g["fw_u"]) < 1e-13
    assert rel(c, g["fw_cost"]) < 1e-14
    xo, uo, co, it, st = cref.tl_fit(g["x"], g["u"], max_iter=40)
    assert np.array_equal(it, g["fit_iters"]) and (st == 1).all()
    assert rel(xo, g["fit_x"]) < 1e-12 and rel(uo, g["fit_u"]) < 1e-12


# -- the line search off its default options ------------------------------------------
def _repeated_product(alpha0, shrink, trial):
    """α of trial j: alpha0 multiplied by shrink j − 1 times in turn (forward_pass.jl:82)."""
    a = alpha0
    for _ in range(trial - 1):
        a *= shrink
    return a


def _lq_search_case():
    g = np.load(os.path.join(GOLD, "quad_t16.npz"), allow_pickle=False)
    from ilqr_amd.problems import LQBatch
    lq = LQBatch(g["A"], g["B"], g["Q"], g["R"], g["Qf"])
    nb = lq.batch
    scales = np.array([1, 3, 6, 12, 24, 48, 96, 400], dtype=float)[np.arange(nb) % 8]
    x, u, K = g["x"], g["u"], g["K"]
    d = g["d"] * scales[:, None, None]
    cl = [O.lq_closures(lq.A[b], lq.B[b], lq.Q[b], lq.R[b], lq.Qf[b]) for b in range(nb)]
    pc = np.array([O.total_cost_generator(np.zeros_like(x[b]), cl[b][1], cl[b][2])(x[b], u[b]) for b in range(nb)])
    py = lambda b, **kw: O.forward_pass(x[b], u[b], np.zeros_like(x[b]), d[b], K[b], pc[b], *cl[b], **kw)  # noqa: E731
    c = lambda **kw: cref.lq_forward(lq, x, u, None, d, K, kw.pop("prev_cost", pc), **kw)  # noqa: E731
    return nb, py, c


def _tl_search_case(nu):
    g = np.load(os.path.join(GOLD, "twolink_t50.npz" if nu == 2 else "twolink_nu1_t50.npz"), allow_pickle=False)
    TL = O.TwoLink
    f = TL.dynamicsf if nu == 2 else TL.dynamicsf_nu1
    scales = np.array([1, 3, 6, 12, 24, 48, 96, 3, 400], dtype=float)   # test_gpu_twolink's search case
    idx = np.arange(len(scales)) % g["u"].shape[0]
    x, u, K = g["x"][idx], g["u"][idx], g["K"][idx]
    d = g["d"][idx] * scales[:, None, None]
    pc = np.array([O.total_cost_generator(np.zeros_like(x[b]), TL.immediate_cost, TL.final_cost)(x[b], u[b])
                   for b in range(len(idx))])
    py = lambda b, **kw: O.forward_pass(x[b], u[b], np.zeros_like(x[b]), d[b], K[b], pc[b], f,  # noqa: E731
                                        TL.immediate_cost, TL.final_cost, **kw)
    c = lambda **kw: cref.tl_forward(x, u, None, d, K, kw.pop("prev_cost", pc), **kw)  # noqa: E731
    return len(idx), py, c


@pytest.mark.parametrize("case", ["lq", "tl_nu2", "tl_nu1"])
def test_forward_pass_off_default_options_numpy_vs_c(case):
    """forward_pass at alpha0 = 0.9, shrink = 0.7 (no step a power of two): the numpy and the C
    restatement accept at the same trial and agree on the rollout to 1e-12, and the α of
    trial j is alpha0 multiplied by shrink j − 1 times in turn, bit for bit — the numpy
    oracle's by its own record, the C oracle's by its accepted rollout being, bit for bit,
    the one trial it runs from that product as alpha0 (a one-ulp change of α moves ū)."""
    a0, sh = 0.9, 0.7
    nb, py, c = {"lq": _lq_search_case, "tl_nu2": lambda: _tl_search_case(2),
                 "tl_nu1": lambda: _tl_search_case(1)}[case]()
    xc, uc, cc, trc = c(alpha0=a0, shrink=sh)
    seen = set()
    for b in range(nb):
        st = {}
        xo, uo, co = py(b, max_trials=64, alpha0=a0, shrink=sh, stats=st)
        assert st["trials"] == trc[b], (b, st, trc[b])
        assert st["alpha"] == _repeated_product(a0, sh, st["trials"]), (b, st)
        assert rel(xc[b], xo) < 1e-12 and rel(uc[b], uo) < 1e-12 and abs(cc[b] - co) <= 1e-12 * abs(co), b
        seen.add(int(trc[b]))
    assert len(seen) >= 4 and max(seen) > 4, seen
    differ = 0
    for j in sorted(seen):
        aj = _repeated_product(a0, sh, j)
        differ += aj != a0 * sh ** (j - 1)
        x1, u1, c1, tr1 = c(alpha0=aj, shrink=sh, max_trials=1, prev_cost=np.inf)
        at = trc == j
        assert (tr1[at] == 1).all()   # (an overshooting trajectory's early trials may cost NaN)
        assert np.array_equal(x1[at], xc[at]) and np.array_equal(u1[at], uc[at]) and np.array_equal(c1[at], cc[at]), j
    assert differ > 0   # the product and the power disagree somewhere: the cases tell them apart


def test_oracle_fits_take_the_search_options():
    """alpha0 and shrink reach the fits: the C LQ and 2-link fits and the numpy fit at
    (0.9, 0.7) agree on iteration and trial counts, and differ from the default fit."""
    lq, x, u = random_lq_batch(3, 12, 4, 9, seed=2)
    xo, uo, co, it, st = cref.lq_fit(lq, x, u, max_iter=4, tol=-1.0, mu=0.05, symmetrize=True, alpha0=0.9, shrink=0.7)
    xd, ud, _, _, _ = cref.lq_fit(lq, x, u, max_iter=4, tol=-1.0, mu=0.05, symmetrize=True)
    assert not np.array_equal(uo, ud)
    for b in range(3):
        h = []
        xp, up = O.fit(x[b], u[b], *O.lq_closures(lq.A[b], lq.B[b], lq.Q[b], lq.R[b], lq.Qf[b]), max_iter=4,
                       tol=-1.0, mu=0.05, symmetrize=True, max_trials=64, history=h, alpha0=0.9, shrink=0.7)
        assert len(h) == it[b] and rel(up, uo[b]) < 1e-9
        for e in h:
            assert e["alpha"] == _repeated_product(0.9, 0.7, e["trials"])
    g = np.load(os.path.join(GOLD, "twolink_t50.npz"), allow_pickle=False)
    r = cref.tl_fit(g["x"], g["u"], max_iter=3, tol=-1.0, symmetrize=True, history=True, alpha0=0.9, shrink=0.7)
    TL = O.TwoLink
    for b in range(g["u"].shape[0]):
        h = []
        xp, up = O.fit(g["x"][b], g["u"][b], TL.dynamicsf, TL.immediate_cost, TL.final_cost, max_iter=3, tol=-1.0,
                       symmetrize=True, max_trials=64, history=h, alpha0=0.9, shrink=0.7)
        assert [e["trials"] for e in h] == r[5]["trials"][:, b].tolist() and rel(up, r[1][b]) < 1e-9


def test_option_sets_tell_the_products_apart():
    """The premise of tests/test_gpu_options.py: at (0.9, 0.7) and (1.5, 0.6) the repeated product
    differs from alpha0·shrink^k and from its own rounding through float in most of 41 trials, and at
    the defaults in none."""
    for (a0, sh), least in (((0.9, 0.7), 20), ((1.5, 0.6), 20), ((1.0, 0.5), 0)):
        rp = np.array([_repeated_product(a0, sh, j) for j in range(1, 42)])
        n_pow = int((rp != np.array([a0 * sh ** (j - 1) for j in range(1, 42)])).sum())
        n_f32 = int((rp != rp.astype(np.float32).astype(np.float64)).sum())
        assert (n_pow >= least and n_f32 >= least) if least else (n_pow == 0 and n_f32 == 0), (a0, sh, n_pow, n_f32)
