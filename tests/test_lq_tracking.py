"""The consistent tracking mode of the LQ family on the CPU: the checker (tests/tracking.py)
against the condensed-QP answer, why the mode exists (today's semantics miss that answer),
and the new entry points' argument validation — no GPU needed.

Inputs: quadrotor_batch(5, T=9), random_lq_batch(5, 12, 4, 9, seed=3) and
random_lq_batch(5, 7, 3, 9, seed=4), x_traj = 0.5·default_rng(7).standard_normal(x.shape).
Measured there: one μ = 0 iteration of track_fit lands on the KKT answer within 8.5e-13,
2.1e-14 and 3.7e-15 (max |u − u*| / max |u*|); the bound is 1e-10.
"""
import ctypes as C

import numpy as np
import pytest

import tracking
from ilqr_amd import _lib
from oracle import cref

CASES = ["quad", "dense", "pad"]


@pytest.mark.parametrize("name", CASES)
def test_checker_one_newton_step_is_the_kkt_answer(name):
    """μ = 0: the backward pass is exact Newton on a quadratic, α = 1 is accepted from
    prev_cost = Inf, so one iteration is the minimiser."""
    lq, x, u, xt = tracking.case(name)
    r = tracking.track_fit(lq, x, u, xt, max_iter=1, mu=0.0)
    X, U = tracking.track_kkt(lq, x[:, 0], u.shape[1], xt)
    print(name, "rel u", tracking.rel(r["u"], U), "rel x", tracking.rel(r["x"], X))
    assert (r["trials"][0] == 1).all()
    assert tracking.rel(r["u"], U) < 1e-10
    assert tracking.rel(r["x"], X) < 1e-10


@pytest.mark.parametrize("name", CASES)
def test_checker_converges_to_the_kkt_answer_at_default_mu(name):
    """μ = 0.01 only damps the steps: the fixed point (δu ≡ 0) is still ∇J = 0. The fit stops
    at Σδu² ≤ tol = 1e-12, i.e. |δu| ≤ 1e-6 a step from it; the bound is 1e-5 relative to
    max |u*| ≥ 0.1 of these inputs."""
    lq, x, u, xt = tracking.case(name)
    r = tracking.track_fit(lq, x, u, xt, tol=1e-12)
    X, U = tracking.track_kkt(lq, x[:, 0], u.shape[1], xt)
    assert np.isin(r["status"], (tracking.CONVERGED, tracking.LS_EXHAUSTED)).all(), r["status"]
    assert np.abs(U).max() >= 0.1
    assert tracking.rel(r["u"], U) < 1e-5


@pytest.mark.parametrize("name", CASES)
def test_forward_only_semantics_miss_the_kkt_answer(name):
    """The reference's behaviour, kept as the default: the recursion differentiates the
    regulator's cost while the line search measures the tracking cost, so a fit with an
    x_traj ends far from the tracking optimum: ‖u − u*‖₂ / ‖u*‖₂ over the batch is 0.93, 0.53
    and 0.68 on these inputs (the bound, 0.5, is the issue's; in the max norm the same fits
    are 0.79, 0.31 and 0.41 away)."""
    lq, x, u, xt = tracking.case(name)
    _, uo, _, _, st = cref.lq_fit(lq, x, u, xt, symmetrize=True)
    _, U = tracking.track_kkt(lq, x[:, 0], u.shape[1], xt)
    print(name, "forward-only rel2 u", tracking.rel2(uo, U), "max-norm", tracking.rel(uo, U), "status", st)
    assert tracking.rel2(uo, U) > 0.5


def test_checker_without_a_reference_is_the_plain_restatement():
    lq, x, u, _ = tracking.case("dense")
    d, K, _ = tracking.track_backward(lq, x, u, None)
    d0, K0, _ = cref.lq_backward(lq, x, u, symmetrize=True)
    np.testing.assert_array_equal(d, d0)
    np.testing.assert_array_equal(K, K0)
    r = tracking.track_fit(lq, x, u, None, max_iter=3)
    xo, uo, co, it, st = cref.lq_fit(lq, x, u, None, max_iter=3, symmetrize=True)
    np.testing.assert_array_equal(r["x"], xo)
    np.testing.assert_array_equal(r["u"], uo)
    np.testing.assert_array_equal(r["iters"], it)
    np.testing.assert_array_equal(r["status"], st)


def test_tracking_argument_validation_needs_no_gpu():
    lib = _lib.load()
    # a NULL handle or an unknown mode: ILQR_ERR_BAD_ARG before any device call
    assert lib.ilqr_set_tracking(None, _lib.TRACK_CONSISTENT) == _lib.ERR_BAD_ARG
    assert lib.ilqr_set_tracking(None, 7) == _lib.ERR_BAD_ARG
    assert lib.ilqr_get_tracking(None) == -1
    assert lib.ilqr_multi_set_tracking(None, _lib.TRACK_CONSISTENT) == _lib.ERR_BAD_ARG
    o = _lib.default_options()
    p = _lib.Problem(_lib.PROBLEM_LQ, 0, None, None, None, None, None)
    assert lib.ilqr_backward_tracking(None, C.byref(p), C.byref(o), None, None, None, None, None,
                                      None) == _lib.ERR_BAD_ARG
    assert lib.ilqr_backward_tracking(None, None, None, None, None, None, None, None, None) == _lib.ERR_BAD_ARG
    assert (_lib.TRACK_FORWARD_ONLY, _lib.TRACK_CONSISTENT) == (0, 1)
    assert lib.ilqr_abi_version() == 2


def test_python_fit_refuses_track_for_other_families():
    import ilqr_amd
    from ilqr_amd.problems import two_link_closures
    x, u = np.zeros((11, 4)), np.zeros((10, 2))
    with pytest.raises(NotImplementedError, match="LQ family"):
        ilqr_amd.fit(x, u, *two_link_closures(), x_traj=np.zeros_like(x), track=True)
    f = lambda x, u: x  # noqa: E731  (arbitrary closures: the tiles path)
    with pytest.raises(NotImplementedError, match="LQ family"):
        ilqr_amd.fit(x, u, f, lambda x, u: 0.0, lambda x: 0.0, track=True)
