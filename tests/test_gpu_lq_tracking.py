"""The consistent tracking mode of the LQ family on the GPU (ILQR_TRACK_CONSISTENT,
ilqr_backward_tracking; include/ilqr.h): the backward kernels differentiate the cost the
forward pass measures, lx_t = (Q + Qᵀ)(x_t − x_traj_t) for t < T, the end state raw.

The checker is tests/tracking.py (the C restatement's backward on x − x_traj, its forward,
fit's bookkeeping) and, independently, the condensed QP with the reference stacked in.
Tolerances are the project's: gains 1e-11 against the symmetrised restatement, rollouts
1e-10, costs 1e-11, fit iterates 1e-8, all as max |a − b| / max |b|. du2 = Σ(ū − u)² is
bounded at 1e-9: a sum of squares carries twice its terms' relative error, and the terms
ū − u are of the rollout's own size on these inputs (u_init is zero or far from the optimum).

Shapes: B = 5 (a full wave of four and a ragged one), T = 9 (no multiple of the four-step
block, T − 5 > 0 for the vector-only look-ahead), T = 3 and T = 1 (the clamp at step 0),
(12, 4) and the padded (7, 3), B = 9 at T = 100 for the long horizon. Exact trial counts are
compared up to max_iter = 3 only: the accept margins are ≥ 5e-6 and ≥ 4.9e-10 in
iterations 2 and 3, but ≈ 5e-13 in iteration 4, below the costs' own tolerance.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tracking
from ilqr_amd import _lib
from ilqr_amd.multi import MultiSolver
from ilqr_amd.solver import Solver
from tracking import case, rel

pytestmark = pytest.mark.gpu
KEYS = ("x", "u", "cost", "iters", "status")


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to("cuda", dtype).contiguous()  # (the shared inputs are read-only)


def solver(lq, T, nb, track=True, **sched):
    s = Solver(lq.nx, lq.nu, T, nb)
    s.set_problem(lq)
    if sched:
        s.set_schedule(**sched)
    s.set_tracking(track)
    return s


def fit_np(s, x, u, xt, **kw):
    r = s.fit(dev(x), dev(u), x_traj=None if xt is None else dev(xt), **kw)
    out = {k: getattr(r, k).cpu().numpy() for k in KEYS}
    out["call_status"] = r.call_status
    if r.history is not None:
        out.update({"hist_" + k: v.cpu().numpy() for k, v in r.history.items()})
    return out


def assert_same(a, b, keys=None):
    for k in keys or sorted(set(a) | set(b)):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def assert_fit_matches(r, want, name, counts=True):
    ex, eu, ec = rel(r["x"], want["x"]), rel(r["u"], want["u"]), rel(r["cost"], want["cost"])
    print(name, "fit rel x", ex, "u", eu, "cost", ec)
    assert ex < 1e-8 and eu < 1e-8, (name, ex, eu)
    assert ec < 1e-11, (name, ec)
    if counts:
        np.testing.assert_array_equal(r["iters"], want["iters"])
        np.testing.assert_array_equal(r["status"], want["status"])
        n = want["trials"].shape[0]
        np.testing.assert_array_equal(r["hist_trials"][:n], want["trials"])


_WANT = {}


def checker_fit(name, T=9, **kw):
    """track_fit of a shared case, computed once per option set and never written to."""
    key = (name, T, tuple(sorted(kw.items())))
    if key not in _WANT:
        lq, x, u, xt = case(name, T)
        _WANT[key] = tracking.track_fit(lq, x, u, xt, **kw)
    return _WANT[key]


# -- 1. the gains ------------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["block", "wave"])
@pytest.mark.parametrize("T", [1, 3, 9])
@pytest.mark.parametrize("name", ["quad", "pad"])
def test_backward_tracking_gains(gpu, name, T, backward):
    lq, x, u, xt = case(name, T)
    dc, Kc, stc = tracking.track_backward(lq, x, u, xt)
    s = solver(lq, T, 5, track=False, backward=backward)  # the entry works whatever the mode
    try:
        d, K, st = s.backward(dev(x), dev(u), x_traj=dev(xt))
        ed, eK = rel(d.cpu().numpy(), dc), rel(K.cpu().numpy(), Kc)
        print(name, T, backward, "rel d", ed, "K", eK)
        assert (st.cpu().numpy() == 0).all() and (stc == 0).all()
        assert ed < 1e-11 and eK < 1e-11, (ed, eK)
        # the reference is honoured: the plain gains' d differs (d_t reads lx of the steps
        # after t only, so not at T = 1; K does not depend on x_traj)
        d0, K0, _ = s.backward(dev(x), dev(u))
        assert T == 1 or rel(d0.cpu().numpy(), dc) > 1e-3
        np.testing.assert_array_equal(K0.cpu().numpy(), K.cpu().numpy())
        # NULL x_traj: ilqr_backward's bits
        d1, K1 = torch.full_like(d0, 7.0), torch.full_like(K0, 7.0)
        st1 = torch.zeros(5, dtype=torch.int32, device="cuda")
        o = _lib.default_options()
        rc = s.lib.ilqr_backward_tracking(s.h, s._p(), C.byref(o), x_ptr(dev(x)), x_ptr(dev(u)), None,
                                          x_ptr(d1), x_ptr(K1), x_ptr(st1))
        assert rc == _lib.OK
        np.testing.assert_array_equal(d1.cpu().numpy(), d0.cpu().numpy())
        np.testing.assert_array_equal(K1.cpu().numpy(), K0.cpu().numpy())
    finally:
        s.close()


_KEEP = []


def x_ptr(t):
    _KEEP.append(t)  # alive until the synchronising call returns
    del _KEEP[:-16]
    return C.c_void_p(t.data_ptr())


# -- 2. one iteration ----------------------------------------------------------------------
@pytest.mark.parametrize("alpha0,trials", [(3.0, 2), (6.0, 3)])
@pytest.mark.parametrize("backward", ["block", "wave"])
@pytest.mark.parametrize("name", ["quad", "dense", "pad"])
def test_iterate_matches_one_checker_iteration(gpu, name, backward, alpha0, trials):
    lq, x, u, xt = case(name)
    prev = tracking.tracking_cost(lq, x, u, xt)  # the start iterate's own tracking cost
    dc, Kc, _ = tracking.track_backward(lq, x, u, xt)
    xn, un, cn, tr = tracking.cref.lq_forward(lq, x, u, xt, dc, Kc, prev, alpha0=alpha0)
    assert (tr == trials).all(), tr  # accept margins ≥ 7.6e-2, reject margins ≥ 3.0e-1
    du2c = ((un - u) ** 2).sum(axis=(1, 2))
    s = solver(lq, 9, 5, backward=backward)
    try:
        xo, uo = s.alloc_traj()
        cost = torch.zeros(5, dtype=torch.float64, device="cuda")
        du2 = torch.zeros(5, dtype=torch.float64, device="cuda")
        ntr = torch.zeros(5, dtype=torch.int32, device="cuda")
        st = torch.zeros(5, dtype=torch.int32, device="cuda")
        xd, ud, xtd, pd = dev(x), dev(u), dev(xt), dev(prev)
        s._bind_stream()
        s.iterate(xd, ud, xo, uo, pd, st, du2=du2, trials=ntr, x_traj=xtd,
                  options=_lib.default_options(alpha0=alpha0), new_cost=cost)
        torch.cuda.synchronize()
        e = {"x": rel(xo.cpu().numpy(), xn), "u": rel(uo.cpu().numpy(), un), "cost": rel(cost.cpu().numpy(), cn),
             "du2": rel(du2.cpu().numpy(), du2c)}
        print(name, backward, alpha0, e)
        np.testing.assert_array_equal(ntr.cpu().numpy(), tr)
        assert (st.cpu().numpy() == _lib.TRAJ_OK).all()
        assert e["x"] < 1e-10 and e["u"] < 1e-10 and e["cost"] < 1e-11 and e["du2"] < 1e-9, e
    finally:
        s.close()


# -- 3. three iterations, counts exact -----------------------------------------------------
@pytest.mark.parametrize("backward", ["block", "wave"])
@pytest.mark.parametrize("name", ["quad", "dense", "pad", "long"])
def test_fit_three_iterations(gpu, name, backward):
    lq, x, u, xt = case(name)
    want = checker_fit(name, max_iter=3)
    s = solver(lq, u.shape[1], u.shape[0], backward=backward)
    try:
        assert_fit_matches(fit_np(s, x, u, xt, max_iter=3, history=True), want, name)
    finally:
        s.close()


# -- 4. convergence ------------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["block", "wave"])
@pytest.mark.parametrize("name", ["quad", "dense", "pad"])
def test_fit_reaches_the_kkt_answer(gpu, name, backward):
    lq, x, u, xt = case(name)
    X, U = tracking.track_kkt(lq, x[:, 0], 9, xt)
    s = solver(lq, 9, 5, backward=backward)
    try:
        # One exact Newton step: μ = 0. A padded handle's H + μI has the padding's zero pivot
        # there (in either mode: every padded call needs μ > 0), so the padded case takes
        # μ = 1e-200, which rounds away in every real entry of H and leaves the same step.
        r = fit_np(s, x, u, xt, max_iter=1, mu=1e-200 if name == "pad" else 0.0)
        ex, eu = rel(r["x"], X), rel(r["u"], U)
        print(name, backward, "newton rel x", ex, "u", eu)
        assert ex < 1e-10 and eu < 1e-10, (ex, eu)
        r = fit_np(s, x, u, xt)  # the default options, to tol
        assert_fit_matches(r, checker_fit(name), name, counts=False)
        near = tracking.rel2(r["u"], U)
        s.set_tracking(False)
        off = tracking.rel2(fit_np(s, x, u, xt)["u"], U)
        print(name, backward, "rel2 to KKT: consistent", near, "forward-only", off)
        assert off > 0.5
    finally:
        s.close()


# -- 5. schedules --------------------------------------------------------------------------
BLOCK_SCHEDULES = {
    "split": dict(fused=False), "register_forward": dict(fused=False, ring_forward=False),
    "sequential_search": dict(sequential_search=True), "full_backward": dict(full_backward=True),
    "reuse_per_call": dict(reuse_per_call=True)}


@pytest.mark.parametrize("name", ["quad", "pad"])
def test_schedules_agree_bit_for_bit(gpu, name):
    lq, x, u, xt = case(name)
    kw = dict(max_iter=3, tol=1e-6, history=True)

    def run(**sched):
        s = solver(lq, 9, 5, **sched)
        try:
            return fit_np(s, x, u, xt, **kw)
        finally:
            s.close()

    base = run(backward="block")  # fused, ring forward, cooperative search, reuse across calls
    assert (base["hist_trials"][0] == 1).all()
    for sid, sched in BLOCK_SCHEDULES.items():
        assert_same(run(backward="block", **sched), base)
    kw = dict(max_iter=3, tol=1e-6)  # the pipelined schedule records no history
    wave = run(backward="wave")
    assert_same(run(pipelined=True), wave)
    assert_fit_matches(wave, checker_fit(name, max_iter=3), name, counts=False)


# -- 6. reuse across calls -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["quad", "pad"])
def test_new_reference_reuses_the_stored_gains(gpu, name):
    lq, x, u, xt = case(name)
    xt2 = 0.5 * np.random.default_rng(8).standard_normal(x.shape)
    kw = dict(max_iter=3, history=True)
    s, f = solver(lq, 9, 5, backward="block"), solver(lq, 9, 5, backward="block")
    try:
        fit_np(s, x, u, xt, **kw)
        assert (s.reuse_record() == 0).all()
        r2 = fit_np(s, x, u, xt2, **kw)
        assert len(s.reuse_record()) == 2 and (s.reuse_record() == 1).all()  # no wave re-factored
        want = fit_np(f, x, u, xt2, **kw)
        assert (f.reuse_record() == 0).all()
        assert_same(r2, want)
        assert rel(r2["u"], fit_np(f, x, u, xt, **kw)["u"]) > 1e-3  # the reference moved the answer
        # switching the mode keeps the stored gains too
        s.set_tracking(False)
        r3 = fit_np(s, x, u, xt2, **kw)
        assert (s.reuse_record() == 1).all()
        f.set_tracking(False)
        assert_same(r3, fit_np(f, x, u, xt2, **kw))
    finally:
        s.close()
        f.close()


# -- 7. mode hygiene -----------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["block", "wave"])
@pytest.mark.parametrize("name", ["quad", "pad"])
def test_mode_on_then_off_and_zero_reference(gpu, name, backward):
    lq, x, u, xt = case(name)
    kw = dict(max_iter=3, history=True)
    plain, s = solver(lq, 9, 5, track=False, backward=backward), solver(lq, 9, 5, backward=backward)
    try:
        assert s.tracking and not plain.tracking
        today = fit_np(plain, x, u, xt, **kw)
        on = fit_np(s, x, u, xt, **kw)
        assert rel(on["u"], today["u"]) > 1e-3
        s.set_tracking(False)
        assert not s.tracking
        assert_same(fit_np(s, x, u, xt, **kw), today)
        s.set_tracking(True)
        zeros = np.zeros_like(x)
        assert_same(fit_np(s, x, u, zeros, **kw), fit_np(plain, x, u, zeros, **kw))
        assert_same(fit_np(s, x, u, None, **kw), fit_np(plain, x, u, None, **kw))
        assert_same(fit_np(s, x, u, zeros, **kw), fit_np(plain, x, u, None, **kw))
        # a refused value leaves the mode as it was
        assert s.lib.ilqr_set_tracking(s.h, 2) == _lib.ERR_BAD_ARG and s.tracking
        assert s.lib.ilqr_set_tracking(s.h, -1) == _lib.ERR_BAD_ARG and s.tracking
    finally:
        plain.close()
        s.close()


def test_two_link_is_refused_in_consistent_mode(gpu):
    nb, T = 3, 6
    s = Solver(4, 2, T, nb, kind=_lib.PROBLEM_TWO_LINK)
    try:
        s.set_tracking(True)
        x, u = s.alloc_traj()
        xo, uo = torch.full_like(x, 7.0), torch.full_like(u, 7.0)
        cost = torch.full((nb,), 7.0, dtype=torch.float64, device="cuda")
        st = torch.full((nb,), 7, dtype=torch.int32, device="cuda")
        o = _lib.default_options(max_iter=2)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        s._bind_stream()
        assert s.lib.ilqr_fit_ex(s.h, s._p(), C.byref(o), p(x), p(u), p(x), p(xo), p(uo), p(cost), None, p(st),
                                 None) == _lib.ERR_UNSUPPORTED
        assert s.lib.ilqr_fit(s.h, s._p(), C.byref(o), p(x), p(u), None, p(xo), p(uo), p(cost), None,
                              p(st)) == _lib.ERR_UNSUPPORTED
        assert s.lib.ilqr_iterate(s.h, s._p(), C.byref(o), p(x), p(u), p(x), p(xo), p(uo), None, p(cost), None,
                                  None, p(st)) == _lib.ERR_UNSUPPORTED
        d = torch.full((nb, T, 2), 7.0, dtype=torch.float64, device="cuda")
        K = torch.full((nb, T, 2, 4), 7.0, dtype=torch.float64, device="cuda")
        assert s.lib.ilqr_backward_tracking(s.h, s._p(), C.byref(o), p(x), p(u), p(x), p(d), p(K),
                                            None) == _lib.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        for t in (xo, uo, cost, st, d, K):
            assert bool((t == 7).all())  # nothing was launched
        s.set_tracking(False)  # ... and the family runs as ever in the default mode
        r = s.fit(x, u, max_iter=1)
        assert r.call_status in (_lib.OK, _lib.ERR_LS_EXHAUSTED)
    finally:
        s.close()


# -- 8. NaN --------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", ["block", "wave"])
def test_nan_in_one_reference_stops_that_trajectory_alone(gpu, backward):
    lq, x, u, xt = case("quad9")
    bad = 5  # the second wave's second slot
    xtn = np.array(xt)
    xtn[bad, 4, 2] = np.nan
    want = checker_fit("quad9", max_iter=3)
    s = solver(lq, 9, 9, backward=backward)
    try:
        r = fit_np(s, x, u, xtn, max_iter=3, history=True)
        assert r["call_status"] == _lib.ERR_NAN
        assert r["status"][bad] == _lib.TRAJ_NAN
        np.testing.assert_array_equal(r["x"][bad], x[bad])  # it keeps its iterate
        np.testing.assert_array_equal(r["u"][bad], u[bad])
        ok = np.arange(9) != bad
        got = {k: (v[:, ok] if k.startswith("hist_") else v[ok]) for k, v in r.items() if k != "call_status"}
        exp = {k: (v[:, ok] if k in ("trials", "du2") else v[ok]) for k, v in want.items()}
        assert_fit_matches(got, exp, "quad9 wave-mates")
    finally:
        s.close()


# -- 9. multi-device -----------------------------------------------------------------------
def test_multi_device_matches_one_handle(gpu):
    lq, x, u, xt = case("quad10")
    one = solver(lq, 9, 10)
    m = MultiSolver([0, 0], 12, 4, 9, 10)
    try:
        want = fit_np(one, x, u, xt, max_iter=3)
        one.set_tracking(False)
        today = fit_np(one, x, u, xt, max_iter=3)
        assert rel(want["u"], today["u"]) > 1e-3
        m.set_tracking(True)
        xo, uo, cost, iters, st, rc = m.fit(lq, x, u, x_traj=xt, max_iter=3)
        got = {"x": xo, "u": uo, "cost": cost, "iters": iters, "status": st}
        assert_same(got, want, KEYS)
        m.set_problem(lq)
        m.load(x, u, xt)
        m.fit_resident(max_iter=3, use_x_traj=True)
        assert_same(m.gather(), want, KEYS)
        m.set_tracking(False)
        m.fit_resident(max_iter=3, use_x_traj=True)
        assert_same(m.gather(), today, KEYS)
        assert m.lib.ilqr_multi_set_tracking(m.h, 5) == _lib.ERR_BAD_ARG
    finally:
        one.close()
        m.close()


# -- 10. the Python mirror -----------------------------------------------------------------
def test_python_fit_track(gpu, monkeypatch):
    import warnings

    import ilqr_amd
    lq, x, u, xt = case("quad")
    x, u, xt = np.array(x), np.array(u), np.array(xt)  # (the mirror wants writable arrays)
    modes = []
    close = Solver.close

    def recording_close(self):
        if getattr(self, "h", None):
            modes.append(self.tracking)
        close(self)

    monkeypatch.setattr(Solver, "close", recording_close)
    xo, uo, info = ilqr_amd.fit(x, u, *lq.closures(), x_traj=xt, max_iter=3, track=True, return_info=True)
    assert modes == [False]  # the mirror's solver was back in the default mode when it let go of it
    s = solver(lq, 9, 5)
    try:
        want = fit_np(s, x, u, xt, max_iter=3)
    finally:
        s.close()
    np.testing.assert_array_equal(xo, want["x"])
    np.testing.assert_array_equal(uo, want["u"])
    np.testing.assert_array_equal(info["cost"], want["cost"])
    np.testing.assert_array_equal(info["iters"], want["iters"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # forward-only tracking may exhaust its line search
        xo0, uo0 = ilqr_amd.fit(x, u, *lq.closures(), x_traj=xt, max_iter=3)
    assert rel(uo0, want["u"]) > 1e-3  # track=False stays the reference's behaviour
