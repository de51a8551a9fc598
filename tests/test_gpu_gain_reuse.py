"""Gain reuse inside one fit (include/ilqr.h ILQR_SCHED_FULL_BACKWARD): on
the fused (12, 4) path iteration 1 of a fit runs the full backward recursion and stores
the solve operands; iterations ≥ 2 read the gains and the operands back and recompute
only d_t and the value gradient. A, B, Q, R, Qf and μ are fixed for the call, so this
must change no bit: every comparison here is `assert_array_equal`.

The shapes (B, T) cover a ragged last wave (B not a multiple of 4), T below, equal to
and above the full loop's block of four steps with its tail, a symmetrisation step
(t % 8 == 0) inside and outside the tail and the one-step one-trajectory corner; the
last two add what the vector-only loop's block of eight needs: whole blocks followed by
a tail of three (T = 19) and of seven (T = 15) steps. `backward="block"` puts these
small batches on the fused path (the default picks the one-trajectory-per-wave backward
below 2048).
"""
import functools

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.problems import quadrotor_batch, random_lq_batch
from ilqr_amd.solver import Solver
from oracle import cref

pytestmark = pytest.mark.gpu
SHAPES = [(6, 5), (5, 3), (9, 8), (1, 1), (7, 19), (3, 15)]
ITERS = 4


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


@functools.lru_cache(maxsize=None)
def problem(nb, T, seed0=0):
    return quadrotor_batch(nb, T=T, seed0=seed0)


def solver(lq, T, nb, **sched):
    s = Solver(lq.nx, lq.nu, T, nb)
    s.set_problem(lq)
    s.set_schedule(backward="block", **sched)
    return s


def result_np(r):
    out = {k: getattr(r, k).cpu().numpy() for k in ("x", "u", "cost", "iters", "status")}
    out["call_status"] = r.call_status
    if r.history is not None:
        out.update({"hist_" + k: v.cpu().numpy() for k, v in r.history.items()})
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def fit_np(lq, x, u, sched, **kw):
    nb, T = u.shape[:2]
    s = solver(lq, T, nb, **sched)
    try:
        return result_np(s.fit(dev(x), dev(u), **kw))
    finally:
        s.close()


@pytest.mark.parametrize("sequential_search", [False, True])
@pytest.mark.parametrize("forward_mfma", [False, True])
@pytest.mark.parametrize("nb,T", SHAPES)
def test_reuse_equals_full_backward(gpu, nb, T, forward_mfma, sequential_search):
    lq, x, u = problem(nb, T)
    sched = dict(forward_mfma=forward_mfma, sequential_search=sequential_search)
    kw = dict(max_iter=ITERS, tol=-1.0, history=True)
    reuse = fit_np(lq, x, u, sched, **kw)
    full = fit_np(lq, x, u, dict(sched, full_backward=True), **kw)
    assert (reuse["hist_trials"][0] > 0).all()  # the fit ran
    assert_same(reuse, full)


@pytest.mark.parametrize("nb,T", SHAPES)
def test_reuse_fit_equals_iterate_chain(gpu, nb, T):
    """fit (reuse on) against ITERS chained ilqr_iterate calls, each a full recursion; a
    trajectory that stops (line search exhausted at the cost floor) keeps its iterate."""
    lq, x, u = problem(nb, T)
    s = solver(lq, T, nb)
    try:
        r = result_np(s.fit(dev(x), dev(u), max_iter=ITERS, tol=-1.0, history=True))
        xi, ui = dev(x), dev(u)
        xn, un = torch.empty_like(xi), torch.empty_like(ui)
        pc = torch.empty((nb,), dtype=torch.float64, device="cuda")
        st = torch.zeros((nb,), dtype=torch.int32, device="cuda")
        tr = torch.zeros((nb,), dtype=torch.int32, device="cuda")
        du2 = torch.zeros((nb,), dtype=torch.float64, device="cuda")
        running = np.ones(nb, bool)
        for it in range(ITERS):
            s.iterate(xi, ui, xn, un, None if it == 0 else pc, st, du2=du2, trials=tr,
                      options=_lib.default_options(tol=-1.0), new_cost=pc)
            torch.cuda.synchronize()
            ok = st.cpu().numpy() == _lib.TRAJ_OK
            acc = running & ok
            np.testing.assert_array_equal(r["hist_cost"][it], np.where(acc, pc.cpu().numpy(), np.nan))
            np.testing.assert_array_equal(r["hist_trials"][it], np.where(running, tr.cpu().numpy(), 0))
            np.testing.assert_array_equal(r["hist_du2"][it], np.where(running, du2.cpu().numpy(), np.nan))
            running = acc
            keep = torch.from_numpy(~ok).cuda()
            xn[keep] = xi[keep]
            un[keep] = ui[keep]
            xi, xn, ui, un = xn, xi, un, ui
        np.testing.assert_array_equal(r["x"], xi.cpu().numpy())
        np.testing.assert_array_equal(r["u"], ui.cpu().numpy())
        stn = st.cpu().numpy()  # fit reports the trajectories still running as MAX_ITER
        np.testing.assert_array_equal(r["status"], np.where(stn == _lib.TRAJ_OK, _lib.TRAJ_MAX_ITER, stn))
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_reuse_with_trajectories_leaving(gpu, nb, T):
    """A NaN trajectory leaves at iteration 1 while its wave-mates go on; with tol at the
    median of iteration 2's Σ(ū − u)² about half of the others stop there."""
    lq, x, u = problem(nb, T)
    u = u.copy()
    bad = nb // 2
    u[bad, T // 2, 1] = np.nan
    first = fit_np(lq, x, u, {}, max_iter=ITERS, tol=-1.0, history=True)
    assert first["status"][bad] == _lib.TRAJ_NAN
    d2 = np.delete(first["hist_du2"][1], bad)
    tol = float(np.median(d2)) if d2.size else 1e-6
    reuse = fit_np(lq, x, u, {}, max_iter=ITERS, tol=tol, history=True)
    full = fit_np(lq, x, u, dict(full_backward=True), max_iter=ITERS, tol=tol, history=True)
    assert reuse["status"][bad] == _lib.TRAJ_NAN and reuse["call_status"] == _lib.ERR_NAN
    others = np.delete(reuse["iters"], bad)
    print("tol", tol, "iters", reuse["iters"], "status", reuse["status"])
    if nb >= 5:
        assert others.min() < others.max(), others  # some stopped early, some went on
    assert_same(reuse, full)


def test_no_stale_cache_across_calls(gpu):
    """Nothing of the first iteration's store survives a call: another problem through new
    tensors, the same tensors rewritten in place, and another μ each equal a fresh handle."""
    nb, T = 6, 5
    lq1, x1, u1 = problem(nb, T, 0)
    lq2, x2, u2 = problem(nb, T, 100)
    keys = ("A", "B", "Q", "R", "Qf")
    kw = dict(max_iter=ITERS, tol=-1.0, history=True)
    fresh2 = fit_np(lq2, x2, u2, {}, **kw)
    fresh2_mu = fit_np(lq2, x2, u2, {}, mu=0.05, **kw)
    assert not np.array_equal(fresh2["u"], fresh2_mu["u"])
    p1 = {k: dev(getattr(lq1, k)) for k in keys}
    p2 = {k: dev(getattr(lq2, k)) for k in keys}
    s = Solver(12, 4, T, nb)
    s.set_schedule(backward="block")
    try:
        s.set_problem(p1)
        r1 = result_np(s.fit(dev(x1), dev(u1), **kw))
        assert_same(r1, fit_np(lq1, x1, u1, {}, **kw))
        s.set_problem(p2)  # new tensors
        assert_same(result_np(s.fit(dev(x2), dev(u2), **kw)), fresh2)
        s.set_problem(p1)
        assert_same(result_np(s.fit(dev(x1), dev(u1), **kw)), r1)
        for k in keys:  # the same pointers, rewritten in place
            p1[k].copy_(p2[k])
        assert_same(result_np(s.fit(dev(x2), dev(u2), **kw)), fresh2)
        assert_same(result_np(s.fit(dev(x2), dev(u2), mu=0.05, **kw)), fresh2_mu)
        assert_same(result_np(s.fit(dev(x2), dev(u2), **kw)), fresh2)
    finally:
        s.close()


def test_reuse_padded_shape(gpu):
    """(6, 2) runs zero-padded on the inner (12, 4) handle: reuse against the full
    recursion bit for bit, and against the C oracle within the padded-shape tolerance
    of test_gpu_parity.test_lq_padded_shapes_vs_oracle."""
    nb, T = 5, 5
    lq, x, u = random_lq_batch(nb, 6, 2, T, seed=17 * 6 + 2)
    kw = dict(max_iter=15, tol=1e-8, history=True)
    reuse = fit_np(lq, x, u, {}, **kw)
    full = fit_np(lq, x, u, dict(full_backward=True), **kw)
    assert_same(reuse, full)
    xf, uf, cf, itf, stf = cref.lq_fit(lq, x, u, max_iter=15, tol=1e-8, symmetrize=True)
    np.testing.assert_array_equal(reuse["iters"], itf)
    assert np.abs(reuse["u"] - uf).max() < 1e-8 * np.abs(uf).max()
    assert np.abs(reuse["x"] - xf).max() < 1e-8 * np.abs(xf).max()


def test_reuse_multi_equals_single_handle(gpu):
    from ilqr_amd.multi import MultiSolver
    nb, T = 10, 5
    lq, x, u = problem(nb, T)
    ms = MultiSolver([0, 0], 12, 4, T, nb)  # two shards of five
    try:
        ms.set_schedule(backward="block")
        xo, uo, co, it, st, rc = ms.fit(lq, x, u, max_iter=ITERS, tol=-1.0)
    finally:
        ms.close()
    r = fit_np(lq, x, u, {}, max_iter=ITERS, tol=-1.0)
    full = fit_np(lq, x, u, dict(full_backward=True), max_iter=ITERS, tol=-1.0)
    assert_same(r, full)
    assert rc == r["call_status"]
    for got, k in ((xo, "x"), (uo, "u"), (co, "cost"), (it, "iters"), (st, "status")):
        np.testing.assert_array_equal(got, r[k], err_msg=k)
