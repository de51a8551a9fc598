"""Gain reuse across fit calls (include/ilqr.h ILQR_SCHED_REUSE_PER_CALL): a
handle keeps the gains and the H factor of its last fit on the fused (12, 4) path, with a
snapshot of the operands they were computed from. The first iteration of the next fit
compares, wave by wave and bit for bit, what it read from the problem with that snapshot
and runs the vector-only backward where they agree, the full recursion (refreshing the
store) where they do not. Whichever branch a wave takes must change no bit: every
comparison here is `assert_array_equal`, and its reference is always a fresh handle fitting
the same inputs (never the handle under test). `Solver.reuse_record()` tells which branch
each wave (trajectories 4w .. 4w+3) took: 1 reused, 0 re-factored.

Shapes as in test_gpu_gain_reuse.py (a ragged last wave, the four- and eight-step loop
tails, the one-step corner), `backward="block"` so that these small batches take the fused
path.
"""
import functools

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.problems import LQBatch, quadrotor_batch, random_lq_batch
from ilqr_amd.solver import Solver

pytestmark = pytest.mark.gpu
SHAPES = [(6, 5), (5, 3), (9, 8), (1, 1), (7, 19), (3, 15)]
KW = dict(max_iter=4, tol=-1.0, history=True)
KEYS = ("A", "B", "Q", "R", "Qf")
REUSE, STORE = 1, 0


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


_PROBLEMS = set()


@functools.lru_cache(maxsize=None)
def problem(nb, T, seed0=0):
    _PROBLEMS.add((nb, T, seed0))
    return quadrotor_batch(nb, T=T, seed0=seed0)


def tensors(lq):
    return {k: dev(getattr(lq, k)) for k in KEYS}


def solver(prob, T, nb, **sched):
    s = Solver(prob["A"].shape[-1] if isinstance(prob, dict) else prob.nx,
               prob["B"].shape[-1] if isinstance(prob, dict) else prob.nu, T, nb)
    s.set_problem(prob)
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


def fit(s, x, u, **kw):
    return result_np(s.fit(dev(x), dev(u), **dict(KW, **kw)))


_FRESH = {}


def fresh(prob, x, u, sched=None, **kw):
    """The reference: a new handle's first fit of these inputs. `prob`: an LQBatch or a dict
    of numpy arrays / tensors (copied, so the handle under test's buffers are not shared).
    References of the shared `problem()` inputs are computed once and never written to."""
    key = None
    if any(prob is q[0] and x is q[1] and u is q[2] for q in (problem(*a) for a in _PROBLEMS)):
        key = (id(prob), tuple(sorted((sched or {}).items())), tuple(sorted(kw.items())))
        if key in _FRESH:
            return _FRESH[key]
    r = _fresh(prob, x, u, sched, **kw)
    if key is not None:
        _FRESH[key] = r
    return r


def _fresh(prob, x, u, sched, **kw):
    if isinstance(prob, dict):
        prob = LQBatch(*(prob[k].cpu().numpy() if torch.is_tensor(prob[k]) else prob[k] for k in KEYS))
    nb, T = u.shape[:2]
    s = solver(prob, T, nb, **(sched or {}))
    try:
        r = fit(s, x, u, **kw)
        assert (s.reuse_record() == STORE).all()  # nothing to reuse on a new handle
        return r
    finally:
        s.close()


def waves(nb):
    return (nb + 3) // 4


def expect(s, nb, store=()):
    want = np.full(waves(nb), REUSE, np.int32)
    want[list(store)] = STORE
    np.testing.assert_array_equal(s.reuse_record(), want)


@pytest.mark.parametrize("sched", [{}, {"forward_mfma": True}, {"sequential_search": True}],
                         ids=["default", "forward_mfma", "sequential_search"])
@pytest.mark.parametrize("nb,T", SHAPES)
def test_same_problem_new_trajectories(gpu, nb, T, sched):
    lq, x, u = problem(nb, T)
    _, x2, u2 = problem(nb, T, 100)  # another seed's rollout
    s = solver(lq, T, nb, **sched)
    try:
        assert_same(fit(s, x, u), fresh(lq, x, u, sched))
        expect(s, nb, store=range(waves(nb)))
        r2 = fit(s, x2, u2)
        expect(s, nb)
        assert_same(r2, fresh(lq, x2, u2, sched))
        assert (r2["hist_trials"][0] > 0).all()  # the fit ran
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_same_values_at_new_pointers(gpu, nb, T):
    lq, x, u = problem(nb, T)
    p = tensors(lq)
    s = solver(p, T, nb)
    try:
        fit(s, x, u)
        q = {k: v.clone() for k, v in p.items()}
        s.set_problem(q)
        for v in p.values():  # the old buffers no longer hold the problem
            v.fill_(float("nan"))
        r = fit(s, x, u)
        expect(s, nb)
        assert_same(r, fresh(lq, x, u))
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_one_instance_rewritten_in_place(gpu, nb, T):
    lq, x, u = problem(nb, T)
    k = nb - 1 if nb % 4 else nb // 2  # in the ragged last wave where there is one
    p = tensors(lq)
    s = solver(p, T, nb)
    try:
        fit(s, x, u)
        p["A"][k] *= 0.97
        r = fit(s, x, u)
        expect(s, nb, store=[k // 4])
        ref = fresh(p, x, u)
        assert_same(r, ref)
        r3 = fit(s, x, u)
        expect(s, nb)
        assert_same(r3, ref)
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_sign_of_zero_is_a_change(gpu, nb, T):
    lq, x, u = problem(nb, T)
    k = nb // 2
    assert lq.B[k, 0, 0] == 0.0 and not np.signbit(lq.B[k, 0, 0])  # structurally zero
    p = tensors(lq)
    s = solver(p, T, nb)
    try:
        fit(s, x, u)
        p["B"][k, 0, 0] = -0.0
        assert np.signbit(p["B"][k, 0, 0].item())
        r = fit(s, x, u)
        expect(s, nb, store=[k // 4])  # a floating compare would have called it equal
        assert_same(r, fresh(p, x, u))
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_mu_changed(gpu, nb, T):
    lq, x, u = problem(nb, T)
    s = solver(lq, T, nb)
    try:
        fit(s, x, u)
        everywhere = range(waves(nb))
        r = fit(s, x, u, mu=0.05)
        expect(s, nb, store=everywhere)
        assert_same(r, fresh(lq, x, u, mu=0.05))
        r = fit(s, x, u)  # the old μ again: the store holds 0.05's gains
        expect(s, nb, store=everywhere)
        assert_same(r, fresh(lq, x, u))
        fit(s, x, u)
        expect(s, nb)
    finally:
        s.close()


def _iterate(s, other, x, u):
    s.set_problem(other)
    xi, ui = dev(x), dev(u)
    st = torch.zeros((u.shape[0],), dtype=torch.int32, device="cuda")
    pc = torch.empty((u.shape[0],), dtype=torch.float64, device="cuda")
    s.iterate(xi, ui, torch.empty_like(xi), torch.empty_like(ui), None, st, new_cost=pc)
    torch.cuda.synchronize()


def _fit_with(sched):
    def run(s, other, x, u):
        s.set_problem(other)
        s.set_schedule(**sched)
        fit(s, x, u)
        s.set_schedule(backward="block")
    return run


@pytest.mark.parametrize("between", [_iterate, _fit_with(dict(backward="block", full_backward=True)),
                                     _fit_with(dict(backward="wave"))],
                         ids=["iterate", "full_backward_fit", "wave_fit"])
@pytest.mark.parametrize("nb,T", SHAPES)
def test_invalidation(gpu, nb, T, between):
    """Whatever else writes the handle's gains, on a different problem, in between: the next
    fit re-factors everywhere."""
    lq, x, u = problem(nb, T)
    other, xo, uo = problem(nb, T, 100)
    s = solver(lq, T, nb)
    try:
        fit(s, x, u)
        between(s, other, xo, uo)
        s.set_problem(lq)
        r = fit(s, x, u)
        expect(s, nb, store=range(waves(nb)))
        assert_same(r, fresh(lq, x, u))
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_nan_in_the_problem(gpu, nb, T):
    """The NaN's bits equal the snapshot's, so its wave reuses; the NaN is found in the
    loaded K_0."""
    lq, x, u = problem(nb, T)
    bad = nb // 2
    A = lq.A.copy()
    A[bad, 3, 5] = np.nan
    lqn = LQBatch(A, lq.B, lq.Q, lq.R, lq.Qf)
    ref = fresh(lqn, x, u)
    assert ref["status"][bad] == _lib.TRAJ_NAN and ref["call_status"] == _lib.ERR_NAN
    assert (np.delete(ref["status"], bad) != _lib.TRAJ_NAN).all()
    s = solver(lqn, T, nb)
    try:
        assert_same(fit(s, x, u), ref)
        r = fit(s, x, u)
        expect(s, nb)
        assert r["status"][bad] == _lib.TRAJ_NAN and r["call_status"] == _lib.ERR_NAN
        assert_same(r, ref)
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_nan_in_u_init_of_the_first_call(gpu, nb, T):
    """K never depended on u: the store of a fit whose trajectory went NaN serves the next."""
    lq, x, u = problem(nb, T)
    ub = u.copy()
    ub[nb // 2, T // 2, 1] = np.nan
    s = solver(lq, T, nb)
    try:
        r1 = fit(s, x, ub)
        assert r1["status"][nb // 2] == _lib.TRAJ_NAN
        r2 = fit(s, x, u)
        expect(s, nb)
        assert_same(r2, fresh(lq, x, u))
    finally:
        s.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_early_stops(gpu, nb, T):
    """tol at the median of iteration 2's Σ(ū − u)² (test_reuse_with_trajectories_leaving):
    about half of the trajectories stop there, in a fit whose every backward is vector-only."""
    lq, x, u = problem(nb, T)
    s = solver(lq, T, nb)
    try:
        first = fit(s, x, u)
        d2 = first["hist_du2"][1]
        tol = float(np.nanmedian(d2)) if np.isfinite(d2).any() else 1e-6
        r = fit(s, x, u, tol=tol)
        expect(s, nb)
        print("tol", tol, "iters", r["iters"], "status", r["status"])
        if nb >= 5:
            assert r["iters"].min() < r["iters"].max(), r["iters"]
        assert_same(r, fresh(lq, x, u, dict(full_backward=True), tol=tol))
    finally:
        s.close()


def test_padded_shape_twice(gpu):
    """(6, 2) runs zero-padded on the inner (12, 4) handle, which re-pads the problem into the
    same scratch on every call: the same bits, so the second fit reuses."""
    nb, T = 5, 5
    lq, x, u = random_lq_batch(nb, 6, 2, T, seed=17 * 6 + 2)
    kw = dict(max_iter=15, tol=1e-8)
    s = solver(lq, T, nb)
    try:
        r1 = fit(s, x, u, **kw)
        expect(s, nb, store=range(waves(nb)))
        r2 = fit(s, x, u, **kw)
        expect(s, nb)
        assert_same(r2, r1)
        assert_same(r2, fresh(lq, x, u, **kw))
    finally:
        s.close()


def test_multi_resident_twice(gpu):
    from ilqr_amd.multi import MultiSolver
    nb, T = 10, 5
    lq, x, u = problem(nb, T)
    ms = MultiSolver([0, 0], 12, 4, T, nb)  # two shards of five
    try:
        ms.set_schedule(backward="block")
        ms.set_problem(lq)
        ms.load(x, u)
        rc1 = ms.fit_resident(max_iter=KW["max_iter"], tol=KW["tol"])
        g1 = ms.gather()
        for shard in (0, 1):
            np.testing.assert_array_equal(ms.reuse_record(shard), [STORE, STORE])
        rc2 = ms.fit_resident(max_iter=KW["max_iter"], tol=KW["tol"])
        g2 = ms.gather()
        for shard in (0, 1):
            np.testing.assert_array_equal(ms.reuse_record(shard), [REUSE, REUSE])
    finally:
        ms.close()
    ref = fresh(lq, x, u, history=False)
    assert rc1 == rc2 == ref["call_status"]
    for k in ("x", "u", "cost", "iters", "status"):
        np.testing.assert_array_equal(g2[k], g1[k], err_msg=k)
        np.testing.assert_array_equal(g2[k], ref[k], err_msg=k)


@pytest.mark.parametrize("nb,T", SHAPES)
def test_per_call_bit(gpu, nb, T):
    lq, x, u = problem(nb, T)
    s = solver(lq, T, nb, reuse_per_call=True)
    try:
        ref = fresh(lq, x, u)
        for _ in range(3):
            assert_same(fit(s, x, u), ref)
            expect(s, nb, store=range(waves(nb)))
    finally:
        s.close()
