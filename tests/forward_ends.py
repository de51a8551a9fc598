"""The rare ends of a line search, checked the same way for every forward kernel of the
2-link and chain families (tests/test_gpu_twolink.py, test_gpu_chain.py, test_gpu_chain6.py).

Expectations are the reference's semantics as the kernels restate them
(src/forward_pass.jl:55-93 and :159-176), not recorded outputs:
  * a search that accepts nothing within max_trials (the reference would loop forever)
    ends LS_EXHAUSTED with trials = max_trials; a standalone forward returns its inputs;
  * a NaN cost compares false at every trial (:77-80), so it ends the same way with NAN;
  * in a fit such a trajectory keeps the iteration's INPUT iterate, and so does one that
    converges (:171 breaks before the update).
Shapes are ragged against every grouping of trajectories (4 per wave, 2 per wave, 16 per
workgroup): B = 5, T = 7 for nx = 4 and B = 3, T = 5 for six joints.

The callers pass adapters over their solver's API:
  forward(x, u, d, K, prev_cost, max_trials) -> (x_new, u_new, cost, trials, status)
  iterate(x, u, x_new, u_new, prev_cost, status, new_cost, du2, trials, x_traj, options)
  fit(x, u, x_traj, max_iter, tol) -> FitResult
"""
import torch

from ilqr_amd import _lib

SENT = -12345.0


def bits(a):
    return a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def gains(x, u, seed):
    """Small seeded δu and K: every trial is a different, finite rollout."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, T, nu = u.shape
    nx = x.shape[2]
    d = (0.02 * torch.randn((B, T, nu), generator=g, dtype=torch.float64)).to(x)
    K = (0.02 * torch.randn((B, T, nu, nx), generator=g, dtype=torch.float64)).to(x)
    return d, K


def check_forward_exhausted(forward, x, u):
    B = x.shape[0]
    d, K = gains(x, u, 5)
    pc = torch.full((B,), float("-inf"), dtype=x.dtype, device=x.device)   # no cost is below it
    xn, un, cost, trials, st = forward(x, u, d, K, pc, 2)
    assert st.cpu().tolist() == [_lib.TRAJ_LS_EXHAUSTED] * B
    assert trials.cpu().tolist() == [2] * B
    assert same_bits(xn, x) and same_bits(un, u)
    assert bool(torch.isfinite(cost).all())


def check_forward_nan(forward, x, u, k=1):
    B = x.shape[0]
    d, K = gains(x, u, 6)
    u = u.clone()
    u[k, 2, 0] = float("nan")
    pc = torch.full((B,), float("inf"), dtype=x.dtype, device=x.device)
    xn, un, cost, trials, st = forward(x, u, d, K, pc, 3)
    want = [_lib.TRAJ_NAN if b == k else _lib.TRAJ_OK for b in range(B)]
    assert st.cpu().tolist() == want
    assert trials.cpu().tolist() == [3 if b == k else 1 for b in range(B)]
    assert same_bits(xn[k], x[k]) and same_bits(un[k], u[k])
    assert bool(torch.isnan(cost[k])) and int(torch.isnan(cost).sum()) == 1


def _iterate(iterate, x, u, prev_cost, x_traj, max_trials):
    B = x.shape[0]
    xn, un = torch.full_like(x, SENT), torch.full_like(u, SENT)
    nc = torch.full((B,), SENT, dtype=x.dtype, device=x.device)
    du2 = torch.full((B,), SENT, dtype=x.dtype, device=x.device)
    tr = torch.full((B,), -7, dtype=torch.int32, device=x.device)
    st = torch.zeros((B,), dtype=torch.int32, device=x.device)
    iterate(x, u, xn, un, prev_cost, st, nc, du2, tr, x_traj,
            _lib.default_options(tol=-1.0, max_trials=max_trials))
    torch.cuda.synchronize()
    return nc, du2, tr, st


def check_iterate_exhausted(iterate, x, u):
    B = x.shape[0]
    pc = torch.full((B,), float("-inf"), dtype=x.dtype, device=x.device)
    nc, du2, tr, st = _iterate(iterate, x, u, pc, None, 2)
    assert st.cpu().tolist() == [_lib.TRAJ_LS_EXHAUSTED] * B
    assert tr.cpu().tolist() == [2] * B
    assert bool((nc == SENT).all())   # prev_cost = new_cost (:168) is for accepted steps only
    assert bool(torch.isfinite(du2).all()) and bool((du2 != SENT).all())


def check_iterate_nan(iterate, x, u, k=1):
    """x_traj enters the line search's objective only: a NaN in it leaves the backward pass
    finite and makes every trial's cost NaN."""
    B = x.shape[0]
    xt = torch.zeros_like(x)
    xt[k, 1, 0] = float("nan")
    nc, du2, tr, st = _iterate(iterate, x, u, None, xt, 3)
    assert st.cpu().tolist() == [_lib.TRAJ_NAN if b == k else _lib.TRAJ_OK for b in range(B)]
    assert tr.cpu().tolist() == [3 if b == k else 1 for b in range(B)]
    assert nc[k].item() == SENT
    others = [b for b in range(B) if b != k]
    assert bool(torch.isfinite(nc[others]).all()) and bool((nc[others] != SENT).all())


def check_fit_input_kept(fit, x, u, k=1):
    """The two ends that name the iteration's input as the result (res_parity)."""
    B = x.shape[0]
    xt = torch.zeros_like(x)
    xt[k, 1, 0] = float("nan")
    r = fit(x, u, xt, 3, -1.0)
    st = r.status.cpu().tolist()
    assert st[k] == _lib.TRAJ_NAN and r.iters[k].item() == 1
    assert all(s in (_lib.TRAJ_MAX_ITER, _lib.TRAJ_LS_EXHAUSTED) for b, s in enumerate(st) if b != k), st
    it = r.iters.cpu().tolist()   # tol < 0: a trajectory runs every iteration unless its search ends it
    assert all(it[b] == 3 for b, s in enumerate(st) if s == _lib.TRAJ_MAX_ITER), (st, it)
    assert all(2 <= it[b] <= 3 for b, s in enumerate(st) if s == _lib.TRAJ_LS_EXHAUSTED), (st, it)
    assert same_bits(r.x[k], x[k]) and same_bits(r.u[k], u[k])
    assert r.call_status == _lib.ERR_NAN
    r = fit(x, u, None, 3, 1e300)   # every Σ(ū − u)² is below it: converged at iteration 1
    assert r.status.cpu().tolist() == [_lib.TRAJ_CONVERGED] * B
    assert r.iters.cpu().tolist() == [1] * B
    assert same_bits(r.x, x) and same_bits(r.u, u)
    assert r.call_status == _lib.OK
