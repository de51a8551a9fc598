"""mu, alpha0 and shrink off their defaults in every kernel family (ilqr_options, include/ilqr.h).

At the defaults (alpha0 = 1, shrink = 0.5) every step α is a power of two and every product
with it is exact, so the several ways the kernels form α — the sequential `alpha *= shrink`
loops, the candidate groups' round and sub-trial loops, the cooperative search's per-trial
product, the history's reconstruction — cannot be told apart, nor from a hard-coded 0.5, an
ignored alpha0, alpha0·pow(shrink, k) or an α rounded through float. Here the searches run at
(alpha0, shrink) = (0.9, 0.7) and, where a family has more than one forward kernel, (1.5, 0.6);
the backward passes at μ = 0.05 and 0.3 (and 2.0 on the padded wide tiles shapes). The
reference of every comparison is the oracle at the same options, run at test time.

Tolerances are the ones the README's parity paragraph and the existing test of the same kernel
state at the default options (imported where that test exports them). Counts are exact.

Decisions near rounding (the LQ searches): prev_cost is placed by test_coop_forced_vs_oracle's
method — the oracle's cost of every trial alone, a target trial drawn up to the argmin,
prev_cost halfway between that trial's cost and the smallest earlier one; every fifth
trajectory gets an unreachable prev_cost. A case is robust when that gap exceeds 1e-8
relative; the cases kept — the robust ones and the unreachable ones, whose prev_cost sits 1e-3 below
every trial's cost — must be at least half the sample, the robust ones alone at least half of the
reachable ones, and their accepted trial counts take at least 8 values. Here, for (0.9, 0.7) /
(1.5, 0.6): kept 0.73 / 0.68 of the sample at (37, 17) and 0.88 / 0.87 at (2051, 9); robust 0.66 /
0.59 and 0.84 / 0.83 of the reachable; 12 / 10 and 11 / 9 values. Every case prints its own.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ilqr_amd import _lib
from ilqr_amd.problems import LQBatch, quadrotor_batch, random_lq_batch
from ilqr_amd.solver import Solver
from oracle import cref
from oracle import ilqr_oracle as O
from oracle.chain_batch import ChainOracle

pytestmark = pytest.mark.gpu
F64 = torch.float64
PRIMARY = (0.9, 0.7)
SECOND = (1.5, 0.6)
SETS = [PRIMARY, SECOND]
MUS = [0.05, 0.3]
LQ_SHAPES = [(37, 17), (2051, 9)]
J_TRIALS = 41          # trials whose cost the placement looks at
ROBUST_GAP = 1e-8
# README parity paragraph / test_gpu_parity.py
TOL_ROLL, TOL_COST, TOL_LQ_FIT, TOL_LQ_FIT_COST = 1e-10, 1e-11, 1e-8, 1e-9


def dev(a, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def rel(a, b):
    a = a.double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, float)
    b = b.double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def inf(nb, dtype=F64):
    return torch.full((nb,), float("inf"), dtype=dtype, device="cuda")


def opts(a0s=None, **kw):
    if a0s is not None:
        kw.update(alpha0=a0s[0], shrink=a0s[1])
    return _lib.default_options(**kw)


def repeated_product(alpha0, shrink, trials):
    """α of trial j: alpha0 multiplied by shrink j − 1 times in turn (forward_pass.jl:82), for
    an array of trial counts (0 → NaN)."""
    tr = np.asarray(trials)
    out = np.full(tr.shape, np.nan)
    a = alpha0
    for j in range(1, int(tr.max(initial=0)) + 1):
        out[tr == j] = a
        a *= shrink
    return out


def assert_alpha_bits(forward_one, out, a0s, what):
    """The search's α of trial j is alpha0 multiplied by shrink j − 1 times in turn, bit for bit: the
    rollout a search accepted at trial j equals, bit for bit, the single trial the same kernel runs
    from that product as alpha0 (a one-ulp change of α moves ū). forward_one(alpha) → that kernel's
    (x̄, ū, cost, …) at alpha0 = alpha, max_trials = 1, prev_cost = Inf."""
    tr, st = out[3].cpu().numpy(), out[4].cpu().numpy()
    checked = []
    for j in np.unique(tr[st == _lib.TRAJ_OK]):
        if j == 1:
            continue
        one = forward_one(float(repeated_product(a0s[0], a0s[1], [j])[0]))
        at = torch.from_numpy((tr == j) & (st == _lib.TRAJ_OK)).cuda()
        for name, a, b in zip(("x", "u", "cost"), out[:3], one[:3]):
            assert torch.equal(a[at], b[at]), (what, int(j), name)
        checked.append(int(j))
    assert len(checked) >= 3, (what, checked)


# =========================================================================================
# LQ at (12, 4)
# =========================================================================================
def lq_cost(lq, x, u, xt):
    """total_cost (forward_pass.jl:185-193) of (x, u) against x_traj, numpy"""
    e = x - xt
    return (np.einsum("bti,bij,btj->b", e[:, :-1], lq.Q, e[:, :-1]) + np.einsum("bti,bij,btj->b", u, lq.R, u)
            + np.einsum("bi,bij,bj->b", x[:, -1], lq.Qf, x[:, -1]))


def forced(lq, x, u, seed=5):
    """test_gpu_line_search.forced_case's construction on any LQ batch: the cold-start iterate
    and a line-search objective offset by a random x_traj per trajectory."""
    d, K, _ = cref.lq_backward(lq, x, u, symmetrize=True)
    x1, u1, _, _ = cref.lq_forward(lq, x, u, None, d, K, np.inf)
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 1, x.shape[0])
    xt = x1 + scale[:, None, None] * rng.standard_normal(x1.shape)
    return x1, u1, xt


@functools.lru_cache(maxsize=None)
def lq_problem(nb, T, nx=12, nu=4):
    if (nx, nu) == (12, 4):
        lq, x, u = quadrotor_batch(nb, T=T, seed0=0)
    else:
        lq, x, u = random_lq_batch(nb, nx, nu, T, seed=17 * nx + nu)
    x1, u1, xt = forced(lq, x, u)
    return lq, x1, u1, xt


def sub_batch(lq, idx):
    return LQBatch(lq.A[idx], lq.B[idx], lq.Q[idx], lq.R[idx], lq.Qf[idx])


@functools.lru_cache(maxsize=None)
def placed(nb, T, a0s, nx=12, nu=4):
    """prev_cost placed above rounding on a sample of the forced workload (the module docstring's
    method), with the oracle's answer at these options. Computed once per (shape, option set)."""
    a0, sh = a0s
    lq, x, u, xt = lq_problem(nb, T, nx, nu)
    idx = np.arange(0, nb, 16 if nb > 512 else 1)
    ns = len(idx)
    sl = sub_batch(lq, idx)
    d, K, _ = cref.lq_backward(sl, x[idx], u[idx], symmetrize=True)
    cj = np.stack([cref.lq_forward(sl, x[idx], u[idx], xt[idx], d, K, -np.inf, max_trials=j, alpha0=a0,
                                   shrink=sh)[2] for j in range(1, J_TRIALS + 1)], 1)   # (sample, J)
    jm = np.argmin(cj, 1)
    js = (np.random.default_rng(3).random(ns) * (jm + 1)).astype(int)          # 0-based target trial
    ar = np.arange(ns)
    before = np.array([cj[k, :js[k]].min() if js[k] > 0 else np.inf for k in range(ns)])
    pc_s = np.where(js > 0, 0.5 * (cj[ar, js] + before), cj[:, 0] + 1e-6 * np.abs(cj[:, 0]))
    robust = (before - cj[ar, js]) > ROBUST_GAP * np.abs(before)
    robust |= js == 0
    unreach = ar % 5 == 0
    pc_s = np.where(unreach, cj.min(1) - 1e-3 * np.abs(cj.min(1)), pc_s)
    keep = robust | unreach
    robust = keep & ~unreach
    xo, uo, co, tro = cref.lq_forward(sl, x[idx], u[idx], xt[idx], d, K, pc_s, alpha0=a0, shrink=sh)
    # the conditions on the sample (not to be relaxed)
    share, values = keep.mean(), np.unique(tro[robust])
    reach_share = robust.sum() / (~unreach).sum()
    print(f"placed({nb}, {T}, {a0s}, ({nx}, {nu})): of the sample of {ns}, share kept {share:.2f} (the unreachable fifth "
          f"included, as test_coop_forced_vs_oracle counts it), gap-robust share of the reachable {reach_share:.2f}, "
          f"{len(values)} accepted trial counts {values.tolist()}")
    assert (tro[robust] > 0).all() and (tro[unreach] < 0).all()
    assert keep.sum() >= 0.5 * ns, share
    assert robust.sum() >= 0.5 * (~unreach).sum(), reach_share    # … and of the placed decisions alone
    assert len(values) >= 8, values
    pc = np.full(nb, np.inf)
    pc[idx] = pc_s
    return dict(lq=lq, x=x, u=u, xt=xt, idx=idx, d=d, K=K, pc=pc, pc_s=pc_s, robust=robust, unreach=unreach,
                xo=xo, uo=uo, co=co, tro=tro)


def check_forward_vs_oracle(c, out, exhausted_returns_inputs, what):
    """Device (x̄, ū, cost, trials, status) on the sample against the oracle: counts and status exact
    on the robust and the unreachable cases, accepted rollouts and costs at the forward tolerances."""
    xn, un, cost, tr, st = (t.cpu().numpy() for t in out)
    idx, keep, acc = c["idx"], c["robust"] | c["unreach"], c["robust"]
    tro = c["tro"]
    np.testing.assert_array_equal(tr[idx][keep], np.where(tro > 0, tro, 64)[keep], err_msg=what)
    np.testing.assert_array_equal(st[idx][keep], np.where(tro > 0, _lib.TRAJ_OK, _lib.TRAJ_LS_EXHAUSTED)[keep],
                                  err_msg=what)
    eu, ex, ec = rel(un[idx][acc], c["uo"][acc]), rel(xn[idx][acc], c["xo"][acc]), rel(cost[idx][acc], c["co"][acc])
    print(f"{what}: u {eu:.3e} x {ex:.3e} cost {ec:.3e}")
    assert eu < TOL_ROLL and ex < TOL_ROLL and ec < TOL_COST, (what, eu, ex, ec)
    if exhausted_returns_inputs:   # test_line_search_exhaustion_returns_inputs
        ex_ = c["unreach"]
        np.testing.assert_array_equal(xn[idx][ex_], c["x"][idx][ex_], err_msg=what)
        np.testing.assert_array_equal(un[idx][ex_], c["u"][idx][ex_], err_msg=what)


FORWARD_KERNELS = {"register": dict(ring_forward=False), "ring": dict(ring_forward=True),
                   "mfma": dict(ring_forward=True, forward_mfma=True)}


@pytest.mark.parametrize("a0s", SETS)
@pytest.mark.parametrize("nb,T,nx,nu", [(37, 17, 12, 4), (2051, 9, 12, 4), (37, 17, 7, 3)])
def test_lq_forward_vs_oracle(gpu, nb, T, nx, nu, a0s):
    """ilqr_forward on the register forward, the ring forward and forward_mfma (selected as
    test_gpu_parity selects them) from the oracle's gains against cref.lq_forward at the same
    alpha0 and shrink, then the fused iteration's cooperative search (ilqr_iterate, its own gains)
    on the same placement. (37, 17) leaves a ragged last wave, (2051, 9) spans workgroups, (7, 3)
    is a padded shape."""
    c = placed(nb, T, a0s, nx, nu)
    lq, idx = c["lq"], c["idx"]
    # the oracle's gains for the sampled trajectories, the device's own for the rest (prev_cost = Inf there)
    s = Solver(nx, nu, T, nb)
    s.set_problem(lq)
    try:
        x, u, xt, pc = dev(c["x"]), dev(c["u"]), dev(c["xt"]), dev(c["pc"])
        d, K, _ = s.backward(x, u)
        d[torch.from_numpy(idx).cuda()] = dev(c["d"])
        K[torch.from_numpy(idx).cuda()] = dev(c["K"])
        outs = {}
        for name, sched in FORWARD_KERNELS.items():
            s.set_schedule(**sched)
            outs[name] = s.forward(x, u, d, K, pc, x_traj=xt, alpha0=a0s[0], shrink=a0s[1])
            check_forward_vs_oracle(c, outs[name], True, f"lq forward[{name}] ({nb}, {T}, {nx}x{nu}) {a0s}")
            assert_alpha_bits(lambda a: s.forward(x, u, d, K, inf(nb), x_traj=xt, alpha0=a, shrink=a0s[1], max_trials=1),
                              outs[name], a0s, f"lq forward[{name}]")
        for a, b in zip(outs["register"], outs["ring"]):   # test_ring_forward_pass_api_equals_register_ring
            torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
        dflt = s.forward(x, u, d, K, pc, x_traj=xt)
        assert not torch.equal(dflt[3], outs["ring"][3])    # the options reached the search
        it = run_iterate(s, c["x"], c["u"], c["xt"], c["pc"], dict(backward="block"), a0s, 64)
        check_forward_vs_oracle(c, (it[0], it[1], it[2], it[5], it[4]), False,
                                f"lq iterate[fused, cooperative] ({nb}, {T}, {nx}x{nu}) {a0s}")
    finally:
        s.close()


def run_iterate(s, x, u, xt, pc, sched, a0s, max_trials, mu=None):
    s.set_schedule(**sched)
    nb = x.shape[0]
    xi, ui = dev(x), dev(u)
    xn = torch.full_like(xi, -7.0)
    un = torch.full_like(ui, -7.0)
    cost = torch.full((nb,), -7.0, dtype=F64, device="cuda")
    du2 = torch.full((nb,), -7.0, dtype=F64, device="cuda")
    st = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    tr = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    s.iterate(xi, ui, xn, un, dev(pc), st, du2=du2, trials=tr, x_traj=dev(xt),
              options=opts(a0s, tol=-1.0, max_trials=max_trials, mu=mu), new_cost=cost)
    torch.cuda.synchronize()
    return [xn, un, cost, du2, st, tr]


ITERATE_SCHEDULES = {
    "fused_coop": dict(backward="block"),
    "fused_seq": dict(backward="block", sequential_search=True),
    "split_ring": dict(backward="block", fused=False),
    "split_register": dict(backward="block", fused=False, ring_forward=False),
    "fused_mfma": dict(backward="block", forward_mfma=True),
    "split_mfma": dict(backward="block", fused=False, forward_mfma=True),
}
ITERATE_PAIRS = [("fused_coop", "fused_seq"), ("fused_coop", "split_ring"), ("split_ring", "split_register"),
                 ("fused_mfma", "split_mfma")]


@pytest.mark.parametrize("max_trials", [7, 64])
@pytest.mark.parametrize("a0s", SETS)
@pytest.mark.parametrize("nb,T", LQ_SHAPES)
def test_lq_iterate_pairs_bit_equal(gpu, nb, T, a0s, max_trials):
    """ilqr_iterate at μ = 0.05 on the placed forced workload (every fifth sampled prev_cost
    unreachable): cooperative = sequential search, fused = two launches, ring = register,
    fused-MFMA = split-MFMA, bit for bit — x̄, ū, cost, Σδu², status and trials."""
    c = placed(nb, T, a0s)
    lq, x, u, xt, pc = c["lq"], c["x"], c["u"], c["xt"], c["pc"]
    s = Solver(12, 4, T, nb)
    s.set_problem(lq)
    try:
        r = {k: run_iterate(s, x, u, xt, pc, v, a0s, max_trials, mu=0.05) for k, v in ITERATE_SCHEDULES.items()}
        dflt = run_iterate(s, x, u, xt, pc, ITERATE_SCHEDULES["fused_coop"], None, max_trials, mu=0.05)
    finally:
        s.close()
    tr, st = r["fused_seq"][5].cpu().numpy(), r["fused_seq"][4].cpu().numpy()
    print(f"lq iterate ({nb}, {T}) {a0s} max_trials {max_trials}: trials {np.bincount(tr).tolist()}")
    assert (tr <= max_trials).all() and (st[c["idx"]][c["unreach"]] == _lib.TRAJ_LS_EXHAUSTED).all()
    assert len(np.unique(tr[st == _lib.TRAJ_OK])) >= (3 if max_trials == 7 else 8)   # the searches spread
    for a, b in ITERATE_PAIRS:
        for name, p, q in zip(("x_new", "u_new", "new_cost", "du2", "status", "trials"), r[a], r[b]):
            torch.testing.assert_close(p, q, rtol=0, atol=0, equal_nan=True, msg=f"{a} vs {b}: {name}")
    assert not torch.equal(dflt[1], r["fused_coop"][1])    # the options reached the search


def result_np(r):
    out = {k: getattr(r, k).cpu().numpy() for k in ("x", "u", "cost", "iters", "status")}
    out["call_status"] = r.call_status
    if r.history is not None:
        out.update({"hist_" + k: v.cpu().numpy() for k, v in r.history.items()})
    return out


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def lq_fit_np(lq, x, u, T, nb, sched, **kw):
    s = Solver(12, 4, T, nb)
    s.set_problem(lq)
    s.set_schedule(backward="block", **sched)
    try:
        return result_np(s.fit(dev(x), dev(u), **kw))
    finally:
        s.close()


FIT_KW = dict(mu=0.05, alpha0=PRIMARY[0], shrink=PRIMARY[1], history=True)


@functools.lru_cache(maxsize=None)
def lq_fit_case(nb, T):
    """The headline problem from cold, and an x_traj for the fits compared bit for bit: a random
    tracking target that makes later iterations shorten their steps or exhaust."""
    lq, x, u = quadrotor_batch(nb, T=T, seed0=0)
    rng = np.random.default_rng(7)
    xt = 0.1 * rng.standard_normal(x.shape) * (10.0 ** rng.uniform(-1, 1, nb))[:, None, None]
    return lq, x, u, xt


@pytest.mark.parametrize("max_iter,tol", [(6, -1.0), (12, 1e-8)])
@pytest.mark.parametrize("nb,T", LQ_SHAPES)
def test_lq_fit_vs_oracle(gpu, nb, T, max_iter, tol):
    """fit at μ = 0.05, alpha0 = 0.9, shrink = 0.7 against cref.lq_fit at the same options: iteration
    counts, statuses and every iteration's trial count exactly, iterates and costs at the parity
    tolerances. Near the optimum an iteration lowers the cost by less than the project's cost parity
    (rel 1e-11, TOL_COST): a trajectory counts when every accept/reject decision of its oracle fit
    stayed further than that from prev_cost (the oracle's own "gap") and every Σδu² further than
    1e-6 relative from tol; those must be at least half the batch. Measured shares: (37, 17) 1.00 with
    tol disabled and 0.54 at tol 1e-8 (whose iterations 6-9 sit at the cost floor); (2051, 9) 0.99
    and 0.75."""
    lq, x, u, _ = lq_fit_case(nb, T)
    r = lq_fit_np(lq, x, u, T, nb, {}, max_iter=max_iter, tol=tol, **FIT_KW)
    xo, uo, co, it, st, h = cref.lq_fit(lq, x, u, max_iter=max_iter, tol=tol, mu=0.05, symmetrize=True,
                                        alpha0=PRIMARY[0], shrink=PRIMARY[1], history=True)
    n = int(it.max())
    ran = h["trials"] > 0
    ok = np.nanmin(np.where(ran, h["gap"], np.inf), 0) > TOL_COST
    if tol > 0:
        ok &= np.nanmin(np.where(ran, np.abs(h["du2"] / tol - 1.0), np.inf), 0) > 1e-6
    print(f"lq fit ({nb}, {T}) max_iter {max_iter} tol {tol}: iterations {np.bincount(it).tolist()}, "
          f"statuses {np.bincount(st).tolist()}, share that counts {ok.mean():.2f}")
    assert ok.sum() >= 0.5 * nb
    np.testing.assert_array_equal(r["iters"][ok], it[ok])
    np.testing.assert_array_equal(r["status"][ok], st[ok])
    np.testing.assert_array_equal(r["hist_trials"][:n, ok], h["trials"][:n, ok])
    eu, ex, ec = rel(r["u"][ok], uo[ok]), rel(r["x"][ok], xo[ok]), rel(r["cost"][ok], co[ok])
    print(f"lq fit ({nb}, {T}): u {eu:.3e} x {ex:.3e} cost {ec:.3e}")
    assert eu < TOL_LQ_FIT and ex < TOL_LQ_FIT and ec < TOL_LQ_FIT_COST, (eu, ex, ec)
    assert_history_alpha(r, PRIMARY)


def assert_history_alpha(r, a0s):
    """The record's alpha is alpha0 multiplied by shrink trials − 1 times in turn, bit for bit
    (NaN where the cost is NaN: include/ilqr.h)."""
    want = repeated_product(a0s[0], a0s[1], r["hist_trials"])
    want[np.isnan(r["hist_cost"])] = np.nan
    np.testing.assert_array_equal(r["hist_alpha"], want)


@pytest.mark.parametrize("nb,T", LQ_SHAPES)
def test_lq_fit_same_bits_across_schedules_handles_and_calls(gpu, nb, T):
    """The same fit (μ = 0.05, (0.9, 0.7), 6 iterations, tol disabled, an x_traj that makes the later
    searches long): the history's alpha is the repeated product over many trial counts; gain reuse =
    full_backward, MultiSolver([0, 0]) = one handle; and on ONE handle fits at the defaults, at
    (0.9, 0.7) and at the defaults again each equal a fresh handle's — the stored gains do not
    depend on α, the results must."""
    from ilqr_amd.multi import MultiSolver
    lq, x, u, xt = lq_fit_case(nb, T)
    kw = dict(max_iter=6, tol=-1.0, **FIT_KW)
    dkw = dict(max_iter=6, tol=-1.0, mu=0.05, history=True)

    def fit(s, k):
        return result_np(s.fit(dev(x), dev(u), x_traj=dev(xt), **k))

    def fresh(k, **sched):
        s = Solver(12, 4, T, nb)
        s.set_problem(lq)
        s.set_schedule(backward="block", **sched)
        try:
            return fit(s, k)
        finally:
            s.close()

    reuse = fresh(kw)
    tr = reuse["hist_trials"]
    print(f"lq fit x_traj ({nb}, {T}): trials {np.bincount(tr.ravel()).tolist()}")
    assert len(np.unique(tr[(tr > 0) & np.isfinite(reuse['hist_cost'])])) >= (3 if nb < 100 else 8)
    assert_history_alpha(reuse, PRIMARY)
    assert_same(reuse, fresh(kw, full_backward=True), "reuse vs full_backward")
    ms = MultiSolver([0, 0], 12, 4, T, nb)
    try:
        ms.set_schedule(backward="block")
        xo, uo, co, it, st, rc = ms.fit(lq, x, u, x_traj=xt, max_iter=6, tol=-1.0, mu=0.05, alpha0=PRIMARY[0],
                                        shrink=PRIMARY[1])
    finally:
        ms.close()
    for k, v in (("x", xo), ("u", uo), ("cost", co), ("iters", it), ("status", st)):
        np.testing.assert_array_equal(v, reuse[k], err_msg=f"multi vs one handle: {k}")
    assert rc == reuse["call_status"]
    fresh_default = fresh(dkw)
    s = Solver(12, 4, T, nb)
    s.set_problem(lq)
    s.set_schedule(backward="block")
    try:
        a = fit(s, dkw)
        b = fit(s, kw)
        c = fit(s, dkw)
        rec = s.reuse_record()
    finally:
        s.close()
    assert_same(a, fresh_default, "first call, defaults")
    assert_same(b, reuse, "second call, (0.9, 0.7)")
    assert_same(c, fresh_default, "third call, defaults")
    assert rec.size and (rec == 1).all()       # … and the third call did reuse the handle's gains
    assert not np.array_equal(a["u"], b["u"])


# =========================================================================================
# Tiles backward
# =========================================================================================
@pytest.mark.parametrize("n,m", [(5, 3), (12, 4), (13, 7), (16, 5), (16, 8)])
def test_tiles_backward_mu(gpu, n, m):
    """ilqr_backward_tiles at μ = 0.05 and 0.3 on the one-tile and the wide kernel against
    cref.tiles_backward(mu=…, symmetrize=True) at test_gpu_tiles' 1e-10; μ = 2.0 as well on the wide
    shapes with padded control rows, whose pivots the kernel sets to 1 − μ."""
    from test_gpu_tiles import random_tiles, to_dev
    nb, T = 5, 9
    tl = random_tiles(nb, T, n, m, seed=4000 + 100 * n + m)
    s = Solver(n, m, T, nb, kind=_lib.PROBLEM_TILES)
    got = {}
    try:
        for mu in MUS + ([2.0] if (n > 12 or m > 4) and m < 8 else []):
            d, K, st = s.backward_tiles(to_dev(tl), mu=mu)
            dr, Kr, _ = cref.tiles_backward(tl, mu=mu, symmetrize=True)
            ed, ek = rel(d, dr), rel(K, Kr)
            print(f"tiles ({n}, {m}) mu {mu}: d {ed:.3e} K {ek:.3e}")
            assert (st.cpu().numpy() == 0).all()
            assert ed < 1e-10 and ek < 1e-10, (mu, ed, ek)
            got[mu] = Kr
    finally:
        s.close()
    assert rel(got[0.05], got[0.3]) > 1e-3     # μ moves the gains: a kernel that ignored it would miss


# =========================================================================================
# Two-link (nu = 1 and 2, the T = 50 fixtures)
# =========================================================================================
TL_SCALES = [1, 3, 6, 12, 24, 48, 96, 3, 400]      # test_gpu_twolink's search case


@functools.lru_cache(maxsize=None)
def tl_fixture(nu):
    import os
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "twolink_t50.npz" if nu == 2 else
                             "twolink_nu1_t50.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def tl_search_case(nu):
    """test_gpu_twolink._search_case on the nu-input fixture."""
    g = tl_fixture(nu)
    TL = O.TwoLink
    idx = np.arange(len(TL_SCALES)) % g["u"].shape[0]
    x, u, K = g["x"][idx], g["u"][idx], g["K"][idx]
    d = g["d"][idx] * np.asarray(TL_SCALES, dtype=float)[:, None, None]
    pc = np.array([O.total_cost_generator(np.zeros_like(x[i]), TL.immediate_cost, TL.final_cost)(x[i], u[i])
                   for i in range(len(idx))])
    return x, u, d, K, pc


def tl_solver(nu, T, B):
    return Solver(4, nu, T, B, kind=_lib.PROBLEM_TWO_LINK)


@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("nu", [1, 2])
def test_tl_backward_mu(gpu, nu, mu):
    from test_gpu_twolink import TOL_GAIN
    g = tl_fixture(nu)
    nb, T = g["u"].shape[:2]
    s = tl_solver(nu, T, nb)
    try:
        d, K, st = s.backward(dev(g["x"]), dev(g["u"]), mu=mu)
    finally:
        s.close()
    dr, Kr, _ = cref.tl_backward(g["x"], g["u"], mu=mu)
    ed, ek = rel(d, dr), rel(K, Kr)
    print(f"two-link nu {nu} mu {mu}: d {ed:.3e} K {ek:.3e}; gains moved by {rel(Kr, g['K']):.2e} from mu 0.01")
    assert (st.cpu().numpy() == _lib.TRAJ_OK).all()
    assert ed < TOL_GAIN and ek < TOL_GAIN, (ed, ek)
    assert rel(Kr, g["K"]) > 1e-4


@pytest.mark.parametrize("max_trials", [64, 6])
@pytest.mark.parametrize("a0s", SETS)
@pytest.mark.parametrize("nu", [1, 2])
def test_tl_forward_candidate_groups(gpu, nu, a0s, max_trials):
    """The four-candidate groups with δu scaled per trajectory (trials from 1 to past the second
    round) against O.forward_pass(alpha0=, shrink=): the trial accepted, its rollout and cost at
    test_tl_forward_candidates_match_sequential's tolerances. max_trials = 6 ends inside the second
    round: the searches that need more are exhausted and return their inputs. Every accept/reject
    decision of the case is further than 1e-8 relative from prev_cost (asserted on the C oracle's
    per-trial costs)."""
    from test_gpu_twolink import TOL_COST as TL_COST
    TL = O.TwoLink
    f = TL.dynamicsf if nu == 2 else TL.dynamicsf_nu1
    x, u, d, K, pc = tl_search_case(nu)
    nb, T = u.shape[:2]
    tro = cref.tl_forward(x, u, None, d, K, pc, max_trials=64, alpha0=a0s[0], shrink=a0s[1])[3]
    for j in range(1, int(tro.max()) + 1):   # the margins of every decision taken
        cj = cref.tl_forward(x, u, None, d, K, -np.inf, max_trials=1,
                             alpha0=float(repeated_product(a0s[0], a0s[1], [j])[0]), shrink=a0s[1])[2]
        took = (tro >= j) & np.isfinite(cj)      # (an overshooting trial may cost NaN: rejected)
        assert (np.abs(cj - pc)[took] > ROBUST_GAP * pc[took]).all(), (j, cj, pc)
        assert ((cj < pc) == (tro == j))[took].all(), j
    s = tl_solver(nu, T, nb)
    try:
        out = s.forward(dev(x), dev(u), dev(d), dev(K), dev(pc), alpha0=a0s[0], shrink=a0s[1], max_trials=max_trials)
        xn, un, cost, trials, st = (t.cpu().numpy() for t in out)
        # the candidate groups' α₀·shrink^(r·L+sub) by two chained loops is the repeated product
        assert_alpha_bits(lambda a: s.forward(dev(x), dev(u), dev(d), dev(K), inf(nb), alpha0=a, shrink=a0s[1],
                                              max_trials=1), out, a0s, f"two-link forward nu {nu}")
    finally:
        s.close()
    seen = set()
    cro = cref.tl_forward(x, u, None, d, K, pc, max_trials=max_trials, alpha0=a0s[0], shrink=a0s[1])
    for i in range(nb):
        so = {}
        try:
            xo, uo, co = O.forward_pass(x[i], u[i], np.zeros_like(x[i]), d[i], K[i], pc[i], f, TL.immediate_cost,
                                        TL.final_cost, max_trials=max_trials, alpha0=a0s[0], shrink=a0s[1], stats=so)
        except O.LineSearchExhausted:
            assert st[i] == _lib.TRAJ_LS_EXHAUSTED and trials[i] == max_trials, i
            assert np.array_equal(xn[i], x[i]) and np.array_equal(un[i], u[i]), i
            seen.add(-1)
            continue
        except ValueError as e:
            assert "math domain error" in str(e), e
            # an overshooting trial's state reached Inf, which the numpy restatement's scalar cos
            # refuses (math domain error): this trajectory is checked against the C restatement,
            # whose IEEE arithmetic makes that trial's cost NaN and goes on (tests/test_oracle.py
            # pins the two restatements to each other at these options)
            if cro[3][i] < 0:
                assert st[i] == _lib.TRAJ_LS_EXHAUSTED and trials[i] == max_trials, i
                seen.add(-1)
                continue
            xo, uo, co, so = cro[0][i], cro[1][i], cro[2][i], {"trials": int(cro[3][i])}
            so["alpha"] = repeated_product(a0s[0], a0s[1], [so["trials"]])[0]
        assert st[i] == _lib.TRAJ_OK and trials[i] == so["trials"] == tro[i], (i, trials[i], so, tro[i])
        assert so["alpha"] == repeated_product(a0s[0], a0s[1], [so["trials"]])[0]
        seen.add(so["trials"])
        assert rel(xn[i], xo) < 1e-11 and rel(un[i], uo) < 1e-11, i
        assert abs(cost[i] - co) / co < TL_COST, i
    print(f"two-link forward nu {nu} {a0s} max_trials {max_trials}: trials {sorted(seen)}")
    if max_trials == 64:
        assert max(seen) > 8 and len(seen) >= 5, seen     # past the second round of four
    else:
        assert -1 in seen and (5 in seen or 6 in seen), seen   # ends inside the second round, both ways


@pytest.mark.parametrize("nu", [1, 2])
def test_tl_forward_wide_batch_equals_grouped_off_defaults(gpu, nu):
    """test_tl_forward_wide_batch_equals_grouped at (0.9, 0.7): one lane per trajectory (sequential
    `alpha *= shrink`, past B = 65536) and the candidate groups' two chained loops give the same bits."""
    x, u, d, K, pc = tl_search_case(nu)
    n, T = len(TL_SCALES), u.shape[1]
    Bw = 65544
    rep = np.arange(Bw) % n
    kw = dict(alpha0=PRIMARY[0], shrink=PRIMARY[1])
    sw, ss = tl_solver(nu, T, Bw), tl_solver(nu, T, n)
    try:
        rw = sw.forward(dev(x[rep]), dev(u[rep]), dev(d[rep]), dev(K[rep]), dev(pc[rep]), **kw)
        rs = ss.forward(dev(x), dev(u), dev(d), dev(K), dev(pc), **kw)
        r0 = ss.forward(dev(x), dev(u), dev(d), dev(K), dev(pc))
    finally:
        sw.close()
        ss.close()
    for a, b in zip(rw, rs):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        for off in (0, n * 1000, Bw - n - (Bw % n)):
            np.testing.assert_array_equal(a[off:off + n], b)
    assert not torch.equal(r0[1], rs[1])


@pytest.mark.parametrize("nu", [1, 2])
def test_tl_fit_vs_oracle(gpu, nu):
    """A fit of 4 iterations (tol disabled) at μ = 0.05, (0.9, 0.7) against cref.tl_fit at the same
    options: statuses, iteration counts and every iteration's trial count exactly, the rest at
    test_gpu_twolink._fit_vs_c_oracle's tolerances; the record's alpha is the repeated product."""
    from test_gpu_twolink import TOL_FIT
    g = tl_fixture(nu)
    nb, T = g["u"].shape[:2]
    s = tl_solver(nu, T, nb)
    try:
        r = result_np(s.fit(dev(g["x"]), dev(g["u"]), max_iter=4, tol=-1.0, **FIT_KW))
    finally:
        s.close()
    xo, uo, co, it, st, h = cref.tl_fit(g["x"], g["u"], max_iter=4, tol=-1.0, mu=0.05, symmetrize=True, history=True,
                                        alpha0=PRIMARY[0], shrink=PRIMARY[1])
    print(f"two-link fit nu {nu}: iterations {it.tolist()} trials {h['trials'].T.tolist()}")
    np.testing.assert_array_equal(r["status"], st)
    np.testing.assert_array_equal(r["iters"], it)
    np.testing.assert_array_equal(r["hist_trials"], h["trials"])
    ex, eu, ec = rel(r["x"], xo), rel(r["u"], uo), rel(r["cost"], co)
    print(f"two-link fit nu {nu}: x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < TOL_FIT and eu < TOL_FIT and ec < 1e-11, (ex, eu, ec)
    ran = r["hist_trials"] > 0
    assert float(np.max(np.abs(r["hist_cost"][ran] - h["cost"][ran]) / np.abs(h["cost"][ran]))) < 1e-11
    assert_history_alpha(r, PRIMARY)


# =========================================================================================
# Chains (oracle.chain_batch: the batched oracle)
# =========================================================================================
def chain_inputs(pr, nb, T, seed):
    """x0 at random, small random torques, the oracle's rollout."""
    rng = np.random.default_rng(seed)
    n = pr.n_joints
    x0 = np.concatenate([rng.uniform(-1, 1, (nb, n)), rng.uniform(-0.5, 0.5, (nb, n))], axis=1)
    u = rng.uniform(-0.5, 0.5, (nb, T, pr.nu))
    return x0, u


def chain_search_case(orc, x, u, d, K, a0s, wanted, scale, gap):
    """δu scaled so that the first trials overshoot, and prev_cost placed halfway between the cost of
    the wanted trial (per trajectory, 0-based; −1 = unreachable) and the smallest earlier one. Every
    decision of the oracle's search is then further than `gap` (relative) from prev_cost."""
    nb = len(x)
    J = max(wanted) + 2
    al = repeated_product(a0s[0], a0s[1], np.arange(1, J + 1))
    ds = d * scale
    cj = np.stack([orc.forward(x, u, ds, K, -np.inf, max_trials=1, alpha0=float(a), shrink=a0s[1])[2] for a in al], 1)
    assert np.isfinite(cj).all(), cj      # (a NaN cost would end the device's search as NAN)
    pc = np.empty(nb)
    for b in range(nb):
        j = wanted[b]
        if j < 0:
            pc[b] = -1.0        # no rollout costs less than 0
            continue
        before = cj[b, :j].min() if j > 0 else 2.0 * cj[b, 0]
        assert cj[b, j] < before * (1 - 2 * gap), (b, j, cj[b])
        pc[b] = 0.5 * (cj[b, j] + before)
        assert (np.abs(cj[b, :j + 1] - pc[b]) > gap * pc[b]).all(), (b, cj[b], pc[b])
    return ds, pc


def check_chain_forward(out, orc_out, x, u, wanted, max_trials, tol, what):
    xn, un, c, tr, st = (t.double().cpu().numpy() for t in out)
    xo, uo, co, tro, ok = orc_out
    want_tr = np.array([w + 1 if w >= 0 else max_trials for w in wanted])
    assert tro.tolist() == want_tr.tolist() and ok.tolist() == [w >= 0 for w in wanted], (tro, ok)
    assert tr.astype(int).tolist() == want_tr.tolist(), (what, tr, want_tr)
    assert st.astype(int).tolist() == [_lib.TRAJ_OK if w >= 0 else _lib.TRAJ_LS_EXHAUSTED for w in wanted], (what, st)
    ex, eu, ec = rel(xn[ok], xo[ok]), rel(un[ok], uo[ok]), rel(c[ok], co[ok])
    print(f"{what}: trials {tr.astype(int).tolist()} x {ex:.3e} u {eu:.3e} cost {ec:.3e}")
    assert ex < tol and eu < tol and ec < tol, (what, ex, eu, ec)
    return ~ok


WANTED = [0, 1, 2, 4, -1]       # accepted trial (0-based) per trajectory; −1: exhausted
OVERSHOOT = 10.0                # δu scaled so that the first five trials still overshoot


# the trajectories test_gpu_chain.py's tolerances are stated for
CHAIN2_FIXTURE = {("rbd", 2): "chain2_t100", ("rbd", 1): "chain2_nu1_t100", ("coupled", 2): "chain2c_t40",
                  ("coupled", 1): "chain2c_nu1_t40"}


@functools.lru_cache(maxsize=None)
def chain2_reference(name, nu, f64):
    """The oracle's side of test_chain2_off_defaults, once per (chain, nu, precision of the inputs), on
    the fixture's trajectories (five rows: the fixture's, repeated)."""
    import os
    from ilqr_amd.chain import coupled_2dof_problem, rbd_2dof_problem
    pr = rbd_2dof_problem(nu) if name == "rbd" else coupled_2dof_problem(nu)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", CHAIN2_FIXTURE[name, nu] + ".npz"), allow_pickle=False)
    idx = np.arange(5) % z["u"].shape[0]
    x, u = z["x"][idx], z["u"][idx]
    orc = ChainOracle(pr, u.shape[1])
    if not f64:     # the device's inputs are these values in fp32: the oracle starts from the same
        x, u = x.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
    (dr, Kr), (d01, K01) = orc.backward(x, u, [0.05, 0.01])
    assert rel(K01, Kr) > 1e-4 and rel(d01, dr) > 1e-4      # μ shows in the gains (far above the fp64 bound)
    ds, pc = chain_search_case(orc, x, u, dr, Kr, PRIMARY, WANTED, OVERSHOOT, 1e-8 if f64 else 2e-2)
    fw_o = orc.forward(x, u, ds, Kr, pc, max_trials=8, alpha0=PRIMARY[0], shrink=PRIMARY[1])
    fit_o = orc.fit(x, u, max_iter=3, tol=-1.0, mu=0.05, max_trials=8, alpha0=PRIMARY[0], shrink=PRIMARY[1])
    # … and to convergence, as test_chain_fit_f32 fits (20 iterations at most, tol 1e-6)
    conv_o = None if f64 else orc.fit(x, u, max_iter=20, tol=1e-6, mu=0.05, alpha0=PRIMARY[0], shrink=PRIMARY[1])
    return pr, x, u, dr, Kr, ds, pc, fw_o, fit_o, conv_o


CHAIN2_CASES = [(torch.float64, "dual"), (torch.float32, "dual"), (torch.float32, "fd")]
FP32_FIT_U = 2e-3     # test_chain_fit_f32, test_config5_nu1_fp32_fd_fixture: u of an fp32 fit


def fp32_fit_u_holds(name, lin):
    """Where FP32_FIT_U is asserted: everywhere but the coupled chain under central differences. The
    existing bound is stated on the reference's arm; the coupled chain's fp32 central differences carry
    A, B errors of 1e-3 (test_coupled_chain_backward, whose gain bound is four times the arm's), and no
    existing test fits it in fp32. Measured on the MI355X, u against the oracle, 3 iterations / to
    convergence: arm "dual" 5e-7 / 5e-5, arm "fd" 1.0e-3 to 1.7e-3 / 0.9e-3 to 1.1e-3, coupled "dual"
    3e-7 / 2e-4 to 5e-4, coupled "fd" 2.8e-3 to 4.9e-3 / 1.4e-3 to 3.7e-3. The bound is kept as it
    stands on every case it can hold for; the coupled
    "fd" fits are held to the statuses, the counts and the cost bound only, their u error printed."""
    return not (name == "coupled" and lin == "fd")


@pytest.mark.parametrize("dyn", ["closed_form", "rnea"])
@pytest.mark.parametrize("dtype,lin", CHAIN2_CASES)
@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("name", ["rbd", "coupled"])
def test_chain2_off_defaults(gpu, name, nu, dtype, lin, dyn):
    """Chains of 2 joints (the reference's arm and the coupled one), nu = 1 and 2, fp64 (dual numbers)
    and fp32 (dual numbers and central differences, as test_chain_fit_f32), closed-form and recursive
    dynamics, on the trajectories of test_gpu_chain.py's fixtures (five rows), against the RBD oracle:
    backward at μ = 0.05, forward at (0.9, 0.7) accepted at trials 1, 2, 3, 5 and exhausted once, a
    3-iteration fit at both and, in fp32, the fit to convergence as well.
    Tolerances: test_gpu_chain.py's — gains TOL[(dtype, linearisation)] with its coupled-chain fp32
    central-difference bound; the forward from given gains TOL[(dtype, "dual")]["fw"], ×10 on the
    coupled chain as test_coupled_chain_forward_rollout; the fp64 fit test_chain_fit_f64's; the fp32
    fits test_chain_fit_f32's: statuses, cost 1e-4, u 2e-3 (fp32_fit_u_holds says where the last is asserted).
    In fp32, μ = 0.05 against 0.01 moves the gains by 2e-3: above the fp32 dual-number gain bound
    (5e-4), below the central-difference one — fp64 and fp32 "dual" can tell a backward that ignored μ."""
    from ilqr_amd.chain import ChainSolver
    from test_gpu_chain import TOL as TOL2
    f64 = dtype == torch.float64
    t = dict(TOL2[(dtype, lin)])
    if (dtype, lin) == (torch.float32, "fd") and name == "coupled":
        t["gain"] = 2e-2          # test_coupled_chain_backward
    pr, x, u, dr, Kr, ds, pc, fw_o, fit_o, conv_o = chain2_reference(name, nu, f64)
    nb, T = u.shape[:2]
    what = f"chain2[{name}, nu {nu}, {dtype}, {lin}, {dyn}]"
    s = ChainSolver(pr, T, nb, dtype=dtype, linearization=lin)
    try:
        s.set_dynamics(dyn)
        assert s.dynamics_mode == dyn
        xd, ud = dev(x, dtype), dev(u, dtype)
        d, K, st = s.backward(xd, ud, options=opts(mu=0.05))
        ek, ed = rel(K, Kr), rel(d, dr)
        print(f"{what} mu 0.05: K {ek:.3e} d {ed:.3e}")
        assert (st.cpu().numpy() == 0).all() and ek < t["gain"] and ed < t["gain"], (ek, ed)
        out = s.forward(xd, ud, dev(ds, dtype), dev(Kr, dtype), dev(pc, dtype), options=opts(PRIMARY, max_trials=8))
        tfw = TOL2[(dtype, "dual")]["fw"] * (10 if name == "coupled" else 1)
        ex_ = check_chain_forward(out, fw_o, x, u, WANTED, 8, tfw, f"{what} forward")
        assert torch.equal(out[0][torch.from_numpy(ex_).cuda()], xd[torch.from_numpy(ex_).cuda()])
        if f64:     # (an fp32 kernel multiplies in fp32: its product is not this one rounded)
            assert_alpha_bits(lambda a: s.forward(xd, ud, dev(ds, dtype), dev(Kr, dtype), inf(nb, dtype),
                                                  options=opts((a, PRIMARY[1]), max_trials=1)), out, PRIMARY,
                              f"{what} forward")
        r = s.fit(xd, ud, options=opts(PRIMARY, max_iter=3, tol=-1.0, mu=0.05, max_trials=8), history=True)
        rc = None if f64 else s.fit(xd, ud, options=opts(PRIMARY, max_iter=20, tol=1e-6, mu=0.05))
    finally:
        s.close()
    eu, ec = rel(r.u, fit_o["u"]), rel(r.cost, fit_o["cost"])
    print(f"{what} fit of 3: iters {r.iters.tolist()} status {r.status.tolist()} u {eu:.3e} cost {ec:.3e}, "
          f"oracle trials {fit_o['history']['trials'].T.tolist()}")
    # the three iterations' decisions are far from rounding in either precision (every iteration lowers
    # the cost by more than 1e-4 of it at its first trial): counts and statuses exactly
    assert r.iters.tolist() == fit_o["iters"].tolist() and r.status.tolist() == fit_o["status"].tolist()
    assert r.history["trials"][:3].cpu().tolist() == fit_o["history"]["trials"].tolist()
    if f64:
        assert eu < 1e-8 and rel(r.x, fit_o["x"]) < 1e-8 and ec < 1e-10, (eu, ec)   # test_chain_fit_f64
        assert_history_alpha(result_np(r), PRIMARY)
        return
    assert ec < 1e-4, ec
    euc, ecc = rel(rc.u, conv_o["u"]), rel(rc.cost, conv_o["cost"])
    print(f"{what} fit to convergence: iters {rc.iters.tolist()} (oracle {conv_o['iters'].tolist()}) status "
          f"{rc.status.tolist()} u {euc:.3e} cost {ecc:.3e}")
    # test_chain_fit_f32's set, and MAX_ITER where the oracle itself is still running after 20 iterations
    assert set(rc.status.tolist()) <= {_lib.TRAJ_CONVERGED, _lib.TRAJ_LS_EXHAUSTED} | set(conv_o["status"].tolist()), rc.status
    assert ecc < 1e-4, ecc
    if fp32_fit_u_holds(name, lin):
        assert eu < FP32_FIT_U and euc < FP32_FIT_U, (eu, euc)


# -- chains of 4 and 7 joints ---------------------------------------------------------------
TASK_GOAL = {4: [1.9, 0.9, 1.0], 7: [2.9, 1.3, 1.3]}      # make_golden_chainN's reachable targets
JOINT_OFFSETS = np.array([[0.0] * 7, [0.35, -0.25, 0.3, -0.4, 0.2, -0.3, 0.25], [-0.3, 0.4, -0.2, 0.25, -0.35, 0.2, -0.15],
                          [0.2, 0.1, -0.3, 0.15, 0.3, -0.2, 0.1], [-0.15, -0.35, 0.25, 0.3, -0.1, 0.35, -0.3]])


def chain_fit_replay_options(s, x0, u0, o):
    """test_gpu_chain6.chain_fit_replay with the caller's options (alpha0, shrink and μ ride along)."""
    nb = x0.shape[0]
    s._bind()
    x, u = x0.clone(), u0.clone()
    pc = inf(nb)
    st = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    tr = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    it_out = torch.zeros((nb,), dtype=torch.int32, device="cuda")
    rx, ru = x0.clone(), u0.clone()
    for it in range(1, o.max_iter + 1):
        run = st == 0
        if not bool(run.any()):
            break
        xn, un = torch.empty_like(x), torch.empty_like(u)
        tr.fill_(-1)
        s.iterate(x, u, xn, un, pc, st, pc, trials=tr, options=o)
        it_out[run & (tr != -1)] = it
        stopped = run & (st != 0)
        rx[stopped], ru[stopped] = x[stopped], u[stopped]
        keep = run & (st == 0)
        x = torch.where(keep[:, None, None], xn, x)
        u = torch.where(keep[:, None, None], un, u)
    run = st == 0
    rx[run], ru[run] = x[run], u[run]
    st = torch.where(run, torch.full_like(st, _lib.TRAJ_MAX_ITER), st)
    return rx, ru, pc, it_out, st


@pytest.mark.parametrize("n,cost,rows", [(4, "joint", False), (4, "task", False), (7, "joint", True), (7, "task", False)])
def test_chainN_off_defaults(gpu, n, cost, rows):
    """coupled_chain_problem(n), fp64, T = 12, B = 5, under the joint-space and the task-space costs and
    once with a goal per trajectory: backward at μ = 0.05 under "fd" and "analytic", forward at (0.9,
    0.7) accepted at trials 1, 2, 3, 5 and exhausted once, a 3-iteration fit with exact iteration and
    trial counts, and the fit equal to its ilqr_chain_iterate replay bit for bit under the same
    options. Tolerances: test_gpu_chain6.py's and test_gpu_chain6_task.py's, imported."""
    from ilqr_amd.chain import ChainSolver, coupled_chain_problem
    from test_gpu_chain6 import COST_TOL, FIT_TOL
    from test_gpu_chain6 import TOL as TOL6
    from test_gpu_chain6_task import TOL as TASK_TOL
    tols = TOL6 if cost == "joint" else TASK_TOL
    pr = coupled_chain_problem(n)
    nb, T = 5, 12
    task = dict(body=n - 1, point=[0.05, 0.02, 0.1], final_target=TASK_GOAL[n], weight=2e3, euclidean=True) \
        if cost == "task" else None
    targets = np.asarray(pr.target, float) + JOINT_OFFSETS[:, :n] if rows else None
    orc = ChainOracle(pr, T, targets=targets, task=task)
    x0, u = chain_inputs(pr, nb, T, seed=60 + n)
    x = orc.rollout(x0, u)
    (dr, Kr), (d01, K01) = orc.backward(x, u, [0.05, 0.01])
    assert rel(K01, Kr) > 10 * tols["fd"]["gain"] and rel(d01, dr) > 10 * tols["fd"]["gain"]   # μ shows
    ds, pc = chain_search_case(orc, x, u, dr, Kr, PRIMARY, WANTED, OVERSHOOT, 1e-8)
    fw_o = orc.forward(x, u, ds, Kr, pc, max_trials=8, alpha0=PRIMARY[0], shrink=PRIMARY[1])
    fit_o = orc.fit(x, u, max_iter=3, tol=-1.0, mu=0.05, max_trials=8, alpha0=PRIMARY[0], shrink=PRIMARY[1])
    xd, ud = dev(x), dev(u)
    what = f"chain{n}[{cost}{', goal per trajectory' if rows else ''}]"

    def solver(lin):
        s = ChainSolver(pr, T, nb, dtype=F64, linearization=lin)
        if task is not None:
            s.set_simple_costs(task["body"], task["point"], task["final_target"], task["weight"], task["euclidean"])
        if rows:
            s.set_joint_targets(dev(targets))
        return s

    for lin in ("fd", "analytic"):
        s = solver(lin)
        try:
            d, K, st = s.backward(xd, ud, options=opts(mu=0.05))
        finally:
            s.close()
        ek, ed = rel(K, Kr), rel(d, dr)
        print(f"{what} backward[{lin}] mu 0.05: K {ek:.3e} d {ed:.3e}")
        tg = tols["fd" if lin == "fd" else "dual"]["gain"]
        assert (st.cpu().numpy() == 0).all() and ek < tg and ed < tg, (lin, ek, ed)
    s = solver("dual")
    try:
        out = s.forward(xd, ud, dev(ds), dev(Kr), dev(pc), options=opts(PRIMARY, max_trials=8))
        ex_ = check_chain_forward(out, fw_o, x, u, WANTED, 8, tols["dual"]["fw"], f"{what} forward")
        assert torch.equal(out[0][torch.from_numpy(ex_).cuda()], xd[torch.from_numpy(ex_).cuda()])
        assert_alpha_bits(lambda a: s.forward(xd, ud, dev(ds), dev(Kr), inf(nb), options=opts((a, PRIMARY[1]), max_trials=1)),
                          out, PRIMARY, f"{what} forward")
        o = opts(PRIMARY, max_iter=3, tol=-1.0, mu=0.05, max_trials=8)
        r = s.fit(xd, ud, options=o, history=True)
        replay = chain_fit_replay_options(s, xd, ud, o)
    finally:
        s.close()
    eu, ex, ec = rel(r.u, fit_o["u"]), rel(r.x, fit_o["x"]), rel(r.cost, fit_o["cost"])
    print(f"{what} fit: iters {r.iters.tolist()} trials {fit_o['history']['trials'].T.tolist()} x {ex:.3e} "
          f"u {eu:.3e} cost {ec:.3e}")
    assert r.iters.tolist() == fit_o["iters"].tolist() and r.status.tolist() == fit_o["status"].tolist()
    assert r.history["trials"][:3].cpu().tolist() == fit_o["history"]["trials"].tolist()
    assert ex < FIT_TOL and eu < FIT_TOL and ec < COST_TOL, (ex, eu, ec)
    assert_history_alpha(result_np(r), PRIMARY)
    for a, b in zip((r.x, r.u, r.cost, r.iters, r.status), replay):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


# =========================================================================================
# Floating base
# =========================================================================================
def test_floating_fit_off_defaults(gpu):
    """A 2-iteration fit at T = 30, B = 4 with (0.9, 0.7) against closure_fit.fit at the same options
    (test_floating_fit_script_shape_vs_closure_oracle's checks and tolerances)."""
    from closures import jet_ns, rbd_cost_quads, rbd_floating_arm
    from ilqr_amd.floating import FloatingSolver, rbd_example_problem
    from oracle import closure_fit as CF
    from test_gpu_floating import script_batch
    nb, T, iters = 4, 30, 2
    x, u = script_batch(nb, T)
    s = FloatingSolver(rbd_example_problem(), T, nb)
    try:
        xd, ud = torch.from_numpy(x).cuda(), torch.from_numpy(u).cuda()
        r = s.fit(xd, ud, options=opts(PRIMARY, max_iter=iters, tol=1e-6), history=True)
        r0 = s.fit(xd, ud, max_iter=iters, tol=1e-6)
    finally:
        s.close()
    fj, lj, lfj = rbd_floating_arm(jet_ns())
    o = CF.fit(x, u, fj, lj, lfj, *rbd_cost_quads(), max_iter=iters, tol=1e-6, alpha0=PRIMARY[0], shrink=PRIMARY[1])
    print(f"floating fit: iters {o['iters'].tolist()} trials {o['history']['trials'].T.tolist()}")
    assert r.iters.tolist() == o["iters"].tolist() and r.status.tolist() == o["status"].tolist()
    assert r.history["trials"][:iters].cpu().tolist() == o["history"]["trials"].tolist()
    assert rel(r.history["cost"][:iters], o["history"]["cost"]) < 1e-8
    assert rel(r.cost, o["cost"]) < 1e-8 and rel(r.x, o["x"]) < 1e-8 and rel(r.u, o["u"]) < 1e-8
    assert_history_alpha(result_np(r), PRIMARY)
    assert rel(r0.u, o["u"]) > 1e-6           # the default options give another iterate


# =========================================================================================
# Refusals
# =========================================================================================
NAN = float("nan")
BAD_OPTIONS = ([dict(shrink=v) for v in (0.0, 1.0, 1.5, NAN)] + [dict(alpha0=v) for v in (0.0, -1.0, NAN)]
               + [dict(mu=NAN), dict(max_trials=0)])
SENT = -7.0


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t.ctypes.data)


class Bufs:
    """Sentinel-filled arguments of one handle's entry points."""

    def __init__(self, nb, T, nx, nu, dtype=F64, host=False):
        def full(*shape, dt=dtype):
            if host:
                return np.full(shape, SENT, dtype=np.float64 if dt.is_floating_point else np.int32)
            return torch.full(shape, SENT, dtype=dt, device="cuda")
        i32 = torch.int32
        self.x, self.u = full(nb, T + 1, nx), full(nb, T, nu)
        self.d, self.K = full(nb, T, nu), full(nb, T, nu, nx)
        self.xn, self.un = full(nb, T + 1, nx), full(nb, T, nu)
        self.pc, self.cost, self.du2 = full(nb), full(nb), full(nb)
        self.tr, self.st, self.it = full(nb, dt=i32), full(nb, dt=i32), full(nb, dt=i32)
        self.hist = {k: full(3, nb, dt=i32 if k == "trials" else F64) for k in ("cost", "trials", "alpha", "du2")}
        self.outs = [self.d, self.K, self.xn, self.un, self.cost, self.du2, self.tr, self.st, self.it] + list(self.hist.values())

    def history(self):
        return _lib.History(*(self.hist[k].data_ptr() for k in ("cost", "trials", "alpha", "du2")))

    def untouched(self):
        return all(bool((t == SENT).all()) if isinstance(t, torch.Tensor) else bool((t == SENT).all()) for t in self.outs)


def refused(calls, b, what):
    """Every call under every bad option set returns BAD_ARG and writes nothing."""
    for bad in BAD_OPTIONS:
        o = _lib.default_options(max_iter=3, **bad)
        for name, call in calls.items():
            rc = call(C.byref(o))
            assert rc == _lib.ERR_BAD_ARG, (what, name, bad, rc)
    torch.cuda.synchronize()
    assert b.untouched(), what


@pytest.mark.parametrize("kind", ["lq", "two_link"])
def test_refusals_ilqr_entries(gpu, kind):
    nb, T = 5, 7
    nx, nu = (12, 4) if kind == "lq" else (4, 2)
    s = Solver(nx, nu, T, nb, kind=_lib.PROBLEM_LQ if kind == "lq" else _lib.PROBLEM_TWO_LINK)
    if kind == "lq":
        s.set_problem(random_lq_batch(nb, nx, nu, T, seed=1)[0])
    b = Bufs(nb, T, nx, nu)
    hst = b.history()
    lib, h, p = s.lib, s.h, s._p()
    s._bind_stream()
    calls = {
        "ilqr_backward": lambda o: lib.ilqr_backward(h, p, o, P(b.x), P(b.u), P(b.d), P(b.K), P(b.st)),
        "ilqr_forward": lambda o: lib.ilqr_forward(h, p, o, P(b.x), P(b.u), None, P(b.d), P(b.K), P(b.pc), P(b.xn),
                                                   P(b.un), P(b.cost), P(b.tr), P(b.st)),
        "ilqr_iterate": lambda o: lib.ilqr_iterate(h, p, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.pc), P(b.cost),
                                                   P(b.du2), P(b.tr), P(b.st)),
        "ilqr_fit": lambda o: lib.ilqr_fit(h, p, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.cost), P(b.it), P(b.st)),
        "ilqr_fit_ex": lambda o: lib.ilqr_fit_ex(h, p, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.cost), P(b.it),
                                                 P(b.st), C.byref(hst)),
    }
    try:
        refused(calls, b, kind)
    finally:
        s.close()


def test_refusals_tiles(gpu):
    nb, T, nx, nu = 5, 7, 13, 7
    s = Solver(nx, nu, T, nb, kind=_lib.PROBLEM_TILES)
    b = Bufs(nb, T, nx, nu)
    shapes = {"A": (nb, T, nx, nx), "B": (nb, T, nx, nu), "lx": (nb, T, nx), "lu": (nb, T, nu), "lxx": (nb, T, nx, nx),
              "lux": (nb, T, nu, nx), "luu": (nb, T, nu, nu), "lfx": (nb, nx), "lfxx": (nb, nx, nx)}
    tiles = {k: torch.zeros(v, dtype=F64, device="cuda") for k, v in shapes.items()}
    tl = _lib.Tiles(*(tiles[k].data_ptr() for k in shapes))
    s._bind_stream()
    try:
        refused({"ilqr_backward_tiles": lambda o: s.lib.ilqr_backward_tiles(s.h, C.byref(tl), o, P(b.d), P(b.K), P(b.st))},
                b, "tiles")
    finally:
        s.close()


@pytest.mark.parametrize("n", [2, 4])
def test_refusals_chain(gpu, n):
    from ilqr_amd.chain import ChainSolver, coupled_chain_problem, rbd_2dof_problem
    pr = rbd_2dof_problem(2) if n == 2 else coupled_chain_problem(n)
    nb, T = 5, 7
    s = ChainSolver(pr, T, nb, dtype=F64)
    b = Bufs(nb, T, pr.nx, pr.nu)
    hst = b.history()
    lib, h = s.lib, s.h
    s._bind()
    calls = {
        "backward": lambda o: lib.ilqr_chain_backward(h, o, P(b.x), P(b.u), P(b.d), P(b.K), P(b.st)),
        "forward": lambda o: lib.ilqr_chain_forward(h, o, P(b.x), P(b.u), None, P(b.d), P(b.K), P(b.pc), P(b.xn), P(b.un),
                                                    P(b.cost), P(b.tr), P(b.st)),
        "iterate": lambda o: lib.ilqr_chain_iterate(h, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.pc), P(b.cost),
                                                    P(b.du2), P(b.tr), P(b.st)),
        "fit": lambda o: lib.ilqr_chain_fit(h, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.cost), P(b.it), P(b.st)),
        "fit_ex": lambda o: lib.ilqr_chain_fit_ex(h, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.cost), P(b.it),
                                                  P(b.st), C.byref(hst)),
    }
    try:
        refused(calls, b, f"chain{n}")
    finally:
        s.close()


def test_refusals_floating(gpu):
    from ilqr_amd.floating import FloatingSolver, rbd_example_problem
    nb, T = 3, 5
    s = FloatingSolver(rbd_example_problem(), T, nb)
    b = Bufs(nb, T, 16, 8)
    hst = b.history()
    lib, h = s.lib, s.h
    s._bind()
    calls = {
        "backward": lambda o: lib.ilqr_floating_backward(h, o, P(b.x), P(b.u), P(b.d), P(b.K), P(b.st)),
        "forward": lambda o: lib.ilqr_floating_forward(h, o, P(b.x), P(b.u), None, P(b.d), P(b.K), P(b.pc), P(b.xn),
                                                       P(b.un), P(b.cost), P(b.tr), P(b.st)),
        "fit": lambda o: lib.ilqr_floating_fit(h, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.cost), P(b.it), P(b.st)),
        "fit_ex": lambda o: lib.ilqr_floating_fit_ex(h, o, P(b.x), P(b.u), None, P(b.xn), P(b.un), P(b.cost), P(b.it),
                                                     P(b.st), C.byref(hst)),
    }
    try:
        refused(calls, b, "floating")
    finally:
        s.close()


def test_refusals_multi(gpu):
    """ilqr_multi_fit and ilqr_multi_fit_resident refuse before anything is uploaded or swapped: the
    host outputs stay as they were, and the resident result of the fit before is still the one
    ilqr_multi_gather returns — also after a refused warm start, which swaps the shards' buffers."""
    from ilqr_amd.multi import MultiSolver
    nb, T = 9, 7
    lq, x, u = random_lq_batch(nb, 12, 4, T, seed=2)
    ms = MultiSolver([0, 0], 12, 4, T, nb)
    try:
        xo, uo, co, it, st, rc = ms.fit(lq, x, u, max_iter=3, tol=-1.0)
        b = Bufs(nb, T, 12, 4, host=True)
        arrs = {k: np.ascontiguousarray(getattr(lq, k)) for k in ("A", "B", "Q", "R", "Qf")}
        prob = _lib.Problem(_lib.PROBLEM_LQ, 0, *(arrs[k].ctypes.data for k in ("A", "B", "Q", "R", "Qf")))
        hd = Bufs(nb, T, 12, 4)
        hst = hd.history()
        calls = {
            "multi_fit": lambda o: ms.lib.ilqr_multi_fit(ms.h, C.byref(prob), o, P(x), P(u), None, P(b.xn), P(b.un),
                                                         P(b.cost), P(b.it), P(b.st)),
            "multi_fit_resident": lambda o: ms.lib.ilqr_multi_fit_resident(ms.h, o, 0, C.byref(hst)),
            "multi_fit_resident_warm": lambda o: ms.lib.ilqr_multi_fit_resident(ms.h, o, _lib.MULTI_WARM_START, C.byref(hst)),
        }
        refused(calls, b, "multi")
        assert hd.untouched()
        g = ms.gather()
        for k, v in (("x", xo), ("u", uo), ("cost", co), ("iters", it), ("status", st)):
            np.testing.assert_array_equal(g[k], v, err_msg=k)
        # … and the resident inputs too: the same fit again, from the resident trajectories
        assert ms.fit_resident(max_iter=3, tol=-1.0) == rc
        np.testing.assert_array_equal(ms.gather()["u"], uo)
    finally:
        ms.close()
