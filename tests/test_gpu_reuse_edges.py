"""The reuse iterations' phase edges (profiles/reuse_edges/): on the fused
(12, 4) path the forward pass loads its cost rows in one round trip, and in the vector-only
and checked kernels its first slot load carries no cache hint. (The cases also covered the
alternates that were measured and not kept, tools/ablation/reuse_edges_alternates.patch:
the Qf rows loaded in the forward's prologue and kept over the trials, the backward
touching the forward's operands ahead of the turn.) Every one of these is a change of WHEN
or WITH WHICH HINT a value is loaded, so no
bit may move: each case below runs the same calls on a handle with the default schedule
(gain reuse within and across fits) and on a handle with `full_backward=True` (every
iteration the full recursion, no stored gains, the storing / checked / vector-only kernels
never launched) and compares x, u, cost, iters and status with `assert_array_equal`. The
full-backward handle keeps no reuse record (include/ilqr.h), so `reuse_record()` of the
handle under test is compared with the branch each wave has to take instead.

Shapes: B = 1, 5, 17 (a lone slot, a ragged second wave, a second workgroup with one live
slot) by T = 1, 2, 7, 8, 9, 12 (below, at and just past the ring's prefetch depth 7, its
depth 8 and the vector-only backward's prefetch depth 8, and the 8 + 4 remainder branch),
`backward="block"` so that these small batches take the fused path. Dense random LQ
instances: on the hover-linearised quadrotors a one-step horizon sits at the fp64 cost
floor and case (d) would exhaust its search.
"""
import functools

import numpy as np
import pytest
import torch

from ilqr_amd.problems import random_lq_batch
from ilqr_amd.solver import Solver
from oracle import cref

pytestmark = pytest.mark.gpu
SHAPES = [(nb, T) for nb in (1, 5, 17) for T in (1, 2, 7, 8, 9, 12)]
KEYS = ("A", "B", "Q", "R", "Qf")
KW = dict(max_iter=3, tol=-1.0)
REUSE, STORE = 1, 0


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", torch.float64).contiguous()


@functools.lru_cache(maxsize=None)
def problem(nb, T):
    return random_lq_batch(nb, 12, 4, T, seed=1000 * nb + T)


class Pair:
    """The handle under test and the full-backward handle, each on its own copy of the
    problem in device memory; `fit` runs the same call on both and compares."""

    def __init__(self, nb, T, **sched):
        lq, self.x, self.u = problem(nb, T)
        self.nb = nb
        self.p, self.s = [], []
        for full in (False, True):
            p = {k: dev(getattr(lq, k)) for k in KEYS}
            s = Solver(12, 4, T, nb)
            s.set_problem(p)
            s.set_schedule(backward="block", full_backward=full, **sched)
            self.p.append(p)
            self.s.append(s)

    def close(self):
        for s in self.s:
            s.close()

    def fit(self, store=None, **kw):
        """`store`: the waves that must re-factor in the first iteration (None: all)"""
        out = []
        for s in self.s:
            r = s.fit(dev(self.x), dev(self.u), **dict(KW, **kw))
            out.append({k: getattr(r, k).cpu().numpy() for k in ("x", "u", "cost", "iters", "status")})
        for k in out[0]:
            np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
        want = np.full((self.nb + 3) // 4, REUSE, np.int32)
        want[list(range(want.size) if store is None else store)] = STORE
        np.testing.assert_array_equal(self.s[0].reuse_record(), want)
        assert self.s[1].reuse_record().size == 0
        return out[0]


@pytest.fixture
def pair(gpu, request):
    made = []

    def make(nb, T, **sched):
        made.append(Pair(nb, T, **sched))
        return made[-1]

    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("nb,T", SHAPES)
def test_second_fit_reuses_in_every_wave(pair, nb, T):
    """(a) two consecutive fits on one handle: the second runs the checked kernel with every
    wave on its vector-only branch"""
    p = pair(nb, T)
    first = p.fit()
    second = p.fit(store=())
    for k in first:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)


@pytest.mark.parametrize("nb,T", SHAPES)
def test_qf_and_a_rewritten_in_place(pair, nb, T):
    """(b) a third fit after one trajectory's Qf and A were rewritten in place: its wave's
    store branch, and the forward's loads of Qf and the cost rows, pick up the new operands"""
    p = pair(nb, T)
    p.fit()
    before = p.fit(store=())
    k = nb - 1  # in the ragged last wave where there is one
    for q in p.p:
        q["Qf"][k] *= 1.25
        q["Qf"][k, 3, 5] += 0.125  # the row, not just its scale (and no longer symmetric)
        q["A"][k] *= 0.97
    after = p.fit(store=[k // 4])
    assert not np.array_equal(before["cost"][k], after["cost"][k])
    others = np.arange(nb) != k
    np.testing.assert_array_equal(before["cost"][others], after["cost"][others])
    p.fit(store=())


@pytest.mark.parametrize("nb,T", SHAPES)
def test_x_traj_given(pair, nb, T):
    """(c) a reference trajectory: the slot's third load carries x_traj itself"""
    p = pair(nb, T)
    rng = np.random.default_rng(7)
    xt = dev(p.x + 0.1 * rng.standard_normal(p.x.shape))
    p.fit(x_traj=xt)
    p.fit(store=(), x_traj=xt)


@functools.lru_cache(maxsize=None)
def oracle_trials(nb, T):
    lq, x, u = problem(nb, T)
    r = cref.lq_fit(lq, x, u, symmetrize=True, alpha0=4.0, shrink=0.5, history=True, **KW)
    return r[-1]["trials"], r[4]


@pytest.mark.parametrize("sched", [{}, {"sequential_search": True}], ids=["default", "sequential_search"])
@pytest.mark.parametrize("nb,T", SHAPES)
def test_first_trial_rejected(pair, nb, T, sched):
    """(d) alpha0 = 4, shrink = 0.5: iterations 2 and 3 reject their first trial, so what a
    wave's prologue loaded serves more than one trial (in its own loop with the sequential
    search; the cooperative search hands the later trials out as candidate passes)"""
    trials, status = oracle_trials(nb, T)
    assert (trials[1:].max(axis=1) >= 2).all(), "the CPU oracle: some trajectory takes two trials or more"
    assert trials.max() < 64 and (status != 3).all(), "the CPU oracle: no search exhausts the cap"
    p = pair(nb, T, **sched)
    p.fit(alpha0=4.0, shrink=0.5)
    p.fit(store=(), alpha0=4.0, shrink=0.5)
