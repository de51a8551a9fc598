"""Every Riccati backward kernel against the truth (tests/ladder.py): the LQ family's
one-per-wave and four-per-wave (block) kernels, their tracking entry, and the narrow and
wide tiles kernels, on the conditioning ladder whose gains oracle/mp_riccati.py computed
at 50 digits (tests/golden/mp_ladder/).

The bound, for K and d separately, as max |a − truth| / max |truth| over the batch:
    error ≤ M · max(e_ref, 4ε)          (· ρ on the indefinite rungs)
e_ref the fp64 references' own recorded error against the truth, M = 2·r11 from the
committed emulation of the device's solve (≈ 12; ladder.margin()). On the plain quadrotor
and the random dense rung the error is also below 1e-12 outright, so that the relative
form cannot hide a joint drift of device and references.

The gains a fused iterate/fit uses are not reachable: the history holds costs, trial
counts and du2, the reuse record one flag per wave, and no entry returns d or K from the
fused kernel. That leg is left out rather than widening the ABI; the fused kernel's
backward is the block kernel's code (ilqr_bw4.hip), which is measured here.

Each test prints `LADDER <rung> <path> <output> <error> <ratio to e_ref>`;
profiles/mp_ladder/README.md holds one run's table.
"""
import numpy as np
import pytest
import torch

import ladder as L
from ilqr_amd import _lib
from ilqr_amd.solver import Solver

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda", torch.float64).contiguous()  # (inputs are read-only)


def check(name, path, d, K, st):
    """Print and assert the ladder's bound for one device result."""
    assert (st.cpu().numpy() == 0).all(), (name, path, st)
    M = L.margin()
    errs = L.errors(d.cpu().numpy(), K.cpu().numpy(), name)
    for out, e, ref in zip(("K", "d"), errs, L.e_ref(name)):
        print(f"LADDER {name} {path} {out} {e:.3e} {e / ref:.2f}")
    for out, e, ref in zip(("K", "d"), errs, L.e_ref(name)):
        assert e <= M * ref, (name, path, out, e, e / ref, M)
        if name in L.ANCHOR_RUNGS:
            assert e < L.ANCHOR, (name, path, out, e)


def lq_solver(r, backward):
    s = Solver(r["lq"].nx, r["lq"].nu, L.T, L.NB)
    s.set_problem(r["lq"])
    s.set_schedule(backward=backward)
    return s


@pytest.mark.parametrize("backward", ["wave", "block"])
@pytest.mark.parametrize("name", L.LQ_RUNGS)
def test_lq_backward_against_mp(gpu, name, backward):
    r = L.rung(name)
    s = lq_solver(r, backward)
    try:
        d, K, st = s.backward(dev(r["x"]), dev(r["u"]), mu=r["mu"])
    finally:
        s.close()
    check(name, backward, d, K, st)


@pytest.mark.parametrize("backward", ["wave", "block"])
@pytest.mark.parametrize("name", L.TRACK_RUNGS)
def test_lq_tracking_backward_against_mp(gpu, name, backward):
    r = L.rung(name)
    s = lq_solver(r, backward)
    try:
        s.set_tracking(True)
        d, K, st = s.backward(dev(r["x"]), dev(r["u"]), mu=r["mu"], x_traj=dev(r["xt"]))
    finally:
        s.close()
    check(name, backward + "+tracking", d, K, st)


@pytest.mark.parametrize("name", L.TILE_RUNGS + L.INDEF_RUNGS)
def test_tiles_backward_against_mp(gpu, name):
    """12×4 and 5×3 run on the narrow kernel (one MFMA tile), 16×8 and 13×5 on the wide
    one; μ = 0 on lfxx·1e4 is the wide kernel's padded-pivot path."""
    r = L.rung(name)
    tl = r["tiles"]
    nb, T, n, m = tl["B"].shape
    s = Solver(n, m, T, nb, kind=_lib.PROBLEM_TILES)
    try:
        d, K, st = s.backward_tiles({k: dev(v) for k, v in tl.items()}, mu=r["mu"])
    finally:
        s.close()
    check(name, "narrow" if n <= 12 and m <= 4 else "wide", d, K, st)


@pytest.mark.parametrize("mfma", [False, True])
@pytest.mark.parametrize("ring", [True, False])
@pytest.mark.parametrize("name", L.FORWARD_RUNGS)
def test_lq_forward_against_mp(gpu, name, ring, mfma):
    """forward_pass at α₀ = 1 with the fixture's fp64 gains against the mp rollout and mp
    total cost of the same inputs: the C forward's trial count, and x̄, ū and the cost
    within M times the C forward's own error (floored at 4ε)."""
    r, fx = L.rung(name), L.fixture(name)
    s = Solver(12, 4, L.T, L.NB)
    try:
        s.set_problem(r["lq"])
        s.set_schedule(ring_forward=ring, forward_mfma=mfma)
        prev = torch.full((L.NB,), float("inf"), dtype=torch.float64, device="cuda")
        xn, un, cost, trials, st = s.forward(dev(r["x"]), dev(r["u"]), dev(fx["d"]), dev(fx["K"]), prev,
                                             alpha0=1.0)
    finally:
        s.close()
    assert (st.cpu().numpy() == 0).all() and (trials.cpu().numpy() == 1).all()
    M = L.margin()
    path = f"forward ring={int(ring)} mfma={int(mfma)}"
    got = {"x": xn, "u": un, "cost": cost}
    errs = {k: L.rel(got[k].cpu().numpy(), fx["fw_" + k]) for k in got}
    refs = dict(zip(("x", "u", "cost"), np.maximum(fx["fw_err_cref"], L.FLOOR)))
    for k in got:
        print(f"LADDER {name} {path} {k} {errs[k]:.3e} {errs[k] / refs[k]:.2f}")
    for k in got:
        assert errs[k] <= M * refs[k], (name, path, k, errs[k], errs[k] / refs[k], M)
