"""The conditioning ladder on the CPU (tests/ladder.py): the multiprecision reference
reproduces its committed fixtures and proves its own convergence, the two fp64 references
sit where the fixtures say they sit, and the ladder can see a reciprocal that is 100 ulp
off where it is blind to the design's 11.

Set ladder.K_DESIGN to 100 and test_ladder_is_sensitive_to_100_ulp's printed table shows
which rungs a device with such a reciprocal would fail on.
"""
import numpy as np
import pytest

import ladder as L
from oracle import mp_riccati as MP


@pytest.mark.parametrize("name", ["quad", "quad_qf1e4"])
def test_mp_reference_reproduces_fixture(name):
    """One benign rung and Qf·1e4, recomputed at 50 digits: the fixture bit for bit."""
    r, fx = L.rung(name), L.fixture(name)
    d, K = MP.backward_tiles(L.tiles_mp(name), r["mu"], dps=L.DPS)
    assert np.array_equal(d, fx["d"]) and np.array_equal(K, fx["K"])


def test_mp_reference_converged():
    """50 and 100 digits agree to 1e-30 before rounding: recorded for every rung by the
    generator, and recomputed here on the odd fifth trajectory of two rungs."""
    for name in L.RUNGS:
        assert 0.0 <= float(L.fixture(name)["conv"]) <= 1e-30, name
    for name in L.FORWARD_RUNGS:
        assert 0.0 <= float(L.fixture(name)["fw_conv"]) <= 1e-30, name
    for name in ("quad", "quad_qf1e4"):
        mu = L.rung(name)["mu"]
        a = MP.backward_tiles(L.tiles_mp(name, 50), mu, dps=50, round=False, batch=[L.NB - 1])
        b = MP.backward_tiles(L.tiles_mp(name, 100), mu, dps=100, round=False, batch=[L.NB - 1])
        conv = max(MP.rel_mp(a[0], b[0]), MP.rel_mp(a[1], b[1]))
        print(name, "dps 50 vs 100:", float(conv))
        assert conv <= 1e-30, (name, float(conv))


def test_literal_mp_recursion_is_wrong():
    """Why the reference symmetrises: the literal update S = Q + AᵀSA + KᵀHK + KᵀG + GᵀK
    amplifies its own rounding asymmetry geometrically, so even at
    60 digits it misses the symmetrised recursion on Qf·1e4 by more than 1e-8.

    Measured: the asymmetry grows ≈ 4.2× per step on this rung. Over the ladder's T = 32
    that is 1e20: a literal run at 60 digits ends 5e-40 from the symmetrised one (twenty
    digits lost, still invisible in fp64), and at 30 digits 3e-10. The 1e-8 miss at 60
    digits needs the headline's horizon, T = 100 (4.2¹⁰⁰ ≈ 1e62), so that is where this
    test pins it; the T = 32 figure is asserted as the loss of at least 15 digits."""
    from ilqr_amd.problems import LQBatch, quadrotor_batch
    name = "quad_qf1e4"
    mu = L.rung(name)["mu"]
    tl = L.tiles_mp(name, 60)
    lit = MP.backward_tiles(tl, mu, dps=60, symmetrize=False, round=False, batch=[0])
    sym = MP.backward_tiles(tl, mu, dps=60, symmetrize=True, round=False, batch=[0])
    e32 = float(max(MP.rel_mp(lit[0], sym[0]), MP.rel_mp(lit[1], sym[1])))
    print("literal mp at 60 digits, T = 32:", e32)
    assert e32 > 1e-45, e32
    lq, x, u = quadrotor_batch(1, T=100)
    tl = MP.lq_tiles(LQBatch(lq.A, lq.B, lq.Q, lq.R, lq.Qf * 1e4), x, u, dps=60)
    dl, Kl = MP.backward_tiles(tl, mu, dps=60, symmetrize=False)
    ds, Ks = MP.backward_tiles(tl, mu, dps=60, symmetrize=True)
    eK, ed = L.rel(Kl, Ks), L.rel(dl, ds)
    print("literal mp at 60 digits, T = 100: K", eK, "d", ed)
    assert max(eK, ed) > 1e-8, (eK, ed)


@pytest.mark.parametrize("name", L.RUNGS)
def test_fp64_references_reproduce_recorded_errors(name):
    """The Python oracle and the C restatement, rerun here, lie within 2× of the errors
    the fixture records for them (at or below the 4ε floor every value is the same).
    Both are "the reference": the larger of the two is the rung's e_ref. They are not held
    to 2× of EACH OTHER: at a given conditioning an fp64 recursion's error depends on its
    summation order and its solve. On the LQ rungs the two agree within 2.1×, on the tiles
    rungs within 3.9× (K of indef_5x3: 1.2e-14 and 4.6e-14), except
    tiles_graded_16x8, where the Python oracle (LAPACK gesv) is at 2.8e-12 and the C
    restatement at 2.5e-13."""
    fx = L.fixture(name)
    for what, (d, K) in (("err_oracle", L.oracle_backward(name)), ("err_cref", L.cref_backward(name))):
        for now, rec, out in zip(L.errors(d, K, name), fx[what], ("K", "d")):
            print(name, what, out, "now", now, "recorded", float(rec))
            lo, hi = max(float(rec), L.FLOOR) / 2, max(float(rec), L.FLOOR) * 2
            assert max(now, L.FLOOR) >= lo and now <= hi, (name, what, out, now, float(rec))


def test_indefinite_rungs_are_what_they_claim():
    """ρ within 1e2 … 1e4, luu indefinite, the leading pivot near 1e-3 of ‖H + μI‖ — and on
    every other rung the unpivoted factorisation does not grow (ρ = 1 up to rounding)."""
    for name in L.INDEF_RUNGS:
        tl = L.rung(name)["tiles"]
        ev = np.linalg.eigvalsh(tl["luu"])
        assert (ev.min(axis=-1) < 0).all() and (ev.max(axis=-1) > 0).all(), name
        lead = (tl["luu"][..., 0, 0] + L.rung(name)["mu"]) / np.abs(tl["luu"]).max(axis=(-1, -2))
        assert 3e-4 < lead.min() and lead.max() < 3e-3, (name, lead.min(), lead.max())
        assert 1e2 < float(L.fixture(name)["rho"]) < 1e4, name
    for name in L.RUNGS:
        if name not in L.INDEF_RUNGS:
            assert float(L.fixture(name)["rho"]) < 1.0 + 1e-12, name


def test_ladder_is_sensitive_to_100_ulp():
    """The design (11 ulp) sets the margin M = 2·r11; a reciprocal 100 ulp off exceeds M on
    at least two rungs. If this fails the ladder has gone blind: rework the rungs, not M."""
    M = L.margin()
    print(f"r11 = {L.r11():.2f}  M = {M:.2f}")
    caught = []
    for name in L.RUNGS:
        a, b = L.emulation_ratio(name, L.K_DESIGN), L.emulation_ratio(name, 100)
        print(f"{name:28s} r{L.K_DESIGN} = {a:8.2f}   r100 = {b:8.2f}{'   > M' if b > M else ''}")
        if b > M:
            caught.append(name)
    assert 2.0 <= L.r11() <= 50.0   # the emulation costs something, and M stays a margin
    assert len(caught) >= 2, caught


def test_forward_fixture_errors_are_rounding():
    """The C forward pass is within rounding of the mp rollout of the same fp64 inputs."""
    from oracle import cref
    for name in L.FORWARD_RUNGS:
        r, fx = L.rung(name), L.fixture(name)
        xc, uc, cc, tr = cref.lq_forward(r["lq"], r["x"], r["u"], None, fx["d"], fx["K"], np.inf)
        now = np.array([L.rel(xc, fx["fw_x"]), L.rel(uc, fx["fw_u"]), L.rel(cc, fx["fw_cost"])])
        print(name, "C forward vs mp: x, u, cost", now, "recorded", fx["fw_err_cref"])
        assert (tr == 1).all()
        assert (now <= 2 * np.maximum(fx["fw_err_cref"], L.FLOOR)).all()
        assert (fx["fw_err_cref"] < 1e-12).all()
