"""Generate tests/golden/mp_ladder/<rung>.npz: the true gains of every rung of
tests/ladder.py, from the multiprecision Riccati reference (oracle/mp_riccati.py).

Per rung: the mp feed-forwards d and gains K at 50 digits, rounded once to fp64; `conv`,
the relative distance of the unrounded 50- and 100-digit results (the reference's proof of
its own convergence, asserted ≤ 1e-30 here); `err_oracle` and `err_cref`, the (K, d)
errors of the Python oracle and of the C restatement against them; `rho`, the element
growth of the unpivoted LDLᵀ of H + μI (1 up to rounding where H is positive definite; the
indefinite rungs are built to land in 1e2 … 1e4). On the two forward rungs also the mp
rollout and total cost of one α = 1 trial with these fp64 gains, and the C forward's
errors against them. The inputs are not stored: tests rebuild them from seeds.

Regenerate with:  python tests/golden/make_golden_mp_ladder.py [rung ...]   (≈ 3 min)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ilqr.jl_amd"), os.path.join(ROOT, "tests")]

import ladder as L  # noqa: E402
from oracle import cref, mp_riccati as MP  # noqa: E402


def forward_case(name, d, K):
    r = L.rung(name)
    lq, x, u = r["lq"], r["x"], r["u"]
    xm, um, cm = MP.lq_forward(lq, x, u, None, d, K, dps=L.DPS, round=False)
    x2, u2, c2 = MP.lq_forward(lq, x, u, None, d, K, dps=2 * L.DPS, round=False)
    conv = float(max(MP.rel_mp(xm, x2), MP.rel_mp(um, u2), MP.rel_mp(cm, c2)))
    assert conv <= 1e-30, (name, conv)
    xm, um, cm = MP.to_f64(xm), MP.to_f64(um), MP.to_f64(cm)
    xc, uc, cc, tr = cref.lq_forward(lq, x, u, None, d, K, np.inf)
    assert (tr == 1).all(), (name, tr)
    return {"fw_x": xm, "fw_u": um, "fw_cost": cm, "fw_conv": np.float64(conv),
            "fw_err_cref": np.array([L.rel(xc, xm), L.rel(uc, um), L.rel(cc, cm)])}


def make(name):
    r = L.rung(name)
    d50, K50, rho = MP.backward_tiles(L.tiles_mp(name, L.DPS), r["mu"], dps=L.DPS, growth=True, round=False)
    d100, K100 = MP.backward_tiles(L.tiles_mp(name, 2 * L.DPS), r["mu"], dps=2 * L.DPS, round=False)
    conv = float(max(MP.rel_mp(d50, d100), MP.rel_mp(K50, K100)))
    assert conv <= 1e-30, (name, conv)
    d, K = MP.to_f64(d50), MP.to_f64(K50)
    assert np.array_equal(d, MP.to_f64(d100)) and np.array_equal(K, MP.to_f64(K100)), name
    if name in L.INDEF_RUNGS:
        assert 1e2 < rho < 1e4, (name, rho)
    do, Ko = L.oracle_backward(name)
    dc, Kc = L.cref_backward(name)
    out = {"d": d, "K": K, "conv": np.float64(conv), "rho": np.float64(rho),
           "err_oracle": np.array([L.rel(Ko, K), L.rel(do, d)]),
           "err_cref": np.array([L.rel(Kc, K), L.rel(dc, d)])}
    if name in L.FORWARD_RUNGS:
        out.update(forward_case(name, d, K))
    os.makedirs(L.GOLD, exist_ok=True)
    np.savez(os.path.join(L.GOLD, name + ".npz"), **out)
    print(f"{name}: conv {conv:.1e} rho {rho:.3g} oracle K {out['err_oracle'][0]:.1e} d {out['err_oracle'][1]:.1e}"
          f" cref K {out['err_cref'][0]:.1e} d {out['err_cref'][1]:.1e}", flush=True)


if __name__ == "__main__":
    for rung_name in sys.argv[1:] or L.RUNGS:
        make(rung_name)
