"""The conditioning ladder of the Riccati backward kernels — TEST INFRASTRUCTURE ONLY.

Every other parity test compares two fp64 programs on benign instances. The rungs here
are seeded instances of rising difficulty whose TRUE gains are known: oracle/mp_riccati.py
computes them at 50 digits, tests/golden/make_golden_mp_ladder.py stores them (rounded
once to fp64) under tests/golden/mp_ladder/, and the tests measure every fp64 program,
host or device, against them. Inputs are never stored: `rung(name)` rebuilds them from
seeds.

The yardstick per rung and output (K or d) is e_ref: the larger of the Python oracle's and
the C restatement's own error against the truth, floored at 4ε. The device may be
M = 2·r11 times that far, where r11 is what `emulate_device` (the device's unpivoted LDLᵀ
with every pivot reciprocal off by up to 11 ulp, ilqr_device.h) costs relative to e_ref,
maximised over rungs and outputs; the factor 2 covers what the emulation does not model
(the summation order of MFMA and DPP products, μ rounded into H's accumulator). M is
computed here, from the committed emulation with a fixed seed; it is not typed in.

On the indefinite rungs the yardstick is ρ·e_ref, ρ the element growth of the unpivoted
factorisation (stored with the fixture): the textbook backward-error growth and no more.
"""
import functools
import os

import numpy as np

from ilqr_amd.problems import LQBatch, quadrotor_batch, random_lq_batch
from oracle import cref, mp_riccati
from oracle import ilqr_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mp_ladder")
EPS = float(np.finfo(np.float64).eps)
FLOOR = 4 * EPS
T, NB = 32, 5          # an odd batch: the block kernel's second wave holds one trajectory
DPS = 50
EMU_SEED = 2024
K_DESIGN = 11          # ulp of rcp<1>: v_rcp_f64 + one Newton step (ilqr_device.h)

LQ_RUNGS = ("quad", "quad_r1e-8", "quad_graded", "quad_qf1e4", "quad_qf1e8", "dense", "dense_rho1.2",
            "pad_qf1e4")
TRACK_RUNGS = ("track_quad", "track_graded")
TILE_SHAPES = ((12, 4), (16, 8), (13, 5))     # one narrow shape, two wide
TILE_RUNGS = tuple(f"tiles_{kind}_{n}x{m}" for n, m in TILE_SHAPES for kind in ("lfxx1e4", "lfxx1e4_mu0", "graded"))
INDEF_RUNGS = ("indef_5x3", "indef_16x8")
RUNGS = LQ_RUNGS + TRACK_RUNGS + TILE_RUNGS + INDEF_RUNGS
FORWARD_RUNGS = ("dense_rho1.2", "quad_graded")
ANCHOR_RUNGS = ("quad", "dense")              # absolute bound 1e-12 beside the relative one
ANCHOR = 1e-12


def grade(n):
    """1e-4 … 1e4, log-spaced along the diagonal."""
    return np.logspace(-4.0, 4.0, n)


def _rollout(lq, x0, u):
    x = np.empty((u.shape[0], u.shape[1] + 1, lq.nx))
    x[:, 0] = x0
    for t in range(u.shape[1]):
        x[:, t + 1] = np.einsum("bij,bj->bi", lq.A, x[:, t]) + np.einsum("bij,bj->bi", lq.B, u[:, t])
    return x


def _lq_rung(name):
    mu = 0.01
    if name in ("dense", "dense_rho1.2"):
        lq, x, u = random_lq_batch(NB, 12, 4, T, seed=31)
        if name == "dense_rho1.2":
            rho = np.abs(np.linalg.eigvals(lq.A)).max(axis=1)
            lq = LQBatch(lq.A * (1.2 / rho)[:, None, None], lq.B, lq.Q, lq.R, lq.Qf)
            x = _rollout(lq, x[:, 0], u)
    elif name == "pad_qf1e4":
        lq, x, u = random_lq_batch(NB, 7, 3, T, seed=32)
        lq = LQBatch(lq.A, lq.B, lq.Q, lq.R, lq.Qf * 1e4)
    else:
        lq, x, u = quadrotor_batch(NB, T=T)
        A, B, Q, R, Qf = lq.A, lq.B, lq.Q, lq.R, lq.Qf
        if name == "quad_r1e-8":
            R, mu = R * 1e-8, 1e-8
        elif name in ("quad_graded", "track_graded"):
            Q, Qf = Q * grade(12), Qf * grade(12)          # diagonal costs: scales the diagonal
        elif name == "quad_qf1e4":
            Qf = Qf * 1e4
        elif name == "quad_qf1e8":
            Qf = Qf * 1e8
        else:
            assert name in ("quad", "track_quad"), name
        lq = LQBatch(A, B, Q, R, Qf)
    xt = None
    if name in TRACK_RUNGS:
        xt = 0.5 * np.random.default_rng(7).standard_normal(x.shape)
    return {"kind": "lq", "mu": mu, "lq": lq, "x": x, "u": u, "xt": xt}


def indefinite_tiles(n, m, seed):
    """luu symmetric and indefinite with a leading entry near 1e-3 of its norm, and a first
    input that barely reaches the state (its column of B is small), so that the leading
    pivot of H + μI stays that small at every step while the pivoted solve is benign."""
    from test_gpu_tiles import random_tiles
    tl = random_tiles(NB, T, n, m, seed)
    rng = np.random.default_rng(seed + 1)
    W = rng.standard_normal((NB, T, m, m))
    luu = 0.1 * (W + W.transpose(0, 1, 3, 2)) / np.sqrt(m)
    luu[..., np.arange(1, m), np.arange(1, m)] += 0.3 * np.where(np.arange(1, m) % 2 == 1, -1.0, 1.0)
    luu[..., 0, 0] = 4e-4
    luu[..., 0, 1:] = luu[..., 1:, 0] = 0.25 * np.sign(luu[..., 0, 1:])
    tl["luu"] = luu
    tl["B"] = tl["B"].copy()
    tl["B"][..., 0] *= 1e-2
    tl["lux"] = tl["lux"].copy()
    tl["lux"][..., 0, :] *= 1e-2
    return tl


def _tiles_rung(name):
    from test_gpu_tiles import random_tiles
    kind, shape = name.rsplit("_", 1)
    kind = kind.split("_", 1)[-1]
    n, m = (int(v) for v in shape.split("x"))
    if name in INDEF_RUNGS:
        return {"kind": "indef", "mu": 1e-4, "tiles": indefinite_tiles(n, m, seed=9100 + 10 * n + m)}
    tl = random_tiles(NB, T, n, m, seed=9000 + 10 * n + m)
    if kind.startswith("lfxx1e4"):
        tl["lfxx"] = tl["lfxx"] * 1e4
    else:
        assert kind == "graded", name
        D = np.sqrt(grade(n))                              # D M D keeps the dense tiles SPD
        tl["lxx"] = tl["lxx"] * D[:, None] * D[None, :]
        tl["lfxx"] = tl["lfxx"] * D[:, None] * D[None, :]
    return {"kind": "tiles", "mu": 0.0 if kind.endswith("mu0") else 0.01, "tiles": tl}


@functools.lru_cache(maxsize=None)
def rung(name):
    """The named rung's inputs, built once and never written to."""
    r = _lq_rung(name) if name in LQ_RUNGS + TRACK_RUNGS else _tiles_rung(name)
    for a in list(r.values()) + list(r.get("tiles", {}).values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def error_xe(r):
    """x − x_traj with the end state raw: what the tracking backward differentiates at."""
    xe = np.array(r["x"], dtype=np.float64)
    if r["xt"] is not None:
        xe[:, :-1] -= r["xt"][:, :-1]
    return xe


def tiles_f64(name):
    """The rung as fp64 tiles (an LQ rung through lq_tiles, its gradients rounded)."""
    r = rung(name)
    if r["kind"] != "lq":
        return r["tiles"]
    from test_gpu_tiles import lq_tiles
    return lq_tiles(r["lq"], error_xe(r), r["u"])


def tiles_mp(name, dps=DPS):
    """The rung as the mp reference reads it (an LQ rung's gradients formed in mp)."""
    r = rung(name)
    if r["kind"] != "lq":
        return r["tiles"]
    return mp_riccati.lq_tiles(r["lq"], r["x"], r["u"], r["xt"], dps=dps)


def rel(a, b):
    """max |a − b| / max |b| over the whole batch (b the reference)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(float).tiny))


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


def errors(d, K, name):
    """(K error, d error) of a result against the rung's mp fixture."""
    fx = fixture(name)
    return rel(K, fx["K"]), rel(d, fx["d"])


# -- the fp64 references ----------------------------------------------------------------
def oracle_backward(name):
    """The Python oracle's L2 algebra (pivoted solve, symmetrised) along the rung's tiles."""
    r, tl = rung(name), tiles_f64(name)
    nb, T_, n, m = tl["B"].shape
    d, K = np.empty((nb, T_, m)), np.empty((nb, T_, m, n))
    for b in range(nb):
        s, S = tl["lfx"][b], tl["lfxx"][b]
        for i in range(T_ - 1, -1, -1):
            P = np.zeros((m, n)) if tl["lux"] is None else tl["lux"][b, i]
            A = tl["A"][b, i]
            g, G, H = O.optimal_controller_param(A, tl["B"][b, i], tl["lu"][b, i], P, tl["luu"][b, i], s, S)
            du, Kt = O.feedback_parameters(g, G, H, r["mu"])
            d[b, i], K[b, i] = du, Kt
            _, s, S = O.step_back(A, 0.0, tl["lx"][b, i], tl["lxx"][b, i], g, G, H, du, Kt, 0.0, s, S)
            S = 0.5 * (S + S.T)
    return d, K


def cref_backward(name):
    """The C restatement: lq_backward on the LQ rungs, tiles_backward on the others."""
    r = rung(name)
    if r["kind"] == "lq":
        d, K, st = cref.lq_backward(r["lq"], error_xe(r), r["u"], r["mu"], symmetrize=True)
    else:
        d, K, st = cref.tiles_backward(r["tiles"], r["mu"], symmetrize=True)
    assert (st == 0).all(), name
    return d, K


def e_ref(name):
    """The yardstick (for K, for d): the larger recorded error of the two fp64 references,
    floored at 4ε; times ρ on the indefinite rungs."""
    fx = fixture(name)
    e = np.maximum(np.maximum(fx["err_oracle"], fx["err_cref"]), FLOOR)
    if name in INDEF_RUNGS:
        e = e * float(fx["rho"])
    return float(e[0]), float(e[1])


# -- the emulation of the device's solve ------------------------------------------------
def emulate_device(name, k, seed=EMU_SEED):
    """The symmetrised fp64 recursion with the device's solve: H + μI = L D Lᵀ without
    pivoting, every pivot reciprocal multiplied by 1 + k·ε·U(−1, 1) (LDLT, ilqr_device.h).
    k = 11 is the design (v_rcp_f64 + one Newton step); k = 100 is what a dropped Newton
    step or a wrong rcp instantiation looks like at a smaller scale. → (d, K)."""
    r, tl = rung(name), tiles_f64(name)
    rng = np.random.default_rng(seed)
    nb, T_, n, m = tl["B"].shape
    mu = r["mu"]
    d, K = np.empty((nb, T_, m)), np.empty((nb, T_, m, n))
    s, S = np.array(tl["lfx"]), np.array(tl["lfxx"])
    tr = lambda a: np.swapaxes(a, -1, -2)
    for i in range(T_ - 1, -1, -1):
        A, B = tl["A"][:, i], tl["B"][:, i]
        BtS = tr(B) @ S
        g = tl["lu"][:, i] + (tr(B) @ s[..., None])[..., 0]
        G = BtS @ A if tl["lux"] is None else tl["lux"][:, i] + BtS @ A
        H = tl["luu"][:, i] + BtS @ B
        L, dinv = np.zeros((nb, m, m)), np.empty((nb, m))
        Tm = np.zeros((nb, m, m))                          # Tm[i][k] = L[i][k]·D[k]
        for c in range(m):
            dk = H[:, c, c] + mu - (L[:, c, :c] * Tm[:, c, :c]).sum(axis=1)
            dinv[:, c] = (1.0 / dk) * (1.0 + k * EPS * rng.uniform(-1.0, 1.0, nb))
            for j in range(c + 1, m):
                Tm[:, j, c] = H[:, j, c] - (L[:, j, :c] * Tm[:, c, :c]).sum(axis=1)
                L[:, j, c] = Tm[:, j, c] * dinv[:, c]
        X = np.concatenate([g[..., None], G], axis=2)
        for j in range(m):                                 # L y = rhs
            X[:, j] -= (L[:, j, :j, None] * X[:, :j]).sum(axis=1)
        X *= dinv[..., None]
        for j in range(m - 1, -1, -1):                     # Lᵀ x = y
            X[:, j] -= (L[:, j + 1:, j, None] * X[:, j + 1:]).sum(axis=1)
        du, Kt = -X[..., 0], -X[..., 1:]
        d[:, i], K[:, i] = du, Kt
        dv = du[..., None]
        s = tl["lx"][:, i] + (tr(A) @ s[..., None] + tr(Kt) @ (H @ dv) + tr(Kt) @ g[..., None] + tr(G) @ dv)[..., 0]
        KtG = tr(Kt) @ G
        S = tl["lxx"][:, i] + tr(A) @ S @ A + tr(Kt) @ H @ Kt + KtG + tr(KtG)
        S = 0.5 * (S + tr(S))
    return d, K


def emulation_ratio(name, k, seed=EMU_SEED):
    """max over K and d of the emulation's error / e_ref on one rung."""
    eK, ed = errors(*emulate_device(name, k, seed), name)
    rK, rd = e_ref(name)
    return max(eK / rK, ed / rd)


@functools.lru_cache(maxsize=None)
def r11():
    """The design ratio: the 11-ulp emulation's worst error / e_ref over every rung."""
    return max(emulation_ratio(name, K_DESIGN) for name in RUNGS)


def margin():
    """M = 2·r11: how many e_ref a device result may lie from the truth."""
    return 2.0 * r11()
