"""ILQR_LINEARIZE_ANALYTIC without a GPU: the constant in the three layers, the refusals of
ilqr_chain_create, and the identity the kernel rests on, restated in numpy on the oracle's
own Newton-Euler pass:

    δq̈ = M⁻¹(δτ − δ[ID(q, q̇, q̈)]),  q̈ held fixed,

chained through the four RK4 stages, against oracle.rbd.ChainModel.linearize (forward-mode
duals through the mass matrix and the solve)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ilqr_amd import _lib
from ilqr_amd.chain import coupled_chain_problem, rbd_2dof_problem
from oracle import rbd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_analytic_constant_in_every_layer():
    assert _lib.LINEARIZE_ANALYTIC == 2
    hdr = read("include", "ilqr.h")
    enum = re.search(r"typedef enum \{([^}]*)\}\s*ilqr_linearization;", hdr).group(1)
    assert dict(re.findall(r"ILQR_LINEARIZE_(\w+) = (\d+)", enum)) == {"DUAL": "0", "CENTRAL_FD": "1", "ANALYTIC": "2"}
    assert re.search(r"#define\s+ILQR_ABI_VERSION\s+2\b", hdr)   # additive: the version stays
    jl = read("ilqr.jl_amd", "julia", "iLQRHIP.jl")
    assert re.search(r"^const ILQR_LINEARIZE_ANALYTIC = Int32\(2\)", jl, re.M)
    assert re.search(r"linearization=ILQR_LINEARIZE_DUAL", jl)   # the default stays


def test_analytic_refusals_without_gpu():
    """ilqr_chain_create's argument checks come before any device call: value 2 is known
    (a bad dtype or dt still answers first), and refused off the tiles path."""
    lib = _lib.load()
    h = C.c_void_p()

    def create(s, dtype, lin):
        return lib.ilqr_chain_create(C.byref(h), 0, C.byref(s), 10, 8, dtype, lin)

    for nu in (2, 1):
        s = rbd_2dof_problem(nu).struct()
        for dtype in (_lib.F64, _lib.F32):
            assert create(s, dtype, _lib.LINEARIZE_ANALYTIC) == _lib.ERR_UNSUPPORTED, (nu, dtype)
            assert b"ILQR_LINEARIZE_ANALYTIC" in lib.ilqr_chain_last_error()
    s6 = coupled_chain_problem(6).struct()
    assert create(s6, _lib.F32, _lib.LINEARIZE_ANALYTIC) == _lib.ERR_UNSUPPORTED
    assert b"ILQR_LINEARIZE_ANALYTIC" in lib.ilqr_chain_last_error()
    for s in (s6, rbd_2dof_problem(2).struct()):
        for lin in (3, 9, -1):
            assert create(s, _lib.F64, lin) == _lib.ERR_BAD_ARG, lin
        assert create(s, 7, _lib.LINEARIZE_ANALYTIC) == _lib.ERR_BAD_ARG
    s6.dt = 0.0
    assert create(s6, _lib.F64, _lib.LINEARIZE_ANALYTIC) == _lib.ERR_BAD_ARG
    assert not h.value


def analytic_linearize(m, X, U):
    """The contract of the analytic mode on the oracle's routines: per stage the primal as
    continuous_dynamics computes it, the tangent of rnea at (q + εδq, q̇ + εδq̇, q̈ constant) and
    a solve with the stage's M; J = δx + ⅙(((δk₁ + 2δk₂) + 2δk₃) + δk₄)."""
    P, nx = X.shape
    n, dt = m.n, m.dt
    nd = nx + n
    x = [X[:, i] for i in range(nx)]
    u = [U[:, i] for i in range(n)]
    dx = [np.tile(np.eye(nd)[i], (P, 1)) for i in range(nx)]       # δx, δu seeds: (P, nd) each
    du = [np.tile(np.eye(nd)[nx + i], (P, 1)) for i in range(n)]
    k = [np.zeros(P)] * nx
    dk = [np.zeros((P, nd))] * nx
    acc = [np.zeros((P, nd))] * nx
    for a, w in ((0.0, 1.0), (0.5, 2.0), (0.5, 2.0), (1.0, 1.0)):
        y = [x[i] + a * k[i] for i in range(nx)]
        dy = [dx[i] + a * dk[i] for i in range(nx)]
        q, qd = y[:n], y[n:]
        M = m.mass_matrix(q)
        b = m.dynamics_bias(q, qd)
        qdd = m._solve(M, [u[i] - b[i] for i in range(n)])
        tau = m.rnea([rbd.Jet(q[i], dy[i]) for i in range(n)], [rbd.Jet(qd[i], dy[n + i]) for i in range(n)],
                     [rbd.Jet(qdd[i], np.zeros((P, nd))) for i in range(n)], gravity=True)
        dqdd = [np.zeros((P, nd)) for _ in range(n)]
        for c in range(nd):        # one solve per direction with the stage's M
            sol = m._solve(M, [du[i][:, c] - tau[i].der[:, c] for i in range(n)])
            for i in range(n):
                dqdd[i][:, c] = sol[i]
        k = [dt * v for v in qd] + [dt * v for v in qdd]
        dk = [dt * dy[n + i] for i in range(n)] + [dt * v for v in dqdd]
        acc = [acc[i] + w * dk[i] for i in range(nx)]
    J = np.stack([dx[i] + (1.0 / 6.0) * acc[i] for i in range(nx)], axis=1)
    return J[:, :, :nx], J[:, :, nx:]


@pytest.mark.parametrize("n", [4, 5, 6, 7])
def test_analytic_identity_matches_forward_mode(n):
    """15 random points (seed 61, q ∈ ±2, q̇ ∈ ±1, u ∈ ±5): the identity reproduces the oracle's
    forward-mode Jacobians to 1e-13 (measured ≈ 4e-16), the ∂q̈/∂q block against its own size."""
    pr = coupled_chain_problem(n)
    m = rbd.ChainModel(pr.chain, pr.dt)
    rng = np.random.default_rng(61)
    X = np.concatenate([rng.uniform(-2, 2, (15, n)), rng.uniform(-1, 1, (15, n))], axis=1)
    U = rng.uniform(-5, 5, (15, n))
    Ar, Br = m.linearize(X, U)
    A, B = analytic_linearize(m, X, U)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())  # noqa: E731
    ea, eb, eq = rel(A, Ar), rel(B, Br), rel(A[:, n:, :n], Ar[:, n:, :n])
    print(f"chain{n} analytic identity A {ea:.3e} B {eb:.3e} A[{n}:, :{n}] {eq:.3e}")
    assert ea < 1e-13 and eb < 1e-13 and eq < 1e-13, (ea, eb, eq)
