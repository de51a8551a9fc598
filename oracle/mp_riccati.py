"""Multiprecision restatement of the Riccati backward pass — TEST INFRASTRUCTURE ONLY.

oracle/ilqr_oracle.py's optimal_controller_param, feedback_parameters and step_back at
`dps` decimal digits (mpmath), on general derivative tiles in cref.tiles_backward's
layout. It is the one place in the repository that knows the true gains: every other
checker is fp64 and is itself 1e-14 … 1e-6 away from them, depending on conditioning
(profiles/mp_ladder/README.md).

  - inputs are converted exactly from their fp64 values (mpf(float) is exact); entries that
    already are mpf (the tracking residual x − x_traj, formed in mp) pass through;
  - H + μI is solved with partial pivoting, step_back uses the unregularised H;
  - S ← (S + Sᵀ)/2 after every step: the literal update amplifies its own rounding
    asymmetry geometrically, so a literal run is wrong even at 60 digits
    (tests/test_mp_ladder.py pins that); symmetrize=False is that literal run;
  - outputs are rounded once to fp64 (round=False returns the mpf arrays).

The matrices are numpy object arrays of mpf: numpy's object matmul calls mpf's own
operators, so the precision in force is mpmath's working precision throughout.
"""
from __future__ import annotations

import numpy as np
from mpmath import mp, mpf

TILE_NAMES = ("A", "B", "lx", "lu", "lxx", "lux", "luu", "lfx", "lfxx")

_to_mp = np.frompyfunc(mpf, 1, 1)


def to_mp(a):
    """fp64 (or mpf) array → object array of mpf, exactly."""
    return _to_mp(np.asarray(a)).astype(object)


def to_f64(a):
    """Object array of mpf → float64, each entry rounded once, to nearest."""
    with mp.workprec(53):
        return np.array(np.frompyfunc(lambda v: float(+v), 1, 1)(a), dtype=np.float64)


def _zeros(*shape):
    z = np.empty(shape, dtype=object)
    z[...] = mpf(0)
    return z


def solve_pivoted(H, R):
    """H⁻¹R by Gaussian elimination with partial pivoting (Julia's `\\`, LAPACK gesv)."""
    m = H.shape[0]
    M = np.concatenate([H, R], axis=1).copy()
    for k in range(m):
        p = k + int(np.argmax([abs(v) for v in M[k:, k]]))
        if p != k:
            M[[k, p]] = M[[p, k]]
        for i in range(k + 1, m):
            f = M[i, k] / M[k, k]
            M[i, k:] = M[i, k:] - f * M[k, k:]
    X = _zeros(m, R.shape[1])
    for i in range(m - 1, -1, -1):
        acc = M[i, m:].copy()
        for j in range(i + 1, m):
            acc = acc - M[i, j] * X[j]
        X[i] = acc / M[i, i]
    return X


def ldlt_growth(H):
    """Element growth of the unpivoted H = L D Lᵀ: max |l_ik d_k l_jk| / max |H|."""
    m = H.shape[0]
    L = _zeros(m, m)
    D = _zeros(m)
    big = mpf(0)
    for k in range(m):
        D[k] = H[k, k] - sum((L[k, p] * L[k, p] * D[p] for p in range(k)), mpf(0))
        L[k, k] = mpf(1)
        for i in range(k + 1, m):
            v = H[i, k] - sum((L[i, p] * L[k, p] * D[p] for p in range(k)), mpf(0))
            L[i, k] = v / D[k]
        for i in range(k, m):
            for j in range(k, m):
                big = max(big, abs(L[i, k] * D[k] * L[j, k]))
    return big / max(abs(v) for v in H.reshape(-1))


def _backward_one(t, b, mu, symmetrize, growth):
    T, n, m = t["B"].shape[1:]
    half, mu = mpf(0.5), mpf(mu)
    S, s = to_mp(t["lfxx"][b]), to_mp(t["lfx"][b])
    d, K = _zeros(T, m), _zeros(T, m, n)
    rho = mpf(0)
    for i in range(T - 1, -1, -1):
        A, B = to_mp(t["A"][b, i]), to_mp(t["B"][b, i])
        q, r = to_mp(t["lx"][b, i]), to_mp(t["lu"][b, i])
        Q, R = to_mp(t["lxx"][b, i]), to_mp(t["luu"][b, i])
        P = _zeros(m, n) if t.get("lux") is None else to_mp(t["lux"][b, i])
        BtS = B.T @ S
        g = r + B.T @ s                                    # optimal_controller_param
        G = P + BtS @ A
        H = R + BtS @ B
        Hreg = H.copy()                                    # feedback_parameters
        for j in range(m):
            Hreg[j, j] = Hreg[j, j] + mu
        X = solve_pivoted(Hreg, np.concatenate([g[:, None], G], axis=1))
        du, Kt = -X[:, 0], -X[:, 1:]
        if growth:
            rho = max(rho, ldlt_growth(Hreg))
        d[i], K[i] = du, Kt
        s = q + A.T @ s + Kt.T @ (H @ du) + Kt.T @ g + G.T @ du          # step_back
        S = Q + A.T @ S @ A + Kt.T @ H @ Kt + Kt.T @ G + G.T @ Kt           # :270, term by term
        if symmetrize:
            S = (S + S.T) * half
    return d, K, rho


def backward_tiles(tiles, mu=0.01, dps=50, symmetrize=True, growth=False, round=True, batch=None):
    """tiles: cref.tiles_backward's dict (lux may be None; entries fp64 or mpf) →
    (d (B, T, m), K (B, T, m, n)) as float64, or as mpf object arrays with round=False;
    with growth=True also ρ, the largest element growth of the unpivoted LDLᵀ of H + μI
    over all steps. batch: the trajectories to run (default all)."""
    nb = tiles["B"].shape[0]
    idx = range(nb) if batch is None else batch
    with mp.workdps(dps):
        out = [_backward_one(tiles, b, float(mu), symmetrize, growth) for b in idx]
        d = np.stack([o[0] for o in out])
        K = np.stack([o[1] for o in out])
        rho = float(max(o[2] for o in out))
        if round:
            d, K = to_f64(d), to_f64(K)
    return (d, K, rho) if growth else (d, K)


def lq_tiles(lq, x, u, x_traj=None, dps=50):
    """The LQ family's tiles along (x, u) with the gradients formed in mp:
    lx_t = (Q + Qᵀ)(x_t − x_traj_t) for t < T, the end state raw (tracking mode);
    x_traj=None is the plain family. Entries are mpf at `dps` digits."""
    nb, T = u.shape[:2]
    with mp.workdps(dps):
        sym = lambda a: to_mp(a) + to_mp(a).transpose(0, 2, 1)
        Qs, Rs, Qfs = sym(lq.Q), sym(lq.R), sym(lq.Qf)
        xe, um = to_mp(x[:, :T]), to_mp(u)
        if x_traj is not None:
            xe = xe - to_mp(x_traj[:, :T])
        rep = lambda a: np.broadcast_to(a[:, None], (nb, T) + a.shape[1:])
        lx = np.stack([np.stack([Qs[b] @ xe[b, i] for i in range(T)]) for b in range(nb)])
        lu = np.stack([np.stack([Rs[b] @ um[b, i] for i in range(T)]) for b in range(nb)])
        lfx = np.stack([Qfs[b] @ to_mp(x[b, T]) for b in range(nb)])
    return {"A": rep(lq.A), "B": rep(lq.B), "lx": lx, "lu": lu, "lxx": rep(Qs), "lux": None,
            "luu": rep(Rs), "lfx": lfx, "lfxx": Qfs}


def lq_forward(lq, x, u, x_traj, d, K, alpha=1.0, dps=50, round=True):
    """One forward-pass trial of the LQ family in mp from fp64 inputs:
    ū_t = u_t + α d_t + K_t (x̄_t − x_t), x̄_{t+1} = A x̄_t + B ū_t, and the total cost
    Σ_t ℓ(x̄_t − x_traj_t, ū_t) + ℓ_f(x̄_T) → (x̄, ū, cost)."""
    nb, T = u.shape[:2]
    with mp.workdps(dps):
        xb = _zeros(*x.shape)
        ub = _zeros(*u.shape)
        cost = _zeros(nb)
        al = mpf(float(alpha))
        for b in range(nb):
            A, B, Q, R, Qf = (to_mp(a[b]) for a in (lq.A, lq.B, lq.Q, lq.R, lq.Qf))
            xm, um, dm, Km = to_mp(x[b]), to_mp(u[b]), to_mp(d[b]), to_mp(K[b])
            xt = _zeros(*x[b].shape) if x_traj is None else to_mp(x_traj[b])
            xb[b, 0] = xm[0]
            c = mpf(0)
            for i in range(T):
                ub[b, i] = um[i] + al * dm[i] + Km[i] @ (xb[b, i] - xm[i])
                xb[b, i + 1] = A @ xb[b, i] + B @ ub[b, i]
                e = xb[b, i] - xt[i]
                c = c + e @ (Q @ e) + ub[b, i] @ (R @ ub[b, i])
            cost[b] = c + xb[b, T] @ (Qf @ xb[b, T])
        if round:
            xb, ub, cost = to_f64(xb), to_f64(ub), to_f64(cost)
    return xb, ub, cost


def rel_mp(a, b):
    """max |a − b| / max |b| of two mpf object arrays, as an mpf."""
    num = max(abs(v) for v in (a - b).reshape(-1))
    return num / max(abs(v) for v in b.reshape(-1))
