"""CPU tests of the velocity weights' boundary (ilqr_chain_set_velocity_weights,
ilqr_chain_get_velocity_weights): the functions are declared, bound, exported and ccalled with one
prototype everywhere, the ABI version stays 2, a NULL handle is refused before any device call,
and the Python side (ChainProblem's fields, the closures that state the cost, the quadratization
helpers) carries the terms. The refusals that need a handle (a 2-joint chain, fp32, a non-finite
weight) are tests/test_gpu_chain_rest.py's: a handle exists only on a device."""
import ctypes as C
import os
import re

import numpy as np

import ilqr_amd
from ilqr_amd import _lib
from ilqr_amd.chain import ChainCost, ChainFinalCost, ChainProblem, ChainSolver, chain_closures, coupled_chain_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET, GET = "ilqr_chain_set_velocity_weights", "ilqr_chain_get_velocity_weights"
PD = C.POINTER(C.c_double)


def header():
    src = open(os.path.join(ROOT, "include", "ilqr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_declared_bound_exported_ccalled():
    h = header()
    assert re.search(r"ilqr_status\s+" + SET + r"\(ilqr_chain_handle\*\s*h,\s*const double\*\s*v_weight,\s*"
                     r"const double\*\s*vf_weight\)", h)
    assert re.search(r"int32_t\s+" + GET + r"\(const ilqr_chain_handle\*\s*h,\s*double\*\s*v_weight,\s*double\*\s*vf_weight\)", h)
    assert _lib.SIGNATURES[SET] == (C.c_int, [C.c_void_p, PD, PD])
    assert _lib.SIGNATURES[GET] == (C.c_int32, [C.c_void_p, PD, PD])
    lib = _lib.load()
    assert hasattr(lib, SET) and hasattr(lib, GET)
    shim = open(os.path.join(ROOT, "ilqr.jl_amd", "julia", "iLQRHIP.jl")).read()
    for name, ret in ((SET, "Cint"), (GET, "Int32")):
        m = re.search(r"ccall\(\(:" + name + r",\s*libilqr\),\s*" + ret + r",\s*\(([^)]*)\)", shim)
        assert m and [a.strip() for a in m.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Float64}", "Ptr{Float64}"], name
    assert "function set_velocity_weights!(s::ChainSolver" in shim and "function velocity_weights(s::ChainSolver" in shim
    assert callable(ChainSolver.set_velocity_weights) and isinstance(ChainSolver.velocity_weights, property)


def test_abi_version_and_header_prose():
    assert _lib.load().ilqr_abi_version() == _lib.ABI_VERSION == 2
    src = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "ilqr.h")).read())
    assert "Without velocity weights its velocity rows and columns are exactly 0" in src
    assert "the call allocates nothing, ever" in src


def test_null_handle_needs_no_device():
    lib = _lib.load()
    w = (C.c_double * 8)(*[1.0] * 8)
    bad = (C.c_double * 8)(*[float("nan")] * 8)
    for a in (None, w, bad):
        for b in (None, w, bad):
            assert lib.ilqr_chain_set_velocity_weights(None, a, b) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_get_velocity_weights(None, w, w) == -1
    assert list(w) == [1.0] * 8          # nothing written


def test_chain_problem_fields_and_closures():
    b = coupled_chain_problem(4)
    assert b.v_weight is None and b.vf_weight is None          # a problem without the fields is as it was
    n = b.n_joints
    args = (b.chain, b.nu, b.dt, b.target, b.q_weight, b.r_weight, b.qf_weight)
    p = ChainProblem(*args, v_weight=2.0)                      # a scalar broadcasts, the other vector is zeros
    assert np.array_equal(p.v_weight, np.full(n, 2.0)) and np.array_equal(p.vf_weight, np.zeros(n))
    vw, vfw = 0.6 + 0.2 * np.arange(n), 80.0 + 14.0 * np.arange(n)
    p = ChainProblem(*args, v_weight=vw, vf_weight=vfw)
    assert bytes(p.struct()) == bytes(b.struct())              # the weights are not part of ilqr_chain
    rng = np.random.default_rng(0)
    x, u = rng.standard_normal(2 * n), rng.standard_normal(n)
    f, l, lf = chain_closures(p)
    assert isinstance(l, ChainCost) and isinstance(lf, ChainFinalCost)
    assert np.isclose(l(x, u), ChainCost(b)(x, u) + np.sum(vw * x[n:] ** 2), rtol=1e-15)
    assert np.isclose(lf(x), ChainFinalCost(b)(x) + np.sum(vfw * x[n:] ** 2), rtol=1e-15)
    # the quadratization helpers: the velocity rows and the velocity diagonal, nothing else there
    q, qv, r, Q, P, R = (np.asarray(v) for v in ilqr_amd.immediate_cost_quadratization(x, u, l))
    q0, qv0, r0, Q0, P0, R0 = (np.asarray(v) for v in ilqr_amd.immediate_cost_quadratization(x, u, ChainCost(b)))
    assert np.isclose(q, l(x, u), rtol=1e-14) and np.array_equal(qv[:n], qv0[:n]) and np.array_equal(qv[n:], 2 * vw * x[n:])
    assert np.array_equal(Q[:n, :n], Q0[:n, :n]) and np.array_equal(Q[n:, n:], np.diag(2 * vw))
    assert not Q[:n, n:].any() and not Q[n:, :n].any() and not P.any() and np.array_equal(r, r0) and np.array_equal(R, R0)
    c, g, H = (np.asarray(v) for v in ilqr_amd.final_cost_quadratization(x, lf))
    c0, g0, H0 = (np.asarray(v) for v in ilqr_amd.final_cost_quadratization(x, ChainFinalCost(b)))
    assert np.isclose(c, lf(x), rtol=1e-14) and np.array_equal(g[:n], g0[:n]) and np.array_equal(g[n:], 2 * vfw * x[n:])
    assert np.array_equal(H[:n, :n], H0[:n, :n]) and np.array_equal(H[n:, n:], np.diag(2 * vfw))
    assert not H[:n, n:].any() and not H[n:, :n].any()
    assert not g0[n:].any() and not H0[n:].any()
