"""CPU tests of the per-trajectory goals' boundary (ilqr_chain_set_joint_targets,
ilqr_chain_set_task_targets, ilqr_chain_get_target_mode): the three functions are declared,
bound, exported and ccalled, the ABI version stays 2, a NULL handle is refused before any
device call, and the fixtures of tests/test_gpu_chain_targets.py hold what their generator
(tests/golden/make_golden_chain_targets.py) asserts."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from ilqr_amd import _lib
from ilqr_amd.chain import coupled_chain_problem, rbd_initial_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["ilqr_chain_set_joint_targets", "ilqr_chain_set_task_targets", "ilqr_chain_get_target_mode"]


def header():
    src = open(os.path.join(ROOT, "include", "ilqr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_bound_exported_ccalled(name):
    assert re.search(r"\b" + name + r"\s*\(", header()), name
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.load(), name)
    shim = open(os.path.join(ROOT, "ilqr.jl_amd", "julia", "iLQRHIP.jl")).read()
    assert name in set(re.findall(r"ccall\(\(:(ilqr_[a-z0-9_]+),\s*libilqr\)", shim))


def test_signatures_as_declared():
    h = header()
    assert re.search(r"ilqr_status\s+ilqr_chain_set_joint_targets\(ilqr_chain_handle\*\s*h,\s*const double\*\s*targets\)", h)
    assert re.search(r"ilqr_status\s+ilqr_chain_set_task_targets\(ilqr_chain_handle\*\s*h,\s*const double\*\s*targets\)", h)
    assert re.search(r"int32_t\s+ilqr_chain_get_target_mode\(const ilqr_chain_handle\*\s*h\)", h)
    P = C.c_void_p
    assert _lib.SIGNATURES["ilqr_chain_set_joint_targets"] == (C.c_int, [P, P])
    assert _lib.SIGNATURES["ilqr_chain_set_task_targets"] == (C.c_int, [P, P])
    assert _lib.SIGNATURES["ilqr_chain_get_target_mode"] == (C.c_int32, [P])


def test_abi_version_stays_2():
    assert _lib.load().ilqr_abi_version() == _lib.ABI_VERSION == 2
    assert re.search(r"#define ILQR_ABI_VERSION 2\b", header())


def test_null_handle_needs_no_device():
    lib = _lib.load()
    assert lib.ilqr_chain_set_joint_targets(None, None) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_set_task_targets(None, None) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_get_target_mode(None) == -1


@pytest.mark.parametrize("kind", ["joint", "task"])
@pytest.mark.parametrize("n", [4, 7])
def test_fixtures_hold_their_conditions(n, kind):
    """B = 3, T = 16; the goals stored, distinct per row and the first the problem's own; every
    fit converged within 20 iterations with every Σδu² a factor ≥ 1.25 from tol; the iteration
    counts not all equal; under 256 KB."""
    path = os.path.join(GOLD, f"chain{n}c_targets_t16.npz" if kind == "joint" else f"chain{n}ctask_targets_t16.npz")
    assert os.path.getsize(path) < 256 * 1024
    g = dict(np.load(path, allow_pickle=False))
    meta = json.loads(str(g["meta"]))
    pr = coupled_chain_problem(n)
    assert g["u"].shape == (3, 16, n) and g["x"].shape == (3, 17, 2 * n)
    assert g["targets"].shape == ((3, n) if kind == "joint" else (3, 3))
    assert len({tuple(r) for r in g["targets"].tolist()}) == 3
    if kind == "joint":
        assert np.array_equal(g["targets"][0], pr.target) and meta["simple"] is None
        assert np.array_equal(g["x"][:, 0], rbd_initial_states(3, n, seed0=81))
    else:
        assert meta["simple"]["euclidean"] is True and "final_target" not in meta["simple"]
    assert (g["fit_status"] == 1).all() and (g["fit_iters"] <= 20).all()
    assert len(set(g["fit_iters"].tolist())) > 1
    tol = meta["tol"]
    for b, it in enumerate(g["fit_iters"]):
        r = g["cond_du2"][b, :it] / tol
        assert ((r >= 1.25) | (r <= 0.8)).all() and r[-1] <= 1.0, (b, r)
        assert np.isnan(g["cond_du2"][b, it:]).all() and (g["cond_trials"][b, :it] >= 1).all()
