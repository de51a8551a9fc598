"""CPU tests of the tool path's boundary (ilqr_chain_set_task_path): the function is declared,
bound, exported and ccalled with one prototype everywhere, ilqr_chain_get_target_mode's new bit
has its name, the ABI version stays 2, and a NULL handle is refused before any device call. The
refusals that need a handle (a 2-joint chain, fp32, a non-finite weight) are
tests/test_gpu_chain_path.py's: a handle exists only on a device."""
import ctypes as C
import os
import re

from ilqr_amd import _lib
from ilqr_amd.chain import ChainSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ilqr_chain_set_task_path"


def header():
    src = open(os.path.join(ROOT, "include", "ilqr.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_declared_bound_exported_ccalled():
    assert re.search(r"ilqr_status\s+" + NAME + r"\(ilqr_chain_handle\*\s*h,\s*const double\*\s*path,\s*double\s+path_weight\)",
                     header())
    assert _lib.SIGNATURES[NAME] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_double])
    assert hasattr(_lib.load(), NAME)
    shim = open(os.path.join(ROOT, "ilqr.jl_amd", "julia", "iLQRHIP.jl")).read()
    m = re.search(r"ccall\(\(:" + NAME + r",\s*libilqr\),\s*Cint,\s*\(([^)]*)\)", shim)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Float64}", "Cdouble"]
    assert "function set_task_path!(s::ChainSolver" in shim
    assert callable(ChainSolver.set_task_path)


def test_target_mode_bit_and_abi_version():
    assert (_lib.CHAIN_TARGETS_JOINT, _lib.CHAIN_TARGETS_TASK, _lib.CHAIN_TARGETS_PATH) == (1, 2, 4)
    assert _lib.load().ilqr_abi_version() == _lib.ABI_VERSION == 2
    src = open(os.path.join(ROOT, "include", "ilqr.h")).read()
    assert "3(T + 1) doubles per trajectory" in re.sub(r"\s*\n \*\s*", " ", src)   # the device-memory paragraph


def test_null_handle_needs_no_device():
    lib = _lib.load()
    for path in (None, C.c_void_p(8)):          # never dereferenced: the handle is checked first
        for w in (1.0, float("nan"), float("inf")):
            assert lib.ilqr_chain_set_task_path(None, path, w) == _lib.ERR_BAD_ARG
    assert lib.ilqr_chain_get_target_mode(None) == -1
