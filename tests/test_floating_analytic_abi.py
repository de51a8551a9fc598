"""ilqr_floating_set_linearization / ilqr_floating_get_linearization without a GPU: the two
symbols in the header, the binding, the library and the Julia shim; the returns that need
no handle; the Python names of the mode."""
import ctypes as C
import os
import re

import pytest

from ilqr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ilqr_floating_set_linearization", "ilqr_floating_get_linearization")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_in_header_binding_and_library():
    hdr = re.sub(r"/\*.*?\*/", "", read("include", "ilqr.h"), flags=re.S)
    assert re.search(r"ilqr_status\s+ilqr_floating_set_linearization\(\s*ilqr_floating_handle\*\s*h,\s*"
                     r"int32_t\s+linearization\s*\)\s*;", hdr)
    assert re.search(r"int32_t\s+ilqr_floating_get_linearization\(\s*const\s+ilqr_floating_handle\*\s*h\s*\)\s*;", hdr)
    assert re.search(r"#define\s+ILQR_ABI_VERSION\s+2\b", hdr)   # additive: the version stays
    # ilqr_floating_create keeps its signature
    assert re.search(r"ilqr_floating_create\(ilqr_floating_handle\*\*\s*out,\s*int device,\s*const ilqr_floating\*\s*"
                     r"model,\s*int T,\s*int batch\)", hdr)
    assert _lib.SIGNATURES[SYMBOLS[0]] == (C.c_int, [C.c_void_p, C.c_int32])
    assert _lib.SIGNATURES[SYMBOLS[1]] == (C.c_int32, [C.c_void_p])
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.ilqr_abi_version() == 2


def test_null_handle_returns():
    """A NULL handle is answered before any device call, whatever the value."""
    lib = _lib.load()
    for lin in (_lib.LINEARIZE_DUAL, _lib.LINEARIZE_CENTRAL_FD, _lib.LINEARIZE_ANALYTIC, 3, -1):
        assert lib.ilqr_floating_set_linearization(None, lin) == _lib.ERR_BAD_ARG, lin
    assert lib.ilqr_floating_get_linearization(None) == -1


def test_enum_comment_names_the_family():
    hdr = read("include", "ilqr.h")
    enum = re.search(r"typedef enum \{([^}]*)\}\s*ilqr_linearization;", hdr).group(1)
    assert dict(re.findall(r"ILQR_LINEARIZE_(\w+) = (\d+)", enum)) == {"DUAL": "0", "CENTRAL_FD": "1", "ANALYTIC": "2"}
    assert "floating" in enum


def test_julia_shim_names_the_setter():
    jl = read("ilqr.jl_amd", "julia", "iLQRHIP.jl")
    assert len(re.findall(r"ccall\(\(:ilqr_floating_set_linearization,\s*libilqr\)", jl)) == 1
    assert re.search(r"function FloatingSolver\(m::FloatingModel, T::Integer, batch::Integer;[^)]*"
                     r"linearization::Symbol=:dual\)", jl)
    assert re.search(r"floating_closures\(m::FloatingModel=rbd_2dof_arm_floating\(\); linearization::Symbol=:dual\)", jl)
    # the mode is part of the cache key
    assert "Dict{Tuple{FloatingModel,Int,Int,Symbol},FloatingSolver}" in jl
    assert "(m, Int(M), Int(nb), lin)" in jl


def test_python_names_of_the_mode():
    import inspect
    from ilqr_amd import floating as F
    assert F._LIN == {"dual": _lib.LINEARIZE_DUAL, "analytic": _lib.LINEARIZE_ANALYTIC}
    assert inspect.signature(F.FloatingSolver.__init__).parameters["linearization"].default == "dual"
    assert inspect.signature(F.floating_closures).parameters["linearization"].default == "dual"
    p = F.rbd_example_problem()
    assert F.FloatingDynamics(p).linearization == "dual"
    dyn, cost, fcost = F.floating_closures(p, linearization="analytic")
    assert dyn.linearization == "analytic" and F.floating_problem_of(dyn, cost, fcost) is p
    for bad in ("fd", "central", ""):
        with pytest.raises(ValueError):
            F.FloatingDynamics(p, linearization=bad)
        with pytest.raises(ValueError):
            F.FloatingSolver(p, 4, 1, linearization=bad)   # refused before the library is touched
