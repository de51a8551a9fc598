"""iLQRHIP.chain_fit(...; costs = simple_costs(…)) on the six-joint chain, replayed from
Python (Julia is not installed; tests/julia_layout.py restates the shim's layouts): the
constructor asks ilqr_chain_supported(n_joints, nu) and, for six joints, ccalls
ilqr_chain_set_task_costs with (Ptr, Int32 mode, Int32 body, Ptr{Float64} point,
Ptr{Float64} final_target, Float64 weight) — collect(::NTuple{3,Float64}) is three
contiguous doubles — then fits (nx, N, batch) column-major arrays."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import julia_layout as J
from ilqr_amd import _lib
from test_gpu_julia_layout import shim_family_fit

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.gpu
def test_shim_chain_fit_simple_costs_six_joints(gpu):
    """The same trajectories, bit for bit, as ChainSolver.fit in the task mode (pinned to the
    oracle by tests/test_gpu_chain6_task.py), and the fixture's iterates."""
    import torch
    from ilqr_amd.chain import ChainSolver, rbd_6dof_problem
    z = np.load(os.path.join(GOLD, "chain6task_b2_t24.npz"), allow_pickle=False)
    c = json.loads(str(z["meta"]))["simple"]
    p = rbd_6dof_problem(gravity=True)
    nb, T = z["u"].shape[:2]
    s = ChainSolver(p, T, nb, dtype=torch.float64)
    try:
        s.set_simple_costs(c["body"], c["point"], c["final_target"], c["weight"], c["euclidean"])
        ref = s.fit(torch.as_tensor(z["x"], device="cuda"), torch.as_tensor(z["u"], device="cuda"), max_iter=20,
                    tol=1e-6)
        rx, ru, rs = ref.x.cpu().numpy(), ref.u.cpu().numpy(), ref.status.cpu().numpy()
    finally:
        s.close()
    lib = _lib.load()
    st = p.struct()

    def create(M, b):   # ChainSolver(c::Chain, …, costs::SimpleCosts) of iLQRHIP.jl
        r = C.c_void_p()
        _lib.check(lib.ilqr_chain_create(C.byref(r), 0, C.byref(st), M, b, _lib.F64, _lib.LINEARIZE_DUAL),
                   "ilqr_chain_create")
        _lib.check(lib.ilqr_chain_set_dynamics(r, _lib.CHAIN_DYN_AUTO), "ilqr_chain_set_dynamics")
        mode = np.int32(_lib.CHAIN_COST_SIMPLE_EUCLIDEAN if c["euclidean"] else _lib.CHAIN_COST_SIMPLE)
        point = J.memory(J.jl(c["point"]))                  # collect(costs.point)
        target = J.memory(J.jl(c["final_target"]))
        dp = C.POINTER(C.c_double)
        assert lib.ilqr_chain_supported(int(st.n_joints), int(st.nu)) == 0     # … so the new entry
        _lib.check(lib.ilqr_chain_set_task_costs(r, int(mode), int(np.int32(c["body"])), point.ctypes.data_as(dp),
                                                 target.ctypes.data_as(dp), float(c["weight"])),
                   "ilqr_chain_set_task_costs")
        assert lib.ilqr_chain_get_cost_mode(r) == int(mode)
        return r

    jx = J.jl(np.transpose(z["x"], (2, 1, 0)))          # x_init[:, t, b]
    ju = J.jl(np.transpose(z["u"], (2, 1, 0)))
    x, u, status = shim_family_fit(create, lib.ilqr_chain_fit, lib.ilqr_chain_destroy, jx, ju, 20, 1e-6, np.float64)
    assert np.array_equal(np.transpose(x, (2, 1, 0)), rx) and np.array_equal(np.transpose(u, (2, 1, 0)), ru)
    assert np.array_equal(status, rs)
    e = np.abs(np.transpose(u, (2, 1, 0)) - z["fit_u"]).max() / np.abs(z["fit_u"]).max()
    assert e < 1e-8, e
