"""What gain reuse across fit calls costs a caller whose problem changes with every call
(DESIGN.md §4): one handle at the headline shape fits two problems in turn, so the first
iteration of every fit finds its snapshot stale, runs the full recursion and rewrites the
snapshot. Against a build without the cross-call reuse, or against --mode per_call, the
difference is the snapshot's traffic: one read and one write of 31 doubles per lane.

  python tools/fit_alternating.py [--mode alternate|same|per_call|mu] [--fits N]
  ILQR_LIB=<other build> python tools/ab_lib.py tools/fit_alternating.py ...

--mode same fits one problem every time (every wave reuses); per_call alternates with
ILQR_SCHED_REUSE_PER_CALL set; mu keeps the problem and alternates μ between 0.01 and 0.02
(every fit launches the storing kernel, as the first fit on a handle does). Prints one JSON
line: the median, 10th and 90th percentile of the host's time per 3-iteration fit (ilqr_fit
synchronises), the first fit's time on the new handle, and the share of waves that reused
in the last fit (null if the library has no ilqr_reuse_record).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ilqr.jl_amd")]
from ilqr_amd import _lib  # noqa: E402
from ilqr_amd.problems import quadrotor_batch  # noqa: E402
from ilqr_amd.solver import Solver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="alternate", choices=["alternate", "same", "per_call", "mu"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--fits", type=int, default=300)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of untimed fits first")
    a = ap.parse_args()
    B, T = a.batch, a.T
    dev = torch.device("cuda", 0)
    lqs = [quadrotor_batch(B, T=T, seed0=s)[0] for s in (0, B)]
    _, x0, u0 = quadrotor_batch(B, T=T, seed0=0)
    s = Solver(12, 4, T, B)
    if a.mode == "per_call":
        s.set_schedule(reuse_per_call=True)
    probs, keep = [], []
    for lq in lqs:
        s.set_problem(lq)
        probs.append(s._problem)
        keep.append(s._keep)
    x, u = torch.from_numpy(x0).to(dev), torch.from_numpy(u0).to(dev)
    xo, uo = torch.empty_like(x), torch.empty_like(u)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    s._bind_stream()
    torch.cuda.synchronize()
    opts = [_lib.default_options(max_iter=a.iters, tol=-1.0, mu=mu) for mu in (0.01, 0.02)]
    args = tuple(C.c_void_p(t.data_ptr()) for t in (x, u)) + (None,) + tuple(
        C.c_void_p(t.data_ptr()) for t in (xo, uo, cost, iters, st))
    n = 0

    def fit():
        nonlocal n
        p = probs[n % 2 if a.mode in ("alternate", "per_call") else 0]
        o = opts[n % 2 if a.mode == "mu" else 0]
        n += 1
        t0 = time.perf_counter()
        rc = s.lib.ilqr_fit(s.h, C.byref(p), C.byref(o), *args)
        dt = time.perf_counter() - t0
        assert rc == _lib.OK, rc
        return dt

    first = fit()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.settle:
        fit()
    t = np.array([fit() for _ in range(a.fits)]) * 1e6
    reused = None
    if hasattr(s.lib, "ilqr_reuse_record"):
        r = s.reuse_record()
        reused = float(r.mean()) if r.size else None
    print(json.dumps({"mode": a.mode, "batch": B, "T": T, "iters": a.iters, "fits": a.fits,
                      "median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)),
                      "p90_us": float(np.percentile(t, 90)), "mean_us": float(t.mean()),
                      "first_fit_us": first * 1e6, "waves_reused_last_fit": reused}), flush=True)
    s.close()


if __name__ == "__main__":
    main()
