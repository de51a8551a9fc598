"""What the consistent tracking mode (ILQR_TRACK_CONSISTENT, include/ilqr.h) costs, and that
the plain mode costs what it did: the headline fit (B = 4096, T = 100, 3 iterations from
the cold trajectories, tol disabled) timed with device events, the configurations
alternated fit by fit within one sitting so that clock and thermal drift hit all alike.

  python tools/bench_lq_tracking.py [--configs plain,zeros_off,zeros_on,on]
                                    [--parent <libilqr_hip.so of the parent commit>]
                                    [--schedule default|per_call|full] [--rounds N] [--out FILE]

Configurations (one handle each, all on the same problem and start; --configs picks):
  plain      no x_traj: bench.py's workload
  zeros_off  x_traj of zeros, ILQR_TRACK_FORWARD_ONLY: the forward streams a reference, the
             backward does not
  zeros_on   x_traj of zeros, ILQR_TRACK_CONSISTENT: the tracking kernels on the same
             iterates, bit for bit (x − 0 = x), so the same line search and the same work but
             for the backward's extra stream (T·nx·8 B = 9.6 KB per trajectory and backward
             pass): zeros_on − zeros_off is what the mode costs
  on         a real reference, 0.5·N(0, 1), ILQR_TRACK_CONSISTENT: a tracking fit as used
  off        the same reference, ILQR_TRACK_FORWARD_ONLY (the reference's behaviour: most line
             searches exhaust their 64 trials, which is what this figure then measures)
  parent     the plain workload on the parent commit's library (--parent)
  parent_b   the same again on a second handle: parent against itself, the spread the plain
             figure has to sit inside
--schedule: default (gains reused across calls: after the first fit every iteration runs the
vector-only backward, the HBM-bound case), per_call (iteration 1 of every fit runs the full
recursion and stores) or full (ILQR_SCHED_FULL_BACKWARD: every iteration the full recursion).
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ilqr.jl_amd")]
from ilqr_amd import _lib  # noqa: E402
from ilqr_amd.problems import quadrotor_batch  # noqa: E402
from ilqr_amd.solver import Solver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="plain,zeros_off,zeros_on,on")
    ap.add_argument("--parent", default=None, help="the parent commit's libilqr_hip.so")
    ap.add_argument("--schedule", default="default", choices=["default", "per_call", "full"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--settle", type=int, default=30, help="untimed rounds first")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T = a.batch, a.T
    dev = torch.device("cuda", 0)
    lq, x0, u0 = quadrotor_batch(B, T=T, seed0=0)
    x, u = torch.from_numpy(x0).to(dev), torch.from_numpy(u0).to(dev)
    xt = (0.5 * torch.from_numpy(np.random.default_rng(7).standard_normal(x0.shape))).to(dev)
    zeros = torch.zeros_like(xt)
    opts = _lib.default_options(max_iter=a.iters, tol=-1.0)
    sched = {"default": {}, "per_call": {"reuse_per_call": True}, "full": {"full_backward": True}}[a.schedule]

    known = {"plain": (None, None, False), "zeros_off": (None, zeros, False), "zeros_on": (None, zeros, True),
             "on": (None, xt, True), "off": (None, xt, False), "parent": (a.parent, None, False),
             "parent_b": (a.parent, None, False)}
    configs = [(n,) + known[n] for n in a.configs.split(",")]
    assert a.parent or not any(n.startswith("parent") for n, *_ in configs), "--parent <library> missing"
    runs = {}
    for name, lib_path, ref, track in configs:
        s = Solver(12, 4, T, B, lib_path=lib_path)
        s.set_problem(lq)
        s.set_schedule(**sched)
        if track:
            s.set_tracking(True)
        s._bind_stream()
        out = (torch.empty_like(x), torch.empty_like(u), torch.empty((B,), dtype=torch.float64, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
        args = (C.c_void_p(x.data_ptr()), C.c_void_p(u.data_ptr()), C.c_void_p(ref.data_ptr()) if ref is not None else None,
                *(C.c_void_p(t.data_ptr()) for t in out))
        runs[name] = (s, args, out, [])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    allowed = (_lib.OK, _lib.ERR_LS_EXHAUSTED)  # forward-only tracking may exhaust a line search

    def fit(name, record):
        s, args, _, times = runs[name]
        e0.record()
        rc = s.lib.ilqr_fit(s.h, s._p(), C.byref(opts), *args)  # synchronises
        e1.record()
        e1.synchronize()
        assert rc in allowed, (name, rc)
        if record:
            times.append(e0.elapsed_time(e1) * 1e3)

    order = [c[0] for c in configs]
    for r in range(a.settle + a.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):  # no configuration always follows the same one
            fit(name, r >= a.settle)
    res = {"batch": B, "T": T, "iters": a.iters, "schedule": a.schedule, "rounds": a.rounds, "unit": "us per fit"}
    for name in order:
        t = np.array(runs[name][3])
        res[name] = {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)),
                     "p90": float(np.percentile(t, 90)), "mean": float(t.mean())}

    def same_bits(p, q):
        return all(torch.equal(runs[p][2][k], runs[q][2][k]) for k in range(5))

    if "plain" in runs and "parent" in runs:  # the plain mode computes what the parent computed
        assert same_bits("plain", "parent"), "plain != parent"
        res["plain_equals_parent_bits"] = True
    if "zeros_on" in runs and "zeros_off" in runs:
        assert same_bits("zeros_on", "zeros_off"), "zeros_on != zeros_off"
        res["zeros_on_minus_zeros_off_us"] = res["zeros_on"]["median"] - res["zeros_off"]["median"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for s, *_ in runs.values():
        s.close()


if __name__ == "__main__":
    main()
