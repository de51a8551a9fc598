"""Where the waves of the fused LQ iteration wait at the edges of their two step loops, from
the trace build (ILQR_COOP_TRACE: `make -C ilqr.jl_amd/csrc tracevariant`):

    ILQR_LIB=ilqr.jl_amd/lib/variants/libilqr_hip_trace.so python tools/phase_edges.py

Lane 0 of every wave stamps the 100 MHz real-time counter at kernel entry, after the
backward prologue's wait, after the backward loop, after the turn's wait and fence, when
slot 0 of the forward's first trial has landed, after that trial's last step, once its Qf
row is in registers, and at exit (ilqr_fwd_ring.h EdgeStamps; records of kinds 4-6 through
ilqr_debug_trace). One handle at the headline shape fits one problem a few times (so the
traced fit's first launch is the checked one with every wave reusing), then one
3-iteration fit is traced. For each of its launches this prints the median and the 90th
percentile over the waves of every interval between two stamps, and the time inside the
launch during which NO wave of the chip is inside a step loop: before the first wave enters
its backward loop, around the turn, and after the last wave leaves its forward loop.
The trace build's run time is not the product's: read the intervals, not the total.
Not product code."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ilqr.jl_amd")]
from ilqr_amd import _lib  # noqa: E402
from ilqr_amd.problems import quadrotor_batch  # noqa: E402
from ilqr_amd.solver import Solver  # noqa: E402

STAMPS = ["entry", "bw_prologue", "bw_loop_end", "turn", "fw_slot0", "fw_loop_end", "fw_qf", "exit"]
INTERVALS = [("backward prologue", 0, 1, False), ("backward loop", 1, 2, True), ("turn (wait + fence)", 2, 3, False),
             ("forward prologue", 3, 4, False), ("forward loop, trial 1", 4, 5, True), ("Qf row", 5, 6, False),
             ("trial end .. exit", 6, 7, False)]
MAXR = 262144


def read_stamps(lib, buf):
    """-> {iteration: array [waves, 8] of ticks} from the records of kinds 4, 5, 6"""
    n = lib.ilqr_debug_trace(buf, MAXR)
    assert n >= 0, "ilqr_debug_trace failed"
    a = np.frombuffer(buf, dtype=np.uint64, count=4 * n).reshape(n, 4).copy()
    kind = (a[:, 0] & 15).astype(int)
    wid = ((a[:, 0] >> 24) & 0xFFFFFF).astype(int)
    gen = ((a[:, 0] >> 48) & 0xFFFF).astype(int)
    out = {}
    for it in sorted(set(gen[(kind >= 4) & (kind <= 6)])):
        nw = wid[gen == it].max() + 1
        t = np.zeros((nw, 8), dtype=np.int64)
        seen = np.zeros((nw, 3), dtype=bool)
        for k, cols in ((4, (0, 1, 2)), (5, (3, 4, 5)), (6, (6, 7))):
            m = (kind == k) & (gen == it)
            for c, col in enumerate(cols):
                t[wid[m], col] = a[m, 1 + c].astype(np.int64)
            seen[wid[m], k - 4] = True
        assert seen.all(), f"iteration {it}: a wave's records are missing"
        out[it] = t
    return out


def uncovered(t):
    """time (ticks) inside [first entry, last exit] with no wave in a step loop, split at the
    first loop entry and the last loop exit: (head, middle, tail)"""
    lo, hi = t[:, 0].min(), t[:, 7].max()
    ev = []
    for a, b in ((1, 2), (4, 5)):
        ok = t[:, b] > t[:, a]
        ev += [(x, 1) for x in t[ok, a]] + [(x, -1) for x in t[ok, b]]
    ev.sort()
    first, last = ev[0][0], max(x for x, s in ev if s < 0)
    depth, gap, prev = 0, 0, first
    for x, s in ev:
        if depth == 0:
            gap += x - prev
        depth += s
        prev = x
    return first - lo, gap, hi - last


def report(it, t, out):
    us = lambda v: v / 100.0  # noqa: E731 (100 MHz -> µs)
    print(f"launch {it}: {t.shape[0]} waves, first entry to last exit {us(t[:, 7].max() - t[:, 0].min()):.2f} µs",
          file=out)
    edges = 0.0
    for name, a, b, loop in INTERVALS:
        d = us(t[:, b] - t[:, a])
        print(f"  {name:<24} median {np.median(d):7.2f}  p90 {np.percentile(d, 90):7.2f} µs", file=out)
        if not loop:
            edges += float(np.median(d))
    print(f"  edges (sum of the medians outside the two loops) {edges:.2f} µs", file=out)
    head, mid, tail = uncovered(t)
    print(f"  no wave in a step loop: {us(head):.2f} µs before the first backward loop, {us(mid):.2f} µs around the "
          f"turn, {us(tail):.2f} µs after the last forward loop", file=out)
    gap = us(t[:, 4].min() - t[:, 2].max())
    print(f"  last wave out of the backward loop to first wave into the forward loop: {gap:.2f} µs", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warm", type=int, default=200, help="untraced fits first (clock, and the handle's gains)")
    a = ap.parse_args()
    path = os.environ.get("ILQR_LIB", os.path.join(ROOT, "ilqr.jl_amd", "lib", "variants", "libilqr_hip_trace.so"))
    _lib._lib = _lib.load(path)
    lib = _lib._lib
    lib.ilqr_debug_trace.restype = C.c_int
    lib.ilqr_debug_trace.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * (4 * MAXR))()

    B, T = a.batch, a.T
    dev = torch.device("cuda", 0)
    lq, x0, u0 = quadrotor_batch(B, T=T, seed0=0)
    s = Solver(12, 4, T, B)
    s.set_problem(lq)
    x, u = torch.from_numpy(x0).to(dev), torch.from_numpy(u0).to(dev)
    xo, uo = torch.empty_like(x), torch.empty_like(u)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    iters = torch.empty((B,), dtype=torch.int32, device=dev)
    st = torch.empty((B,), dtype=torch.int32, device=dev)
    s._bind_stream()
    torch.cuda.synchronize()
    o = _lib.default_options(max_iter=a.iters, tol=-1.0)
    args = tuple(C.c_void_p(t.data_ptr()) for t in (x, u)) + (None,) + tuple(
        C.c_void_p(t.data_ptr()) for t in (xo, uo, cost, iters, st))

    def fit():
        rc = s.lib.ilqr_fit(s.h, C.byref(s._problem), C.byref(o), *args)
        assert rc == _lib.OK, rc

    for _ in range(a.warm):
        fit()
        lib.ilqr_debug_trace(buf, 0)  # reset the count: the record array never fills
    fit()
    stamps = read_stamps(lib, buf)
    reused = float(s.reuse_record().mean()) if hasattr(s.lib, "ilqr_reuse_record") else None
    print(f"{os.path.basename(path)}: B {B}, T {T}, one {a.iters}-iteration fit after {a.warm} untraced ones; "
          f"waves that reused in its first launch: {reused}")
    for it, t in stamps.items():
        report(it, t, sys.stdout)
    s.close()


if __name__ == "__main__":
    main()
