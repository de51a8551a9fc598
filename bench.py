"""Headline benchmark: batched iLQR iterations/s, nx=12 nu=4 T=100, batch 4096 per GPU.

Protocol (with the iteration count measured): the workload is `iLQR.fit`
(/root/reference/src/forward_pass.jl:148-179) run for I = 3 iterations from the cold
trajectory (u = 0 and its rollout, prev_cost = Inf) with the convergence test disabled
(tol < 0), through the C ABI (`ilqr_fit`: init, I × (backward_pass + forward_pass with
its line search), result gather, status fold — one host synchronisation per fit).
Iteration 1 accepts α = 1 against prev_cost = Inf; iterations 2-3 run real line
searches against finite costs (trials per iteration are measured in an untimed replay
and reported). SURVEY §8(d) asked for I = 5 on the assumption that the LQ line search
always accepts α = 1; measured, iterations 4-5 reach the fp64 cost floor (the cost
decrease is at rounding level): iteration 5 averages ~3.7 trials and ~3 % of the
trajectories exhaust the 64-trial cap, where the reference's unbounded
`while true` (forward_pass.jl:70-87) would spin forever. The headline `value` uses the
I = 3 that every trajectory completes with accepted steps; SURVEY §8(d)'s I = 5 fit is
the CO-HEADLINE (`co_headline`, same metric, timed the same way: median over fits),
with the cooperative line search of the fused kernel (include/ilqr.h
ILQR_SCHED_SEQUENTIAL_SEARCH) resolving the floor's long searches; the
reference's default call (tol = 1e-6, max_iter = 100) is reported beside them.

A "step" is one batched fit iteration. The timed region runs exactly `--steps` of
them as ⌊K/I⌋ fits of I iterations (plus one fit of K mod I), bracketed by a
barrier + device synchronisation; `value` = N × K / (max over ranks of that time).
Each fit's wall time is also recorded and the median over fits is reported.

Before any timing the GPU runs untimed fits for `--settle` seconds (time-based
clock settle, reported as its own field), then `--warmup` untimed steps.

Inputs are resident in HBM before the timed region. Data: synthetic, per-instance
randomised hover-linearised quadrotors (ilqr_amd.problems.quadrotor_batch).

Multi-GPU (one process per GPU, torch.distributed over RCCL): trajectories are
independent, so each rank solves its own 4096 instances (seeds rank·4096 + i) with
no data-path collective (weak scaling); after the timed region the per-trajectory
costs are all-gathered once (the fit result exchange) and that time is reported
separately.

A plain run (`--gpus N --steps K --warmup W`) does only that: set-up, settle, warm-up,
the K timed steps, the result line with the headline's fields. `--dump-outputs DIR`
also writes what the last timed fit returned (x, u, cost, iters, status of `ilqr_fit`,
rank 0's) as DIR/<name>.npy in float64, a fixed seeded sample of the trajectories when
the whole would pass 64 MB; the instances are seeded, so two builds run with the same
arguments are comparable output for output. `--full` adds every other section of the
line, each measured after the timed region in runs of its own: the kernel legs and
rooflines, the one-iteration step, the co-headline and default-options fits, the
line-search replay and its checks, the result all-gather of a multi-rank run, the
secondary configurations (`--no-secondary` skips them) and the CPU baseline (`--no-cpu`).

Prints ONE JSON line (rank 0).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ilqr.jl_amd")]

from ilqr_amd import _lib  # noqa: E402
from ilqr_amd.problems import quadrotor_batch  # noqa: E402
from ilqr_amd.solver import Solver, _ptr  # noqa: E402

NX, NU = 12, 4
FIT_ITERS = 3             # iterations per timed fit from cold, tol disabled (module docstring)
FP64_PEAK_TFLOPS = 78.6   # MI355X FP64 dense (vector = matrix), AMD spec; not listed in the container guides
HBM_PEAK_GBPS = 8000.0    # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_COPY_GBPS = 6290.0    # MI355X_MICROARCH.md: 6.29 TB/s measured float4 copy


def algorithmic_counts(T, nx=NX, nu=NU):
    """SURVEY.md §8(d) per-trajectory algorithmic bytes / flops (fused design)."""
    w = 8
    P = 3 * nx * nx + nx * nu + nu * nu
    traj = (T + 1) * nx + T * nu
    gains = T * nu * (nx + 1)
    bw_bytes = w * (traj + gains + P)                       # backward: read x,u,P; write K,d
    fw_bytes = w * (2 * traj + gains + P)                   # forward: read x,u,K,d,P; write x̄,ū (1 trial)
    n, m = nx, nu
    bw_flops_step = 2 * (2 * n**3 + 4 * n * n * m + 2 * n * m * m + 2 * n * n + 4 * n * m
                         + m**3 / 3 + (n + 3) * m * m)
    fw_flops_step = 2 * (2 * n * n + 2 * n * m + m * m + 2 * n + 3 * m)
    return dict(bw_bytes=bw_bytes, fw_bytes=fw_bytes, bw_flops=bw_flops_step * T,
                fw_flops=fw_flops_step * T)


_HEADLINE_RECORD = re.compile(r"^(pmc|mfma)_r(\d+)\.json$")


def _latest_headline_record(profiles_dir, prefix):
    """The newest HEADLINE record `profiles/<prefix>_rNN.json` (highest round NN), by
    name: records of other benchmarks (`pmc_tiles_r05.json`, variants like
    `pmc_r01_v6.json`) never match. → (path, record) or (None, None)."""
    best = None
    if os.path.isdir(profiles_dir):
        for f in os.listdir(profiles_dir):
            m = _HEADLINE_RECORD.match(f)
            if m and m.group(1) == prefix and (best is None or int(m.group(2)) > best[0]):
                best = (int(m.group(2)), f)
    if best is None:
        return None, None
    path = os.path.join(profiles_dir, best[1])
    with open(path) as fh:
        return path, json.load(fh)   # a malformed committed record fails loudly


def load_pmc_traffic(profiles_dir, batch=4096, T=100):
    """HBM bytes per launch of the headline kernels from the newest committed
    rocprofv3 PMC record of bench.py (profiles/pmc_rNN.json, written by
    profiles/collect_pmc.py). → (record, source) where record is None when the
    record was taken at another batch / horizon than this run's (source says why).
    A headline record missing its batch, T or per-launch byte fields raises."""
    path, rec = _latest_headline_record(profiles_dir, "pmc")
    if rec is None:
        return None, "no profiles/pmc_rNN.json"
    missing = [k for k in ("batch", "T", "hbm_bytes_per_backward_launch", "hbm_bytes_per_fused_launch")
               if k not in rec]
    if missing:
        raise ValueError(f"{path}: headline PMC record lacks {missing}")
    src = os.path.relpath(path, os.path.dirname(profiles_dir))
    if rec["batch"] != batch or rec["T"] != T:
        return None, f"{src} was taken at batch={rec['batch']} T={rec['T']}, this run is batch={batch} T={T}"
    return rec, src


def load_mfma_pmc(profiles_dir):
    """MFMA utilisation per kernel from the newest committed rocprofv3 pass of bench.py
    (profiles/mfma_rNN.json, written by profiles/collect_mfma.py), or None."""
    return _latest_headline_record(profiles_dir, "mfma")[1]


def mfma_summary(m, key):
    e = (m or {}).get(key)
    if not e:
        return None
    return {"mfma_busy_pct": e.get("MfmaUtil"), "mfma_tflops": e.get("mfma_tflops"),
            "mfma_frac_of_fp64_peak": e.get("mfma_frac_of_peak"),
            "f64_mfma_insts_per_launch": e.get("SQ_INSTS_VALU_MFMA_F64"),
            "valu_insts_per_launch": e.get("SQ_INSTS_VALU"),
            "source": "rocprofv3 --pmc MfmaUtil MfmaFlopsF64 (profiles/mfma_*.json)"}


def cpu_threads():
    """Host threads for the CPU baseline: every CPU this process may run on, capped
    at the box's CPU share when the operator sets one (OMP_NUM_THREADS = 16 per GPU
    on the GPU pool)."""
    visible = len(os.sched_getaffinity(0))
    share = os.environ.get("OMP_NUM_THREADS")
    n = min(visible, int(share)) if share and share.isdigit() and int(share) > 0 else visible
    return n, visible


def cpu_baseline(lq, x, u, budget_s):
    """Time the C restatement (oracle/ilqr_ref.c, kind 'port'; the Julia reference
    cannot run in this pipeline) on a bounded sample of the same workload: the
    FIT_ITERS-iteration fit from cold (tol disabled) of n trajectories, OpenMP over
    trajectories, on the host threads of cpu_threads() and on one core."""
    from oracle import cref

    def rate(threads, budget):
        n = 16
        while True:
            idx = np.arange(n) % lq.batch
            sub = type(lq)(lq.A[idx], lq.B[idx], lq.Q[idx], lq.R[idx], lq.Qf[idx])
            t0 = time.perf_counter()
            cref.lq_fit(sub, x[idx], u[idx], max_iter=FIT_ITERS, tol=-1.0, symmetrize=True,
                        nthreads=threads)
            elapsed = time.perf_counter() - t0
            if elapsed > budget or n >= 1 << 15:
                return n, elapsed, n * FIT_ITERS / elapsed  # trajectory-iterations / s
            n *= 2

    threads, visible = cpu_threads()
    n, elapsed, r = rate(threads, budget_s / 3)
    n1, elapsed1, r1 = rate(1, budget_s / 6)
    return {"value": r / lq.batch, "unit": f"batched iterations/s (batch={lq.batch})", "cores": threads,
            "kind": "port",
            "cores_note": f"{threads} threads = this GPU's CPU share on the box (OMP_NUM_THREADS, set by the "
                          f"operator; {visible} CPUs visible, shared by the node's GPUs) — not all host cores",
            "value_1core": r1 / lq.batch,
            "host_cpus_visible": visible, "nproc": os.cpu_count(),
            "sample": f"{n} trajectories x {FIT_ITERS}-iteration fit from cold, tol disabled (C restatement "
                      f"oracle/ilqr_ref.c, -O3, OpenMP {threads} threads), {elapsed:.2f} s; "
                      f"trajectory-iterations/s={r:.1f}; 1 core: {n1} trajectories in {elapsed1:.2f} s, "
                      f"trajectory-iterations/s={r1:.1f}. Julia reference not runnable in this "
                      f"pipeline (no Julia toolchain); C restatement timed."}


def secondary_configs(device):
    """BASELINE config 2 (2-link arm nu = 1, B = 1024, T = 50, fp64) and config 5 (RBD
    2-DoF arm, fp32, central differences, B = 2048, T = 100): one cold-start fit iteration
    per step, HIP events; each with its forward's step latency and lane occupancy."""
    from ilqr_amd.chain import coupled_2dof_problem
    from tools import bench_rbd, bench_twolink
    out = {}
    for name, fn in (("config2_twolink_nu1_B1024_T50_f64",
                      lambda: bench_twolink.measure(1024, 50, 1, steps=200, warmup=300, device=device)),
                     ("config5_rbd_2dof_fd_f32_B2048_T100",
                      lambda: bench_rbd.measure("fd", 2048, 100, 1, "f32", steps=100, warmup=100, device=device)),
                     # the same step on the coupled 2-joint chain (tilted joint, offset COMs,
                     # gravity): the reference's 2Dof_arm.urdf has a constant mass matrix and
                     # no bias, so config 5 alone does not exercise q-dependent dynamics
                     ("config5_shape_coupled_chain_fd_f32_B2048_T100",
                      lambda: bench_rbd.measure("fd", 2048, 100, 1, "f32", steps=100, warmup=100, device=device,
                                                problem=coupled_2dof_problem(1)))):
        try:
            r = fn()
            fw = r["roofline"]["forward"]
            out[name] = {"batched_it_per_s": r["value"], "ms_per_iteration": r["ms_per_step"],
                         "traj_iters_per_s": r["traj_iters_per_s"], "all_ok": r["all_ok"],
                         "forward_ns_per_step": fw["step_latency_ns"],
                         "forward_lanes_busy_frac": fw["lanes_busy_frac"],
                         "forward_avg_launch_ms": fw["avg_launch_ms"], "forward_frac_of_peak": fw["frac"],
                         "dtype": r["dtype"], "config": r["config"]}
            if "fit" in r:  # ChainSolver.fit end to end (config 5)
                out[name]["fit3_ms"] = r["fit"]["fit3"]["median_ms"]
                out[name]["fit_default_ms"] = r["fit"]["fit_default"]["median_ms"]
                out[name]["fit_default_mean_iterations"] = r["fit"]["fit_default"]["mean_iterations"]
        except Exception as e:  # reported, never required
            out[name] = {"error": repr(e)}
    # row f3: the tiles backward of arbitrary closures at the reference RBD caller's shape
    # (nx = 16, nu = 8; animate_RBD_2_link.jl fits ONE trajectory at T = 1000: a latency
    # chain) and at a chip-filling batch (HBM-bound: GB/s against the 8 TB/s spec)
    from tools import bench_tiles
    for name, args in (("tiles_wide_rbd_caller_B1_T1000", (16, 8, 1, 1000)),
                       ("tiles_wide_B4096_T100", (16, 8, 4096, 100))):
        try:
            out[name] = bench_tiles.measure(*args, reps=20, device=device)
        except Exception as e:  # reported, never required
            out[name] = {"error": repr(e)}
    # the reference's RBD script (animate_RBD_2_link.jl: floating 2Dof_arm, nx = 16, nu = 8,
    # T = 1000, one trajectory) fitted natively by the floating-base family
    from tools import bench_floating
    try:
        out["rbd_floating_native_B1_T1000"] = bench_floating.measure(1, iters=3, reps=2)
    except Exception as e:  # reported, never required
        out["rbd_floating_native_B1_T1000"] = {"error": repr(e)}
    return out


def _free_port():
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


# Every per-rank time behind an aggregate field of the JSON line. The job ends with its
# slowest rank, so each is reduced with MAX over ranks before any field is formed; the
# per-trajectory mean iteration count of the default-options fit is averaged over ranks.
RANK_TIMES = ("ms_step", "fit5_ms", "dflt_ms", "single_ms", "bw_ms", "fw_ms", "fused_ms")


def reduce_over_ranks(times, dflt_iters, world, device):
    """→ (dict of max-over-ranks times, mean-over-ranks default-fit iterations)."""
    if world == 1:
        return dict(times), dflt_iters
    import torch.distributed as tdist
    keys = [k for k in RANK_TIMES if k in times]   # a plain run has ms_step alone
    t = torch.tensor([times[k] for k in keys], dtype=torch.float64, device=device)
    tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
    it = torch.tensor([dflt_iters], dtype=torch.float64, device=device)
    tdist.all_reduce(it, op=tdist.ReduceOp.SUM)
    return dict(zip(keys, t.tolist())), float(it.item()) / world


DUMP_LIMIT_BYTES = 64e6


def dump_outputs(path, out, seed=0):
    """`--dump-outputs`: the last timed fit's results (`out`: name -> host array, batch
    first) as path/<name>.npy in float64. When they would pass DUMP_LIMIT_BYTES together,
    the same seeded sample of trajectories is kept of each (its indices: sample_index.npy)."""
    batch = len(out["cost"])
    per_traj = 8 * (1 + sum(int(np.prod(a.shape[1:])) for a in out.values()))
    idx = None
    if batch * per_traj > DUMP_LIMIT_BYTES:
        keep = int(DUMP_LIMIT_BYTES // per_traj)
        idx = np.sort(np.random.default_rng(seed).choice(batch, keep, replace=False))
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        kept = a if idx is None else a[idx]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(kept, dtype=np.float64))
    if idx is not None:
        np.save(os.path.join(path, "sample_index.npy"), idx.astype(np.float64))


def aggregate_fields(tm, dflt_iters, world):
    """The whole-job rates of the JSON line from max-over-ranks times (ms)."""
    return {"value": world * 1000.0 / tm["ms_step"],
            "co_headline": world * 5000.0 / tm["fit5_ms"],
            "fit_default_batched_it_per_s": world * 1000.0 * dflt_iters / tm["dflt_ms"],
            "single_iteration_batched_it_per_s": world * 1000.0 / tm["single_ms"],
            "fit5_batched_it_per_s": world * 5000.0 / tm["fit5_ms"]}


def fake_rank_times(rank):
    """--dist-selftest's stand-in per-rank times (ms): rank r is (1 + r/4)× rank 0, so the
    max over ranks is the last rank's (tests/test_dist.py checks every aggregate field)."""
    f = 1.0 + rank / 4.0
    return {k: f * v for k, v in zip(RANK_TIMES, (0.154, 3.4, 2.0, 0.15, 0.097, 0.05, 0.146))}, 4.0 + rank


def spawn_ranks(n):
    """`--gpus N` (N > 1) without a launcher (WORLD_SIZE unset): start N rank processes of
    this script, one per GPU, the way torch.distributed.run would (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT), and return the worst exit code.
    Runs before this process makes any GPU call; the ranks inherit stdout, so rank 0's
    JSON line is the run's one line. A rank that fails ends the others (their PIDs)."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    while procs:
        for p in list(procs):
            r = p.poll()
            if r is None:
                continue
            procs.remove(p)
            if r != 0:
                rc = rc or r
                for q in procs:  # the survivors would wait at a barrier forever
                    q.terminate()
        time.sleep(0.05)
    return rc


def dist_selftest(args, world, rank):
    """`--dist-selftest`: the multi-rank plumbing of this bench WITHOUT a GPU (gloo):
    process group, barrier-bracketed timed region, max over ranks, the per-trajectory
    result all-gather (ilqr_amd.dist.gather_fit_results) of `--batch` entries per rank,
    one JSON line from rank 0. No solve runs: `value` is null. tests/test_dist.py."""
    import torch.distributed as tdist
    from ilqr_amd.dist import gather_fit_results
    if world > 1:
        tdist.init_process_group("gloo")
    B = args.batch
    lq, x0, u0 = quadrotor_batch(B, T=args.T, seed0=rank * B)
    # the cold trajectories' costs stand in for a fit's (ℓ = xᵀQx + uᵀRu, ℓ_f = xᵀQf x)
    xs = x0[:, :-1]
    cost = (np.einsum("bti,bij,btj->b", xs, lq.Q, xs) + np.einsum("bi,bij,bj->b", x0[:, -1], lq.Qf, x0[:, -1]))
    if world > 1:
        tdist.barrier()
    t0 = time.perf_counter()
    wall = time.perf_counter() - t0
    tt = torch.tensor([wall], dtype=torch.float64)
    if world > 1:
        tdist.all_reduce(tt, op=tdist.ReduceOp.MAX)
    st = torch.zeros((B,), dtype=torch.int32)
    gc, gs = gather_fit_results(torch.from_numpy(cost), st) if world > 1 else (torch.from_numpy(cost), st)
    ok = bool(np.allclose(gc[rank * B:(rank + 1) * B].numpy(), cost))
    # the aggregate fields from stand-in per-rank times, reduced exactly as main() does
    times, iters = fake_rank_times(rank)
    tm, it_mean = reduce_over_ranks(times, iters, world, "cpu")
    if rank == 0:
        print(json.dumps({"metric": "dist-selftest (plumbing only, no solve)", "value": None, "n_gpus": world,
                          "allgather_check": {"trajectories": int(gc.numel()), "own_block_matches": ok,
                                              "finite_costs": int(torch.isfinite(gc).sum().item())},
                          "rank_times_max": tm, "dflt_iters_mean": it_mean,
                          "aggregates": aggregate_fields(tm, it_mean, world)}),
              flush=True)
    if world > 1:
        tdist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed batched fit iterations")
    ap.add_argument("--warmup", type=int, default=10, help="untimed batched fit iterations after the settle phase")
    ap.add_argument("--settle", type=float, default=1.0,
                    help="seconds of untimed fits before warmup (the GPU clock settles after ~0.1-0.5 s of load)")
    ap.add_argument("--batch", type=int, default=4096, help="trajectories per GPU")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline (module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed fit's x, u, cost, iters, status as DIR/<name>.npy")
    ap.add_argument("--cpu-budget", type=float, default=15.0, help="seconds for the CPU baseline sample (--full)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: no CPU baseline")
    ap.add_argument("--forward", default="dpp", choices=["dpp", "mfma"],
                    help="the ring forward's mat-vecs: DPP row broadcasts or the 4-block f64 MFMA")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the configs 2 and 5 lines")
    ap.add_argument("--dist-selftest", action="store_true",
                    help="multi-rank plumbing only, no GPU (gloo; tests/test_dist.py)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))  # no GPU call has been made in this process
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dist_selftest:
        return dist_selftest(args, world, int(os.environ.get("RANK", "0")))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = world > 1
    # one process per GPU; ILQR_DIST_BACKEND=gloo rehearses the multi-rank path on a
    # box with fewer GPUs than ranks (ranks then share devices round-robin)
    backend = os.environ.get("ILQR_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and local >= ndev:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but {ndev} visible GPU(s); one process per GPU "
                         f"(ILQR_DIST_BACKEND=gloo rehearses more ranks than GPUs)")
    gpu = local % max(ndev, 1) if backend != "nccl" else local
    if dist:
        import torch.distributed as tdist
        torch.cuda.set_device(gpu)
        if backend == "nccl":
            tdist.init_process_group("nccl", device_id=torch.device("cuda", gpu))
        else:
            tdist.init_process_group(backend)
    local = gpu
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    B, T = args.batch, args.T
    lq, x0, u0 = quadrotor_batch(B, T=T, seed0=rank * B)
    s = Solver(NX, NU, T, B, device=local)
    s.set_problem(lq)
    s.set_schedule(forward_mfma=args.forward == "mfma")
    lib, h = s.lib, s.h
    x = torch.from_numpy(x0).to(dev)
    u = torch.from_numpy(u0).to(dev)
    stream = torch.cuda.current_stream(dev)
    s._bind_stream()

    # every buffer the timed region and the kernel legs touch, allocated and first
    # touched up front (a first touch between legs idles the GPU and drops its clock)
    xo, uo = torch.empty_like(x), torch.empty_like(u)
    fcost = torch.empty((B,), dtype=torch.float64, device=dev)
    fiters = torch.empty((B,), dtype=torch.int32, device=dev)
    fst = torch.empty((B,), dtype=torch.int32, device=dev)
    if args.full:  # the sections after the timed region
        xn, un = torch.empty_like(x), torch.empty_like(u)
        pc = torch.empty((B,), dtype=torch.float64, device=dev)
        st = torch.zeros((B,), dtype=torch.int32, device=dev)
        trials = torch.empty((B,), dtype=torch.int32, device=dev)
        d = torch.empty((B, T, NU), dtype=torch.float64, device=dev)
        K = torch.empty((B, T, NU, NX), dtype=torch.float64, device=dev)
        pinf = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
        fwx, fwu = torch.empty_like(x), torch.empty_like(u)
        fwc = torch.empty((B,), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    prob = s._p()
    fit_opts = {n: _lib.default_options(max_iter=n, tol=-1.0) for n in range(1, 6)}
    fit_args = (_ptr(x), _ptr(u), None, _ptr(xo), _ptr(uo), _ptr(fcost), _ptr(fiters), _ptr(fst))
    fit_rc = []

    def fit(n_iter):  # iLQR.fit, n_iter iterations from cold, tol disabled (synchronises)
        rc = lib.ilqr_fit(h, prob, C.byref(fit_opts[n_iter]), *fit_args)
        if rc != _lib.OK:
            fit_rc.append(rc)

    def run_steps(k):
        plan = [FIT_ITERS] * (k // FIT_ITERS) + ([k % FIT_ITERS] if k % FIT_ITERS else [])
        times = []
        for n in plan:
            t0 = time.perf_counter()
            fit(n)
            times.append((time.perf_counter() - t0, n))
        return times

    # clock settle (time-based, nothing timed), then the warmup steps
    t_settle = time.perf_counter()
    n_settle = 0
    while time.perf_counter() - t_settle < args.settle:
        fit(FIT_ITERS)
        n_settle += 1
    settle_s = time.perf_counter() - t_settle
    run_steps(args.warmup)

    torch.cuda.synchronize()
    if dist:
        tdist.barrier()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    fit_times = run_steps(args.steps)
    e1.record(stream)
    torch.cuda.synchronize()
    if dist:
        tdist.barrier()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = e0.elapsed_time(e1) / args.steps
    ms_wall = wall * 1000.0 / args.steps
    ms_step = max(ms, ms_wall)   # this rank's; reduced over ranks with the other times below
    full = [t * 1000.0 / n for t, n in fit_times if n == FIT_ITERS]
    fit_stats = None
    if full:
        fit_stats = {"fits": len(full), "median_ms_per_iteration": float(np.median(full)),
                     "p10_ms": float(np.percentile(full, 10)), "p90_ms": float(np.percentile(full, 90)),
                     "median_fit_ms": float(np.median(full)) * FIT_ITERS}
    dumped = None
    if args.dump_outputs and rank == 0:
        # device copies, taken now: the sections of --full reuse the fit's result buffers
        dumped = {"x": xo.clone(), "u": uo.clone(), "cost": fcost.clone(), "iters": fiters.clone(),
                  "status": fst.clone()}
    cnt = algorithmic_counts(T)
    it_bytes = (cnt["bw_bytes"] + cnt["fw_bytes"]) * B
    it_flops = (cnt["bw_flops"] + cnt["fw_flops"]) * B

    def headline_result(ms_step):  # the fields of every run's line; ms_step: max over ranks
        return {
            "metric": "batched iLQR iterations/sec (fwd+bwd pass), nx=12 nu=4 T=100, 1/2/4/8 MI355X",
            "value": world * 1000.0 / ms_step,
            "unit": "batched iterations/s (one batched iteration = 4096 trajectories per GPU, backward+forward "
                    f"with line search, inside a {FIT_ITERS}-iteration fit from cold)",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic: per-instance randomised hover-linearised quadrotor LQ (SURVEY.md §8d)",
            "config": {"workload": f"quadrotor-style LQ iLQR.fit, {FIT_ITERS} iterations from cold, tol disabled",
                       "nx": NX, "nu": NU, "T": T, "batch_per_gpu": B, "global_batch": B * world,
                       "parallelism": f"independent trajectories, {world} rank(s), no data-path collective",
                       "forward": args.forward},
            "full": args.full,
            "clock_settle_s": settle_s, "clock_settle_fits": n_settle,
            "fit_timing": fit_stats,
            "fit_calls_ok": not fit_rc,
            "iteration": {"traj_iters_per_s": world * B * 1000.0 / ms_step,
                          "algorithmic_bytes": it_bytes, "algorithmic_flops": it_flops,
                          "hbm_gbps": it_bytes / (ms_step * 1e-3) / 1e9,
                          "hbm_frac": it_bytes / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                          "fp64_tflops": it_flops / (ms_step * 1e-3) / 1e12,
                          "event_ms": ms, "wall_ms": ms_wall},
        }

    def write_dump():
        if dumped is not None:
            dump_outputs(args.dump_outputs, {n: t.cpu().numpy() for n, t in dumped.items()})

    if not args.full:  # a plain run ends here
        tm, _ = reduce_over_ranks({"ms_step": ms_step}, 0.0, world, dev if backend == "nccl" else "cpu")
        write_dump()
        if rank == 0:
            print(json.dumps(headline_result(tm["ms_step"])), flush=True)
        s.close()
        if dist:
            tdist.destroy_process_group()
        return

    # secondary: the round-1 step (one iteration from cold per step, ilqr_iterate)
    opts1 = _lib.default_options(tol=-1.0)

    def cold_iteration():
        s.iterate(x, u, xn, un, None, st, trials=trials, options=opts1, new_cost=pc)

    t_run = time.perf_counter()   # run-in by time (see the fused chains below)
    while time.perf_counter() - t_run < 0.3:
        for _ in range(10):
            cold_iteration()
        torch.cuda.synchronize()
    n1 = max(50, args.steps)
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record(stream)
    for _ in range(n1):
        cold_iteration()
    a1.record(stream)
    torch.cuda.synchronize()
    single_ms = a0.elapsed_time(a1) / n1

    # dominant kernel: the backward pass, timed alone on the launch stream right after
    # the timed region (GPU still at its loaded clock), after a short untimed run-in
    o = _lib.default_options()

    def backward_only():
        lib.ilqr_backward(h, prob, C.byref(o), _ptr(x), _ptr(u), _ptr(d), _ptr(K), None)

    def forward_only():  # forward_pass with the backward's gains, prev_cost = Inf (1 trial)
        lib.ilqr_forward(h, prob, C.byref(o), _ptr(x), _ptr(u), None, _ptr(d), _ptr(K), _ptr(pinf),
                         _ptr(fwx), _ptr(fwu), _ptr(fwc), None, None)

    def leg(fn, nrep):
        t_run = time.perf_counter()
        while time.perf_counter() - t_run < 0.2:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
        b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b0.record(stream)
        for _ in range(nrep):
            fn()
        b1.record(stream)
        torch.cuda.synchronize()
        return b0.elapsed_time(b1) / nrep

    nrep = max(50, args.steps)
    bw_ms = leg(backward_only, nrep)
    fw_ms = leg(forward_only, nrep)

    # secondary (after the kernel legs: its empty launches idle the GPU): the 5-iteration fit (SURVEY §8d's I) and the reference's default call
    def timed_fit(o, reps=10):
        ts = []
        for _ in range(reps + 2):
            t0 = time.perf_counter()
            rc = lib.ilqr_fit(h, prob, C.byref(o), *fit_args)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[2:])) * 1000.0, rc

    fit5_ms, fit5_rc = timed_fit(fit_opts[5], reps=20)
    fit5_status = {int(k): int(v) for k, v in zip(*np.unique(fst.cpu().numpy(), return_counts=True))}
    dflt_ms, dflt_rc = timed_fit(_lib.default_options())
    dflt_iters = float(fiters.double().mean().item())
    dflt_status = {int(k): int(v) for k, v in zip(*np.unique(fst.cpu().numpy(), return_counts=True))}

    # untimed replay of the fit's 5 iterations (ilqr_iterate chained exactly as fit
    # chains them) for the line-search statistics and the monotone-cost check
    xa, ua, xb, ub = x.clone(), u.clone(), xn, un
    st.zero_()
    trials_per_iter, costs = [], []
    for it in range(5):
        s.iterate(xa, ua, xb, ub, None if it == 0 else pc, st, trials=trials, options=opts1, new_cost=pc)
        trials_per_iter.append(float(trials.double().mean().item()))
        costs.append(pc.clone())
        xa, xb, ua, ub = xb, xa, ub, ua
        if it + 1 == FIT_ITERS:
            ok = bool((st == 0).all().item()) and not fit_rc
            c = torch.stack(costs)
            monotone = bool((c[1:] < c[:-1]).all().item())
            x_last, u_last = xa.clone(), ua.clone()
    # fit output equals the replay's last iterate (same kernels, same order)
    fit(FIT_ITERS)
    fit_matches_replay = bool(torch.equal(xo, x_last) and torch.equal(uo, u_last))

    # the timed region's dominant kernel, lq_iter_fused4, launched exactly as fit launches
    # it: FIT_ITERS chained iterations from cold (ilqr_iterate = one fused launch each),
    # `reps` such chains back to back between ONE pair of HIP events on the launch stream
    # (an event pair around every launch adds its own ≈5-10 µs of stream bubbles); the
    # chains need no state reset: iterations 1-3 from cold accept (status stays OK)
    def fused_chain():
        xa, ua, xb, ub = x, u, xn, un
        for it in range(FIT_ITERS):
            s.iterate(xa, ua, xb, ub, None if it == 0 else pc, st, trials=trials, options=opts1, new_cost=pc)
            if it == 0:
                xa, ua, xb, ub = xn, un, fwx, fwu
            else:
                xa, xb, ua, ub = xb, xa, ub, ua

    # run-in by time: the sections after the timed region start from an idle GPU (host
    # work between them), and a few launches do not bring its clock back (rocprofv3 trace,
    # round 4: 157 µs for the first launches after an idle gap against 145 µs in the fits)
    st.zero_()
    t_run = time.perf_counter()
    while time.perf_counter() - t_run < 0.3:
        fused_chain()
        torch.cuda.synchronize()
    reps = 20
    f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    f0.record(stream)
    for _ in range(reps):
        fused_chain()
    f1.record(stream)
    torch.cuda.synchronize()
    fused_ok = bool((st == 0).all().item())
    fused_ms = f0.elapsed_time(f1) / (reps * FIT_ITERS)

    # every per-rank time behind an aggregate field, max over ranks (RANK_TIMES)
    rank_times = {"ms_step": ms_step, "fit5_ms": fit5_ms, "dflt_ms": dflt_ms, "single_ms": single_ms,
                  "bw_ms": bw_ms, "fw_ms": fw_ms, "fused_ms": fused_ms}
    tm, dflt_iters_all = reduce_over_ranks(rank_times, dflt_iters, world,
                                           dev if backend == "nccl" else "cpu")
    agg = aggregate_fields(tm, dflt_iters_all, world)
    ms_step, fit5_ms, dflt_ms, single_ms = tm["ms_step"], tm["fit5_ms"], tm["dflt_ms"], tm["single_ms"]
    bw_ms, fw_ms, fused_ms = tm["bw_ms"], tm["fw_ms"], tm["fused_ms"]

    # result exchange (fit output): all-gather the per-trajectory costs over RCCL, timed
    # with HIP events on the launch stream (it waits for the collective's stream) and by
    # the host clock, max over ranks
    gather_ms = gather_ev_ms = None
    gathered = None
    if dist:
        from ilqr_amd.dist import gather_fit_results
        tdist.barrier()
        torch.cuda.synchronize()
        g_e0, g_e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g0 = time.perf_counter()
        g_e0.record(stream)
        src_c, src_s = (fcost, fst) if backend == "nccl" else (fcost.cpu(), fst.cpu())
        gc, gs = gather_fit_results(src_c, src_s)
        g_e1.record(stream)
        torch.cuda.synchronize()
        gt = torch.tensor([(time.perf_counter() - g0) * 1000.0, g_e0.elapsed_time(g_e1)], dtype=torch.float64,
                          device=dev if backend == "nccl" else "cpu")
        tdist.all_reduce(gt, op=tdist.ReduceOp.MAX)
        gather_ms, gather_ev_ms = gt.tolist()
        gathered = {"trajectories": int(gc.numel()), "finite_costs": int(torch.isfinite(gc).sum().item()),
                    "status_max_iter": int((gs == _lib.TRAJ_MAX_ITER).sum().item())}

    # BASELINE configs 2 and 5 (tools/bench_twolink.py, tools/bench_rbd.py): their fit-
    # iteration rates and forward step latencies, after the headline's timed region
    secondary = None
    if world == 1 and not args.no_secondary:
        secondary = secondary_configs(local)

    bw_flops = cnt["bw_flops"] * B
    bw_bytes = cnt["bw_bytes"] * B
    fw_bytes = cnt["fw_bytes"] * B
    pmc, pmc_src = load_pmc_traffic(os.path.join(ROOT, "profiles"), B, T)
    traffic = pmc["hbm_bytes_per_backward_launch"] if pmc else None
    fused_traffic = pmc["hbm_bytes_per_fused_launch"] if pmc else None
    mf = load_mfma_pmc(os.path.join(ROOT, "profiles"))
    achieved_tf = bw_flops / (bw_ms * 1e-3) / 1e12
    # serial ceiling of the backward-then-forward schedule: backward at the FP64 spec
    # peak + forward at the guide's measured streaming-copy rate
    bw_floor_us = bw_flops / (FP64_PEAK_TFLOPS * 1e12) * 1e6
    fw_floor_us = fw_bytes / (HBM_COPY_GBPS * 1e9) * 1e6

    result = headline_result(ms_step)
    result["iteration"].update({"mean_line_search_trials": float(np.mean(trials_per_iter[:FIT_ITERS])),
                                "line_search_trials_per_iteration": trials_per_iter[:FIT_ITERS],
                                "cost_strictly_decreasing": monotone, "all_ok": ok,
                                "fit_equals_replay": fit_matches_replay})
    result.update({
        # the kernel the timed region spends ≈97 % of its time in (one launch per fit
        # iteration): algorithmic flops and bytes of one batched iteration ÷
        # its mean launch time inside the fit chain; FP64-issue-bound, HBM beside it
        "roofline": {"bound": "mfma", "kernel": "lq_iter_fused4 (backward_pass + forward_pass with line search, "
                                                "4 trajectories per wave, v_mfma_f64_4x4x4_4b + DPP ring forward)",
                     "achieved": it_flops / (fused_ms * 1e-3) / 1e12, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": it_flops / (fused_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                     "traffic": fused_traffic, "traffic_source": pmc_src,
                     "avg_launch_ms": fused_ms, "chains_all_ok": fused_ok,
                     "algorithmic_flops_per_launch": it_flops, "algorithmic_bytes_per_launch": it_bytes,
                     "hbm_achieved_gbps": it_bytes / (fused_ms * 1e-3) / 1e9,
                     "hbm_frac": it_bytes / (fused_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                     "timing": "HIP events around 20 back-to-back chains of the fit's 3 launches (iterations "
                               "1-3 from cold) on the launch stream, after 0.3 s of run-in chains; includes "
                               "the launches' gaps (rocprofv3 kernel stats: profiles/r05/)",
                     "mfma_pmc": mfma_summary(mf, "fused")},
        "backward_leg": {"bound": "mfma", "kernel": "lq_iter_backward4 (backward_pass alone, 4 trajectories per wave)",
                         "achieved": achieved_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved_tf / FP64_PEAK_TFLOPS, "traffic": traffic,
                         "traffic_source": pmc_src,
                         "avg_launch_ms": bw_ms, "algorithmic_flops_per_launch": bw_flops,
                         "algorithmic_bytes_per_launch": bw_bytes,
                         "hbm_achieved_gbps": bw_bytes / (bw_ms * 1e-3) / 1e9,
                         "mfma_pmc": mfma_summary(mf, "backward_api")},
        "forward_kernel": {"bound": "hbm", "kernel": "lq_forward (forward_pass + line search, LDS-ring input stream)",
                           "avg_launch_ms": fw_ms, "algorithmic_bytes_per_launch": fw_bytes,
                           "achieved_gbps": fw_bytes / (fw_ms * 1e-3) / 1e9,
                           "frac_of_spec": fw_bytes / (fw_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                           "frac_of_measured_copy": fw_bytes / (fw_ms * 1e-3) / 1e9 / HBM_COPY_GBPS},
        "serial_ceiling": {"backward_us_at_fp64_peak": bw_floor_us, "forward_us_at_copy_rate": fw_floor_us,
                           "batched_it_per_s": 1e6 / (bw_floor_us + fw_floor_us),
                           "note": "backward then forward, serialised per trajectory; 10k it/s needs overlap"},
        "fit_5_iterations": {"ms_per_iteration": fit5_ms / 5, "batched_it_per_s": agg["fit5_batched_it_per_s"],
                             "line_search_trials_per_iteration": trials_per_iter, "call_status": fit5_rc,
                             "trajectory_status_counts": fit5_status,
                             "note": "iterations 4-5 at the fp64 cost floor: capped line searches (status 3 = exhausted)"},
        "fit_default_options": {"ms_per_fit": dflt_ms, "mean_iterations": dflt_iters_all,
                                "batched_it_per_s": agg["fit_default_batched_it_per_s"], "call_status": dflt_rc,
                                "trajectory_status_counts": dflt_status,
                                "note": "the reference's default call: tol = 1e-6, max_iter = 100 (converged trajectories leave the batch)"},
        "single_iteration_cold": {"ms": single_ms, "batched_it_per_s": agg["single_iteration_batched_it_per_s"],
                                  "note": "one iteration from cold per step (ilqr_iterate = one launch of "
                                          "lq_iter_fused4: every wave's backward then its forward)"},
        "iteration_kernel": {"kernel": "lq_iter_fused4 (backward_pass + forward_pass, 4 trajectories per wave)",
                             "avg_launch_ms": single_ms,
                             "achieved_tflops": it_flops / (single_ms * 1e-3) / 1e12,
                             "frac_fp64_peak": it_flops / (single_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                             "achieved_gbps": it_bytes / (single_ms * 1e-3) / 1e9,
                             "frac_hbm_peak": it_bytes / (single_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                             "algorithmic_bytes_per_launch": it_bytes,
                             "traffic": fused_traffic,
                             "mfma_pmc": mfma_summary(mf, "fused")},
        "co_headline": {"metric": "batched iLQR iterations/sec (fwd+bwd pass), nx=12 nu=4 T=100, 1/2/4/8 MI355X",
                        "value": agg["co_headline"], "unit": "batched iterations/s",
                        "protocol": "SURVEY.md §8(d): 5-iteration fit from cold, tol disabled, median of 20 fits after "
                                    "2 warm-ups (iterations 4-5 at the fp64 cost floor, long line searches)",
                        "ms_per_fit": fit5_ms, "n_gpus": world},
        "secondary_configs": secondary,
        "allgather_costs_ms": gather_ms,
        "allgather_costs_event_ms": gather_ev_ms,
        "rank_reduction": "every time in this line is the max over ranks (the per-GPU kernel legs too: "
                          "roofline, backward_leg, forward_kernel, iteration_kernel); mean_iterations is the "
                          "mean over ranks; rank0_times are rank 0's own",
        "rank0_times": rank_times,
        "allgather_check": gathered,
        "cpu_baseline": None,
    })
    write_dump()
    if rank == 0 and world == 1 and not args.no_cpu:  # the CPU baseline: rank 0 at N = 1 only
        try:
            result["cpu_baseline"] = cpu_baseline(lq, x0, u0, args.cpu_budget)
        except Exception as e:  # the baseline is reported, never required
            result["cpu_baseline"] = {"error": repr(e)}
    if rank == 0:
        print(json.dumps(result), flush=True)
    s.close()
    if dist:
        tdist.destroy_process_group()


if __name__ == "__main__":
    main()
