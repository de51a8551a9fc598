"""Compile-only check of the measured build alternates (no GPU needed: hipcc
cross-compiles gfx950 here). The product sources hold one path per kernel; the
alternates they were measured against — the backward's round-2
instruction cuts undone and its probe bits (ABL), the one-wave backward's variants,
the ring forward's LDS row broadcasts, cache hints and timing-only ablations, the
chain's Rodrigues-form / unpacked evaluations, the 2-link forward on the generic RK4
— live in tools/archive/ablation/restore_alternates.patch, and those of rounds 5-6 — the
one-exchange sixteen-trial pass, Q rows from the LDS, fixed grab widths, the earlier
hand-out orders, the de-phase probe, the floating forward's two-barrier rollout — in
restore_alternates_r06.patch beside it. This test applies the patches to one
copy of the current sources and compiles them with the alternates switched on, so
that record stays reproducible against the product tree."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "tools", "archive", "ablation", "restore_alternates.patch")
PATCH_R06 = os.path.join(ROOT, "tools", "archive", "ablation", "restore_alternates_r06.patch")
HIPCC = "/opt/rocm/bin/hipcc"


def _hipcc():
    return HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None or shutil.which("patch") is None, reason="no hipcc / patch")
def test_restore_alternates_patch_builds(tmp_path):
    os.makedirs(tmp_path / "ilqr.jl_amd")
    shutil.copytree(os.path.join(ROOT, "ilqr.jl_amd", "csrc"), tmp_path / "ilqr.jl_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    with open(PATCH) as f:
        r = subprocess.run(["patch", "-p1", "--fuzz=3", "--no-backup-if-mismatch", "-s"], stdin=f,
                           cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, "restore_alternates.patch no longer applies: " + r.stdout + r.stderr
    with open(PATCH_R06) as f:
        r = subprocess.run(["patch", "-p1", "--fuzz=3", "--no-backup-if-mismatch", "-s"], stdin=f,
                           cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, "restore_alternates_r06.patch no longer applies: " + r.stdout + r.stderr
    csrc = tmp_path / "ilqr.jl_amd" / "csrc"
    base = [_hipcc(), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-c"]
    mf = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
    chain = mf + ["-fno-slp-vectorize", "-DILQR_CHAIN_FD_ROT=0", "-DILQR_CHAIN_FD_PAIR=0", "-DILQR_CHAIN_F2_FAST=0"]
    jobs = [
        # the backward with the round-2 instruction cuts undone, slot loads without nt; the
        # cooperative search in four-trial grabs, its hand-out key without the deep class and
        # smallest-`next` first at the frontier, Q rows of the sixteen-trial pass from the LDS
        mf + ["-DILQR_BW4_MU_IN_H=0", "-DILQR_BW4_SEL_FMA=0", "-DILQR_BW4_SLOW_MFMA=0",
              "-DILQR_BW4_MFMA_T=0", "-DILQR_FW_LD_NT=0", "-DILQR_COOP_WIDTH=4", "-DILQR_COOP_DEEP_FIRST=0",
              "-DILQR_COOP_FRONTIER_DEEP=0", "-DILQR_CAND16_QREG=0", "ilqr_bw4.hip"],
        # the ring forward's LDS row broadcasts, one-wave workgroups, ablation bits
        ["-DILQR_FW_LDS_BCAST=1", "-DILQR_FW_WAVES=1", "-DILQR_FW_ABLATE=3", "ilqr_lq.hip"],
        # the 2-link forward on the generic RK4 with a 4-deep prefetch
        mf + ["-DILQR_TL_RK4_SHIFT=0", "-DILQR_FW_GROUP_PF=4", "ilqr_twolink.hip"],
        # the chain's Rodrigues-form central differences, unpacked ±h and fp32 step: the 2-joint
        # object and the tiles path's object of every joint count (below)
        chain + ["ilqr_chain.hip"],
        # the fused kernel's de-phase probe, the sixteen-trial pass with one exchange a step
        mf + ["-DILQR_FUSED_DEPHASE_PROBE=1", "-DILQR_CAND16_FORM=2", "ilqr_bw4.hip"],
        # the floating forward's two-barrier rollout on three waves
        ["-ffp-contract=on", "-DILQR_FB_LOOKAHEAD=0", "ilqr_floating.hip"],
    ] + [chain + [f"-DILQR_CHAIN_NJ={nj}", "ilqr_chain_tiles.hip"] for nj in (4, 5, 6, 7)]

    def build(job):
        i, args = job
        src = args[-1]
        cmd = base + args[:-1] + [str(csrc / src), "-o", str(tmp_path / f"{src}.{i}.o")]
        return src, subprocess.run(cmd, capture_output=True, text=True, timeout=900)

    with ThreadPoolExecutor(8) as ex:
        for src, r in ex.map(build, enumerate(jobs)):
            assert r.returncode == 0, (src, r.stderr[-2000:])
