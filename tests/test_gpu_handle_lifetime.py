"""Every family's handle gives back what it acquired (ilqr_owned.h), on the GPU and
without a sanitizer: tools/san/abi_driver.cpp's `lifetime` mode, built here against the product
libilqr_hip.so, creates, uses once and destroys an LQ (12, 4) handle (one fused fit), a padded
LQ (6, 2) handle (one iteration: the padded scratch), a 2-link handle, a 2-joint fp32 chain with
cost_functions.jl's final cost, a 4-joint fp64 chain with a goal per trajectory in both cost
families, a floating-base handle and a one-device multi handle with two resident fits whose
history scratch regrows — three rounds of it, and the device memory in use after round 3 may
exceed that after round 2 by no more than 2 MiB, the runtime's sub-allocator chunk (the driver's
own criterion). One child process, run once.
"""
import os
import re
import shutil
import subprocess

import pytest

from ilqr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_three_rounds_of_every_handle_leave_device_memory_where_it_was(gpu, tmp_path):
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"
    cxx = rocm_clang if os.path.exists(rocm_clang) else (shutil.which("g++") or shutil.which("c++"))
    assert cxx, "no host C++ compiler"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "abi_driver"
    # the Makefile's abi_driver rule without -fsanitize
    subprocess.run([cxx, "-O1", "-g", "-fno-omit-frame-pointer", "-o", str(exe),
                    os.path.join(ROOT, "tools", "san", "abi_driver.cpp"), "-L" + libdir, "-lilqr_hip",
                    "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib",
                    "-lpthread"], check=True)
    # no sanitizer in this build: its options must not switch the driver's own check off
    env = {k: v for k, v in os.environ.items() if k != "ASAN_OPTIONS"}
    run = subprocess.run([str(exe), "lifetime"], capture_output=True, text=True, timeout=300, env=env)
    print(run.stdout)
    print(run.stderr[-4000:])
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    assert "handle lifetimes: 0 failed checks" in run.stdout
    m = re.search(r"round 3 − round 2: (-?\d+) B\)", run.stdout)
    assert m, run.stdout
    assert int(m.group(1)) <= 2 << 20, run.stdout
