"""The owner of a handle's device resources (ilqr.jl_amd/csrc/ilqr_owned.h), on the CPU with a
counting fake runtime (tests/owned_driver.cpp, built here with a host compiler under
AddressSanitizer and UBSan, leak checking on).

Every handle of the C ABI acquires its device memory, pinned memory, events and streams through
one owner and releases them by destroying it. The driver runs a plan of
ilqr_create's shape — required buffers, a zeroed one, a pinned one, two events, a stream, two
optional groups with a partner each — and fails each of its acquisitions in turn.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_STEPS = 15  # owned_driver.cpp's PLAN_STEPS: the sweep leaves no acquisition out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"
    cxx = shutil.which("g++") or (rocm_clang if os.path.exists(rocm_clang) else None) or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("owned") / "owned_driver"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ilqr.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "owned_driver.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    res = {}
    for line in run.stdout.splitlines():
        name, verdict = line.split(" ", 1)
        res[name] = verdict
    # a sanitizer report (a leak among them) ends the program with a non-zero status
    res["exit"] = (run.returncode, run.stderr[-2000:])
    return res


def test_driver_ran_clean_under_the_sanitizers(results):
    failed = {k: v for k, v in results.items() if k != "exit" and v != "ok"}
    assert results["exit"][0] == 0 and not failed, (results["exit"], failed)
    assert sum(k.startswith("fail_at_") for k in results) == PLAN_STEPS


@pytest.mark.parametrize("k", range(1, PLAN_STEPS + 1))
def test_failing_acquisition_k_releases_everything_once_in_reverse(results, k):
    assert results[f"fail_at_{k}"] == "ok"


@pytest.mark.parametrize("scenario", ["no_failure", "swapped", "zero_failure", "optional", "refill", "destructor"])
def test_scenario(results, scenario):
    assert results[scenario] == "ok"
