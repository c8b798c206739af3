"""The host side of rollout ingestion under the sanitizers (VERDICT r04 "no sanitizer build of the host side").

mjrl_amd/csrc/host_ingest.h -- persistent gather pools, the converting gather, per-path sums, the asynchronous staging jobs and
their hand-over to the copy queue -- is plain C++ behind three device hooks; tests/c/host_san.cpp binds the hooks to memcpy, drives
every entry point from four caller threads at once (what train_step does: two staging jobs and the trainer's own gathers in flight
together) and checks the results.  Built and run here under -fsanitize=address,undefined and under -fsanitize=thread.
(The ThreadSanitizer build found a real race on HostPool::owner between two first-time callers: fixed in r05.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "host_san.cpp")
SRC_LS = os.path.join(ROOT, "tests", "c", "launch_state_san.cpp")
SRC_LP = os.path.join(ROOT, "tests", "c", "lw_plan.cpp")
SRC_UH = os.path.join(ROOT, "tests", "c", "update_host.cpp")
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
SAN = [("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]), ("tsan", ["-fsanitize=thread"])]


@pytest.mark.parametrize("name,flags", SAN)
def test_host_ingestion_under_sanitizers(tmp_path, name, flags):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("host_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread"] + flags + [SRC, "-o", exe], capture_output=True, text=True, cwd=os.path.dirname(SRC))
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no %s runtime" % name)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=600, env=env)
    # (the pools are leaked on purpose -- no joins in static destructors -- hence detect_leaks=0)
    assert r.returncode == 0 and "host_san ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])


@pytest.mark.parametrize("name,flags", SAN)
def test_launch_state_under_sanitizers(tmp_path, name, flags):
    """mjrl_amd/csrc/launch_state.h -- the dynamic-LDS attribute per (device, kernel), CU counts, scratch blocks per (site, device,
    stream) -- is plain host C++ over a handful of HIP runtime calls; tests/c/launch_state_san.cpp supplies those calls itself (a
    fake runtime with TWO devices, no HIP library) and runs every rule of the layer from four threads at once.  Only the HIP
    headers are needed, for the types."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    if not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("no HIP headers under %s" % HIP_INC)
    exe = str(tmp_path / ("launch_state_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC] + flags + [SRC_LS, "-o", exe],
                       capture_output=True, text=True, cwd=os.path.dirname(SRC_LS))
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no %s runtime" % name)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=600, env=env)
    # (the tables and the scratch blocks live as long as the process, like the state they stand for -- hence detect_leaks=0)
    assert r.returncode == 0 and "launch_state_san ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-500:], r.stderr[-4000:])


def test_lw_plan_under_sanitizers(tmp_path):
    """mjrl_amd/csrc/lw_plan.h -- routes, split counts, column slices and GemmArgs builders of the layer-wise path -- is plain
    host C++ without a HIP call; tests/c/lw_plan.cpp (its route table, tests/test_lw_plan_cpu.py) once more under
    -fsanitize=address,undefined: the column slices do pointer arithmetic on every operand."""
    name, flags = SAN[0]
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    if not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("no HIP headers under %s" % HIP_INC)
    exe = str(tmp_path / ("lw_plan_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC] + flags + [SRC_LP, "-o", exe],
                       capture_output=True, text=True, cwd=os.path.dirname(SRC_LP))
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no %s runtime" % name)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=0"))
    assert r.returncode == 0 and "lw_plan ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])


def test_update_host_under_sanitizers(tmp_path):
    """mjrl_amd/csrc/peer_layout.h and the plain-C++ top of mjrl_amd/csrc/update_host.h -- the peer buffer's layout and views, the
    exchange counter, the CG and folding routes, the profiling brackets' pick -- are host C++ without a HIP call;
    tests/c/update_host.cpp (their tables, tests/test_update_host_cpu.py) once more under -fsanitize=address,undefined: the views
    are pointer arithmetic on every rank's base, the counter wraps on purpose."""
    name, flags = SAN[0]
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("update_host_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags + [SRC_UH, "-o", exe], capture_output=True, text=True, cwd=os.path.dirname(SRC_UH))
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no %s runtime" % name)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=0"))
    assert r.returncode == 0 and "update_host ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
