"""The route ladder of the learned-model entries without a GPU: which MFMA routes an entry tries, in which order, and what a call
without rows reports, from what was asked, the entry's two switches and its two shape answers (the plain-C++ top of
mjrl_amd/csrc/model_host.h).  tests/c/model_host.cpp compares all 32 combinations with a table written out by hand; no HIP header
is needed.  Built and run plainly, and once more as an ordinary program under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "model_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("name,flags", [("plain", ["-Wall", "-Werror"]), ("asan_ubsan", SAN)])
def test_model_host_route_table(tmp_path, name, flags):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / ("model_host_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags + [SRC, "-o", exe], capture_output=True, text=True, cwd=os.path.dirname(SRC))
    if b.returncode != 0 and "sanitize" in b.stderr and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no %s runtime" % name)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="abort_on_error=0"))
    assert r.returncode == 0 and "model_host ok" in r.stdout and "Sanitizer" not in r.stderr, (r.stdout[-4000:], r.stderr[-4000:])
