"""The host side of the update path without a GPU: the peer exchange's buffer layout, the producer's and the consumer's view of
an exchange and the exchange counter (mjrl_amd/csrc/peer_layout.h), the CG vector update's route, the condition under which the
peer exchange is folded into the solve's kernels, and which launches mjx_profile_enable brackets (the plain-C++ top of
mjrl_amd/csrc/update_host.h).  tests/c/update_host.cpp compares them with tables written out by hand; no HIP header is needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "update_host.cpp")


def test_update_host_layout_views_routes_and_brackets(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "update_host")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", SRC, "-o", exe], capture_output=True, text=True, cwd=os.path.dirname(SRC))
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "update_host ok" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])
