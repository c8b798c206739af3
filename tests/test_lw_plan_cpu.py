"""The routing of the layer-wise path without a GPU: mjrl_amd/csrc/lw_plan.h (which k_gemm<BM, BN, NTH> / k_gemm_p<LB, EPI>
instances serve a product, in which column slices, over how many sample splits, under every MJX_LW_* switch that changes a
route) is plain host C++; tests/c/lw_plan.cpp feeds it product descriptions and compares the plans with a table written out by
hand.  Only the HIP headers are needed, for the types; no HIP library is linked."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "lw_plan.cpp")
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_lw_plan_routes(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    if not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("no HIP headers under %s" % HIP_INC)
    exe = str(tmp_path / "lw_plan")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC, SRC, "-o", exe],
                       capture_output=True, text=True, cwd=os.path.dirname(SRC))
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lw_plan ok" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])
