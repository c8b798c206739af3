"""Who owns what among the fused path's headers (no GPU; the HIP compiler cross-compiles for gfx950):
  * csrc/mfma_prims.h and csrc/bf16x3.h stand alone: a translation unit that includes only one of them and uses one of its primitives
    in a small kernel compiles device-only;
  * none of the nine headers that are written with those primitives sees the fused policy kernel: preprocessed alone, their text
    names neither k_fused nor FusedArgs.
csrc/fused_layout.h is written for the HIP compiler (__host__ __device__ members; its header comment says so): there is no host-
compiler check of it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mjrl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEVICE = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-Wno-unused-value", "--cuda-device-only", "-I" + CSRC]

CONSUMERS = ["lw_gemm.h", "lw_gemm_p.h", "lw_head.h", "layerwise.h", "mlp_fit.h", "policy_fit.h", "dyn_fit_ens.h", "dfe_tiles.h",
             "mfma_chain.h"]

KERNELS = {
    "mfma_prims.h": """
__global__ void k_probe(const float* a, const float* b, float* out) {
  mjx::f32x16 z = (mjx::f32x16)(0.f), h;
  z = MJX_MFMA(a[threadIdx.x], b[threadIdx.x], z);
  mjx::fast_tanh16(h, z);
  for (int r = 0; r < 16; ++r) out[16 * threadIdx.x + r] = h[r];
}
""",
    "bf16x3.h": """
__global__ void k_probe(const float* a, const float* b, float* out) {
  float x[8], y[8];
  for (int i = 0; i < 8; ++i) { x[i] = a[8 * threadIdx.x + i]; y[i] = b[8 * threadIdx.x + i]; }
  const mjx::f32x16 z = mjx::mfma_bf3(mjx::split3(x), mjx::split3(y), (mjx::f32x16)(0.f));
  for (int r = 0; r < 16; ++r) out[16 * threadIdx.x + r] = z[r];
}
""",
}


@pytest.mark.parametrize("header", sorted(KERNELS))
def test_primitive_header_stands_alone(tmp_path, header):
    src = tmp_path / "probe.hip"
    src.write_text('#include "%s"\n%s' % (header, KERNELS[header]))
    out = tmp_path / "probe.s"
    subprocess.check_call(DEVICE + ["-O3", "-S", "-o", str(out), str(src)])
    text = out.read_text()
    assert "k_probe" in text and "v_mfma_f32_32x32x" in text


@pytest.mark.parametrize("header", CONSUMERS)
def test_consumer_header_does_not_see_the_fused_kernel(tmp_path, header):
    src = tmp_path / "only.hip"
    src.write_text('#include "%s"\n' % header)
    text = subprocess.check_output(DEVICE + ["-E", str(src)], text=True)
    assert "fast_tanh16" in text                        # the primitives did arrive
    for name in ("k_fused", "FusedArgs"):
        assert not re.search(r"\b%s\b" % name, text), (header, name)
