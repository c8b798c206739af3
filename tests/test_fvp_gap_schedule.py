"""The compiled schedule of the bf16x3 cached Fisher-vector product's R2 and R8 phases (csrc/fused_policy.h, the XBF3 branches):
what stands between consecutive v_mfma_f32_32x32x16_bf16 of the tile loop, read from the device assembly (tools/isa_gaps.py).
No GPU: the eight instances (NPC 20 / 12 / 8 / 0 x BF3R9 on / off) are compiled for gfx950 once per run, from a translation unit
that holds nothing but them, with the flags of the library build.

Per instance:
  * 48 bf16 MFMAs per bf16x3 phase of a tile: 192 with R9 on bf16x3 (R2, R3, R8, R9), 144 with R9 on fp32 MFMAs (BF3R9 off);
  * in R2 and in R8, no gap but the phase's last carries more than 5 vector-ALU instructions (v_accvgpr moves included) or more
    than 3 DS instructions.  5 is what one wave per SIMD hides per 32-cycle gap of this MFMA; the source
    places 4 split instructions and at most 2 DS instructions.  The last gap is exempt: the VA burst, resp. R9's front burst,
    stands there by design;
  * no scratch, at most 512 registers.
Before the phases were placed by program order, every instance had a gap of 37 .. 88 vector-ALU instructions in R2 and of
33 .. 71 in R8, with up to 60 DS instructions."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mjrl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_spec = importlib.util.spec_from_file_location("isa_gaps", os.path.join(ROOT, "tools", "isa_gaps.py"))
isa_gaps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_gaps)

INSTANCES = [(npc, r9) for npc in (20, 12, 8, 0) for r9 in (True, False)]
MAX_VALU, MAX_DS = 5, 3
PHASE = isa_gaps.PHASE


def mangled(npc, r9):
    return "_ZN3mjx7k_fusedILi64ELi64ELi1ELi8ELi1ELb0ELi%dELb1ELb1ELb%dEEEvNS_9FusedArgsE" % (npc, int(r9))


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("fvp_asm")
    src, out = str(d / "fvp_bf3.hip"), str(d / "fvp_bf3.s")
    with open(src, "w") as f:
        f.write('#include "fused_policy.h"\nnamespace mjx {\n')
        for npc, r9 in INSTANCES:
            f.write("template __global__ void k_fused<64, 64, 1, 8, MODE_FVP, false, %d, true, true, %s>(FusedArgs);\n" % (npc, "true" if r9 else "false"))
        f.write("}\n")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-mllvm", "-amdgpu-mfma-vgpr-form",
                           "--cuda-device-only", "-I" + CSRC, "-S", "-o", out, src])
    text = open(out).read()
    return text, isa_gaps.kernel_gaps(out, "k_fusedILi64ELi64ELi1ELi8ELi1E")


@pytest.mark.parametrize("npc,r9", INSTANCES, ids=["npc%d_r9_%d" % (n, int(r)) for n, r in INSTANCES])
def test_r2_r8_gaps(asm, npc, r9):
    text, found = asm
    name = mangled(npc, r9)
    assert name in found, sorted(found)
    gl = found[name]
    print(isa_gaps.table(gl))
    assert len(gl) == (4 if r9 else 3) * PHASE, len(gl)
    for phase, first in (("R2", 0), ("R8", 2 * PHASE)):
        for k, g in enumerate(gl[first:first + PHASE - 1]):
            assert g["valu"] + g["acc"] <= MAX_VALU and g["ds"] <= MAX_DS and g["mfma"] == 0, \
                "%s gap %d (group %d): %s" % (phase, k, k // 12, isa_gaps.fmt(g))
    # the kernel's resource lines follow its code and its descriptor: the first ones behind its label
    tail = text[text.index("\n" + name + ":"):]
    regs = int(re.search(r"; TotalNumVgprs: (\d+)", tail).group(1))
    scratch = int(re.search(r"; ScratchSize: (\d+)", tail).group(1))
    assert scratch == 0 and regs <= 512, (regs, scratch)
