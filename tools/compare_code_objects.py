"""Two gfx950 device-only objects of csrc/mjx.hip (hipcc --cuda-device-only -c, as tools/kernel_resources.py builds them), kernel by
kernel: the disassembly with addresses and comments stripped, compared by equality only, and the resource rows of the kernels that
differ (no GPU needed).   python tools/compare_code_objects.py parent.co branch.co [out.md]"""
import re, subprocess, sys, tempfile, os
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(co):
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "x.elf")
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + co, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", elf], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", elf], capture_output=True, text=True, check=True).stdout
    body, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1); body[name] = []
        elif name and line.strip():
            # "  addr:  insn  // comment" -> insn; branch targets keep their label (<name+0x...> offsets are relative to the function)
            body[name].append(re.sub(r"\s*//.*$", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", line)).strip())
    res = {}
    for k in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        g = lambda key: re.search(r"\.%s:\s+(\S+)" % key, k).group(1)
        res[g("name")] = dict(agpr=int(re.match(r"\s*(\d+)", k).group(1)), vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")),
                              scratch=int(g("private_segment_fixed_size")), vgpr_spills=int(g("vgpr_spill_count")),
                              static_lds=int(g("group_segment_fixed_size")))
    return {n: b for n, b in body.items() if n in res}, res


def waves(vgpr):                                            # waves per SIMD the unified register file (512 per lane) allows, 8 at most
    return min(8, 512 // (((vgpr + 7) // 8) * 8))


pa, ra = kernels(sys.argv[1]); pb, rb = kernels(sys.argv[2])
names = subprocess.run(["c++filt"], input="\n".join(sorted(set(pa) | set(pb))), capture_output=True, text=True).stdout.splitlines()
short = dict(zip(sorted(set(pa) | set(pb)), (re.sub(r"\(.*$", "", n.replace("void ", "").replace("mjx::", "")) for n in names)))
same = [n for n in pa if n in pb and pa[n] == pb[n]]
diff = [n for n in pa if n in pb and pa[n] != pb[n]]
rows_same = sum(1 for n in pa if n in pb and ra[n] == rb[n])
out = ["# Code object of csrc/mjx.hip, parent against this change", "",
       "Kernels: %d at the parent, %d here; only at the parent: %s; only here: %s." % (len(pa), len(pb), sorted(short[n] for n in set(pa) - set(pb)) or "none",
                                                                                  sorted(short[n] for n in set(pb) - set(pa)) or "none"),
       "Resource rows (VGPRs, AGPRs, SGPRs, scratch, VGPR spills, static LDS): %d of %d identical." % (rows_same, len(same) + len(diff)), "",
       "Disassembly (llvm-objdump -d, addresses and comments stripped, compared by equality): %d kernels identical, %d not." % (len(same), len(diff)), ""]
if diff:
    out += ["| kernel that differs | instructions parent -> here | vgpr (agpr) | sgpr | scratch B | vgpr spills | waves/SIMD |", "|---|---|---|---|---|---|---|"]
    for n in sorted(diff, key=short.get):
        a, b = ra[n], rb[n]
        out.append("| `%s` | %d -> %d | %d (%d) -> %d (%d) | %d -> %d | %d -> %d | %d -> %d | %d -> %d |" % (
            short[n], len(pa[n]), len(pb[n]), a["vgpr"], a["agpr"], b["vgpr"], b["agpr"], a["sgpr"], b["sgpr"], a["scratch"], b["scratch"],
            a["vgpr_spills"], b["vgpr_spills"], waves(a["vgpr"]), waves(b["vgpr"])))
text = "\n".join(out) + "\n"
print(text)
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write(text)
