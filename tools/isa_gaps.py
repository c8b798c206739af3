"""What stands between the bf16 MFMAs of a kernel's tile loop, gap by gap, from the library's assembly (hipcc -S --cuda-device-only
of csrc/mjx.hip, the flags of tools/isa_mix.py):   python tools/isa_gaps.py <mjx.s> <mangled-name-substring> [--per-row 12]
The loop is the kernel's largest backward-branch span.  Its v_mfma_f32_32x32x16_bf16 are listed in order, in phases of 48 (the
bf16x3 cached Fisher-vector product: R2, R3, R8 and, where it runs on bf16x3, R9), one K-step group of 12 gaps per row.  A gap is
what lies between one bf16 MFMA and the next: `N` vector-ALU instructions, `aN` v_accvgpr moves, `dN` DS instructions, `nN` s_nop,
`wN` s_waitcnt, `mN` other MFMAs (a phase's last gap holds whatever separates it from the next phase).  By the issue model of
DESIGN section 4 a gap hides up to 5 single-issue vector instructions; a lump is paid in full."""
import re
import sys

BF16_MFMA = "v_mfma_f32_32x32x16_bf16"
PHASE = 48                                     # 64 x 64 product on bf16x3: 4 K-step groups x 2 tiles x 6 piece products
PHASES = ("R2", "R3", "R8", "R9")


def kernels(lines, pat):
    """(mangled name, first line, last line) of every kernel whose mangled name contains `pat`"""
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and pat in m.group(1):
            end = next((k for k in range(i, len(lines)) if "s_endpgm" in lines[k]), None)
            if end is not None:
                out.append((m.group(1), i, end))
    return out


def tile_loop(body):
    """opcodes of the largest backward-branch span of a kernel body"""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    best = (0, 0, 0)
    for i, l in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[0]:
            best = (i - labels[m.group(1)], labels[m.group(1)], i)
    ops = []
    for l in body[best[1]:best[2] + 1]:
        s = l.strip()
        if s and not s.startswith((";", ".")) and not s.endswith(":"):
            ops.append(s.split()[0])
    return ops


def gaps(ops):
    """one dict of counts per bf16 MFMA of the loop: what follows it up to the next one (the last: up to the loop's end)"""
    out, cur = [], None
    for o in ops:
        if o.startswith(BF16_MFMA):
            cur = dict(valu=0, acc=0, ds=0, nop=0, wait=0, mfma=0)
            out.append(cur)
        elif cur is None:
            continue
        elif "mfma" in o:
            cur["mfma"] += 1
        elif o.startswith("v_accvgpr"):
            cur["acc"] += 1
        elif o.startswith("v_"):
            cur["valu"] += 1
        elif o.startswith("ds_"):
            cur["ds"] += 1
        elif o == "s_nop":
            cur["nop"] += 1
        elif o == "s_waitcnt":
            cur["wait"] += 1
    return out


def kernel_gaps(path, pat):
    """{mangled name: gap list} for every kernel of the assembly file whose name contains `pat`"""
    lines = open(path).read().split("\n")
    return {name: gaps(tile_loop(lines[a:b])) for name, a, b in kernels(lines, pat)}


def fmt(g):
    s = str(g["valu"])
    for key, tag in (("acc", "a"), ("ds", "d"), ("nop", "n"), ("wait", "w"), ("mfma", "m")):
        if g[key]:
            s += "%s%d" % (tag, g[key])
    return s


def table(gl, per_row=12):
    rows = []
    for i in range(0, len(gl), per_row):
        ph, off = divmod(i, PHASE)
        name = PHASES[ph] if ph < len(PHASES) else "P%d" % ph
        rows.append("%s g%d: %s" % (name, off // per_row, " ".join(fmt(g) for g in gl[i:i + per_row])))
    return "\n".join(rows)


if __name__ == "__main__":
    per_row = int(sys.argv[sys.argv.index("--per-row") + 1]) if "--per-row" in sys.argv else 12
    found = kernel_gaps(sys.argv[1], sys.argv[2])
    if not found:
        sys.exit("no kernel matches %r" % sys.argv[2])
    for name, gl in found.items():
        print("%s: %d bf16 MFMAs in the tile loop" % (name[:110], len(gl)))
        print(table(gl, per_row))
