"""Worker of tests/test_gpu_fvp_bf3_bits.py and of tests/golden/make_golden_fvp_bf3_bits.py: the bits of the bf16x3 cached
Fisher-vector product (k_fused<64, 64, 1, 8, MODE_FVP, ..., CACHED, BF3, BF3R9>, csrc/fused_policy.h).

    python _fvp_bf3_bits_worker.py <out.npz>

Runs every case of CASES with the library mjrl_amd._lib names (MJX_LIB) and the MJX_FVP_BF16X3_R9 setting of its environment
(read once per process, so one worker per setting): K1 at old == new, which fills the activation cache, then two consecutive
products of one direction -- the first walks the tiles back to front, the second front to back -- each into a NaN-prefilled
buffer.  Writes <case>_p0 / <case>_p1 (uint32 views of the two products) plus `cu` (the device's CU count; the grouping of the
workgroup partials follows the grid) and `r9` (the setting it ran with)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests._fused_matrix_worker import fused_info, fused_inputs  # noqa: E402

M, HID = 6, (64, 64)
WIDTHS = {17: 20, 9: 12, 5: 8, 21: 0}          # observation width -> the instance's compile-time feature count NPC
# 65 553 = 2 x 256 CUs x 4 waves x 32 rows + 17: the smallest count at which waves walk two tiles (the next-tile prefetch in
# R8 runs) and the last tile is masked
SIZES = (1, 33, 65553)
CASES = [(n, N) for n in WIDTHS for N in SIZES]


def case_name(n, N):
    return "n%d_N%d" % (n, N)


def r9_setting():
    return 0 if os.environ.get("MJX_FVP_BF16X3_R9") == "0" else 1


def encode(r1, r0):
    """the fixture's arrays from the two workers' results (r9 = 1, r9 = 0): see tests/golden/make_golden_fvp_bf3_bits.py"""
    out = dict(cu=r1["cu"])
    for n, N in CASES:
        c = case_name(n, N)
        out["r9_1_%s_p0" % c] = r1[c + "_p0"]
        out["r9_1_%s_p1" % c] = r1[c + "_p1"] ^ r1[c + "_p0"]
        out["r9_0_%s_p0" % c] = r0[c + "_p0"] ^ r1[c + "_p0"]
        out["r9_0_%s_p1" % c] = r0[c + "_p1"] ^ r1[c + "_p1"]
    return out


def decode(gold):
    """-> {(r9, case name, product index): uint32 words}"""
    out = {}
    for n, N in CASES:
        c = case_name(n, N)
        out[1, c, 0] = gold["r9_1_%s_p0" % c]
        out[1, c, 1] = gold["r9_1_%s_p1" % c] ^ out[1, c, 0]
        out[0, c, 0] = gold["r9_0_%s_p0" % c] ^ out[1, c, 0]
        out[0, c, 1] = gold["r9_0_%s_p1" % c] ^ out[1, c, 1]
    return out


def run_case(n, N):
    import torch
    from mjrl_amd.engine import UpdateEngine
    eng = UpdateEngine(n, M, HID)
    variant, npc, _, _ = fused_info(eng)
    assert eng.fused and (variant, npc) == (1, WIDTHS[n]), (n, variant, npc)
    inp = fused_inputs(n, M, HID, N, 1000 * n + N % 997)
    eng.set_batch(inp["obs"], inp["act"], inp["adv"])
    eng.set_policy(inp["th"], inp["th"], inp["pk"], inp["pk"])
    eng.surr_vpg()
    v = torch.from_numpy(inp["v"]).to(eng.device)
    out = []
    for _ in range(2):
        buf = torch.full_like(eng.Ap, float("nan"))
        eng.fvp(v, buf)
        out.append(buf.cpu().numpy().view(np.uint32).copy())
    eng.close()
    return out


def main():
    import torch
    res = dict(cu=np.int64(torch.cuda.get_device_properties(0).multi_processor_count), r9=np.int64(r9_setting()))
    for n, N in CASES:
        res[case_name(n, N) + "_p0"], res[case_name(n, N) + "_p1"] = run_case(n, N)
    np.savez(sys.argv[1], **res)


if __name__ == "__main__":
    main()
