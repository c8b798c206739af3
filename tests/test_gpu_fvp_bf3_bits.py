"""The bits of the bf16x3 cached Fisher-vector product (k_fused<64, 64, 1, 8, MODE_FVP, ..., CACHED, BF3, BF3R9>,
csrc/fused_policy.h) against tests/golden/fvp_bf3_bits.npz, recorded on an MI355X from the build before the R2 / R8 phases were
re-placed gap by gap (tests/golden/make_golden_fvp_bf3_bits.py).  A schedule change moves no MFMA within its accumulator chain
and changes no operand, so every output word must stay what it was: the comparison is bit equality.

Cases (tests/_fvp_bf3_bits_worker.py): observation widths 17, 9, 5, 21 (the instances with NPC 20 / 12 / 8 / 0) with 6 actions,
at N = 1, 33 and 65 553 rows (the smallest count at which waves walk two tiles: R8's next-tile prefetch and the masked last tile
both run).  Each case runs K1 and two consecutive products into NaN-prefilled buffers, so both sweep directions are compared.
One worker process per MJX_FVP_BF16X3_R9 setting (the switch is read once per process).  The fixture holds the CU count it was
recorded on; the grouping of the workgroup partials follows the grid, so the test skips on a device with another count."""
import os
import sys

import numpy as np
import pytest

from tests._fvp_bf3_bits_worker import CASES, case_name, decode
from tests._worker_run import arm_runner, run_child

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fvp_bf3_bits.npz")
SCRUB = ("MJX_FORCE_LAYERWISE", "MJX_RAW_SLAB", "MJX_FVP_BF16X3", "MJX_NO_HCACHE", "MJX_FVP_SWEEP")


@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(GOLD))
    return int(g["cu"]), decode(g)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """r9 -> the worker's results; each worker runs once, on first use.  A worker that fails (an error, a fault, a timeout) is
    never started again, and neither is the other one: the GPU may be left in a bad state (arm_runner)."""
    def start(r9, out_dir):
        path = os.path.join(out_dir, "out.npz")
        run_child([sys.executable, os.path.join(HERE, "_fvp_bf3_bits_worker.py"), path], 300, "r9 = %d" % r9, scrub=SCRUB,
                  env={"MJX_FVP_BF16X3_R9": str(r9)})
        return dict(np.load(path))
    return arm_runner(start, lambda r9: str(tmp_path_factory.mktemp("r9_%d" % r9)), "r9 = %d")


@pytest.mark.parametrize("n,N", CASES, ids=[case_name(n, N) for n, N in CASES])
@pytest.mark.parametrize("r9", [1, 0], ids=["r9_1", "r9_0"])
def test_bits_unchanged(gold, runs, r9, n, N):
    cu, want = gold
    r = runs(r9)
    if int(r["cu"]) != cu:
        pytest.skip("fixture recorded on %d CUs, this device has %d: the partials are grouped by the grid" % (cu, int(r["cu"])))
    assert int(r["r9"]) == r9
    c = case_name(n, N)
    for p in (0, 1):
        got, ref = r["%s_p%d" % (c, p)], want[r9, c, p]
        assert got.shape == ref.shape
        assert np.isfinite(got.view(np.float32)).all(), "%s product %d: NaN prefill left standing or non-finite output" % (c, p)
        diff = np.flatnonzero(got != ref)
        assert diff.size == 0, "%s product %d (r9 = %d): %d of %d words differ, first at %d: %08x vs %08x" % (
            c, p, r9, diff.size, got.size, diff[0], got[diff[0]], ref[diff[0]])
