"""The W2 gradient (R9: gW2 += delta2^T h1) of the cached Fisher-vector product on bf16x3 MFMAs (csrc/fused_policy.h,
k_fused<..., BF3 = true, BF3R9 = true>): against the kernel that keeps R9 on fp32 MFMAs (MJX_FVP_BF16X3_R9=0) and against the fp64
oracle.  The switch is read once per process, so each kernel runs every case in one child process (two children for the whole
file); the tests below only compare what they returned.

Bounds: TOL_FVP and the 1e-6 distance between two kernels are the project's bars (tests/test_gpu_fvp_bf16x3.py).  The W2 block
alone may be at most 2 x as far from fp64 as the fp32-R9 kernel's W2 block on the same inputs: the six-product split drops only
terms of relative size about 2^-24, the size of an fp32 rounding, so it should sit at the fp32 product's distance and not beat
it.  At the edge sizes (no second kernel to compare with) the W2 block is held to TOL_FVP like the vector: a padded sample that
contributed anything at N = 1 (31 padded rows beside one real one) would put the block off by its own size."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import npg_oracle as O
from tests._worker_run import run_child
from tests.test_gpu_fvp_bf16x3 import _CHILD, HID, INSTANCES, ROOT, TOL_FVP, case, rel

pytestmark = pytest.mark.gpu

N_INST = 40000                       # > 32 rows x 1 024 waves: some waves accumulate two tiles in their AGPRs, the others one
EDGES = [1, 31, 32, 33, 32768 + 33]  # one sample, the partial-tile edges, a wave's partial second tile
SCALES = (1e-8, 1.0, 1e8, 0.0)

# both kernels run every spec: the 7 instances, the scaled / zero vectors, saturated units, the edge sizes, repeated launches
SPECS = ([dict(n=n, m=m, N=N_INST) for n, m in INSTANCES]
         + [dict(n=17, m=6, N=N_INST, seed=1, scales=SCALES)]
         + [dict(n=17, m=6, N=N_INST, seed=2, wscale=8.0)]
         + [dict(n=17, m=6, N=N, seed=3) for N in EDGES]
         + [dict(n=17, m=6, N=32768 + 33, seed=4, reps=3)])
K_SCALE, K_SAT, K_EDGE, K_REP = len(INSTANCES), len(INSTANCES) + 1, len(INSTANCES) + 2, len(INSTANCES) + 2 + len(EDGES)


def blocks(n, m):
    """name -> slice of the flat parameter vector (FlatOff: W1, b1, W2, b2, W3, b3, log_std)"""
    out, o = {}, 0
    for name, size in (("W1", n * HID[0]), ("b1", HID[0]), ("W2", HID[1] * HID[0]), ("b2", HID[1]), ("W3", m * HID[1]), ("b3", m), ("log_std", m)):
        out[name] = slice(o, o + size)
        o += size
    return out


def oracle(spec):
    kw = {k: spec[k] for k in ("seed", "wscale") if k in spec}
    obs, act, adv, th, v = case(spec["n"], spec["m"], spec["N"], **kw)
    return O.fvp(th.astype(np.float64), obs.astype(np.float64), v.astype(np.float64), spec["n"], spec["m"], HID)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(new kernel's results, fp32-R9 kernel's results), keys "<spec index>_<h<i> | rep<r>>" """
    tmp, res = tmp_path_factory.mktemp("r9"), []
    for on in (1, 0):
        path = os.path.join(str(tmp), "out_%d.npz" % on)
        run_child([sys.executable, "-c", _CHILD, ROOT, json.dumps(SPECS), path], 600, "MJX_FVP_BF16X3_R9 = %d" % on,
                  env={"MJX_FVP_BF16X3": "1", "MJX_FVP_BF16X3_R9": str(on)}, cwd=ROOT)
        res.append(dict(np.load(path)))
    return res


@pytest.mark.parametrize("k", range(len(INSTANCES)), ids=["%dx%d" % nm for nm in INSTANCES])
def test_r9_every_instance(runs, k):
    """only the W2 block changes; it stays at the fp32 product's distance from fp64"""
    a, b = runs
    n, m = INSTANCES[k]
    h, hp, ref = a["%d_h0" % k], b["%d_h0" % k], oracle(SPECS[k])
    bl = blocks(n, m)
    assert h.size == bl["log_std"].stop
    assert not np.array_equal(h[bl["W2"]], hp[bl["W2"]]), "the switch selected the same kernel"
    for name, sl in bl.items():
        if name != "W2":
            assert np.array_equal(h[sl].view(np.uint32), hp[sl].view(np.uint32)), name
    e_new, e_par = rel(h[bl["W2"]], ref[bl["W2"]]), rel(hp[bl["W2"]], ref[bl["W2"]])
    print("R9 W2-block rel-L2 vs fp64 (n %d, m %d): bf16x3 %.3e, fp32 %.3e; whole vector %.3e / %.3e, between the kernels %.3e"
          % (n, m, e_new, e_par, rel(h, ref), rel(hp, ref), rel(h, hp)))
    assert rel(h, hp) < 1e-6
    assert rel(h, ref) < TOL_FVP
    assert e_new <= 2.0 * e_par


def test_r9_scaled_and_zero_vectors(runs):
    """the split is exact at any exponent; v = 0 gives exactly 0"""
    a, b = runs
    ref, w2 = oracle(SPECS[K_SCALE]), blocks(17, 6)["W2"]
    for i, s in enumerate(SCALES[:3]):
        h, hp = a["%d_h%d" % (K_SCALE, i)] / s, b["%d_h%d" % (K_SCALE, i)] / s
        print("R9 v x %g: W2 block %.3e (fp32 R9 %.3e), whole %.3e" % (s, rel(h[w2], ref[w2]), rel(hp[w2], ref[w2]), rel(h, ref)))
        assert rel(h, ref) < TOL_FVP, s
        assert rel(h[w2], ref[w2]) <= 2.0 * rel(hp[w2], ref[w2]), s
    assert not np.any(a["%d_h3" % K_SCALE])


def test_r9_saturated_units(runs):
    """wscale = 8: h1 about +-1 and delta2 tiny, the worst case for the piece products"""
    a, b = runs
    ref, w2 = oracle(SPECS[K_SAT]), blocks(17, 6)["W2"]
    h, hp = a["%d_h0" % K_SAT], b["%d_h0" % K_SAT]
    print("R9 saturated: W2 block %.3e (fp32 R9 %.3e), whole %.3e" % (rel(h[w2], ref[w2]), rel(hp[w2], ref[w2]), rel(h, ref)))
    assert rel(h, hp) < 1e-6
    assert rel(h, ref) < TOL_FVP
    assert rel(h[w2], ref[w2]) <= 2.0 * rel(hp[w2], ref[w2])


@pytest.mark.parametrize("e", range(len(EDGES)), ids=["N%d" % N for N in EDGES])
def test_r9_edge_sizes(runs, e):
    """padded samples contribute nothing: the vector and the W2 block alone against fp64"""
    h, ref, w2 = runs[0]["%d_h0" % (K_EDGE + e)], oracle(SPECS[K_EDGE + e]), blocks(17, 6)["W2"]
    print("R9 N = %d: W2 block %.3e, whole %.3e" % (EDGES[e], rel(h[w2], ref[w2]), rel(h, ref)))
    assert np.all(np.isfinite(h))
    assert rel(h, ref) < TOL_FVP
    assert rel(h[w2], ref[w2]) < TOL_FVP


def test_r9_repeatable(runs):
    """launches of the same sweep direction are bitwise equal (the directions alternate), the other direction within 1e-6"""
    a = runs[0]
    h, r0, r1, r2 = (a["%d_%s" % (K_REP, key)] for key in ("h0", "rep0", "rep1", "rep2"))
    assert np.array_equal(h.view(np.uint32), r1.view(np.uint32)) and np.array_equal(r0.view(np.uint32), r2.view(np.uint32))
    assert rel(r0, h) < 1e-6
