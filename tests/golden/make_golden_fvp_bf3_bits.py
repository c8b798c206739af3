"""Records tests/golden/fvp_bf3_bits.npz: the bits of the bf16x3 cached Fisher-vector product as the library named by MJX_LIB
(default: the tree's build) computes them on this GPU -- the fixture of tests/test_gpu_fvp_bf3_bits.py.  Record it from the
build whose bits are to be kept BEFORE changing the kernel's schedule:

    MJX_LIB=<the parent build's libmjx.so> python tests/golden/make_golden_fvp_bf3_bits.py [out.npz]

One child process per MJX_FVP_BF16X3_R9 setting (tests/_fvp_bf3_bits_worker.py; the switch is read once per process).  Stored,
as uint32 words: r9_1's first product of every case as it is, its second product XOR the first, and r9_0's two products XOR
r9_1's (the settings differ in the W2 gradient only, the sweep directions in the last bits: mostly zeros, which compress); `cu`
is the CU count of the device the record was made on."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))

from tests._fvp_bf3_bits_worker import CASES, case_name, encode  # noqa: E402


def run_worker(r9, path):
    env = dict(os.environ, MJX_FVP_BF16X3_R9=str(r9))
    subprocess.run([sys.executable, os.path.join(TESTS, "_fvp_bf3_bits_worker.py"), path], check=True, env=env, timeout=600)
    r = dict(np.load(path))
    assert int(r["r9"]) == r9
    return r


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fvp_bf3_bits.npz")
    with tempfile.TemporaryDirectory() as tmp:
        r1 = run_worker(1, os.path.join(tmp, "r9_1.npz"))
        r0 = run_worker(0, os.path.join(tmp, "r9_0.npz"))
    assert int(r1["cu"]) == int(r0["cu"])
    for r in (r1, r0):
        for n, N in CASES:
            for p in ("_p0", "_p1"):
                assert np.isfinite(r[case_name(n, N) + p].view(np.float32)).all(), (case_name(n, N), p)
    np.savez_compressed(dst, **encode(r1, r0))
    size = os.path.getsize(dst)
    print("%s: %d cases x 2 products x 2 settings, %d CUs, %d bytes" % (dst, len(CASES), int(r1["cu"]), size))
    assert size < (1 << 20), "over the size limit for a committed file"


if __name__ == "__main__":
    main()
