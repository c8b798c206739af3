"""Every output array of the fused policy kernels (k_fused) over the cases of tests/test_gpu_fused_matrix.py, for comparing two builds
bit by bit (a refactor's evidence; needs the GPU):
    MJX_LIB=<libmjx.so> python tools/bits_fused.py dump out.npz      one run per library
    python tools/bits_fused.py compare a.npz b.npz [out.json]         equality of the raw bytes of every array
The cases are the test's own, arm by arm, each arm in a fresh tests/_fused_matrix_worker.py process (the switches are read once per
process or context): the default (accumulator-order partials, bf16x3 cached product with R9), MJX_RAW_SLAB=0 (flat-order partials),
MJX_FVP_BF16X3=0 (fp32 cached product), MJX_NO_HCACHE=1 (recompute products, K3 without K1's caches) and, on the fp32 arm's cases,
MJX_FVP_BF16X3_R9=0 (bf16x3 product with R9 on fp32 MFMAs).  A case leaves K1's gradient (old == new and old != new), the
recompute and cached products (both sweep directions, a prefix, output-row probes) and K3's scalars in its four input situations."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ARM_TIMEOUT = 600       # seconds per worker process (the test's own limit)


def arms():
    from tests import test_gpu_fused_matrix as T
    out = {arm: (dict(env), list(cases), arm) for arm, (env, cases) in T.ARMS.items()}
    out["bf3_r9_0"] = ({"MJX_FVP_BF16X3_R9": "0"}, list(T.ARMS["bf3_0"][1]), "default")
    return T, out


def dump(path):
    T, table = arms()
    out = {}
    for arm, (env, cases, spec_arm) in table.items():
        with tempfile.TemporaryDirectory() as tmp:
            specs = [T.spec(nm, spec_arm) for nm in cases]
            with open(os.path.join(tmp, "spec.json"), "w") as f:
                json.dump({"cases": specs}, f)
            child_env = {k: v for k, v in os.environ.items() if k not in T.SCRUB and k != "MJX_FVP_BF16X3_R9"}
            child_env.update(env)
            rc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_fused_matrix_worker.py"), os.path.join(tmp, "spec.json"), tmp],
                                env=child_env, cwd=ROOT, timeout=ARM_TIMEOUT).returncode
            if rc != 0:             # nothing more runs on the device after a worker that ended badly
                print("arm %s: worker exit status %d" % (arm, rc))
                return 1
            for c in specs:
                for k, v in np.load(os.path.join(tmp, c["name"] + ".npz")).items():
                    out["%s/%s/%s" % (arm, c["name"], k)] = v
        print("arm %s: %d cases" % (arm, len(cases)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("dumped", len(out), "arrays from", os.environ.get("MJX_LIB") or "the tree's libmjx.so")
    return 0


def compare(pa, pb, out_json=None):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    differ = [k for k in a.files if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes())]
    per_arm = {}
    for k in a.files:
        arm = k.split("/")[0]
        per_arm.setdefault(arm, dict(cases=set(), arrays=0))
        per_arm[arm]["cases"].add(k.split("/")[1]); per_arm[arm]["arrays"] += 1
    res = dict(arrays=len(a.files), elements=int(sum(a[k].size for k in a.files)),
               nan=int(sum(int(np.isnan(a[k]).sum()) for k in a.files if a[k].dtype.kind == "f")),
               arms={arm: dict(cases=len(v["cases"]), arrays=v["arrays"]) for arm, v in sorted(per_arm.items())},
               differ=differ, identical=not differ)
    print(json.dumps(res, indent=1))
    if out_json:
        json.dump(res, open(out_json, "w"), indent=1)
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(*sys.argv[2:]))
