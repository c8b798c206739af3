"""The update path of one libmjx build, for a comparison with another build (profiles/r21_update_owner/): one NPG, one TRPO and one
DAPG update through the one-call entries, on a fused shape (17-64-64-6) and under MJX_FORCE_LAYERWISE=1, each without a
transport and with the peer exchange in loop-back at world 2 -- twelve cases in one process.

    MJX_LIB=<libmjx.so> python tools/update_path_parity.py dump <out.npz>      theta, x, gradient and the result doubles per case
    MJX_LIB=<libmjx.so> rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python tools/update_path_parity.py dump <out.npz>
    python tools/update_path_parity.py launches <dir>/.../t_kernel_trace.csv <out.json>    (kernel, grid, workgroup) in dispatch order + SHA-256
    python tools/update_path_parity.py compare a.npz b.npz a.json b.json       array_equal per array, equal hashes
"""
import csv
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, HID, ROWS, ROWS_ON, ITERS = 17, 6, (64, 64), 3000, 2400, 10


def one_case(algo, layerwise, peer):
    """a fresh child process per path would hide nothing here: MJX_FORCE_LAYERWISE is read per context"""
    from mjrl_amd import _lib
    from mjrl_amd.engine import UpdateEngine
    import _synth as synth              # (tools/ keeps its own initialiser: nothing here imports oracle/)
    os.environ["MJX_FORCE_LAYERWISE"] = "1" if layerwise else "0"
    rng = np.random.RandomState(11)
    theta = synth.perturbed_params(synth.init_params(N, M, HID), scale=0.05)
    tr = np.concatenate([np.zeros(N), np.ones(N), np.zeros(M), np.ones(M)]).astype(np.float32)
    obs, act, adv = rng.randn(ROWS, N), rng.randn(ROWS, M), rng.randn(ROWS)
    eng = UpdateEngine(N, M, HID)
    assert eng.backend.fused == (not layerwise)
    if peer:
        h = ctypes.create_string_buffer(64)
        _lib.check(eng.lib.mjx_peer_export(eng.ctx, 0, 2, h))
        _lib.check(eng.lib.mjx_peer_connect(eng.ctx, None))
    eng.set_policy(theta, theta, tr, tr)
    eng.set_batch(obs, act, adv)
    if algo == "npg":
        eng.npg_update(ITERS, 1e-4, 0.05, -3.0)
    elif algo == "trpo":
        eng.trpo_update(ITERS, 1e-4, 0.02, 0.002, -3.0)
    else:
        eng.dapg_update(ITERS, 1e-4, 0.05, -3.0, ROWS_ON, adv[:ROWS_ON].copy())
    out = dict(theta=eng.theta_new.cpu().numpy(), x=eng.x.cpu().numpy(), grad=eng.grad.cpu().numpy(), results=eng.results.cpu().numpy())
    eng.close()
    return out


def dump(path):
    arrays = {}
    for layerwise in (False, True):
        for peer in (False, True):
            for algo in ("npg", "trpo", "dapg"):
                name = "%s_%s_%s" % (algo, "layerwise" if layerwise else "fused", "peer2" if peer else "alone")
                for k, v in one_case(algo, layerwise, peer).items():
                    arrays[name + "." + k] = v
    np.savez(path, **arrays)
    print(json.dumps({"cases": len(arrays) // 4, "arrays": len(arrays), "file": path}))


def launches(trace_csv, out_json):
    rows = list(csv.DictReader(open(trace_csv)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"] if "Dispatch_Id" in r else r["Start_Timestamp"]))
    names = subprocess.run(["c++filt"], input="\n".join(r["Kernel_Name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    seq = [[n, [int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])],
            [int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"])]] for n, r in zip(names, rows)]
    mine = [s for s in seq if "mjx::" in s[0]]
    digest = lambda s: hashlib.sha256(json.dumps(s).encode()).hexdigest()
    kinds = {}
    for s in mine:
        kinds[json.dumps(s)] = kinds.get(json.dumps(s), 0) + 1
    out = {"launches": len(seq), "sha256": digest(seq), "libmjx_launches": len(mine), "libmjx_sha256": digest(mine), "libmjx_distinct": len(kinds),
           "libmjx_by_shape": sorted(([json.loads(k), v] for k, v in kinds.items()), key=lambda e: e[0][0])}
    json.dump(out, open(out_json, "w"), indent=1)
    print(json.dumps({k: out[k] for k in ("launches", "sha256", "libmjx_launches", "libmjx_sha256", "libmjx_distinct")}))


def compare(npz_a, npz_b, json_a, json_b):
    a, b = np.load(npz_a), np.load(npz_b)
    differ = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
    ta, tb = json.load(open(json_a)), json.load(open(json_b))
    out = {"arrays": len(a.files), "arrays_differ": differ + [k for k in b.files if k not in a.files],
           "finite": bool(all(np.all(np.isfinite(a[k])) for k in a.files if not k.endswith(".results"))),
           "launches": [ta["launches"], tb["launches"]], "libmjx_launches": [ta["libmjx_launches"], tb["libmjx_launches"]],
           "same_sequence": ta["sha256"] == tb["sha256"], "same_libmjx_sequence": ta["libmjx_sha256"] == tb["libmjx_sha256"]}
    print(json.dumps(out))
    return 0 if not out["arrays_differ"] and out["same_libmjx_sequence"] else 1


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "dump":
        dump(sys.argv[2])
    elif mode == "launches":
        launches(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(*sys.argv[2:6]))
