"""Worker of tests/test_gpu_fused_matrix.py: runs a list of cases through the fused kernels (k_fused, csrc/fused_policy.h) with
whatever MJX_* switches the parent set in the environment (MJX_FVP_BF16X3 is read once per process, the others when a context
is created) and writes one .npz of device results per case.

    python _fused_matrix_worker.py <spec.json> <out_dir>

spec.json: {"cases": [{name, n, m, hid, N, seed, variant, npc, raw, prefix, probes}, ...]}.  N = 0 stands for
N_big = 2 x grid x 128 + 33 with the grid mjx_fused_info reports; every result carries the N it ran at.  The inputs are rebuilt
from the case's seed by fused_inputs(), which the parent calls too (for the fp64 oracle)."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import npg_oracle as O  # noqa: E402
from tests._dispatch_matrix_worker import _pack, head_inputs, probe_actions, probe_direction  # noqa: E402

PREFIX_CUT = 40         # bind_rows(N - 40): the prefix ends inside a 32-row tile of K1's caches (16 rows into it at N_big)


def n_big(grid):
    """more rows than two workgroups per CU x 4 waves x 32 rows hold: K3 with up to 8 actions (2 x grid workgroups) gives one
    wave a partial second tile, every other launch (grid workgroups) a second or third tile per wave"""
    return 2 * grid * 128 + 33


def fused_inputs(n, m, hid, N, seed):
    """head_inputs() (per-action log_std / out_scale / out_shift permuted, non-identity input transforms, on-policy actions)
    plus what K3's four input situations need: a second old network and a second input transform of the new policy"""
    inp = head_inputs(n, m, hid, N, seed)
    tr = inp["tr"]
    # (theta_old moved in place: half of th2's distance, on the other side of th)
    inp["th3"] = (inp["th"].astype(np.float64) - 0.5 * (inp["th2"].astype(np.float64) - inp["th"])).astype(np.float32)
    inp["tr2"] = O.Transforms(n, m, tr.in_shift + 0.05, tr.in_scale * 1.1, tr.out_shift, tr.out_scale)
    inp["pk2"] = _pack(inp["tr2"])
    return inp


def fused_info(eng):
    out = (ctypes.c_int32 * 4)()
    rc = eng.lib.mjx_fused_info(eng.ctx, out)
    assert rc == 0, rc
    return [int(x) for x in out]


def fused_route(eng, n, m, hid):
    out = (ctypes.c_int32 * 4)()
    rc = eng.lib.mjx_fused_route(n, m, (ctypes.c_int * len(hid))(*hid), len(hid), out)
    assert rc == 0, rc
    return [int(x) for x in out]


def run_case(c):
    import torch
    from mjrl_amd.engine import UpdateEngine
    n, m, hid = c["n"], c["m"], tuple(c["hid"])
    eng = UpdateEngine(n, m, hid)
    variant, npc, raw_dr, grid = fused_info(eng)
    assert eng.fused, (c["name"], "layer-wise")
    assert (variant, npc) == (c["variant"], c["npc"]), (c["name"], variant, npc)
    assert (raw_dr > 0) == bool(c["raw"]), (c["name"], raw_dr)
    # the context's instance is the one the table's route names for the shape (MJX_RAW_SLAB=0 is mjx_create's decision alone)
    route = fused_route(eng, n, m, hid)
    assert [variant, npc] == route[:2], (c["name"], variant, npc, route)
    assert raw_dr == (0 if os.environ.get("MJX_RAW_SLAB") == "0" else route[2]), (c["name"], raw_dr, route)
    N = c["N"] if c["N"] > 0 else n_big(grid)
    inp = fused_inputs(n, m, hid, N, c["seed"])
    th, th2, pk = inp["th"], inp["th2"], inp["pk"]
    dev = lambda a: torch.from_numpy(a).to(eng.device)
    host = lambda t: t.cpu().numpy().copy()
    v = dev(inp["v"])
    out = dict(N=N, grid=grid, variant=variant, npc=npc, raw_dr=raw_dr)

    # the recompute product (CACHED = false): nothing cached before the first K1
    eng.set_batch(inp["obs"], inp["act"], inp["adv"])
    eng.set_policy(th, th, pk, pk)
    out["hv_rc"] = host(eng.fvp(v))
    # K1 at old == new: fills the activation cache, the old-policy outputs and the parameter snapshot
    g, out["surr"] = eng.surr_vpg()
    out["g"] = host(g)
    # two cached products of the same direction: the first walks the tiles back to front, the second front to back
    out["hv"] = host(eng.fvp(v))
    out["hv_fwd"] = host(eng.fvp(v))
    if c["prefix"]:
        # a prefix that ends inside a cached tile; the third product since K1 walks in reverse again
        eng.bind_rows(N - PREFIX_CUT, N_global=N - PREFIX_CUT)
        out["hv_pre"] = host(eng.fvp(v))
        eng.bind_rows(N, N_global=N)
    for a in probe_actions(m)[:c["probes"]]:
        out["hv_a%d" % a] = host(eng.fvp(dev(probe_direction(inp["v"], n, m, hid, a))))

    # K3 (1): K1's old-policy outputs and its observation image
    eng.set_policy(th2, th, pk, pk)
    out["s1"], out["kl1"] = eng.eval_surr_kl()
    if c["prefix"]:
        eng.bind_rows(N - PREFIX_CUT, N_global=N - PREFIX_CUT)
        out["s_pre"], out["kl_pre"] = eng.eval_surr_kl()
        eng.bind_rows(N, N_global=N)
    # K3 (2): theta_old changed in place (no binding call): the kernel's snapshot compare has to notice
    eng.theta_old.copy_(dev(inp["th3"]))
    out["s2"], out["kl2"] = eng.eval_surr_kl()
    eng.theta_old.copy_(dev(th))
    # K3 (3): the new policy's input transform changed in place: the observation image belongs to another transform
    eng.tr_new.copy_(dev(inp["pk2"]))
    out["s3"], out["kl3"] = eng.eval_surr_kl()
    eng.tr_new.copy_(dev(pk))
    # K3 (4): a fresh batch binding: nothing stored applies
    eng.set_batch(inp["obs"], inp["act"], inp["adv"])
    out["s4"], out["kl4"] = eng.eval_surr_kl()
    # K1 with an explicit old network
    out["g2"] = host(eng.surr_vpg()[0])
    eng.close()
    return out


def main():
    spec_path, out_dir = sys.argv[1], sys.argv[2]
    with open(spec_path) as f:
        spec = json.load(f)
    for c in spec["cases"]:
        np.savez(os.path.join(out_dir, c["name"] + ".npz"), **run_case(c))


if __name__ == "__main__":
    main()
