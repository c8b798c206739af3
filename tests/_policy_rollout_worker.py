"""GPU worker of tests/test_gpu_policy_rollout.py: every check of mjx_policy_rollout in one process; prints one RESULT line (JSON).
Every output block starts as NaN with 64 NaN guard elements behind it; after a call no NaN may stay inside and nothing behind it
may be touched (asserted here, per call)."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build()
from mjrl_amd import _lib  # noqa: E402
from mjrl_amd._lib import ptr  # noqa: E402
import _refine_oracle as F  # noqa: E402
from tests._worker_dev import checked_block, emit, ints, nan_block as guarded, same_bits as bits, switch, up  # noqa: E402

lib = _lib.load()


def unguard(buf, shape, what):
    return checked_block(buf, int(np.prod(shape)), what).reshape(shape).copy()


def blocks(c):
    return dict(P=up(np.stack(c["dyn_thetas"])), tr=up(np.stack(c["dyn_trs"])), pP=up(c["pol_theta"]), ptr=up(c["pol_tr"]),
                b=[None] * 4 if c["bounds"] is None else [up(v) for v in c["bounds"]])


def policy_rollout(c, mfma, s0=None, noise="case"):
    """one mjx_policy_rollout under MJX_POLICY_ROLLOUT_MFMA = mfma -> (obs, act, route)"""
    K, N, H, n, m = c["K"], c["N"], c["H"], c["n"], c["m"]
    d = blocks(c)
    s0 = c["s0"] if s0 is None else s0
    nz = c["noise"] if isinstance(noise, str) else noise
    s0_d, nz_d = up(s0), up(nz)
    ob, ab = guarded(K * N * H * n), guarded(K * N * H * m)
    route = ctypes.c_int(-9)
    with switch("MJX_POLICY_ROLLOUT_MFMA", "1" if mfma else "0"):
        rc = lib.mjx_policy_rollout(ptr(s0_d), n if s0.ndim == 2 else 0, N, H, K, ints(c["pol_sizes"]), len(c["pol_sizes"]), ptr(d["pP"]),
                                    ptr(d["ptr"]), ptr(nz_d), H * N * m if (nz is not None and nz.ndim == 4) else 0, ints(c["dyn_sizes"]),
                                    len(c["dyn_sizes"]), ptr(d["P"]), ptr(d["tr"]), c["act"], c["flags"], ptr(d["b"][0]), ptr(d["b"][1]),
                                    ptr(d["b"][2]), ptr(d["b"][3]), ptr(ob), ptr(ab), ctypes.byref(route), None)
    _lib.check(rc)
    return unguard(ob, (K, N, H, n), "obs"), unguard(ab, (K, N, H, m), "act"), route.value


def model_rollout(c):
    """mjx_model_rollout on the case's inputs, tiled and expanded on the host"""
    K, N, H, n, m = c["K"], c["N"], c["H"], c["n"], c["m"]
    d = blocks(c)
    s0_d, nz_d = up(F.case_s0_rows(c)), up(F.case_noise_members(c))
    ob, ab = guarded(K * N * H * n), guarded(K * N * H * m)
    rc = lib.mjx_model_rollout(ptr(s0_d), N, H, K, ints(c["pol_sizes"]), len(c["pol_sizes"]), ptr(d["pP"]), ptr(d["ptr"]), ptr(nz_d), None,
                               ints(c["dyn_sizes"]), len(c["dyn_sizes"]), ptr(d["P"]), ptr(d["tr"]), c["act"], c["flags"], ptr(d["b"][0]),
                               ptr(d["b"][1]), ptr(d["b"][2]), ptr(d["b"][3]), ptr(ob), ptr(ab), None)
    _lib.check(rc)
    return unguard(ob, (K, N, H, n), "obs"), unguard(ab, (K, N, H, m), "act")


def main():
    res = dict(step={"1": {}, "0": {}}, routes={}, route_out={}, route_fn={}, differ={}, free={}, bits={}, shared={})
    for name in sorted(F.KCASES):
        c = F.kernel_case(name)
        res["route_fn"][name] = lib.mjx_policy_rollout_route(ints(c["pol_sizes"]), len(c["pol_sizes"]), ints(c["dyn_sizes"]), len(c["dyn_sizes"]))
        o1, a1, r1 = policy_rollout(c, True)
        o0, a0, r0 = policy_rollout(c, False)
        res["route_out"][name] = [r1, r0]
        res["step"]["1"][name] = list(F.step_errors(c, o1, a1))
        res["step"]["0"][name] = list(F.step_errors(c, o0, a0))
        res["routes"][name] = [F.rel_max(a1, a0), F.rel_max(o1, o0)]
        res["differ"][name] = not (bits(o1, o0) and bits(a1, a0))
        if c["noise"] is not None and c["noise"].ndim == 3 and c["s0"].ndim == 1 and c["K"] > 1:
            res["shared"][name] = all(bits(a1[k, :, 0], a1[0, :, 0]) for k in range(c["K"]))
        if name == "p2":                                  # flags 3: a masked output column is exactly 0 in every stored next state
            res["masked_zero"] = bool(np.all(o1[:, :, 1:, F.P2_MASKED] == 0.0) and np.all(o0[:, :, 1:, F.P2_MASKED] == 0.0))
        print(name, res["step"]["1"][name], res["step"]["0"][name], res["routes"][name], flush=True)
    # free-running, one case, both routes
    c = F.kernel_case(F.FREE_CASE, F.FREE_H)
    o64, a64 = F.free_rollout(c)
    for mfma in (True, False):
        o, a, r = policy_rollout(c, mfma)
        assert r == (1 if mfma else 0)
        res["free"]["1" if mfma else "0"] = [F.rel_max(a, a64), F.rel_max(o, o64)]
    # route 0's bits: per-member noise and (N, n) states against mjx_model_rollout; one state and shared noise against the same
    # call on pre-tiled inputs, and against mjx_model_rollout
    c = F.kernel_case("p6")
    o0, a0, _ = policy_rollout(c, False)
    om, am = model_rollout(c)
    res["bits"]["member"] = bits(o0, om) and bits(a0, am)
    c = F.kernel_case("p1")
    o0, a0, _ = policy_rollout(c, False)
    ot, at, _ = policy_rollout(c, False, s0=F.case_s0_rows(c), noise=F.case_noise_members(c))
    om, am = model_rollout(c)
    res["bits"]["tiled"] = bits(o0, ot) and bits(a0, at)
    res["bits"]["tiled_model"] = bits(o0, om) and bits(a0, am)
    emit(res)


if __name__ == "__main__":
    main()
