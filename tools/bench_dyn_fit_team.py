#!/usr/bin/env python
"""Ensemble dynamics fit: route 2 (mjx_dyn_fit_ensemble_team, a team of G workgroups per member, csrc/dyn_fit_ens_team.h) against
route 1 (mjx_dyn_fit_ensemble, one workgroup per member, csrc/dyn_fit_ens.h) on the same members, rows and index draws: `--steps`
Adam steps of K = 4 members in one call between two HIP events, the two routes alternating in one process, at
    [13, 256, 256, 11] batch 16 and 64,  [13, 128, 128, 11] batch 64,  [13, 64, 64, 11] batch 64
Prints one JSON line: per shape the microseconds per Adam step of every pass, their median and spread (max - min) per route, and
`wins`: route 2 beats route 1 by more than the larger spread.  The first failure ends the run.
    python tools/bench_dyn_fit_team.py [--passes 5] [--steps 2000] [--out FILE]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (([13, 256, 256, 11], 16), ([13, 256, 256, 11], 64), ([13, 128, 128, 11], 64), ([13, 64, 64, 11], 64))
K, N = 4, 4000


def arg(name, dflt):
    return type(dflt)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def main():
    import numpy as np
    import torch
    from mjrl_amd import _lib
    from mjrl_amd._lib import check, ptr
    from tests._dyn_check import rand_theta, rand_tr
    passes, steps = arg("--passes", 5), arg("--steps", 2000)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"passes": passes, "steps": steps, "K": K, "device": torch.cuda.get_device_name(0)}
    for sizes, batch in SHAPES:
        rng = np.random.RandomState(5)
        din, dout = sizes[0], sizes[-1]
        csz = (ctypes.c_int * 4)(*sizes)
        th0 = torch.as_tensor(rand_theta(rng, sizes, K)).to(dev)
        tr = np.stack([rand_tr(rng, din, dout) for _ in range(K)])
        in_tr, out_tr = (torch.as_tensor(np.ascontiguousarray(t)).to(dev) for t in (tr[:, :2 * din], tr[:, 2 * din:]))
        x = torch.randn(N, din, device=dev)
        y = (0.8 * x[:, :dout] + 0.3 * torch.randn(N, dout, device=dev)).contiguous()
        idx = torch.as_tensor(rng.randint(0, N, (K, steps * batch)).astype(np.int32)).to(dev)
        loss = torch.zeros(K, steps, device=dev)
        step0 = (ctypes.c_int64 * K)()

        def fit(entry):
            p, m, v = th0.clone(), torch.zeros_like(th0), torch.zeros_like(th0)
            route = ctypes.c_int(-1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            check(getattr(lib, entry)(ptr(x), 0, ptr(y), 0, N, K, csz, 4, ptr(in_tr), ptr(out_tr), 2, 0, ptr(p), ptr(m), ptr(v), step0, ptr(idx),
                                      steps, batch, 1e-3, 1e-3, ptr(loss), ctypes.byref(route), st))
            e1.record()
            e1.synchronize()
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(p).all()), (entry, sizes, batch)
            return e0.elapsed_time(e1) * 1e3 / steps, route.value

        entries = {"route1": "mjx_dyn_fit_ensemble", "route2": "mjx_dyn_fit_ensemble_team"}
        r = {"G": lib.mjx_dyn_fit_team_route(csz, 4, batch, 2, K)}
        for key, entry in entries.items():              # warm-up: code objects, LDS attribute, scratch, the exchange block
            r[key + "_route"] = fit(entry)[1]
        assert r["route1_route"] == 1 and r["route2_route"] == 2, r
        us = {key: [] for key in entries}
        for _ in range(passes):
            for key, entry in entries.items():
                us[key].append(round(fit(entry)[0], 3))
        for key, ts in us.items():
            r[key + "_us"], r[key + "_us_median"], r[key + "_us_spread"] = ts, sorted(ts)[len(ts) // 2], round(max(ts) - min(ts), 3)
        r["wins"] = bool(r["route1_us_median"] - r["route2_us_median"] > max(r["route1_us_spread"], r["route2_us_spread"]))
        out["w%d_%d_b%d" % (sizes[1], sizes[2], batch)] = r
    print(json.dumps(out))
    if "--out" in sys.argv:
        json.dump(out, open(arg("--out", ""), "w"), indent=1)


if __name__ == "__main__":
    main()
