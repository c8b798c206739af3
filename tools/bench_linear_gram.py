#!/usr/bin/env python
"""One NPG update of a LinearPolicy: route 1 of mjx_npg_update_linear (the Gram route, csrc/linear_policy.h: one pass for the second
moments, the CG on the closed form, one closing pass) against route 0 (mjx_npg_update on the layer-wise path), one HIP-event pair
around each update, MJX_LINEAR_GRAM alternating 1, 0 in one process, at
    (6, 2) x 10 000 rows (configs[0])    (17, 6) x 1M rows    (63, 17) x 1M rows
The child process runs under a time limit.  Prints one JSON line: per shape the microseconds of every update after the warm-up,
their median and spread (max - min) per route, a second route-0 series (route 0 against itself: what two series of the same code
differ by) and `wins` (route 1 beats route 0 by more than the largest spread).
--mode trpo: one TRPO update (kl_dist 0.025) -- route 1 is ONE mjx_trpo_update_linear call (the line search inside the solve), route 0
what a caller runs when that entry reports route 0: mjx_trpo_update with its first batch of 3 trials.  --mode dapg: one DAPG update
with 5 000 demonstration rows behind the on-policy rows, mjx_dapg_update_linear on either side of the switch.
--wide (npg, trpo): the wide route for 64 to 127 observations (route 2 of mjx_npg_update_linear_wide / mjx_trpo_update_linear_wide,
csrc/linear_policy_wide.h) against route 0, MJX_LINEAR_GRAM_WIDE alternating 1, 0, at
    (111, 8) x 10 000 rows    (111, 8) x 1M rows    (127, 32) x 1M rows
    python tools/bench_linear_gram.py [--mode npg|trpo|dapg] [--wide] [--passes 9] [--out FILE]"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(6, 2, 10000), (17, 6, 1000000), (63, 17, 1000000)]      # (n, m, rows)
WIDE_SHAPES = [(111, 8, 10000), (111, 8, 1000000), (127, 32, 1000000)]
WARMUP = 3
DEMO_ROWS, KL_DIST = 5000, 0.025


def arg(name, dflt):
    return type(dflt)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def child(passes, mode, wide):
    import numpy as np
    import torch
    from mjrl_amd._lib import check, load, ptr
    dev = torch.device("cuda", 0)
    lib = load()
    out = {}
    env, on = ("MJX_LINEAR_GRAM_WIDE", 2) if wide else ("MJX_LINEAR_GRAM", 1)
    npg_entry = lib.mjx_npg_update_linear_wide if wide else lib.mjx_npg_update_linear
    trpo_entry = lib.mjx_trpo_update_linear_wide if wide else lib.mjx_trpo_update_linear
    for n, m, N in (WIDE_SHAPES if wide else SHAPES):
        rng = np.random.RandomState(3)
        d = m * n + 2 * m
        th = torch.as_tensor(np.concatenate([0.3 * rng.randn(m * n) / np.sqrt(n), 0.1 * rng.randn(m), np.full(m, -0.5)]).astype(np.float32)).to(dev)
        rows = N + (DEMO_ROWS if mode == "dapg" else 0)
        obs = torch.randn(rows, n, device=dev) * (1 + 2 * torch.rand(n, device=dev)) + torch.randn(n, device=dev)
        act, adv = 0.7 * torch.randn(rows, m, device=dev), torch.randn(rows, device=dev)
        if mode == "dapg":                             # dapg.py:62-70: 1e-2 [adv / std ; lam_0 lam_1^iter], the whitened advantages apart
            adv_on = adv[:N].clone()
            adv = 1e-2 * torch.cat([adv_on / (adv_on.std() + 1e-8), torch.ones(DEMO_ROWS, device=dev)])
        tho = th.clone()
        g, x, new = (torch.zeros(d, device=dev) for _ in range(3))
        res = torch.zeros(64, dtype=torch.float64, device=dev)
        ctx = ctypes.c_void_p()
        check(lib.mjx_create(ctypes.byref(ctx), 0, n, m, (ctypes.c_int * 1)(), 0))
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        out4 = (ptr(g), ptr(x), ptr(new), ptr(res), st)

        def update(switch):
            os.environ[env] = switch
            check(lib.mjx_bind_batch(ctx, ptr(obs), ptr(act), ptr(adv), rows, rows))       # (DAPG leaves the on-policy prefix bound)
            check(lib.mjx_bind_policy(ctx, ptr(th), ptr(tho), None, None, 1))
            route = ctypes.c_int32(-1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if mode == "trpo":
                check(trpo_entry(ctx, 10, 1e-4, 1e-10, 2 * KL_DIST, KL_DIST, 100, -3.0, *out4, ctypes.byref(route)))
                if route.value == 0:
                    check(lib.mjx_trpo_update(ctx, 10, 1e-4, 1e-10, 2 * KL_DIST, KL_DIST, 3, 1, -3.0, *out4))
            elif mode == "dapg":
                check(lib.mjx_dapg_update_linear(ctx, 10, 1e-4, 1e-10, 2 * KL_DIST, -3.0, N, N, ptr(adv_on), *out4, ctypes.byref(route)))
            else:
                check(npg_entry(ctx, 10, 1e-4, 1e-10, 0.05, float("nan"), -3.0, *out4, ctypes.byref(route)))
            e1.record()
            e1.synchronize()
            assert route.value == on * int(switch), route.value
            return round(e0.elapsed_time(e1) * 1e3, 1), new.clone()

        for _ in range(WARMUP):
            a, b = update("1")[1], update("0")[1]
        agree = float(((a - th) - (b - th)).norm() / (b - th).norm())
        # recorded, not bounded: ten iterations on a handful of parameters run past convergence, where route 0's fp32 residuals
        # are rounding noise that 1 / damping amplifies (tests/test_gpu_linear_gram.py prints both routes' distance to fp64)
        assert agree == agree, agree
        series = {"gram_us": [], "layerwise_us": [], "layerwise_again_us": []}
        for _ in range(passes):
            series["gram_us"].append(update("1")[0])
            series["layerwise_us"].append(update("0")[0])
            series["layerwise_again_us"].append(update("0")[0])
        series["step_agreement"] = agree
        out["n%d_m%d_N%d" % (n, m, N)] = series
        torch.cuda.synchronize()
        lib.mjx_destroy(ctx)
    print("CHILD " + json.dumps(out), flush=True)


def main():
    passes, mode, wide = arg("--passes", 9), arg("--mode", "npg"), "--wide" in sys.argv
    assert not (wide and mode == "dapg"), "the wide route serves NPG and TRPO"
    out = {"passes": passes, "warmup": WARMUP, "mode": mode, "wide": wide}
    p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "--passes", str(passes), "--mode", mode] + (["--wide"] if wide else []),
                       capture_output=True, text=True, cwd=ROOT)
    line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
    if p.returncode != 0 or not line:
        out["failed"], out["log"] = p.returncode, (p.stdout + p.stderr)[-1500:]
    else:
        for name, b in json.loads(line[-1][6:]).items():
            for key in ("gram_us", "layerwise_us", "layerwise_again_us"):
                ts = sorted(b[key])
                b[key + "_median"], b[key + "_spread"] = ts[len(ts) // 2], round(ts[-1] - ts[0], 1)
            spread = max(b[k + "_spread"] for k in ("gram_us", "layerwise_us", "layerwise_again_us"))
            b["wins"] = bool(b["layerwise_us_median"] - b["gram_us_median"] > max(spread, abs(b["layerwise_us_median"] - b["layerwise_again_us_median"])))
            out[name] = b
    print(json.dumps(out))
    if "--out" in sys.argv:
        json.dump(out, open(arg("--out", ""), "w"), indent=1)
    sys.exit(1 if "failed" in out else 0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--passes", 9), arg("--mode", "npg"), "--wide" in sys.argv)
    else:
        main()
