#!/usr/bin/env python
"""MLP-baseline fit at minibatches of 128 .. 512 rows: the team trainer (csrc/mlp_fit_team.h, B / 64 workgroups a step) against the
launch route (MJX_FIT_TEAM=0: ~14 launches a step), one epoch of mjx_mlp_fit_adam between two HIP events, the two routes
alternating in one process, at
    d_in 15 (reacher 11 + 4) and 21 (HalfCheetah 17 + 4),  B = 128, 256, 512,  N = 12 500 (250 paths x 50) and 1 000 000
and, for scale, the batch-64 route of the same d_in and N.  Each (d_in, N) runs in a child process of its own under a time limit,
and the first failure ends the run.  Prints one JSON line: per shape the microseconds per Adam step of every pass, their median
and spread (max - min) per route, and `wins`: the team route beats the launch route by more than the larger spread.
    python tools/bench_mlp_fit_team.py [--passes 5] [--out FILE]"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D_INS, SIZES, BATCHES = (15, 21), (12500, 1000000), (128, 256, 512)


def arg(name, dflt):
    return type(dflt)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def child(d_in, N, passes):
    import numpy as np
    import torch
    from mjrl_amd import _lib
    from mjrl_amd._lib import check, ptr
    from tests._dyn_check import rand_theta
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rng = np.random.RandomState(11)
    hid = (ctypes.c_int * 2)(128, 128)
    th0 = torch.as_tensor(rand_theta(rng, [d_in, 128, 128, 1])).to(dev)
    x = torch.randn(N, d_in, device=dev)
    y = (1.0 + torch.randn(N, device=dev)).contiguous()
    perm = torch.as_tensor(rng.permutation(N).astype(np.int32)).to(dev)
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fit(batch, team):
        os.environ["MJX_FIT_TEAM"] = "1" if team else "0"
        route = (ctypes.c_int32 * 6)()
        check(lib.mjx_mlp_fit_route(d_in, hid, 2, batch, N, 1, route))
        p, m, v = th0.clone(), torch.zeros_like(th0), torch.zeros_like(th0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        check(lib.mjx_mlp_fit_adam(ptr(x), ptr(y), N, d_in, hid, 2, ptr(p), ptr(m), ptr(v), 0, ptr(perm), 1, batch, 1e-3, 1e-3, ptr(loss), st))
        e1.record()
        e1.synchronize()
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(p).all())
        return e0.elapsed_time(e1) * 1e3 / (N // batch - 1), int(route[0])

    out = {}
    for batch in (64,) + BATCHES:
        fit(batch, True); fit(batch, False)             # warm-up: code objects, LDS attribute, scratch, the exchange block
        team, launches = [], []
        for _ in range(passes):
            team.append(fit(batch, True))
            if batch != 64:
                launches.append(fit(batch, False))
        r = {"route": team[0][1], "team_us": [round(t, 3) for t, _ in team]}
        if launches:
            r.update(launch_route=launches[0][1], launch_us=[round(t, 3) for t, _ in launches])
        out["B%d" % batch] = r
    print("CHILD " + json.dumps(out), flush=True)


def main():
    passes = arg("--passes", 5)
    out = {"passes": passes}

    def leave(code):
        print(json.dumps(out))
        if "--out" in sys.argv:
            json.dump(out, open(arg("--out", ""), "w"), indent=1)
        sys.exit(code)
    for d_in in D_INS:
        for N in SIZES:
            name = "d%d_N%d" % (d_in, N)
            # ~0.3 ms a launch-route step is far above either route; the limit only ends a run that has stopped making progress
            limit = 60 + int((passes + 1) * 2 * 4 * (N / 128) * 3e-4)
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(d_in), "--N", str(N),
                                "--passes", str(passes)], capture_output=True, text=True, cwd=ROOT)
            line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
            if p.returncode != 0 or not line:
                out[name] = {"failed": p.returncode, "log": (p.stdout + p.stderr)[-1500:]}
                leave(1)                                 # nothing more is started on the GPU after a failure
            r = json.loads(line[-1][6:])
            for b in r.values():
                for key in ("team_us", "launch_us"):
                    if key in b:
                        ts = sorted(b[key])
                        b[key + "_median"], b[key + "_spread"] = ts[len(ts) // 2], round(ts[-1] - ts[0], 3)
                if "launch_us" in b:
                    b["wins"] = bool(b["launch_us_median"] - b["team_us_median"] > max(b["team_us_spread"], b["launch_us_spread"]))
            out[name] = r
    leave(0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", 0), arg("--N", 0), arg("--passes", 5))
    else:
        main()
