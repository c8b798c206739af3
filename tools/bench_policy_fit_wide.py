#!/usr/bin/env python
"""BC / PPO minibatch fit of the manipulation-sized policies: route 2 of mjx_policy_minibatch_adam_wide (k_policy_fit_wide,
csrc/policy_fit_wide.h: every step in one launch) against route 0, the existing entry mjx_policy_minibatch_adam (per-step launches
for these shapes), `--steps` Adam steps between two HIP events, the two routes alternating in one process, at
    (39, 28, 32 x 32) B 32 and 64, (46, 26, 32 x 32) B 64, (45, 24, 64 x 64) B 32 and 64    behaviour cloning, MSE
    (39, 28, 32 x 32) B 64, (45, 24, 64 x 64) B 32                                            PPO with a fixed old policy
The child process runs under a time limit.  Prints one JSON line: per shape the microseconds per Adam step of every pass, their
median and spread (max - min) per route, `wins` (route 2 beats route 0 by more than the larger spread) and `agree_over_lr`, the
largest parameter difference between the two routes after 10 steps in units of lr.
    python tools/bench_policy_fit_wide.py [--passes 5] [--steps 4000] [--out FILE]"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (n, m, H, B, loss, old_tracks_new)
SHAPES = [(39, 28, 32, 32, 0, 0), (39, 28, 32, 64, 0, 0), (46, 26, 32, 64, 0, 0), (45, 24, 64, 32, 0, 0), (45, 24, 64, 64, 0, 0),
          (39, 28, 32, 64, 2, 0), (45, 24, 64, 32, 2, 0)]
N_ROWS, LR, CLIP = 20000, 1e-3, 0.2


def arg(name, dflt):
    return type(dflt)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def child(passes, steps):
    import numpy as np
    import torch
    from mjrl_amd._lib import check, load, ptr
    from mjrl_amd.engine import UpdateEngine
    from tests._dyn_check import rand_theta
    dev = torch.device("cuda", 0)
    lib = load()
    out = {}
    for n, m, H, B, loss, track in SHAPES:
        rng = np.random.RandomState(17)
        th = np.concatenate([rand_theta(rng, [n, H, H, m]), np.full(m, -0.5)]).astype(np.float32)
        th0 = torch.as_tensor(th).to(dev)
        tho = torch.as_tensor(th + 0.01 * rng.randn(th.size).astype(np.float32)).to(dev)
        obs, act, adv = torch.randn(N_ROWS, n, device=dev), 0.5 * torch.randn(N_ROWS, m, device=dev), torch.randn(N_ROWS, device=dev)
        idx = torch.as_tensor(rng.randint(0, N_ROWS, size=steps * B).astype(np.int32)).to(dev)
        eng = UpdateEngine(n, m, (H, H))
        route3 = (ctypes.c_int32 * 3)()
        check(lib.mjx_policy_fit_wide_route(n, m, (ctypes.c_int * 2)(H, H), 2, B, loss, track, route3))

        def fit(wide, k):
            p, am, av = th0.clone(), torch.zeros_like(th0), torch.zeros_like(th0)
            args = (eng.ctx, loss, ptr(obs), ptr(act), ptr(adv), ptr(idx), k, B, ptr(p), None, ptr(tho), None, track, ptr(am), ptr(av), 0, LR,
                    CLIP, None, eng.stream())
            ran = ctypes.c_int(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            check(lib.mjx_policy_minibatch_adam_wide(*args, ctypes.byref(ran)) if wide else lib.mjx_policy_minibatch_adam(*args))
            e1.record()
            e1.synchronize()
            assert ran.value == (2 if wide else 0), ran.value
            return e0.elapsed_time(e1) * 1e3 / k, p

        agree = float((fit(True, 10)[1] - fit(False, 10)[1]).abs().max()) / LR       # (also the warm-up of both routes)
        assert agree < 0.1, agree                                                     # (NaN fails too)
        wide, launches = [], []
        for _ in range(passes):
            wide.append(round(fit(True, steps)[0], 3))
            launches.append(round(fit(False, steps)[0], 3))
        out["n%d_m%d_H%d_B%d_loss%d" % (n, m, H, B, loss)] = {"route": list(route3), "wide_us": wide, "launch_us": launches, "agree_over_lr": agree}
        eng.close()
    print("CHILD " + json.dumps(out), flush=True)


def main():
    passes, steps = arg("--passes", 5), arg("--steps", 4000)
    out = {"passes": passes, "steps": steps}
    # ~0.2 ms a launch-route step is far above either route; the limit only ends a run that has stopped making progress
    limit = 120 + int(len(SHAPES) * (passes + 1) * 2 * steps * 2e-4)
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", "--passes", str(passes), "--steps",
                        str(steps)], capture_output=True, text=True, cwd=ROOT)
    line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
    if p.returncode != 0 or not line:
        out["failed"], out["log"] = p.returncode, (p.stdout + p.stderr)[-1500:]
    else:
        for name, b in json.loads(line[-1][6:]).items():
            for key in ("wide_us", "launch_us"):
                ts = sorted(b[key])
                b[key + "_median"], b[key + "_spread"] = ts[len(ts) // 2], round(ts[-1] - ts[0], 3)
            b["wins"] = bool(b["launch_us_median"] - b["wide_us_median"] > max(b["wide_us_spread"], b["launch_us_spread"]))
            out[name] = b
    print(json.dumps(out))
    if "--out" in sys.argv:
        json.dump(out, open(arg("--out", ""), "w"), indent=1)
    sys.exit(1 if "failed" in out else 0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--passes", 5), arg("--steps", 4000))
    else:
        main()
