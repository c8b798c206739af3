#!/usr/bin/env python
"""Ensemble fit timings: one mjx_dyn_fit_ensemble call (a workgroup per member, csrc/dyn_fit_ens.h) against K mjx_dyn_fit_adam
calls one after the other (the path before the ensemble entry existed), 1e4 Adam steps each time, alternating in one process,
at
    [13, 256, 256, 11]  batch 64  K = 4     (configs/reacher.txt)
    [8, 256, 256, 6]    batch 16  K = 3     (configs/point_mass.txt)
    [10, 64, 64, 8]     batch 64  K = 4     (the narrow route: k_dyn_fit)
and, for the reward nets, one mjx_reward_fit_ensemble call against K mjx_dyn_fit_adam calls in target mode 0, at
    [24, 100, 100, 1]   batch 64  K = 4     (RewardNet at reacher: n 11, m 2)
    [14, 100, 100, 1]   batch 16  K = 3     (RewardNet at point mass)
Host clock around calls that end in a stream synchronisation; both paths start every pass from the same parameters and zero
moments.  Each shape runs in a child process of its own under a time limit, and the first failure ends the run.  Prints one
JSON line: per shape and path the microseconds per Adam step of every pass (a step = all K members advanced by one), their
median and spread (max - min), and `wins`: the ensemble call beats the sequential path by more than the larger spread.
--dynamics-only: the three dynamics shapes alone; --lib PATH: another build of the library (a parent commit's, for an A/B on
one box: only the entries timed are bound, so a build without the reward entries serves with --dynamics-only).
    python tools/bench_dyn_fit.py [--passes 5] [--steps 10000] [--out FILE] [--dynamics-only] [--lib PATH]"""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, sizes, batch, K, target mode (0: the reward entry against mode-0 mjx_dyn_fit_adam calls)
SHAPES = [("w256_b64_K4", [13, 256, 256, 11], 64, 4, 2), ("w256_b16_K3", [8, 256, 256, 6], 16, 3, 2), ("w64_b64_K4", [10, 64, 64, 8], 64, 4, 2),
          ("rw100_b64_K4", [24, 100, 100, 1], 64, 4, 0), ("rw100_b16_K3", [14, 100, 100, 1], 16, 3, 0)]


def arg(name, dflt):
    return type(dflt)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else dflt


def child(name, passes, steps):
    import numpy as np
    import torch
    from mjrl_amd import _lib
    from mjrl_amd._lib import ptr
    from tests._dyn_check import rand_theta, rand_tr
    _, sizes, batch, K, tmode = [s for s in SHAPES if s[0] == name][0]
    dev = torch.device("cuda", 0)
    if "--lib" in sys.argv:                           # another build: bind the timed entries alone
        lib = ctypes.CDLL(arg("--lib", ""))
        for fn in ("mjx_dyn_fit_adam", "mjx_dyn_fit_ensemble") + (("mjx_reward_fit_ensemble",) if tmode == 0 else ()):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = _lib.PROTOTYPES[fn]
    else:
        lib = _lib.load()

    def check(rc):
        if rc != 0:
            raise RuntimeError("libmjx error %d" % rc)
    rng = np.random.RandomState(5)
    N, din, dout = 4000, sizes[0], sizes[-1]
    th0 = torch.as_tensor(rand_theta(rng, sizes, K)).to(dev)
    tr = np.stack([rand_tr(rng, din, dout) for _ in range(K)])
    in_tr, out_tr = torch.as_tensor(tr[:, :2 * din].copy()).to(dev), torch.as_tensor(tr[:, 2 * din:].copy()).to(dev)
    x = torch.as_tensor(rng.randn(N, din).astype(np.float32)).to(dev)
    y = (x[:, :dout] * 0.8 + 0.3 * torch.randn(N, dout, device=dev)).contiguous()
    per = (N // batch) * batch
    idx = np.stack([np.concatenate([rng.permutation(N)[:per] for _ in range(steps * batch // per + 1)])[:steps * batch] for _ in range(K)])
    idx_d = torch.as_tensor(idx.astype(np.int32)).to(dev)
    loss = torch.empty((K, steps), device=dev)
    csz = (ctypes.c_int * len(sizes))(*sizes)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    step0 = (ctypes.c_int64 * K)(*[0] * K)
    route = ctypes.c_int(-1)

    def fresh():
        return th0.clone(), torch.zeros_like(th0), torch.zeros_like(th0)

    def ensemble(n):
        P, m, v = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if tmode == 0:
            check(lib.mjx_reward_fit_ensemble(ptr(x), 0, ptr(y), 0, N, K, csz, len(sizes), ptr(in_tr), ptr(out_tr), 0, ptr(P), ptr(m), ptr(v), step0,
                                              ptr(idx_d), n, batch, 1e-3, 1e-5, ptr(loss), ctypes.byref(route), st))
        else:
            check(lib.mjx_dyn_fit_ensemble(ptr(x), 0, ptr(y), 0, N, K, csz, len(sizes), ptr(in_tr), ptr(out_tr), tmode, 0, ptr(P), ptr(m), ptr(v), step0,
                                           ptr(idx_d), n, batch, 1e-3, 1e-5, ptr(loss), ctypes.byref(route), st))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6, float(loss[:, n - 1].mean())

    def sequential(n):
        P, m, v = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            check(lib.mjx_dyn_fit_adam(ptr(x), ptr(y), N, csz, len(sizes), ptr(in_tr[k]), ptr(out_tr[k]), tmode, 0, ptr(P[k]), ptr(m[k]), ptr(v[k]), 0,
                                       ptr(idx_d[k]), n, batch, 1e-3, 1e-5, ptr(loss[k]), st))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6, float(loss[:, n - 1].mean())

    ensemble(50); sequential(50)                      # warm-up: code objects, LDS attribute, scratch
    ens, seq = [], []
    for _ in range(passes):
        ens.append(ensemble(steps))
        seq.append(sequential(steps))
    print("CHILD " + json.dumps({"route": route.value, "ens_us": [round(t, 3) for t, _ in ens], "seq_us": [round(t, 3) for t, _ in seq],
                                 "last_loss_ens": ens[-1][1], "last_loss_seq": seq[-1][1]}), flush=True)


def main():
    passes, steps = arg("--passes", 5), arg("--steps", 10000)
    out = {"steps": steps, "passes": passes}
    extra = (["--lib", arg("--lib", "")] if "--lib" in sys.argv else [])
    for name, sizes, batch, K, tmode in SHAPES:
        if tmode == 0 and "--dynamics-only" in sys.argv:
            continue
        # ~0.5 ms a step is far above either path; the limit only ends a run that has stopped making progress
        limit = 60 + int(passes * steps * 2 * 5e-4)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", name, "--passes", str(passes),
                            "--steps", str(steps)] + extra, capture_output=True, text=True, cwd=ROOT)
        line = [l for l in p.stdout.splitlines() if l.startswith("CHILD ")]
        if p.returncode != 0 or not line:
            out[name] = {"failed": p.returncode, "log": (p.stdout + p.stderr)[-1500:]}
            print(json.dumps(out))
            if "--out" in sys.argv:
                json.dump(out, open(arg("--out", ""), "w"), indent=1)
            sys.exit(1)                              # nothing more is started on the GPU after a failure
        r = json.loads(line[-1][6:])
        for key in ("ens_us", "seq_us"):
            ts = sorted(r[key])
            r[key + "_median"], r[key + "_spread"] = ts[len(ts) // 2], round(ts[-1] - ts[0], 3)
        r["wins"] = bool(r["seq_us_median"] - r["ens_us_median"] > max(r["ens_us_spread"], r["seq_us_spread"]))
        r.update(sizes=sizes, batch=batch, K=K, target_mode=tmode)
        out[name] = r
    print(json.dumps(out))
    if "--out" in sys.argv:
        json.dump(out, open(arg("--out", ""), "w"), indent=1)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(arg("--child", ""), arg("--passes", 5), arg("--steps", 10000))
    else:
        main()
