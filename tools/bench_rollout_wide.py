#!/usr/bin/env python
"""mjx_policy_rollout_wide alone between HIP events (median and best of 20 calls, ms): the production shape (K 4, N 250, H 50,
256 x 256 dynamics, 64 x 64 policy) at two horizons, narrower nets that separate the K loops from the fixed cost of a step's
phases, one workgroup, n % 4 == 0 (four-weight loads in layer 1), and the same entry under MJX_POLICY_ROLLOUT_WIDE=0 (route 0
at 256 x 256, the register-resident route 1 at 128 x 128).  Prints one JSON object: tag -> [route, median, best]
(profiles/r18_rollout_wide/bench_rollout_wide.json).    python tools/bench_rollout_wide.py"""
import ctypes, os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from mjrl_amd import _lib
lib = _lib.load()
dev = torch.device("cuda", 0)
ints = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
def run(n, m, dh, ph, K, N, H, wide, reps=20):
    ds, ps = (n + m,) + dh + (n,), (n,) + ph + (m,)
    Pd = sum(ds[i] * ds[i + 1] + ds[i + 1] for i in range(3)); Pp = sum(ps[i] * ps[i + 1] + ps[i + 1] for i in range(3)) + m
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.05).to(dev)
    P, pP = r(K, Pd), r(Pp)
    tr = torch.cat([torch.zeros(K, n + m), torch.ones(K, n + m), torch.zeros(K, n), torch.ones(K, n)], 1).to(dev)
    ptr_ = torch.cat([torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m)]).to(dev)
    s0, nz = r(N, n), r(K, H, N, m)
    obs, act = torch.empty(K * N * H * n, device=dev), torch.empty(K * N * H * m, device=dev)
    route = ctypes.c_int(-1)
    os.environ["MJX_POLICY_ROLLOUT_WIDE"] = wide
    def call():
        _lib.check(lib.mjx_policy_rollout_wide(ptr(s0), n, N, H, K, ints(ps), 4, ptr(pP), ptr(ptr_), ptr(nz), H * N * m, ints(ds), 4, ptr(P), ptr(tr), 0, 7,
                                               None, None, None, None, ptr(obs), ptr(act), ctypes.byref(route), None))
    call(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    os.environ.pop("MJX_POLICY_ROLLOUT_WIDE")
    return route.value, round(float(np.median(ts)), 4), round(float(min(ts)), 4)
out = {}
for tag, a in {"prod_H50": (11, 2, (256, 256), (64, 64), 4, 250, 50), "prod_H10": (11, 2, (256, 256), (64, 64), 4, 250, 10),
               "dyn32_H50": (11, 2, (32, 32), (64, 64), 4, 250, 50), "dyn32_pol1_H50": (11, 2, (32, 32), (1, 1), 4, 250, 50),
               "dyn256x32_H50": (11, 2, (256, 32), (64, 64), 4, 250, 50), "dyn128_H50": (11, 2, (128, 128), (64, 64), 4, 250, 50),
               "prod_N32_K1_H50": (11, 2, (256, 256), (64, 64), 1, 32, 50), "n12_H50": (12, 4, (256, 256), (64, 64), 4, 250, 50)}.items():
    out[tag + "_wide"] = run(*a, "1")
out["prod_H50_route0"] = run(11, 2, (256, 256), (64, 64), 4, 250, 50, "0")
out["dyn128_H50_narrow"] = run(11, 2, (128, 128), (64, 64), 4, 250, 50, "0")
print(json.dumps(out, indent=1))
