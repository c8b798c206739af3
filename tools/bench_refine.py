#!/usr/bin/env python
"""The policy rollout's two routes and ModelAccelNPG.get_refined_action on the MI355X -> one JSON line.

Per shape -- (n, m) in (11, 2), (17, 6); dynamics 64 x 64 and 128 x 128; policy 32 x 32 and 64 x 64; K 4; N 100 and 1 024;
H 10 and 32 -- HIP events around mjx_policy_rollout alone (shared noise, one start state, bounds +-1e2: the refined call's
arguments) with MJX_POLICY_ROLLOUT_MFMA at 0 and at 1 in alternating pairs in one process: median, best and quartiles per
route, and the route the dispatch takes.  The switch-0 side is k_model_rollout, the kernel every rollout ran before the route
existed.  Then get_refined_action on the host clock (members that learn rewards, so nothing but the action is read back) over
CALLS calls per route in four alternating blocks.
    python tools/bench_refine.py [--calls 200] [--pairs 50] [--quick]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build()
from mjrl_amd._lib import check, load, ptr  # noqa: E402
from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG  # noqa: E402
from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel  # noqa: E402
from mjrl_amd.baselines.linear_baseline import LinearBaseline  # noqa: E402
from mjrl_amd.policies.gaussian_mlp import MLP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--pairs", type=int, default=50)
ap.add_argument("--quick", action="store_true", help="the corner shapes only")
args = ap.parse_args()
SWITCH = "MJX_POLICY_ROLLOUT_MFMA"


def rollout_ms(n, m, dh, ph, K, N, H, pairs):
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = load()
    ds, ps = (n + m,) + tuple(dh) + (n,), (n,) + tuple(ph) + (m,)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    count = lambda sz: sum(sz[i] * sz[i + 1] + sz[i + 1] for i in range(len(sz) - 1))
    g = torch.Generator(device="cpu").manual_seed(5)
    dP = (torch.randn((K, count(ds)), generator=g) * 0.1).to(dev)
    pP = torch.cat([torch.randn(count(ps), generator=g) * 0.1, torch.full((m,), -0.5)]).to(dev)
    dtr = torch.cat([torch.zeros(n + m), torch.ones(n + m), torch.zeros(n), torch.full((n,), 0.3)]).repeat(K, 1).to(dev)
    ptr_ = torch.cat([torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m)]).to(dev)
    s0, nz = (torch.randn(n, generator=g) * 0.5).to(dev), torch.randn((H, N, m), generator=g).to(dev)
    b = [torch.full((d,), v, device=dev) for d, v in ((m, -1e2), (m, 1e2), (n, -1e2), (n, 1e2))]
    obs, act = torch.empty((K, N, H, n), device=dev), torch.empty((K, N, H, m), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    route = ctypes.c_int(-1)

    def launch(mfma):
        os.environ[SWITCH] = mfma
        check(lib.mjx_policy_rollout(ptr(s0), 0, N, H, K, ints(ps), len(ps), ptr(pP), ptr(ptr_), ptr(nz), 0, ints(ds), len(ds), ptr(dP),
                                     ptr(dtr), 0, 7, ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(obs), ptr(act), ctypes.byref(route), st))

    for mfma in ("0", "1", "0", "1"):
        launch(mfma)
    served = route.value
    torch.cuda.synchronize()
    ev = {"0": [], "1": []}
    for _ in range(pairs):
        for mfma in ("0", "1"):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); launch(mfma); e.record()
            ev[mfma].append((a, e))
    torch.cuda.synchronize()
    os.environ.pop(SWITCH, None)
    res = {}
    for mfma in ("0", "1"):
        ts = sorted(a.elapsed_time(e) for a, e in ev[mfma])
        res[mfma] = [round(v, 4) for v in (ts[len(ts) // 2], ts[0], ts[len(ts) // 4], ts[3 * len(ts) // 4])]
    return res, served


def refined_ms(n, m, dh, ph, K, N, H, calls):
    spec = types.SimpleNamespace(observation_dim=n, action_dim=m, horizon=H)
    pol = MLP(spec, hidden_sizes=tuple(ph), seed=3, init_log_std=-0.5)
    models = []
    for k in range(K):
        wm = WorldModel(n, m, hidden_size=tuple(dh), seed=70 + k, learn_reward=True)
        wm.dynamics_net.set_transformations(torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m), torch.full((n,), -0.02),
                                            torch.full((n,), 0.3))
        models.append(wm)
    agent = ModelAccelNPG(learned_model=models, env=None, policy=pol, baseline=LinearBaseline(spec), normalized_step_size=0.05, seed=1,
                          refine=True, kappa=5.0, plan_horizon=H, plan_paths=N)
    o = np.random.RandomState(0).randn(n) * 0.5
    torch.manual_seed(0)

    def block(c):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(c):
            agent.get_action(o)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / c

    lat = {"0": [], "1": []}
    for mfma in ("0", "1"):
        os.environ[SWITCH] = mfma
        block(5)
    for _ in range(4):
        for mfma in ("0", "1"):
            os.environ[SWITCH] = mfma
            lat[mfma].append(round(block((calls + 3) // 4), 4))
    os.environ.pop(SWITCH, None)
    return lat, agent.refine_route()


out = {"side": "mi355x", "calls": args.calls, "pairs": args.pairs}
shapes = [(nm, dh, ph, N, H) for nm in ((11, 2), (17, 6)) for dh in ((64, 64), (128, 128)) for ph in ((32, 32), (64, 64))
          for N in (100, 1024) for H in (10, 32)]
if args.quick:
    shapes = [s for s in shapes if s[0] == (17, 6) and s[2] == (64, 64)]
for (n, m), dh, ph, N, H in shapes:
    name = "%d_%d_dyn%d_pol%d_N%d_H%d" % (n, m, dh[0], ph[0], N, H)
    res, served = rollout_ms(n, m, dh, ph, 4, N, H, args.pairs)
    out[name + "_route"] = served
    out[name + "_rollout_ms_generic"], out[name + "_rollout_ms_mfma"] = res["0"], res["1"]      # median, best, quartiles
for (n, m), dh, ph, N, H in [((11, 2), (64, 64), (32, 32), 100, 10), ((17, 6), (64, 64), (64, 64), 100, 10),
                             ((17, 6), (128, 128), (64, 64), 1024, 32)]:
    name = "%d_%d_dyn%d_pol%d_N%d_H%d" % (n, m, dh[0], ph[0], N, H)
    lat, served = refined_ms(n, m, dh, ph, 4, N, H, args.calls)
    out[name + "_refined_ms_generic_blocks"], out[name + "_refined_ms_mfma_blocks"] = lat["0"], lat["1"]
print(json.dumps(out))
