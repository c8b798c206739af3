#!/usr/bin/env python
"""mjx_plan_rollout_wide alone between HIP events, MJX_PLAN_WIDE alternating 1 / 0 in one process (route 2, the wide MFMA kernel
of csrc/plan_wide.h, against route 0, which is the parent commit's kernel for these shapes bit for bit): per shape a warm-up on each
side, then PAIRS alternations; per side the median [min .. max] in ms, and whether route 2 was faster in EVERY alternation by more
than route 0's own spread (max - min) -- the rule a default-on dispatch in MPCPolicy has to meet.  Shapes: K 4, N 250, H 50 and
H 10 on dynamics [13, 256, 256, 11] and [23, 256, 256, 17]; K 1, N 32 (one workgroup).  Then MPCPolicy.get_action on the host clock
ending in the read-back of the sequence, reward='learned' with 100 x 100 reward nets, K 4, N 250, H 50, MJX_PLAN_WIDE and
MJX_PATH_REWARDS_WIDE flipped together on a planner built with wide=True, CALLS calls a side, alternating.  Prints one JSON object
(profiles/r21_plan_wide/bench_plan_wide.json).    python tools/bench_plan_wide.py [pairs] [calls]"""
import ctypes, json, os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from mjrl_amd import _lib
lib = _lib.load()
dev = torch.device("cuda", 0)
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 40
CALLS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ints = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
stat = lambda ts: [round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)]
def kernel_row(n, m, dh, K, N, H):
    ds = (n + m,) + dh + (n,)
    Pd = sum(ds[i] * ds[i + 1] + ds[i + 1] for i in range(3))
    g = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.05).to(dev)
    P = r(K, Pd)
    tr = torch.cat([torch.zeros(K, n + m), torch.ones(K, n + m), torch.zeros(K, n), torch.ones(K, n)], 1).to(dev)
    s0, acts = r(N, n), r(N, H, m)
    obs = torch.empty(K * N * H * n, device=dev)
    route = ctypes.c_int(-1)
    def timed(wide):
        os.environ["MJX_PLAN_WIDE"] = wide
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.mjx_plan_rollout_wide(ptr(s0), n, N, H, K, ptr(acts), ints(ds), 4, ptr(P), ptr(tr), 0, 7, ptr(obs), ctypes.byref(route), None))
        e1.record(); torch.cuda.synchronize()
        os.environ.pop("MJX_PLAN_WIDE")
        return e0.elapsed_time(e1), route.value
    routes = {}
    for wide in "10":                                       # the warm-up of each side
        for _ in range(3):
            routes[wide] = timed(wide)[1]
    t2, t0 = [], []
    for _ in range(PAIRS):
        t2.append(timed("1")[0]); t0.append(timed("0")[0])
    spread0 = max(t0) - min(t0)
    return dict(routes=[routes["1"], routes["0"]], route2_ms=stat(t2), route0_ms=stat(t0), pairs=PAIRS, route0_spread_ms=round(spread0, 4),
                pairs_route2_faster=int(sum(a < b for a, b in zip(t2, t0))),
                faster_in_every_pair_by_more_than_route0_spread=bool(all(b - a > spread0 for a, b in zip(t2, t0))))
def planner_row(n, m, K, N, H):
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    members = [WorldModel(n, m, hidden_size=(256, 256), seed=20 + k, learn_reward=True) for k in range(K)]
    env = types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=types.SimpleNamespace()))
    pol = MPCPolicy(env=env, plan_horizon=H, plan_paths=N, kappa=5.0, gamma=0.95, filter_coefs=[0.3, 0.25, 0.8, 0.0], fitted_model=members,
                    omega=1.0, reward='learned', wide=True)
    np.random.seed(4)
    o = np.random.randn(n) * 0.3
    def timed(wide):
        os.environ["MJX_PLAN_WIDE"] = os.environ["MJX_PATH_REWARDS_WIDE"] = wide
        t = time.perf_counter()
        pol.get_action(o)                                   # (ends in the read-back of the planned sequence)
        dt = (time.perf_counter() - t) * 1e3
        os.environ.pop("MJX_PLAN_WIDE"); os.environ.pop("MJX_PATH_REWARDS_WIDE")
        return dt, pol.last_routes()
    routes = {}
    for wide in "10":
        for _ in range(5):
            routes[wide] = timed(wide)[1]
    tw, tn = [], []
    for _ in range(CALLS):
        tw.append(timed("1")[0]); tn.append(timed("0")[0])
    return dict(routes=[routes["1"], routes["0"]], wide_ms=stat(tw), narrow_ms=stat(tn), calls_a_side=CALLS,
                pairs_wide_faster=int(sum(a < b for a, b in zip(tw, tn))))
out = {}
for tag, a in {"d13_K4_N250_H50": (11, 2, (256, 256), 4, 250, 50), "d23_K4_N250_H50": (17, 6, (256, 256), 4, 250, 50),
               "d13_K4_N250_H10": (11, 2, (256, 256), 4, 250, 10), "d23_K4_N250_H10": (17, 6, (256, 256), 4, 250, 10),
               "d13_K1_N32_H50": (11, 2, (256, 256), 1, 32, 50), "d23_K1_N32_H50": (17, 6, (256, 256), 1, 32, 50)}.items():
    out[tag] = kernel_row(*a)
out["get_action_d13_K4_N250_H50_learned"] = planner_row(11, 2, 4, 250, 50)
out["dispatch_on_by_rule"] = bool(out["d13_K4_N250_H50"]["faster_in_every_pair_by_more_than_route0_spread"]
                                  and out["d23_K4_N250_H50"]["faster_in_every_pair_by_more_than_route0_spread"])
print(json.dumps(out, indent=1))
