#!/usr/bin/env python
"""Host cost of the four _wide learned-model entries and of mjx_plan_rollout, for the library MJX_LIB names (one process per build,
alternating, for a host-side refactor's evidence; needs the GPU): ns per call without rows (it returns before any device work: parse,
check, route ladder), us per enqueue of a small real call (K 2, N 32, H 3, 256 x 256 dynamics; no synchronisation inside the timed
batches of 50), and MPCPolicy.get_action (K 4, N 250, H 50, reward='learned', wide=True) on the host clock over 300 calls.  Every
figure as [lower quartile, median, upper quartile, route].  Prints one JSON object (profiles/r23_model_ladder/data/host_*.json).
    python tools/bench_model_host.py"""
import ctypes, json, os, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from mjrl_amd import _lib
lib = _lib.load()
dev = torch.device("cuda", 0)
ints = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
q3 = lambda ts: [round(float(np.percentile(ts, p)), 4) for p in (25, 50, 75)]
n, m, K, N, H = 11, 2, 2, 32, 3
ds, ps, rs = (n + m, 256, 256, n), (n, 64, 64, m), (2 * n + m, 100, 100, 1)
cnt = lambda s: sum(s[i] * s[i + 1] + s[i + 1] for i in range(3))
g = torch.Generator(device="cpu").manual_seed(0)
r = lambda *s: (torch.randn(*s, generator=g) * 0.05).to(dev)
P, pP, rP = r(K, cnt(ds)), r(cnt(ps) + m), r(K, cnt(rs))
tr = torch.cat([torch.zeros(K, n + m), torch.ones(K, n + m), torch.zeros(K, n), torch.ones(K, n)], 1).to(dev)
ptr_ = torch.cat([torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m)]).to(dev)
rtr = torch.cat([torch.zeros(K, 2 * n + m), torch.ones(K, 2 * n + m), torch.zeros(K, 1), torch.ones(K, 1)], 1).to(dev)
s0, acts, nz = r(N, n), r(N, H, m), r(K, H, N, m)
obs, act = torch.zeros(K * N * H * n, device=dev), torch.zeros(K * N * H * m, device=dev)
r32, err = torch.zeros(K * N * H, device=dev), torch.zeros(K * N * H, device=dev)
route = ctypes.c_int(-1)
rt = ctypes.byref(route)
dsi, psi, rsi = ints(ds), ints(ps), ints(rs)
def entries(N_, rows, Pn):
    return {
        "plan_rollout_wide": lambda: lib.mjx_plan_rollout_wide(ptr(s0), n, N_, H, K, ptr(acts), dsi, 4, ptr(P), ptr(tr), 0, 7, ptr(obs), rt, None),
        "plan_rollout": lambda: lib.mjx_plan_rollout(ptr(s0), n, N_, H, K, ptr(acts), dsi, 4, ptr(P), ptr(tr), 0, 7, ptr(obs), None),
        "policy_rollout_wide": lambda: lib.mjx_policy_rollout_wide(ptr(s0), n, N_, H, K, psi, 4, ptr(pP), ptr(ptr_), ptr(nz), H * N_ * m, dsi, 4, ptr(P), ptr(tr), 0, 7,
                                                                   None, None, None, None, ptr(obs), ptr(act), rt, None),
        "path_rewards_wide": lambda: lib.mjx_path_rewards_wide(ptr(obs), ptr(act), rows * m, rows, K, dsi, 4, ptr(P), ptr(tr), 0, 7, rsi, 4, ptr(rP), ptr(rtr), 0,
                                                               ptr(r32), None, rt, None),
        "rollout_disagreement_wide": lambda: lib.mjx_rollout_disagreement_wide(ptr(obs), ptr(act), Pn, H, K, dsi, 4, ptr(P), ptr(tr), 0, 7, ptr(err), rt, None),
    }
out = {"lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH), "empty_ns": {}, "enqueue_us": {}}
for name, f in entries(0, 0, 0).items():
    assert f() == 0, name
    best = []
    for _ in range(9):
        t = time.perf_counter()
        for _ in range(5000): f()
        best.append((time.perf_counter() - t) / 5000 * 1e9)
    out["empty_ns"][name] = q3(best) + [route.value]
for name, f in entries(N, N * H, N * K).items():
    for _ in range(5): assert f() == 0, name
    torch.cuda.synchronize()
    ts = []
    for _ in range(60):
        t = time.perf_counter()
        for _ in range(50): f()
        ts.append((time.perf_counter() - t) / 50 * 1e6)
        torch.cuda.synchronize()
    out["enqueue_us"][name] = q3(ts) + [route.value]
from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
members = [WorldModel(11, 2, hidden_size=(256, 256), seed=20 + k, learn_reward=True) for k in range(4)]
env = types.SimpleNamespace(observation_dim=11, action_dim=2, env=types.SimpleNamespace(env=types.SimpleNamespace()))
pol = MPCPolicy(env=env, plan_horizon=50, plan_paths=250, kappa=5.0, gamma=0.95, filter_coefs=[0.3, 0.25, 0.8, 0.0], fitted_model=members,
                omega=1.0, reward='learned', wide=True)
np.random.seed(4)
o = np.random.randn(11) * 0.3
for _ in range(10): pol.get_action(o)
ts = []
for _ in range(300):
    t = time.perf_counter(); pol.get_action(o); ts.append((time.perf_counter() - t) * 1e3)
out["get_action_ms"] = q3(ts) + [pol.last_routes()]
print(json.dumps(out))
