#!/usr/bin/env python
"""MPC planning timings: latency of one MPCPolicy.get_action (host clock around calls that end in the read-back of the planned
sequence; warm-up, then >= 200 calls) and the time of the rollout launch alone (HIP events around mjx_plan_rollout), at
    (n, m) = (11, 2),  64 x 64,   K = 4, N = 256,  H = 16
    (n, m) = (17, 6),  128 x 128, K = 4, N = 1024, H = 32
    (n, m) = (11, 2),  256 x 256, K = 4, N = 250,  H = 50      (the generic rollout on both sides: the control)
    (n, m) = (6, 2),   64 x 64,   K = 3, N = 40,   H = 8  and  32 x 32, K = 1, N = 33, H = 5   (small plans: part-filled tiles)
with MJX_PLAN_MFMA=0 and =1 alternating in one process (=0 runs k_model_rollout exactly as before the MFMA route existed: the
baseline) -- on the MI355X (default) or, with --reference, the unmodified reference on the CPU, one thread (build box only: it
imports the reference through tests/golden/_ref_import.py).  Prints one JSON line.
    python tools/bench_mpc.py [--reference] [--calls 200]

--learned: planning on LEARNED rewards instead (one JSON line of its own).  (a) get_action with reward='learned' (mjx_path_rewards
between the rollout and the scoring, no host callback) against the only way to plan on learned rewards without it: reward='env'
behind a stand-in environment whose compute_path_rewards hands the k-th call to member k % K's WorldModel.compute_path_rewards
(read-back, K host calls, upload), alternating in one process, at (11, 2) 64 x 64 K 4 N 256 H 16 and (17, 6) 64 x 64 K 4 N 1024 H 32.
(b) mjx_path_rewards alone, MJX_PATH_REWARDS_MFMA=1 against =0 in alternating HIP-event pairs (median of >= 50 each), on one shape
per k_path_rewards instance at the two planners' row counts.
    python tools/bench_mpc.py --learned [--calls 200]"""
import ctypes
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "--reference" in sys.argv
LEARNED = "--learned" in sys.argv
if REF and LEARNED:
    sys.exit("--learned times this package on the GPU; it has no --reference side")
CALLS = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 200
if LEARNED:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _mpc_learned_oracle import CyclingInner      # the stand-in behind the host-callback side (the fixture's)
if REF:
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import _ref_import
    _ref_import.install()
    sys.modules.setdefault("mjrl.envs", types.ModuleType("mjrl.envs"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

if REF:
    torch.set_num_threads(1)
    from mjrl.algos.model_accel.model_learning_mpc import MPCPolicy
    from mjrl.algos.model_accel.nn_dynamics import WorldModel
else:
    from mjrl_amd._lib import check, load, ptr
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel

SHAPES = [(11, 2, (64, 64), 4, 256, 16), (17, 6, (128, 128), 4, 1024, 32), (11, 2, (256, 256), 4, 250, 50),
          (6, 2, (64, 64), 3, 40, 8), (6, 2, (32, 32), 1, 33, 5)]       # + the smallest plans of the test fixture: few, part-filled tiles


def step_flops(n, m, hid):
    """one member, one trajectory, one step: 2 (K1 h1 + h1 h2 + h2 n) with K1 = n + m"""
    return 2 * ((n + m) * hid[0] + hid[0] * hid[1] + hid[1] * n)


class Inner:
    def compute_path_rewards(self, paths):
        paths["rewards"] = -np.mean(paths["observations"] ** 2, -1) - 0.1 * np.mean(paths["actions"] ** 2, -1)


def planner(n, m, hid, K, N, H):
    models = []
    for k in range(K):
        wm = WorldModel(n, m, hidden_size=hid, seed=70 + k)
        wm.dynamics_net.set_transformations(torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m), torch.full((n,), -0.02),
                                            torch.full((n,), 0.3))
        models.append(wm)
    env = types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=Inner()))
    return MPCPolicy(env=env, plan_horizon=H, plan_paths=N, kappa=5.0, gamma=0.95, filter_coefs=[0.3, 0.25, 0.8, 0.0], fitted_model=models,
                     omega=1.0)


def time_calls(pol, obs, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        pol.get_action(obs)
    return (time.perf_counter() - t0) / calls * 1e3


def rollout_launch_ms(pol, obs, reps):
    """HIP events around mjx_plan_rollout alone, on the planner's packed members"""
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = load()
    pk = pol._packed(dev)
    K, N, H, n, m = len(pol.fitted_model), pol.num_traj, pol.plan_horizon, pol.n, pol.m
    a32 = torch.randn((N, H, m), device=dev) * 0.3
    s0 = torch.as_tensor(obs, dtype=torch.float32).to(dev)
    out = torch.empty((K, N, H, n), device=dev)
    sizes = (ctypes.c_int * len(pk["sizes"]))(*pk["sizes"])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        check(lib.mjx_plan_rollout(ptr(s0), 0, N, H, K, ptr(a32), sizes, len(pk["sizes"]), ptr(pk["P"]), ptr(pk["tr"]), pk["act"], pk["flags"],
                                   ptr(out), st))

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); launch(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2], ts[0]


def learned_models(n, m, hid, K):
    models = []
    for k in range(K):
        wm = WorldModel(n, m, hidden_size=hid, seed=70 + k, learn_reward=True)
        wm.dynamics_net.set_transformations(torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m), torch.full((n,), -0.02),
                                            torch.full((n,), 0.3))
        models.append(wm)
    return models


def path_rewards_ms(n, m, dh, rh, K, rows, pairs):
    """HIP events around mjx_path_rewards alone (random nets and rows, fp64 output as the planner asks for it), the two routes
    alternating pair by pair -> {route: (median, best)}, the route the dispatch takes"""
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = load()
    ds, rs = (n + m,) + tuple(dh) + (n,), (2 * n + m,) + tuple(rh) + (1,)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    count = lambda sz: sum(sz[i] * sz[i + 1] + sz[i + 1] for i in range(len(sz) - 1))
    g = torch.Generator(device="cpu").manual_seed(5)
    dP, rP = (torch.randn((K, count(ds)), generator=g) * 0.1).to(dev), (torch.randn((K, count(rs)), generator=g) * 0.1).to(dev)
    dtr = torch.cat([torch.zeros(n + m), torch.ones(n + m), torch.zeros(n), torch.full((n,), 0.3)]).repeat(K, 1).to(dev)
    rtr = torch.cat([torch.zeros(2 * n + m), torch.ones(2 * n + m), torch.zeros(1), torch.ones(1)]).repeat(K, 1).to(dev)
    obs, act = torch.randn((K, rows, n), generator=g).to(dev), torch.randn((rows, m), generator=g).to(dev)
    r64 = torch.empty((K, rows), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    route = ctypes.c_int(-1)

    def launch(mfma):
        os.environ["MJX_PATH_REWARDS_MFMA"] = mfma
        check(lib.mjx_path_rewards(ptr(obs), ptr(act), 0, rows, K, ints(ds), len(ds), ptr(dP), ptr(dtr), 0, 7, ints(rs), len(rs), ptr(rP),
                                   ptr(rtr), 0, None, ptr(r64), ctypes.byref(route), st))

    for mfma in ("0", "1", "0", "1"):
        launch(mfma)
    served = route.value
    torch.cuda.synchronize()
    ev = {"0": [], "1": []}
    for _ in range(pairs):
        for mfma in ("0", "1"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); launch(mfma); b.record()
            ev[mfma].append((a, b))
    torch.cuda.synchronize()
    os.environ.pop("MJX_PATH_REWARDS_MFMA", None)
    res = {}
    for mfma in ("0", "1"):
        ts = sorted(a.elapsed_time(b) for a, b in ev[mfma])
        res[mfma] = (ts[len(ts) // 2], ts[0], ts[len(ts) // 4], ts[3 * len(ts) // 4])
    return res, served


def learned_bench():
    out = {"side": "mi355x", "mode": "learned", "calls": CALLS}
    for n, m, hid, K, N, H in [(11, 2, (64, 64), 4, 256, 16), (17, 6, (64, 64), 4, 1024, 32)]:
        name = "%d_%d_%dx%d_K%d_N%d_H%d" % (n, m, hid[0], hid[1], K, N, H)
        models = learned_models(n, m, hid, K)
        kw = dict(plan_horizon=H, plan_paths=N, kappa=5.0, gamma=0.95, filter_coefs=[0.3, 0.25, 0.8, 0.0], fitted_model=models, omega=1.0)
        bare = types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=types.SimpleNamespace()))
        cyc = types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=CyclingInner(models)))
        pols = {"learned": MPCPolicy(env=bare, reward='learned', **kw), "host_callback": MPCPolicy(env=cyc, **kw)}
        obs = np.random.RandomState(0).randn(n) * 0.5
        np.random.seed(0)
        out[name + "_reward_route"] = pols["learned"].reward_route()
        for pol in pols.values():
            time_calls(pol, obs, 5)
        lat = {k: [] for k in pols}
        for rnd in range(4):
            for k, pol in pols.items():
                lat[k].append(time_calls(pol, obs, (CALLS + 3) // 4))
        for k in pols:
            out["%s_get_action_ms_%s" % (name, k)] = round(sorted(lat[k])[1], 4)
            out["%s_get_action_ms_%s_blocks" % (name, k)] = [round(v, 4) for v in lat[k]]
    # one shape per k_path_rewards instance <HB, NB, RB>: dynamics 32 HB wide, n = 17 (NB 1) or 39 (NB 2), reward 64 x 64 (RB 2) or 100 x 100 (RB 4)
    for hb in (1, 2, 3, 4):
        for n in (17, 39):
            for rh in ((64, 64), (100, 100)):
                for rows in (256 * 16, 1024 * 32, 165):
                    name = "pr_%dx%d_n%d_rew%dx%d_rows%d" % (32 * hb, 32 * hb, n, rh[0], rh[1], rows)
                    res, served = path_rewards_ms(n, 6, (32 * hb, 32 * hb), rh, 4, rows, 50)
                    out[name + "_route"] = served
                    for mfma, tag in (("0", "generic"), ("1", "mfma")):
                        out["%s_ms_%s" % (name, tag)] = [round(v, 4) for v in res[mfma]]      # median, best, quartiles
    print(json.dumps(out))


if LEARNED:
    learned_bench()
    sys.exit(0)

out = {"side": "reference_cpu_1_thread" if REF else "mi355x", "calls": CALLS}
for n, m, hid, K, N, H in SHAPES:
    name = "%dx%d_K%d_N%d_H%d" % (hid[0], hid[1], K, N, H)
    pol = planner(n, m, hid, K, N, H)
    obs = np.random.RandomState(0).randn(n) * 0.5
    np.random.seed(0)
    out[name + "_step_flops"] = step_flops(n, m, hid)
    if REF:
        calls = max(3, min(CALLS, int(20000 / (K * N * H * step_flops(n, m, hid) * 1e-6 + 1))))
        time_calls(pol, obs, 1)
        out[name + "_get_action_ms"] = round(time_calls(pol, obs, calls), 3)
        out[name + "_calls"] = calls
        continue
    out[name + "_route"] = pol.route()
    for mfma in ("0", "1"):                              # warm-up of both routes
        os.environ["MJX_PLAN_MFMA"] = mfma
        time_calls(pol, obs, 5)
    lat = {"0": [], "1": []}
    for rnd in range(4):                                 # alternating blocks in the same process
        for mfma in ("0", "1"):
            os.environ["MJX_PLAN_MFMA"] = mfma
            lat[mfma].append(time_calls(pol, obs, (CALLS + 3) // 4))
    for mfma, tag in (("0", "generic"), ("1", "mfma")):
        os.environ["MJX_PLAN_MFMA"] = mfma
        med, best = rollout_launch_ms(pol, obs, 50)
        out["%s_get_action_ms_%s" % (name, tag)] = round(sorted(lat[mfma])[1], 4)
        out["%s_get_action_ms_%s_blocks" % (name, tag)] = [round(v, 4) for v in lat[mfma]]
        out["%s_rollout_ms_%s" % (name, tag)] = round(med, 4)
        out["%s_rollout_ms_%s_best" % (name, tag)] = round(best, 4)
        out["%s_rollout_us_per_step_%s" % (name, tag)] = round(med * 1e3 / H, 3)
        out["%s_rollout_tflops_%s" % (name, tag)] = round(K * N * H * step_flops(n, m, hid) / (med * 1e-3) * 1e-12, 3)
    os.environ.pop("MJX_PLAN_MFMA", None)
print(json.dumps(out))
