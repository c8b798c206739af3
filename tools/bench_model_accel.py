#!/usr/bin/env python
"""Model-based NPG timings: fit time per Adam step at (64, 64) and (256, 256), minibatch 16 and 64 (persistent route and the
launch route), one policy_rollout over K = 4 models, N = 250, H = 50, and one ModelAccelNPG.train_step (3 models, 250 paths,
horizon 25) -- on the MI355X (default) or, with --reference, the unmodified reference on the CPU for the same seeded inputs
(build box only: it imports the reference through tests/golden/_ref_import.py).  Prints one JSON line.

On the MI355X the train_step is then timed on both of its routes in one process -- host and resident (train_step(resident=True)),
five alternations after a warm-up of each, with a host reward_function and with learned rewards: median [min .. max] of the whole
step and of its sampling part (the logged time_sampling: everything up to the finished paths), and the resident route's routes.
Before that, at the reference's own width (256 x 256 dynamics, 64 x 64 policy): rollout_models_device at K = 4, N = 250, H = 50 and
the resident train_step (3 models, 250 paths, horizon 25) with MJX_POLICY_ROLLOUT_WIDE=1 (route 2, csrc/policy_rollout_wide.h)
and =0 (route 0) in one process, a warm-up of each and five alternations: median [min .. max] and whether route 2 won every one.
--step-only: only the train_step rows.
    python tools/bench_model_accel.py [--reference] [--step-only]"""
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "--reference" in sys.argv
if REF:
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import _ref_import
    _ref_import.install()
    sys.modules.setdefault("mjrl.envs", types.ModuleType("mjrl.envs"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

if REF:
    from mjrl.algos.model_accel import nn_dynamics as D, sampling as S
    from mjrl.algos.model_accel.model_accel_npg import ModelAccelNPG
    from mjrl.baselines.linear_baseline import LinearBaseline
    from mjrl.policies.gaussian_mlp import MLP
else:
    from mjrl_amd.algos.model_accel import nn_dynamics as D, sampling as S
    from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP

n, m = 11, 2                         # the reference's reacher config shapes (run_experiments/configs/reacher.txt)


def sync():
    if not REF:
        torch.cuda.synchronize()


def data(N, seed):
    rng = np.random.RandomState(seed)
    s = rng.randn(N, n).astype(np.float32)
    a = rng.randn(N, m).astype(np.float32)
    W = rng.randn(n + m, n).astype(np.float32) * 0.3
    return s, a, (s + np.tanh(np.concatenate([s, a], 1) @ W) * 0.5).astype(np.float32)


class Env:
    def __init__(self, horizon):
        self.horizon = horizon
        self.spec = types.SimpleNamespace(observation_dim=n, action_dim=m, horizon=horizon)

    def reset(self):
        return np.zeros(n)

    def set_seed(self, seed=None):
        pass


if REF:
    from mjrl.utils.gym_env import GymEnv
    Env = type("Env", (GymEnv,), {"__init__": Env.__init__, "horizon": None, "spec": None, "reset": Env.reset, "set_seed": Env.set_seed})

out = {"side": "reference_cpu" if REF else "mi355x"}
STEP_ONLY = "--step-only" in sys.argv and not REF
routes = [None] if REF else ["0", "1"]
for hid in [] if STEP_ONLY else [(64, 64), (256, 256)]:
    for bs in (16, 64):
        for route in routes:
            if route is not None:
                os.environ["MJX_DYN_FIT_LAUNCHES"] = route
            N = bs * (100 if REF else 400)
            s, a, sp = data(N, 1)
            np.random.seed(0)
            wm = D.WorldModel(n, m, hidden_size=hid, seed=1)
            wm.fit_dynamics(s[:bs * 4], a[:bs * 4], sp[:bs * 4], bs, 1)          # warm-up
            sync()
            t0 = time.perf_counter()
            wm.fit_dynamics(s, a, sp, bs, 1)
            sync()
            key = "fit_us_per_step_%dx%d_mb%d%s" % (hid[0], hid[1], bs, "" if route is None else ("_launch" if route == "1" else ""))
            out[key] = round((time.perf_counter() - t0) / (N // bs) * 1e6, 2)
os.environ.pop("MJX_DYN_FIT_LAUNCHES", None)

env = Env(50)
pol = MLP(env.spec, hidden_sizes=(64, 64), seed=2)
models = [D.WorldModel(n, m, hidden_size=(256, 256), seed=10 + k) for k in range(4)]
init = np.random.RandomState(3).randn(250, n).astype(np.float32)
if not STEP_ONLY:
    S.policy_rollout(250, env, pol, models[0], init_state=init, eval_mode=False, horizon=2)
    sync()
    t0 = time.perf_counter()
    for mdl in models:
        S.policy_rollout(250, env, pol, mdl, init_state=init, eval_mode=False, horizon=50)
    sync()
    out["rollout_ms_K4_N250_H50_per_model_calls"] = round((time.perf_counter() - t0) * 1e3, 2)
if not REF and not STEP_ONLY:
    noise = S.draw_rollout_noise(4, 50, 250, m)
    sync()
    t0 = time.perf_counter()
    S.rollout_models(models, pol, init, 50, noise)
    sync()
    out["rollout_ms_K4_N250_H50_one_launch"] = round((time.perf_counter() - t0) * 1e3, 2)

env = Env(25)
pol = MLP(env.spec, hidden_sizes=(64, 64), seed=4)
models = [D.WorldModel(n, m, hidden_size=(64, 64), seed=20 + k) for k in range(3)]


def reward_function(paths):
    paths["rewards"] = -np.sum(paths["observations"] ** 2, -1)
    return paths


agent = ModelAccelNPG(learned_model=models, env=env, policy=pol, baseline=LinearBaseline(env.spec), normalized_step_size=0.05,
                      seed=0, save_logs=True, reward_function=reward_function)
init = [x for x in np.random.RandomState(5).randn(250, n)]
agent.train_step(250, env=env, init_states=init, truncate_lim=1.0)     # warm-up
sync()
t0 = time.perf_counter()
agent.train_step(250, env=env, init_states=init, truncate_lim=1.0)
sync()
out["train_step_ms_3models_250paths_H25"] = round((time.perf_counter() - t0) * 1e3, 2)


def spread(v):
    return [round(float(np.median(v)), 3), round(float(min(v)), 3), round(float(max(v)), 3)]


def both_routes(agent, tag, rounds=5):
    """host and resident steps in alternation -> median [min, max] of the step and of its sampling part, in ms"""
    times = {False: ([], []), True: ([], [])}
    for resident in (False, True):
        agent.train_step(250, env=env, init_states=init, truncate_lim=1.0, resident=resident)      # warm-up
    for _ in range(rounds):
        for resident in (False, True):
            sync()
            t0 = time.perf_counter()
            agent.train_step(250, env=env, init_states=init, truncate_lim=1.0, resident=resident)
            sync()
            times[resident][0].append((time.perf_counter() - t0) * 1e3)
            times[resident][1].append(agent.logger.log["time_sampling"][-1] * 1e3)
            info = agent.train_step_info()
            assert info["resident"] is resident, info
    for resident, name in ((False, "host"), (True, "resident")):
        out["train_step_%s_%s_ms" % (tag, name)] = spread(times[resident][0])
        out["train_step_%s_%s_sampling_ms" % (tag, name)] = spread(times[resident][1])
    out["train_step_%s_resident_info" % tag] = {k: info[k] for k in ("routes", "paths", "rows", "truncated")}


def wide_ab(call, rounds=5):
    """`call` under MJX_POLICY_ROLLOUT_WIDE=1 and =0 in alternation after a warm-up of each -> {switch: (times in ms, last result)}"""
    times, last = {"1": [], "0": []}, {}
    try:
        for wide in ("1", "0"):
            os.environ["MJX_POLICY_ROLLOUT_WIDE"] = wide
            call()
        for _ in range(rounds):
            for wide in ("1", "0"):
                os.environ["MJX_POLICY_ROLLOUT_WIDE"] = wide
                sync()
                t0 = time.perf_counter()
                last[wide] = call()
                sync()
                times[wide].append((time.perf_counter() - t0) * 1e3)
    finally:
        os.environ.pop("MJX_POLICY_ROLLOUT_WIDE", None)
    return {wide: (times[wide], last[wide]) for wide in times}


def wide_rows():
    """the wide MFMA policy rollout (mjx_policy_rollout_wide, route 2) against route 0 at the reference's own width, 256 x 256"""
    wenv = Env(50)
    wpol = MLP(wenv.spec, hidden_sizes=(64, 64), seed=2)
    wide = [D.WorldModel(n, m, hidden_size=(256, 256), seed=10 + k) for k in range(4)]
    s0 = np.random.RandomState(3).randn(250, n).astype(np.float32)
    if not STEP_ONLY:
        noise = S.draw_rollout_noise(4, 50, 250, m)
        pk = D.pack_dynamics_members(wide, D._device())
        info = {}

        def rollout():
            S.rollout_models_device(wide, wpol, s0, 50, noise, packed=pk, info=info)
            return info["route"]

        r = wide_ab(rollout)
        for sw in ("1", "0"):
            out["rollout_device_ms_K4_N250_H50_256x256_wide%s" % sw] = spread(r[sw][0])
            out["rollout_device_route_wide%s" % sw] = r[sw][1]
        out["rollout_device_wide_faster_in_every_alternation"] = all(a < b for a, b in zip(r["1"][0], r["0"][0]))
    tenv = Env(25)
    wagent = ModelAccelNPG(learned_model=wide[:3], env=tenv, policy=MLP(tenv.spec, hidden_sizes=(64, 64), seed=4),
                           baseline=LinearBaseline(tenv.spec), normalized_step_size=0.05, seed=0, save_logs=True,
                           reward_function=reward_function)

    def step():
        wagent.train_step(250, env=tenv, init_states=init, truncate_lim=1.0, resident=True)
        info = wagent.train_step_info()
        assert info["resident"] is True, info
        return [info["routes"]["rollout"], wagent.logger.log["time_sampling"][-1] * 1e3]

    r = wide_ab(step)
    for sw in ("1", "0"):
        out["train_step_resident_256x256_ms_wide%s" % sw] = spread(r[sw][0])
        out["train_step_resident_256x256_rollout_route_wide%s" % sw] = r[sw][1][0]
    out["train_step_resident_256x256_wide_faster_in_every_alternation"] = all(a < b for a, b in zip(r["1"][0], r["0"][0]))


if not REF:
    wide_rows()
    both_routes(agent, "reward_function")
    learned = [D.WorldModel(n, m, hidden_size=(64, 64), seed=20 + k, learn_reward=True) for k in range(3)]
    both_routes(ModelAccelNPG(learned_model=learned, env=env, policy=MLP(env.spec, hidden_sizes=(64, 64), seed=4),
                              baseline=LinearBaseline(env.spec), normalized_step_size=0.05, seed=0, save_logs=True), "learned_rewards")
print(json.dumps(out))
