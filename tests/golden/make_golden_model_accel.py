#!/usr/bin/env python
"""Fixtures for model-based NPG from the UNMODIFIED reference (mjrl/algos/model_accel/), run on the CPU through _ref_import:
initial DynamicsNet parameters, short fit_dynamics / fit_reward runs (epoch losses, parameters, compute_loss), policy_rollout
outputs (eval and noisy, with bounds) and one whole ModelAccelNPG.train_step (3 models, truncate_lim set).  Also the state of
NumPy's and torch's global streams after a fit and a noisy rollout (the next draw of each).
    python tests/golden/make_golden_model_accel.py      ->  tests/golden/model_accel.npz
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install()
sys.modules.setdefault("mjrl.envs", types.ModuleType("mjrl.envs"))       # model_accel_npg.py:6 (the real one registers gym envs)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mjrl.algos.model_accel import nn_dynamics, sampling  # noqa: E402
from mjrl.algos.model_accel.model_accel_npg import ModelAccelNPG  # noqa: E402
from mjrl.baselines.linear_baseline import LinearBaseline  # noqa: E402
from mjrl.policies.gaussian_mlp import MLP  # noqa: E402
from mjrl.utils.gym_env import GymEnv  # noqa: E402

torch.set_num_threads(1)
TRUNC = float(os.environ.get('TRUNC', '0.005'))


class StandInEnv(GymEnv):
    def __init__(self, n, m, horizon, seed=0):
        self.n, self.m, self._horizon = n, m, horizon
        self.rng = np.random.RandomState(seed)

    @property
    def horizon(self):
        return self._horizon

    @property
    def spec(self):
        return types.SimpleNamespace(observation_dim=self.n, action_dim=self.m, horizon=self._horizon)

    def reset(self):
        return self.rng.randn(self.n)

    def set_seed(self, seed=None):
        self.rng = np.random.RandomState(seed)


def data(N, n, m, seed, zero_col=True):
    rng = np.random.RandomState(seed)
    s = rng.randn(N, n).astype(np.float32)
    a = rng.randn(N, m).astype(np.float32)
    W = rng.randn(n + m, n).astype(np.float32) * 0.3
    sp = (s + np.tanh(np.concatenate([s, a], 1) @ W) * 0.5).astype(np.float32)
    if zero_col:
        sp[:, 1] = s[:, 1]                   # a state column whose residual target has no variance: the mask
    return s, a, sp


def params(net):
    return np.concatenate([p.detach().numpy().ravel() for p in net.parameters()])


def main():
    out = {}
    n, m = 6, 2
    for hid in [(64, 64), (256, 256)]:
        for seed in ((123, 7) if hid[0] == 64 else (123,)):
            wm = nn_dynamics.WorldModel(n, m, hidden_size=hid, seed=seed)
            out["init_%dx%d_s%d" % (hid[0], hid[1], seed)] = params(wm.dynamics_net)
    # short fits: (hidden, batch, wd, residual, epochs, N, max_steps)
    fits = [((64, 64), 16, 0.0, True, 2, 400, 1e4), ((64, 64), 64, 1e-5, False, 3, 600, 1e4),
            ((256, 256), 64, 0.0, True, 2, 500, 1e4), ((64, 64), 16, 1e-5, True, 10, 200, 30),
            ((100, 100), 32, 0.0, False, 2, 300, 1e4)]
    for i, (hid, bs, wd, res, ep, N, ms) in enumerate(fits):
        s, a, sp = data(N, n, m, 10 + i)
        np.random.seed(100 + i)
        wm = nn_dynamics.WorldModel(n, m, hidden_size=hid, seed=3 + i, fit_wd=wd, residual=res)
        losses = wm.fit_dynamics(s, a, sp, bs, ep, max_steps=ms)
        out["fit%d_cfg" % i] = np.array([hid[0], hid[1], bs, wd, float(res), ep, N, ms], np.float64)
        out["fit%d_params" % i] = params(wm.dynamics_net)
        out["fit%d_losses" % i] = np.array(losses, np.float64)
        out["fit%d_loss" % i] = np.float64(wm.compute_loss(s, a, sp))
        out["fit%d_pred" % i] = wm.predict(s[:50], a[:50])
        if i == 0:
            out["rng_after_fit"] = np.array([np.random.rand(), torch.rand(1).item()])
    # fit_reward
    s, a, sp = data(300, n, m, 40, zero_col=False)
    r = (-np.sum(s ** 2, 1, keepdims=True) + 0.1 * a[:, :1]).astype(np.float32)
    np.random.seed(41)
    wm = nn_dynamics.WorldModel(n, m, learn_reward=True, hidden_size=(32, 32), seed=5)
    wm.fit_dynamics(s, a, sp, 32, 1)
    out["rew_dyn_params"] = params(wm.dynamics_net)
    # (set_transformations=True raises in the reference, nn_dynamics.py:138 reads r_shift before assigning it)
    out["rew_losses"] = np.array(wm.fit_reward(s, a, r, 32, 2, set_transformations=False), np.float64)
    out["rew_params"] = params(wm.reward_net)
    out["rew_pred"] = wm.reward(s[:40], a[:40]).detach().numpy()
    # policy_rollout: eval and noisy (bounds), N not a multiple of 8
    env = StandInEnv(n, m, 9)
    pol = MLP(env.spec, hidden_sizes=(16, 16), seed=2, init_log_std=-0.5)
    s, a, sp = data(400, n, m, 50)
    wm = nn_dynamics.WorldModel(n, m, hidden_size=(32, 32), seed=6)
    np.random.seed(51)
    wm.fit_dynamics(s, a, sp, 32, 1)
    out["roll_dyn_params"] = params(wm.dynamics_net)
    out["roll_dyn_tr"] = np.concatenate([t.numpy().ravel() for t in wm.dynamics_net.get_params()["transforms"]])
    out["roll_pol_params"] = pol.get_param_values()
    init = np.random.RandomState(52).randn(21, n).astype(np.float32)
    out["roll_init"] = init
    r_eval = sampling.policy_rollout(21, env, pol, wm, init_state=init, eval_mode=True, horizon=30)
    out["roll_eval_obs"], out["roll_eval_act"] = r_eval["observations"], r_eval["actions"]
    torch.manual_seed(53)
    r_noisy = sampling.policy_rollout(21, env, pol, wm, init_state=list(init), eval_mode=False, horizon=30,
                                      a_min=-0.4, a_max=0.4, s_min=torch.full((n,), -2.0), s_max=torch.full((n,), 2.5))
    out["roll_noisy_obs"], out["roll_noisy_act"] = r_noisy["observations"], r_noisy["actions"]
    out["rng_after_rollout"] = np.array([np.random.rand(), torch.rand(1).item()])
    # one ModelAccelNPG.train_step: 3 models, truncate_lim set
    models = []
    for k in range(3):
        s, a, sp = data(300, n, m, 60 + k)
        np.random.seed(61 + k)
        wm = nn_dynamics.WorldModel(n, m, hidden_size=(32, 32), seed=70 + k)
        wm.fit_dynamics(s, a, sp, 32, 2)
        out["ts_model%d" % k] = params(wm.dynamics_net)
        out["ts_model%d_tr" % k] = np.concatenate([t.numpy().ravel() for t in wm.dynamics_net.get_params()["transforms"]])
        models.append(wm)
    env = StandInEnv(n, m, 12)
    pol = MLP(env.spec, hidden_sizes=(8, 8), seed=4, init_log_std=-0.5)
    out["ts_pol0"] = pol.get_param_values()

    def reward_function(paths):
        paths["rewards"] = -np.sum(paths["observations"] ** 2, -1) - 0.1 * np.sum(paths["actions"] ** 2, -1)
        return paths

    agent = ModelAccelNPG(learned_model=models, env=env, policy=pol, baseline=LinearBaseline(env.spec), normalized_step_size=0.05,
                          seed=9, save_logs=True, reward_function=reward_function)
    lens = []
    fit0 = agent.baseline.fit

    def fit(paths, return_errors=False):
        lens.extend(len(p["rewards"]) for p in paths)
        return fit0(paths, return_errors=return_errors)

    agent.baseline.fit = fit
    init = [x for x in np.random.RandomState(80).randn(40, n)]
    torch.manual_seed(81)
    stats = agent.train_step(40, env=env, init_states=init, truncate_lim=TRUNC, truncate_reward=-1.0)
    out["ts_init"] = np.array(init)
    out["ts_stats"] = np.array(stats, np.float64)
    out["ts_pol1"] = pol.get_param_values()
    out["ts_lens"] = np.array(lens, np.int64)
    out["ts_keys"] = np.array(sorted(agent.logger.log.keys()))
    out["ts_seed"] = np.int64(agent.seed)
    out["ts_trunc"] = np.float64(TRUNC)
    path = os.path.join(HERE, "model_accel.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; truncated path lengths:", lens)


if __name__ == "__main__":
    main()
