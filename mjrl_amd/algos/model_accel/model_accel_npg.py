"""NPG on learned-model rollouts (reference mjrl/algos/model_accel/model_accel_npg.py:23-196).

``train_step`` rolls the policy out on every ensemble member in ONE launch (sampling.rollout_models; the noise is drawn
from torch's global stream in the reference's order, model by model, step by step), hands the rollouts to the host
reward / termination callables, truncates on ensemble disagreement with the batched forward plus one reduction
(``mjx_dyn_pred_error``), and then runs the NPG agent's own compute_returns -> compute_advantages -> train_from_paths
-> baseline.fit unchanged.
"""
import time as timer

import numpy as np
import torch

from ..._lib import check, load, ptr
from ...utils import process_samples
from ..npg_cg import NPG
from .nn_dynamics import WorldModel, _device, _stream, ensemble_forward, ensemble_path_rewards
from .sampling import _as_env, draw_rollout_noise, rollout_models


def truncation_points(models, paths, truncate_lim):
    """model_accel_npg.py:137-155's violation search for every path at once -> list of (first violating row or -1).
    Rows: s = obs[:-1], a = act[:-1], s_next = obs[1:]; error = max over models of mean_j (s_next - pred)^2."""
    dev = _device()
    n = models[0].dynamics_net.state_dim
    lens = [max(p['observations'].shape[0] - 1, 0) for p in paths]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = int(off[-1])
    if rows == 0:
        return [-1] * len(paths)
    s = np.concatenate([p['observations'][:-1] for p in paths]).astype(np.float32)
    a = np.concatenate([p['actions'][:-1] for p in paths]).astype(np.float32)
    sn = torch.from_numpy(np.concatenate([p['observations'][1:] for p in paths]).astype(np.float32)).to(dev)
    pred = ensemble_forward([mdl.dynamics_net for mdl in models], np.concatenate([s, a], -1), dev)
    off_d = torch.from_numpy(off).to(dev)
    err = torch.empty(rows, dtype=torch.float32, device=dev)
    first = torch.empty(len(paths), dtype=torch.int32, device=dev)
    check(load().mjx_dyn_pred_error(ptr(pred), len(models), rows, n, ptr(sn), ptr(off_d), len(paths), float(truncate_lim),
                                    ptr(err), ptr(first), _stream(dev)))
    return [int(v) for v in first.cpu().numpy()]


class ModelAccelNPG(NPG):
    def __init__(self, learned_model=None,
                 refine=False,
                 kappa=5.0,
                 plan_horizon=10,
                 plan_paths=100,
                 reward_function=None,
                 termination_function=None,
                 **kwargs):
        """Arguments as in the reference (model_accel_npg.py:24-41)."""
        super(ModelAccelNPG, self).__init__(**kwargs)
        if learned_model is None:
            raise ValueError("Algorithm requires a (list of) learned dynamics model")
        elif isinstance(learned_model, WorldModel):
            self.learned_model = [learned_model]
        else:
            self.learned_model = learned_model
        self.refine, self.kappa, self.plan_horizon, self.plan_paths = refine, kappa, plan_horizon, plan_paths
        self.reward_function, self.termination_function = reward_function, termination_function

    def to(self, device):
        for model in self.learned_model:
            model.to(device)
        try:
            self.baseline.model.to(device)
        except Exception:
            pass

    def is_cuda(self):
        model_cuda = any([model.is_cuda() for model in self.learned_model])
        try:
            baseline_cuda = next(self.baseline.model.parameters()).is_cuda
        except Exception:
            baseline_cuda = False
        return any([model_cuda, baseline_cuda])

    def train_step(self, N,
                   env=None,
                   sample_mode='trajectories',
                   horizon=1e6,
                   gamma=0.995,
                   gae_lambda=0.97,
                   num_cpu='max',
                   env_kwargs=None,
                   init_states=None,
                   reward_function=None,
                   termination_function=None,
                   truncate_lim=None,
                   truncate_reward=0.0,
                   **kwargs,
                   ):
        """model_accel_npg.py:58-183"""
        ts = timer.time()
        env = self.env if env is None else _as_env(env, env_kwargs)
        reward_function = self.reward_function if reward_function is None else reward_function
        termination_function = self.termination_function if termination_function is None else termination_function
        if reward_function:
            assert callable(reward_function)
        if termination_function:
            assert callable(termination_function)

        init_states = np.array([env.reset() for _ in range(N)]) if init_states is None else init_states
        assert type(init_states) == list
        assert len(init_states) == N

        # every member's rollout in one launch; the noise is what the reference's per-model policy_rollout calls draw
        horizon = int(min(horizon, env.horizon))
        m = self.learned_model[0].dynamics_net.act_dim
        noise = draw_rollout_noise(len(self.learned_model), horizon, N, m)
        obs_all, act_all = rollout_models(self.learned_model, self.policy, np.array(init_states), horizon, noise)
        paths = []
        obs = None
        # every member's learned rewards in one batched call (one upload, two launches, one read-back) when all members learn them
        rew_all = ensemble_path_rewards(self.learned_model, obs_all, act_all) if all(mdl.learn_reward for mdl in self.learned_model) else None
        for k, model in enumerate(self.learned_model):
            rollouts = dict(observations=obs_all[k], actions=act_all[k])
            if rew_all is not None:
                rollouts['rewards'] = rew_all[k]
            elif model.learn_reward:
                model.compute_path_rewards(rollouts)
            else:
                rollouts = reward_function(rollouts)
            num_traj, horizon, state_dim = rollouts['observations'].shape
            for i in range(num_traj):
                obs = rollouts['observations'][i, :, :]
                paths.append(dict(observations=obs, actions=rollouts['actions'][i, :, :], rewards=rollouts['rewards'][i, :],
                                  terminated=False))

        if callable(termination_function):
            paths = termination_function(paths)
        paths = [path for path in paths if path['observations'].shape[0] >= 5]

        # truncation on ensemble disagreement (model_accel_npg.py:137-155); `obs` is the last rollout row block, as there
        if truncate_lim is not None and len(self.learned_model) > 1:
            firsts = truncation_points(self.learned_model, paths, truncate_lim)
            for path, v in zip(paths, firsts):
                truncated = v >= 0
                T = v + 1 if truncated else obs.shape[0]
                T = max(4, T)
                path["observations"] = path["observations"][:T]
                path["actions"] = path["actions"][:T]
                path["rewards"] = path["rewards"][:T]
                if truncated:
                    path["rewards"][-1] += truncate_reward
                path["terminated"] = False if T == obs.shape[0] else True

        if self.save_logs:
            self.logger.log_kv('time_sampling', timer.time() - ts)
        self.seed = self.seed + N if self.seed is not None else self.seed

        process_samples.compute_returns(paths, gamma)
        process_samples.compute_advantages(paths, self.baseline, gamma, gae_lambda)
        eval_statistics = self.train_from_paths(paths)
        eval_statistics.append(N)
        if self.save_logs:
            num_samples = np.sum([p["rewards"].shape[0] for p in paths])
            self.logger.log_kv('num_samples', num_samples)
        if self.save_logs:
            ts = timer.time()
            error_before, error_after = self.baseline.fit(paths, return_errors=True)
            self.logger.log_kv('time_VF', timer.time() - ts)
            self.logger.log_kv('VF_error_before', error_before)
            self.logger.log_kv('VF_error_after', error_after)
        else:
            self.baseline.fit(paths)
        return eval_statistics

    def get_action(self, observation):
        if self.refine is False:
            return self.policy.get_action(observation)
        return self.get_refined_action(observation)

    def get_refined_action(self, observation):
        raise NotImplementedError
