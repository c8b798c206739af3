"""NPG on learned-model rollouts (reference mjrl/algos/model_accel/model_accel_npg.py:23-196).

``train_step`` rolls the policy out on every ensemble member in ONE launch (sampling.rollout_models; the noise is drawn
from torch's global stream in the reference's order, model by model, step by step), hands the rollouts to the host
reward / termination callables, truncates on ensemble disagreement with the batched forward plus one reduction
(``mjx_dyn_pred_error``), and then runs the NPG agent's own compute_returns -> compute_advantages -> train_from_paths
-> baseline.fit unchanged.  With ``resident=True`` the rollouts stay on the device from the rollout to ingestion
(:meth:`ModelAccelNPG._resident_paths`: the MFMA policy rollout on cached members, learned rewards, disagreement, truncation and
packing in HIP, one read-back for the host ``paths``, the packed blocks registered with utils/ingest).  ``get_refined_action`` keeps the members on the device through ``nn_dynamics.cached_members_pack``, the
cache ``MPCPolicy`` uses, with the refinement's default bound vectors as its extras.
"""
import time as timer

import numpy as np
import torch

from ..._lib import check, load, ptr
from ...utils import ingest, process_samples
from ..npg_cg import NPG
from .nn_dynamics import (WorldModel, _device, _ints, _stream, cached_members_pack, ensemble_forward, ensemble_path_rewards,
                          members_share_kind, path_rewards_call, predicted_route, rollout_disagreement_device)
from .sampling import (_as_env, draw_rollout_noise, pack_rollouts_device, rollout_bounds, rollout_models, rollout_models_device,
                       wide_rollout_shape)

REFINE_LARGE_VALUE = float(1e2)     # the refined call's state / action bounds: policy_rollout's default large_value
TRAIN_LARGE_VALUE = float(1e2)      # train_step's: rollout_models' default (the same number today; each caller names its own)
MIN_PATH_LEN = 5                    # train_step drops shorter paths (model_accel_npg.py:134)
MIN_TRUNCATED_LEN = 4               # ... and keeps at least this much of a truncated one (:150)


def _gpu_available():
    return torch.cuda.is_available()


def _distributed():
    return torch.distributed.is_available() and torch.distributed.is_initialized()


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
    # (an instance pickled before the refinement existed acts as it did)
    refine_gamma, refine_omega, _refine_pack, _refine_last, _refine_packs = 1.0, 0.0, None, None, 0
    resident, _step_info = False, None

    def __init__(self, learned_model=None,
                 refine=False,
                 kappa=5.0,
                 plan_horizon=10,
                 plan_paths=100,
                 reward_function=None,
                 termination_function=None,
                 refine_gamma=1.0,
                 refine_omega=0.0,
                 resident=False,
                 **kwargs):
        """Arguments as in the reference (model_accel_npg.py:24-41), plus refine_gamma and refine_omega: the discount and the
        weight of the per-trajectory ensemble disagreement in get_refined_action's trajectory scores; and resident: whether
        train_step keeps the model rollouts on the device up to ingestion (off by default; train_step's own keyword overrides it)."""
        super(ModelAccelNPG, self).__init__(**kwargs)
        if learned_model is None:
            raise ValueError("Algorithm requires a (list of) learned dynamics model")
        elif isinstance(learned_model, WorldModel):
            self.learned_model = [learned_model]
        else:
            self.learned_model = learned_model
        self.refine, self.kappa, self.plan_horizon, self.plan_paths = refine, kappa, plan_horizon, plan_paths
        self.reward_function, self.termination_function = reward_function, termination_function
        self.refine_gamma, self.refine_omega = refine_gamma, refine_omega
        self.resident = bool(resident)
        self._step_info = None      # train_step_info() of the last train_step
        self._refine_pack = None    # (key, device blocks, held tensors) of the members' parameters and transforms
        self._refine_last = None    # (R, S, route) of the last refined call, on the device
        self._refine_packs = 0      # how often the members were packed

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
                   resident=None,
                   **kwargs,
                   ):
        """model_accel_npg.py:58-183.  resident (None: the constructor's): the device-resident route of :meth:`_resident_paths`
        where :meth:`_resident_decline` has no objection, the host route otherwise; :meth:`train_step_info` says which ran."""
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
        resident = self.resident if resident is None else bool(resident)
        why = self._resident_decline(horizon, termination_function) if resident else "resident=False"
        self._step_info = dict(resident=why is None, why=why, routes=None, paths=None, rows=None, truncated=None)
        if why is None:
            paths = self._resident_paths(np.array(init_states), horizon, noise, reward_function, truncate_lim, truncate_reward)
        else:
            paths = self._host_paths(np.array(init_states), horizon, noise, reward_function, termination_function, truncate_lim,
                                     truncate_reward)

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

    def _host_paths(self, init_states, horizon, noise, reward_function, termination_function, truncate_lim, truncate_reward):
        """the host route's paths (model_accel_npg.py:95-155): rollout, rewards, termination, the length filter, truncation"""
        obs_all, act_all = rollout_models(self.learned_model, self.policy, init_states, horizon, noise)
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
        return paths

    # ---- the device-resident route
    def train_step_info(self):
        """what the last ``train_step`` did: dict(resident, why (the reason the host route ran, else None), routes (dict(rollout,
        rewards, disagreement): 1 = the MFMA kernel, 0 = the generic route, None = no device call; each may also be 2 = the
        wide MFMA kernel for nets up to 256 wide: csrc/policy_rollout_wide.h for rollout, csrc/rows_wide.h for rewards and
        disagreement, where ``nn_dynamics.wide_rows_shape`` sends them to the ``_wide`` entries), paths, rows, truncated);
        None before any call.  The last three are filled by the resident route alone."""
        return None if self._step_info is None else dict(self._step_info)

    def _resident_decline(self, horizon, termination_function):
        """why the resident route does not serve this call, or None"""
        models = self.learned_model
        learned = [bool(mdl.learn_reward) for mdl in models]
        if callable(termination_function):
            return "termination_function"               # a host callable over the paths, before the truncation
        if any(learned) and not all(learned):
            return "mixed rewards"
        if not members_share_kind(models, all(learned)):
            return "members differ"
        if horizon < MIN_PATH_LEN:
            return "horizon < %d" % MIN_PATH_LEN        # the length filter drops every path
        if _distributed():
            return "distributed"
        if not _gpu_available():
            return "no gpu"
        return None

    def _resident_paths(self, init_states, H, noise, reward_function, truncate_lim, truncate_reward):
        """the same paths with the rollouts left on the device: one upload (start states, noise), ``mjx_policy_rollout`` on the
        members ``get_refined_action`` caches, ``mjx_path_rewards`` (or one read-back, the host ``reward_function`` per member and
        one upload), ``mjx_rollout_disagreement`` (both through their ``_wide`` entries for dynamics nets wider than 128,
        ``nn_dynamics.wide_rows_shape``), ``mjx_rollout_pack``, one read-back of the packed blocks.  The host ``paths``
        are per-path views of that read-back; the packed device blocks are registered for them (utils/ingest.register_device_batch),
        so returns, advantages, the update and the baseline read those and upload nothing."""
        dev = _device()
        models = self.learned_model
        K, N = len(models), init_states.shape[0]
        learned = self._refine_learned()
        pk = self._refine_packed(dev)
        info, routes = {}, dict(rollout=None, rewards=None, disagreement=None)
        obs_d, act_d = rollout_models_device(models, self.policy, init_states, H, noise, large_value=TRAIN_LARGE_VALUE, packed=pk, info=info)
        routes["rollout"] = info["route"]
        if learned:
            rew_d = torch.empty((K, N, H), dtype=torch.float32, device=dev)
            routes["rewards"] = path_rewards_call(pk["rew"], obs_d, act_d, False, N * H, K, rew_d, None, dev, wide=True)
        else:
            obs_h, act_h = obs_d.cpu().numpy(), act_d.cpu().numpy()
            rew_h = [np.asarray(reward_function(dict(observations=obs_h[k], actions=act_h[k]))['rewards']) for k in range(K)]
            rew_h = np.stack(rew_h)
            rew_d = torch.from_numpy(np.ascontiguousarray(rew_h, np.float32 if rew_h.dtype == np.float32 else np.float64)).to(dev)
        err_d = None
        if truncate_lim is not None and K > 1:
            err_d = rollout_disagreement_device(models, obs_d, act_d, packed=pk, info=info, wide=True)
            routes["disagreement"] = info["route"]
        pb = pack_rollouts_device(obs_d, act_d, rew_d, err_d, 0.0 if truncate_lim is None else truncate_lim, MIN_TRUNCATED_LEN,
                                  truncate_reward)
        # one read-back: the offsets, then the packed rows
        off = pb["off"].cpu().numpy()
        rows = int(off[-1])
        term = pb["term"].cpu().numpy()
        blocks = dict(observations=pb["obs"][:rows], actions=pb["act"][:rows], rewards=pb["rew"][:rows])
        obs_p, act_p = blocks["observations"].cpu().numpy(), blocks["actions"].cpu().numpy()
        rew_p = blocks["rewards"].cpu().numpy()
        if rew_d.dtype == torch.float32:
            rew_p = rew_p.astype(np.float32)                   # (exact: every packed value is an fp32 number)
        for a in (obs_p, act_p, rew_p):
            a.setflags(write=False)                            # the device blocks stay registered for these arrays (utils/ingest.py)
        paths = [dict(observations=obs_p[off[i]:off[i + 1]], actions=act_p[off[i]:off[i + 1]], rewards=rew_p[off[i]:off[i + 1]],
                      terminated=bool(term[i])) for i in range(K * N)]
        h = ingest.DeviceHandle(torch, dev, load())
        shared = dict(offsets_dev=pb["off"], terminated_dev=pb["term"])
        ingest.register_device_batch(
            h, paths, dict(observations=dict(f32=blocks["observations"], raw=blocks["observations"]),
                           actions=dict(f32=blocks["actions"], raw=blocks["actions"]),
                           rewards=dict(f32=None, raw=blocks["rewards"])),
            derived=dict(observations=dict(obs64=pb["obs64"][:rows], tpos=pb["tpos"][:rows]), rewards=shared))
        self._step_info.update(routes=routes, paths=K * N, rows=rows, truncated=int(term.sum()))
        return paths

    def get_action(self, observation):
        if self.refine is False:
            return self.policy.get_action(observation)
        return self.get_refined_action(observation)

    # ---- reward-based refinement around the policy (the reference's stub, model_accel_npg.py:191-196)
    def __getstate__(self):
        d = super(ModelAccelNPG, self).__getstate__()          # (device blocks stay with the process that made them)
        d["_refine_pack"], d["_refine_last"] = None, None
        return d

    def _refine_learned(self):
        return all(getattr(mdl, "learn_reward", False) for mdl in self.learned_model)

    def _refine_packed(self, dev):
        """the members' parameters and transforms on the device, packed once and again when a member changed
        (nn_dynamics.cached_members_pack, as MPCPolicy keeps its own copy), with the default bound vectors beside them"""
        def bounds(pk):
            n, m = pk["sizes"][-1], pk["sizes"][0] - pk["sizes"][-1]
            pk["bnd"], pk["bnd_value"] = rollout_bounds(n, m, dev, large_value=REFINE_LARGE_VALUE), REFINE_LARGE_VALUE

        self._refine_pack, fresh = cached_members_pack(self._refine_pack, self.learned_model, dev, self._refine_learned(), bounds)
        self._refine_packs += fresh
        return self._refine_pack[1]

    def invalidate(self):
        """drop the device copy of the members (after a write to ``p.data`` that went round this package's own functions)"""
        self._refine_pack = None

    def refine_route(self):
        """the route of the last refined call's rollout (2: the wide MFMA policy rollout for nets up to 256 wide, 1: the
        register-resident MFMA policy rollout, 0: the generic one); before any call, what the route functions answer for the
        policy and the members: ``mjx_policy_rollout_wide_route`` (served: 2) for the shapes ``sampling.wide_rollout_shape``
        sends to the wide entry, ``mjx_policy_rollout_route`` for the others and for a wide shape that is not served"""
        if self._refine_last is not None:
            return self._refine_last[2]
        net = self.learned_model[0].dynamics_net
        ds = tuple(net.layer_sizes)
        ps = (net.state_dim,) + tuple(self.policy.hidden_sizes) + (net.act_dim,)
        return predicted_route(load(), wide_rollout_shape(ps, ds), (), "mjx_policy_rollout_wide_route", "mjx_policy_rollout_route",
                               _ints(ps), len(ps), _ints(ds), len(ds))

    def last_scores(self):
        """(R, S) of the last refined call: the K N trajectory scores and their softmax weights (fp64, read back on demand)"""
        if self._refine_last is None:
            return None
        return self._refine_last[0].cpu().numpy(), self._refine_last[1].cpu().numpy()

    def get_refined_action(self, observation):
        """Roll ``plan_paths`` noisy policy trajectories of ``plan_horizon`` steps out from ``observation`` on every learned
        model and return the reward-weighted first action, as ``[action, {'mean': action, 'evaluation': action, 'log_std': ...}]``
        (the shape ``policy.get_action`` returns, so ``sample_paths`` and ``evaluate_policy`` take it).

        One call, with K = len(learned_model), N = plan_paths, H = plan_horizon:

        1. noise = ``draw_rollout_noise(1, H, N, m)`` from torch's global stream, SHARED by all members: every member starts
           from the same state with the same noise, so the first action of trajectory i is the same on every member and the
           members differ only in where their dynamics take it (as ``MPCPolicy``'s members share action sequences);
        2. ``mjx_policy_rollout`` (one launch; bounds +-1e2 as ``policy_rollout`` defaults; ``mjx_policy_rollout_wide`` for
           nets wider than its MFMA route takes, ``sampling.wide_rollout_shape``: :meth:`refine_route` is then 2);
        3. rewards: every member's reward net on the device (``mjx_path_rewards``, ``mjx_path_rewards_wide`` for dynamics nets
           wider than 128, ``nn_dynamics.wide_rows_shape``; nothing read back) when all members learn
           rewards, else one read-back and ``self.reward_function(dict(observations, actions))`` per member as ``train_step``
           calls it and one upload; with neither, ``ValueError``;
        4. ``mjx_plan_score`` with ``kappa``, ``refine_gamma`` and ``refine_omega`` (the per-trajectory disagreement term; off
           at 0) on member 0's actions widened to fp64;
        5. one read-back of row 0 of the weighted sequence: sum_i (sum_k S[k N + i]) a[i, 0] / (sum S + 1e-6).  Rows t >= 1 are
           member 0's later actions under the same weights; they are not used.

        ``termination_function`` and ensemble-disagreement truncation play no part: every trajectory counts for all H steps."""
        learned = self._refine_learned()
        if not learned and not callable(self.reward_function):
            raise ValueError("get_refined_action needs members that learn rewards (WorldModel(learn_reward=True)) or a reward_function")
        dev = _device()
        lib = load()
        pk = self._refine_packed(dev)
        net = self.learned_model[0].dynamics_net
        K, N, H, n, m = len(self.learned_model), int(self.plan_paths), int(self.plan_horizon), net.state_dim, net.act_dim
        st = _stream(dev)
        noise = draw_rollout_noise(1, H, N, m)[0]
        info = {}
        s0 = np.ascontiguousarray(np.asarray(observation).reshape(-1))
        obs_d, act_d = rollout_models_device(self.learned_model, self.policy, s0, H, noise, large_value=REFINE_LARGE_VALUE, num_traj=N,
                                             packed=pk, info=info)
        if learned:
            r_d = torch.empty((K, N, H), dtype=torch.float64, device=dev)
            path_rewards_call(pk["rew"], obs_d, act_d, False, N * H, K, None, r_d, dev, wide=True)
        else:
            obs_h, act_h = obs_d.cpu().numpy(), act_d.cpu().numpy()
            rewards = np.empty((K, N, H), np.float64)
            for k in range(K):
                rewards[k] = self.reward_function(dict(observations=obs_h[k], actions=act_h[k]))['rewards']
            r_d = torch.from_numpy(rewards).to(dev)
        a64 = torch.empty((N, H, m), dtype=torch.float64, device=dev)
        check(lib.mjx_cast_f32_f64(ptr(act_d), N * H * m, ptr(a64), st))
        out = torch.empty(H * m + 2 * K * N, dtype=torch.float64, device=dev)
        seq_d, R_d, S_d = out[:H * m], out[H * m:H * m + K * N], out[H * m + K * N:]
        omega = float(self.refine_omega)
        check(lib.mjx_plan_score(ptr(obs_d) if omega != 0.0 else None, ptr(r_d), ptr(a64), K, N, H, n, m, float(self.kappa),
                                 float(self.refine_gamma), omega, 1, ptr(R_d), ptr(S_d), ptr(seq_d), st))
        action = seq_d[:m].cpu().numpy()
        self._refine_last = (R_d, S_d, info["route"])
        return [action, {'mean': action, 'evaluation': action, 'log_std': self.policy.log_std_val}]
