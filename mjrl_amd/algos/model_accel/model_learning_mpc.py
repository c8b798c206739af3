"""MPC planning on learned-model ensembles, on the GPU.

Mirrors ``mjrl.algos.model_accel.model_learning_mpc`` (reference model_learning_mpc.py:5-110): ``MPCPolicy`` with the same
constructor arguments, attributes and ``get_action`` semantics, the warm-start shift included.  One ``get_action`` is

1. ``plan_paths`` perturbed action sequences from NumPy's global stream: one ``np.random.normal(size=(N, H, m))`` and the
   three-tap filter vectorised over N, which gives the numbers of the reference's N ``generate_perturbed_actions`` calls bit
   for bit and leaves the stream where they leave it;
2. one upload of the fp64 actions, cast to fp32 on the device (the reference's ``.float()``);
3. ``mjx_plan_rollout``: all K members in one launch (csrc/plan.h; the register-resident MFMA rollout where the net's shape
   allows it -- ``mjx_plan_route`` -- and the generic persistent rollout otherwise).  With ``wide=True`` members with two
   hidden layers and a dynamics width above 128 (``nn_dynamics.wide_rows_shape``; 256 x 256 is the reference's own configs) go
   to ``mjx_plan_rollout_wide`` instead: the same arguments, the wide MFMA rollout of csrc/plan_wide.h (route 2), and on
   ``reward='learned'`` ``mjx_path_rewards_wide`` (csrc/rows_wide.h).  ``MJX_PLAN_WIDE=0`` / ``MJX_PATH_REWARDS_WIDE=0`` make
   those calls the narrow entries, bit for bit.  ``wide`` is False by default: a planner built as before makes the calls and
   reports the routes it did before (``route()`` is 0 on a 256-wide ensemble), although the wide route is the faster one
   there;
4. one read-back of the (K, N, H, n) observations and K calls of ``env.env.env.compute_path_rewards(paths)``, the reference's
   reward contract, which stays a host callback: it gets a dict of that member's fp32 observations and the fp64 actions;
5. one upload of the (K, N, H) rewards, ``mjx_plan_score`` (disagreement, discounted returns, softmax weights and the weighted
   sequence in fp64), one read-back of the (H, m) sequence.

The members' parameters and transforms are packed on the device once per planner and again when a member changed.  The cache is
``nn_dynamics.cached_members_pack`` (``ModelAccelNPG``'s refinement keeps its copy through the same function) and its key is
``nn_dynamics.members_pack_key``, which says what it sees.  A write to ``p.data`` from outside the package is the one change it
cannot see: :meth:`MPCPolicy.invalidate`.

``fitted_model`` is a list of ``WorldModel`` (a list of one works: its disagreement is 0) or a bare ``WorldModel``.  For a
bare model the reference raises ``TypeError`` (it calls ``generate_paths(fitted_model=...)``, which has no such argument);
this class does what that branch evidently intends: the same draws, one rollout, ``score_trajectory`` (no disagreement term).

``reward='learned'`` (the reference's driver switches to learned rewards where the environment has no reward function,
run_model_accel_npg.py:106-108; its MPCPolicy has no such switch): steps 4 and 5 become ``mjx_path_rewards`` -- every member's
``WorldModel.compute_path_rewards`` on its own device observations and the shared fp32 actions, written as fp64
(csrc/path_reward.h) -- and ``mjx_plan_score``: one upload of the actions, three device calls, one read-back of (H, m).  The
environment is never asked for rewards, so it needs no ``compute_path_rewards``.

``reference_indexing``: score_trajectory_ensemble adds ``disagreement[i // num_traj]`` (model_learning_mpc.py:95), which is
the MEMBER index of row i, so the disagreement of trajectories 0 .. K-1 is what every member's rows get.  True (default)
reproduces that; False uses the evidently intended per-trajectory index ``i % num_traj``.
"""
import ctypes

import numpy as np
import torch

from ..._lib import check, load, ptr
from .nn_dynamics import (_device, _ints, _stream, cached_members_pack, members_pack_key, path_rewards_call, predicted_route, wide_entry,
                          wide_rows_shape)


def perturbed_action_batch(num_traj, base_act, filter_coefs):
    """num_traj consecutive generate_perturbed_actions(base_act, filter_coefs) calls (sampling.py:204-215) as one draw
    -> (num_traj, H, m) fp64.  normal(size=(N, H, m)) consumes the stream exactly as N draws of (H, m) do."""
    sigma, b0, b1, b2 = filter_coefs
    eps = np.random.normal(loc=0, scale=1.0, size=(int(num_traj),) + base_act.shape) * sigma
    u = base_act + eps
    u[:, 0] = u[:, 0] * (b0 + b1 + b2)
    u[:, 1] = b0 * u[:, 1] + (b1 + b2) * u[:, 0]
    for t in range(2, u.shape[1]):
        u[:, t] = b0 * u[:, t] + b1 * u[:, t - 1] + b2 * u[:, t - 2]
    return u


class MPCPolicy(object):
    reward = 'env'              # (an instance pickled before the keyword existed plans as it did)
    _routes = None
    wide = False                # (an instance pickled before the keyword existed plans as it did)

    def __init__(self, env,
                 plan_horizon,
                 plan_paths=10,
                 kappa=1.0,
                 gamma=1.0,
                 mean=None,
                 filter_coefs=None,
                 seed=123,
                 warmstart=True,
                 fitted_model=None,
                 omega=5.0,
                 reference_indexing=True,
                 reward='env',
                 wide=False,
                 **kwargs,
                 ):
        """Arguments as in the reference (model_learning_mpc.py:6-40), plus reference_indexing, reward ('env': the
        environment's compute_path_rewards on the host; 'learned': the members' reward nets on the device; module docstring) and
        wide (True: ensembles wider than 128 plan on the wide MFMA entries; module docstring, step 3)."""
        self.env, self.seed = env, seed
        self.n, self.m = env.observation_dim, env.action_dim
        self.plan_horizon, self.num_traj = plan_horizon, plan_paths
        if fitted_model is None:
            print("Policy requires a fitted dynamics model")
            raise SystemExit
        self.fitted_model = fitted_model
        self.mean, self.filter_coefs, self.kappa, self.gamma = mean, filter_coefs, kappa, gamma
        if mean is None:
            self.mean = np.zeros(self.m)
        if filter_coefs is None:
            self.filter_coefs = [np.ones(self.m), 1.0, 0.0, 0.0]
        self.act_sequence = np.ones((self.plan_horizon, self.m)) * self.mean
        self.init_act_sequence = self.act_sequence.copy()
        self.warmstart = warmstart
        self.omega = omega
        self.reference_indexing = reference_indexing
        if reward not in ('env', 'learned'):
            raise ValueError("reward is 'env' or 'learned'")
        if reward == 'learned' and not all(getattr(mdl, "learn_reward", False) for mdl in self._members()):
            raise ValueError("reward='learned' needs every member to be a WorldModel(learn_reward=True)")
        self.reward = reward
        self.wide = bool(wide)
        self._pack = None           # (key, device blocks) of the members' parameters and transforms
        self._last = None           # device blocks of the last call's scores (and, on learned rewards, the rewards)
        self._routes = None         # the routes the last call's entries reported

    # ---- device state
    def __getstate__(self):
        d = dict(self.__dict__)
        d["_pack"], d["_last"], d["_routes"] = None, None, None
        return d

    def _members(self):
        return self.fitted_model if type(self.fitted_model) == list else [self.fitted_model]

    def _pack_key(self, dev):
        """(key, held tensors) of the members' device copy: ``nn_dynamics.members_pack_key``, the reward nets too on reward='learned'"""
        return members_pack_key(self._members(), dev, self.reward == 'learned')

    def _dims_are_the_envs(self, pk):
        net0 = self._members()[0].dynamics_net
        assert (net0.state_dim, net0.act_dim) == (self.n, self.m), "the models' dims are not the environment's"

    def _packed(self, dev):
        self._pack, _ = cached_members_pack(self._pack, self._members(), dev, self.reward == 'learned', self._dims_are_the_envs)
        return self._pack[1]

    def invalidate(self):
        """drop the device copy of the members (after a write to ``p.data`` that went round this package's own functions)"""
        self._pack = None

    def _wide(self):
        """whether these members go to the ``_wide`` entries: asked for (``wide=True``) and ``nn_dynamics.wide_rows_shape`` (plain
        Python, narrower than the kernels)"""
        return self.wide and wide_rows_shape(tuple(self._members()[0].dynamics_net.layer_sizes))

    def route(self):
        """2: the wide MFMA rollout serves these members (mjx_plan_rollout_wide_route, asked for the shapes :meth:`_wide` sends
        there, with MJX_PLAN_WIDE and MJX_PLAN_MFMA as they stand now), 1: the register-resident MFMA rollout, 0: the generic
        rollout (mjx_plan_route)"""
        sizes = tuple(self._members()[0].dynamics_net.layer_sizes)
        return predicted_route(load(), self._wide(), ("MJX_PLAN_WIDE", "MJX_PLAN_MFMA"), "mjx_plan_rollout_wide_route", "mjx_plan_route",
                               _ints(sizes), len(sizes), int(self.m))

    # ---- the planner
    def get_action(self, obs):
        ensemble = type(self.fitted_model) == list
        dev = _device()
        lib = load()
        pk = self._packed(dev)
        K, N, H, n, m = len(self._members()), int(self.num_traj), int(self.plan_horizon), int(self.n), int(self.m)
        actions = perturbed_action_batch(N, self.act_sequence, self.filter_coefs)
        st = _stream(dev)
        a64 = torch.from_numpy(np.ascontiguousarray(actions)).to(dev)
        a32 = torch.empty((N, H, m), dtype=torch.float32, device=dev)
        check(lib.mjx_cast_f64_f32(ptr(a64), N * H * m, ptr(a32), st))
        s0 = np.asarray(obs)
        s0_d = torch.from_numpy(np.ascontiguousarray(s0)).to(dev, torch.float32)
        assert s0.shape in ((n,), (N, n)), "obs is one state (n) or one per trajectory (N, n)"
        obs_d = torch.empty((K, N, H, n), dtype=torch.float32, device=dev)
        roll_args = (ptr(s0_d), 0 if s0.ndim == 1 else n, N, H, K, ptr(a32), _ints(pk["sizes"]), len(pk["sizes"]),
                     ptr(pk["P"]), ptr(pk["tr"]), pk["act"], pk["flags"], ptr(obs_d))
        wide = self._wide()
        route = ctypes.c_int(-1)
        tail = (ctypes.byref(route), st) if wide else (st,)  # (the narrow entry takes no route pointer and reports none: route())
        check(wide_entry(lib, "plan_rollout", wide)(*roll_args, *tail))
        routes = dict(rollout=route.value if wide else None, rewards=None)
        if self.reward == 'learned':
            # r = RewardNet_k(s, a, DynamicsNet_k(s, a)) on the device, widened to fp64 for the scoring
            r_d = torch.empty((K, N, H), dtype=torch.float64, device=dev)
            routes["rewards"] = path_rewards_call(pk["rew"], obs_d, a32, True, N * H, K, None, r_d, dev, wide=self.wide)
        else:
            obs_h = obs_d.cpu().numpy()
            rewards = np.empty((K, N, H), np.float64)
            for k in range(K):
                paths = dict(observations=obs_h[k], actions=actions)
                self.env.env.env.compute_path_rewards(paths)        # populates paths['rewards']
                rewards[k] = paths["rewards"]
            r_d = torch.from_numpy(rewards).to(dev)
        out = torch.empty(H * m + 2 * K * N, dtype=torch.float64, device=dev)
        seq_d, R_d, S_d = out[:H * m], out[H * m:H * m + K * N], out[H * m + K * N:]
        check(lib.mjx_plan_score(ptr(obs_d) if ensemble else None, ptr(r_d), ptr(a64), K, N, H, n, m, float(self.kappa),
                                 float(self.gamma), float(self.omega), 0 if self.reference_indexing else 1, ptr(R_d), ptr(S_d),
                                 ptr(seq_d), st))
        act_sequence = seq_d.cpu().numpy().reshape(H, m)
        self._last = (R_d, S_d, r_d if self.reward == 'learned' else None)
        self._routes = routes
        action = act_sequence[0].copy()
        if self.warmstart:
            self.act_sequence[:-1] = act_sequence[1:]
            self.act_sequence[-1] = self.mean.copy()
        else:
            self.act_sequence = self.init_act_sequence.copy()
        return action

    def last_scores(self):
        """(R, S) of the last get_action: the K N trajectory scores and their softmax weights (fp64, read back on demand)"""
        if self._last is None:
            return None
        return self._last[0].cpu().numpy(), self._last[1].cpu().numpy()

    def last_rewards(self):
        """the (K, N, H) learned rewards of the last get_action (the fp32 net outputs as fp64, read back on demand); None on
        reward='env', where the rewards were the environment's"""
        if self._last is None or self._last[2] is None:
            return None
        return self._last[2].cpu().numpy()

    def last_routes(self):
        """dict(rollout=..., rewards=...) of the last get_action: the routes its entries reported (2 wide MFMA, 1 register-resident
        MFMA, 0 generic; ``rewards`` None on reward='env', ``rollout`` None where the members went to ``mjx_plan_rollout``, which
        reports none: :meth:`route`); None before the first call"""
        return None if self._routes is None else dict(self._routes)

    def reward_route(self):
        """2: the wide MFMA path-reward kernel serves these members (mjx_path_rewards_wide_route, asked for the shapes
        ``nn_dynamics.wide_rows_shape`` sends there, with MJX_PATH_REWARDS_WIDE and MJX_PATH_REWARDS_MFMA as they stand now), 1: the
        register-resident one, 0: the generic route (mjx_path_rewards_route); None on reward='env'"""
        if self.reward != 'learned':
            return None
        mdl = self._members()[0]
        ds, rs = tuple(mdl.dynamics_net.layer_sizes), tuple(mdl.reward_net.layer_sizes)
        return predicted_route(load(), self.wide and wide_rows_shape(ds, rs), ("MJX_PATH_REWARDS_WIDE", "MJX_PATH_REWARDS_MFMA"),
                               "mjx_path_rewards_wide_route", "mjx_path_rewards_route", _ints(ds), len(ds), _ints(rs), len(rs))

    # ---- the reference's scoring functions, in NumPy, for callers that use them
    def score_trajectory_ensemble(self, paths, paths_list):
        """model_learning_mpc.py:85-99; the same per-score summation order (omega * disagreement first, then t ascending)"""
        total_traj, horizon = paths['rewards'].shape[0], paths['rewards'].shape[1]
        predictions = [p['observations'] for p in paths_list]
        disagreement = np.std(predictions, axis=0)
        disagreement = np.sum(disagreement, axis=(1, 2))
        idx = np.arange(total_traj) // self.num_traj if self.reference_indexing else np.arange(total_traj) % self.num_traj
        scores = np.zeros(total_traj)
        scores += self.omega * disagreement[idx]
        for t in range(horizon):
            scores += (self.gamma ** t) * paths["rewards"][:, t]
        return scores

    def score_trajectory(self, paths):
        """model_learning_mpc.py:101-110"""
        num_traj, horizon = paths["rewards"].shape[0], paths["rewards"].shape[1]
        scores = np.zeros(num_traj)
        for t in range(horizon):
            scores += (self.gamma ** t) * paths["rewards"][:, t]
        return scores
