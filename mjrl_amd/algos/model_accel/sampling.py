"""Rollouts on learned models, on the GPU.

Mirrors ``mjrl.algos.model_accel.sampling`` (reference sampling.py): ``policy_rollout`` and ``trajectory_rollout`` run as
ONE persistent launch (``mjx_model_rollout``, csrc/dynamics.h) in which each workgroup walks a tile of trajectories of one
ensemble member through all H steps: policy mean, + noise * exp(log_std), action clamp, dynamics, state clamp.  The noise
is the reference's: ``torch.randn((N, m))`` once per step, drawn on the host from torch's global stream in the same order
(:func:`draw_rollout_noise`) and uploaded once, so the noisy rollouts see the same numbers.  Both rollouts read the members as
``nn_dynamics.pack_dynamics_members`` packs them and their bounds as :func:`rollout_bounds` forms them.  Real-environment sampling
(``sample_paths``, ``evaluate_policy``) are host loops around ``policy.get_action`` -- for an
:class:`~mjrl_amd.algos.model_accel.model_learning_mpc.MPCPolicy` that call is where the GPU work happens.
"""
import ctypes

import numpy as np
import torch

from ..._lib import check, load, ptr
from .nn_dynamics import _device, _f32, _ints, _stream, pack_dynamics_members, wide_entry


def _as_env(env, env_kwargs=None):
    if type(env) == str:
        from mjrl.utils.gym_env import GymEnv
        return GymEnv(env)
    if hasattr(env, 'reset') and hasattr(env, 'horizon'):
        return env
    if callable(env):
        return env(**(env_kwargs or {}))
    print("Unsupported environment format")
    raise AttributeError


def draw_rollout_noise(num_models, horizon, num_traj, act_dim):
    """the reference's draws for `num_models` consecutive noisy policy_rollout calls: torch.randn((N, m)) per step
    (sampling.py:73) -> (K, H, N, m) fp32 CPU tensor"""
    return torch.stack([torch.stack([torch.randn((num_traj, act_dim)) for _ in range(horizon)]) if horizon > 0
                        else torch.zeros((0, num_traj, act_dim)) for _ in range(num_models)])


def _bound(v, dim, default):
    if v is None:
        v = default
    if isinstance(v, torch.Tensor):
        v = v.detach().to('cpu', torch.float32).reshape(-1)
        return v.expand(dim).contiguous() if v.numel() == 1 else v
    return torch.full((dim,), float(v), dtype=torch.float32)


def rollout_models(models, policy, init_states, horizon, noise=None, s_min=None, s_max=None, a_min=None, a_max=None,
                   large_value=float(1e2), actions=None):
    """K learned models (WorldModel) from the same N initial states in one launch -> (obs (K, N, H, n), act (K, N, H, m))
    as NumPy fp32.  noise: (K, H, N, m) or None (eval_mode); actions (N, H, m): trajectory_rollout (no policy, no clamp)."""
    dev = _device()
    net0 = models[0].dynamics_net
    n, m = net0.state_dim, net0.act_dim
    K = len(models)
    s0 = _f32(init_states, dev).reshape(-1, n)
    N = s0.shape[0]
    H = int(horizon)
    pk = pack_dynamics_members(models, dev)
    sizes, P, tr, act, flags = pk["sizes"], pk["P"], pk["tr"], pk["act"], pk["flags"]
    obs = torch.empty((K, N, H, n), dtype=torch.float32, device=dev)
    act_out = torch.empty((K, N, H, m), dtype=torch.float32, device=dev)
    lib = load()
    if actions is None:
        pol_sizes = (n,) + tuple(policy.hidden_sizes) + (m,)
        pol_P = _f32(policy.get_param_values(), dev)
        pol_tr = _f32(policy.model.packed_transforms(), dev)
        nz = None if noise is None else _f32(noise, dev)
        bnd = rollout_bounds(n, m, dev, s_min, s_max, a_min, a_max, large_value)
        check(lib.mjx_model_rollout(ptr(s0), N, H, K, _ints(pol_sizes), len(pol_sizes), ptr(pol_P), ptr(pol_tr), ptr(nz), None,
                                    _ints(sizes), len(sizes), ptr(P), ptr(tr), act, flags, ptr(bnd[0]), ptr(bnd[1]),
                                    ptr(bnd[2]), ptr(bnd[3]), ptr(obs), ptr(act_out), _stream(dev)))
    else:
        ad = _f32(actions, dev).reshape(N, H, m)
        check(lib.mjx_model_rollout(ptr(s0), N, H, K, None, 0, None, None, None, ptr(ad), _ints(sizes), len(sizes), ptr(P),
                                    ptr(tr), act, flags, None, None, None, None, ptr(obs), ptr(act_out), _stream(dev)))
    return obs.cpu().numpy(), act_out.cpu().numpy()


def rollout_bounds(n, m, dev, s_min=None, s_max=None, a_min=None, a_max=None, large_value=float(1e2)):
    """[a_min, a_max, s_min, s_max] as fp32 device vectors (m, m, n, n); None = -/+ large_value (enforce_tensor_bounds)"""
    return [_bound(a_min, m, -large_value).to(dev), _bound(a_max, m, large_value).to(dev),
            _bound(s_min, n, -large_value).to(dev), _bound(s_max, n, large_value).to(dev)]


def wide_rollout_shape(pol_sizes, dyn_sizes):
    """whether :func:`rollout_models_device` hands a (policy, dynamics) pair to ``mjx_policy_rollout_wide``: both nets with two
    hidden layers and a dynamics width above 128 or a policy width above 64 -- wider than anything the register-resident route
    of ``mjx_policy_rollout`` takes.  Plain Python, no library call; narrower on purpose than what the wide kernel serves
    (``mjx_policy_rollout_wide_route``): the shapes that have a route today keep their call."""
    if len(pol_sizes) != 4 or len(dyn_sizes) != 4:
        return False
    return max(dyn_sizes[1:3]) > 128 or max(pol_sizes[1:3]) > 64


def rollout_models_device(models, policy, s0, horizon, noise=None, s_min=None, s_max=None, a_min=None, a_max=None,
                          large_value=float(1e2), num_traj=None, packed=None, info=None):
    """The policy on K learned models in one ``mjx_policy_rollout`` launch (``mjx_policy_rollout_wide`` with the same arguments
    where :func:`wide_rollout_shape` says so), results left on the device
    -> (obs (K, N, H, n), act (K, N, H, m)) fp32 device tensors.

    s0: one state (n,) for every trajectory, or (N, n).  noise: (H, N, m) shared by all members, (K, H, N, m), or None
    (eval mode).  N comes from s0, else from the noise, else from ``num_traj``.  ``packed``: the members already on the device
    (``nn_dynamics.pack_dynamics_members``; with ``bnd`` / ``bnd_value`` also the default bound vectors, ``rollout_bounds``);
    otherwise they are flattened and uploaded here.  The policy's parameters and transforms are uploaded on every call.
    ``info`` (a dict) receives ``route``: 2 = the wide MFMA rollout (csrc/policy_rollout_wide.h: nets up to 256 wide),
    1 = the register-resident MFMA rollout (csrc/policy_rollout.h), 0 = the generic persistent rollout."""
    dev = _device()
    net0 = models[0].dynamics_net
    n, m = net0.state_dim, net0.act_dim
    K, H = len(models), int(horizon)
    if packed is None:
        packed = pack_dynamics_members(models, dev)
    sizes = tuple(packed["sizes"])
    assert (sizes[0], sizes[-1]) == (n + m, n) and packed["P"].shape[0] == K
    s0_d = _f32(s0, dev)
    nz = None if noise is None else _f32(noise, dev)
    if s0_d.dim() == 2:
        N = s0_d.shape[0]
    elif nz is not None:
        N = nz.shape[-2]
    else:
        N = int(num_traj)
    assert tuple(s0_d.shape) in ((n,), (N, n)), "s0 is one state (n) or one per trajectory (N, n)"
    if nz is not None:
        assert tuple(nz.shape) in ((H, N, m), (K, H, N, m)), "noise is (H, N, m) or (K, H, N, m)"
    pol_sizes = (n,) + tuple(policy.hidden_sizes) + (m,)
    pol_P = _f32(policy.get_param_values(), dev)
    pol_tr = _f32(policy.model.packed_transforms(), dev)
    if a_min is None and a_max is None and s_min is None and s_max is None and packed.get("bnd_value") == large_value:
        bnd = packed["bnd"]                               # the default +-large_value blocks, already on the device
    else:
        bnd = rollout_bounds(n, m, dev, s_min, s_max, a_min, a_max, large_value)
    obs = torch.empty((K, N, H, n), dtype=torch.float32, device=dev)
    act_out = torch.empty((K, N, H, m), dtype=torch.float32, device=dev)
    route = ctypes.c_int(-1)
    lib = load()
    entry = wide_entry(lib, "policy_rollout", wide_rollout_shape(pol_sizes, sizes))
    check(entry(ptr(s0_d), n if s0_d.dim() == 2 else 0, N, H, K, _ints(pol_sizes), len(pol_sizes), ptr(pol_P),
                ptr(pol_tr), ptr(nz), H * N * m if (nz is not None and nz.dim() == 4) else 0, _ints(sizes),
                len(sizes), ptr(packed["P"]), ptr(packed["tr"]), packed["act"], packed["flags"], ptr(bnd[0]),
                ptr(bnd[1]), ptr(bnd[2]), ptr(bnd[3]), ptr(obs), ptr(act_out), ctypes.byref(route), _stream(dev)))
    if info is not None:
        info["route"] = route.value
    return obs, act_out


def pack_rollouts_device(obs_d, act_d, rew_d, err_d=None, lim=0.0, min_len=4, truncate_reward=0.0, obs64=True, tpos=True):
    """model_accel_npg.py:149-155 for every path at once, on the device (``mjx_rollout_pack``, csrc/rollout_batch.h): obs_d (..., H, n),
    act_d (..., H, m) fp32, rew_d (..., H) fp32 or fp64, err_d (P, H - 1) fp32 (``rollout_disagreement_device``) or None (nothing is
    truncated) -> dict(off (P + 1) int64, first (P) int32, term (P) uint8, obs (P H, n) fp32, act (P H, m) fp32, rew (P H) fp64,
    obs64 (P H, n) fp64 or None, tpos (P H) int32 or None), all on the device; rows [0, off[P]) hold the packed batch."""
    dev = obs_d.device
    n, m, H = obs_d.shape[-1], act_d.shape[-1], obs_d.shape[-2]
    assert obs_d.is_cuda and obs_d.dtype == act_d.dtype == torch.float32 and rew_d.dtype in (torch.float32, torch.float64)
    assert obs_d.shape[:-1] == act_d.shape[:-1] == rew_d.shape and H >= 1
    obs_d, act_d, rew_d = obs_d.contiguous(), act_d.contiguous(), rew_d.contiguous()
    P = rew_d.numel() // H
    assert err_d is None or (err_d.dtype == torch.float32 and err_d.is_contiguous() and err_d.numel() == P * (H - 1))
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)        # noqa: E731
    out = dict(off=new((P + 1,), torch.int64), first=new((P,), torch.int32), term=new((P,), torch.uint8), obs=new((P * H, n), torch.float32),
               act=new((P * H, m), torch.float32), rew=new((P * H,), torch.float64),
               obs64=new((P * H, n), torch.float64) if obs64 else None, tpos=new((P * H,), torch.int32) if tpos else None)
    r32 = rew_d.dtype == torch.float32
    check(load().mjx_rollout_pack(ptr(obs_d), ptr(act_d), ptr(rew_d) if r32 else None, None if r32 else ptr(rew_d), ptr(err_d), P, H, n, m,
                                  float(lim), int(min_len), float(truncate_reward), ptr(out["off"]), ptr(out["first"]), ptr(out["term"]),
                                  ptr(out["obs"]), ptr(out["act"]), ptr(out["rew"]), ptr(out["obs64"]), ptr(out["tpos"]), _stream(dev)))
    return out


# ===========================================================
# Rollout parameteric policy on learned env to collect data
# ===========================================================

def policy_rollout(
        num_traj,
        env,
        policy,
        learned_model,
        init_state=None,
        eval_mode=False,
        horizon=1e6,
        env_kwargs=None,
        seed=None,
        s_min=None,
        s_max=None,
        a_min=None,
        a_max=None,
        large_value=float(1e2),
        ):
    """sampling.py:16-89: same arguments, same draws, same (num_traj, horizon, dim) outputs"""
    env = _as_env(env, env_kwargs)
    if seed is not None:
        env.set_seed(seed)
        torch.manual_seed(seed)
    if init_state is None:
        st = np.array([env.reset() for _ in range(num_traj)])
    elif type(init_state) == np.ndarray:
        st = init_state
    elif type(init_state) == list:
        st = np.array(init_state)
    elif type(init_state) == torch.Tensor:
        assert init_state.device == 'cpu'
        st = init_state
    else:
        raise TypeError("Unsupported format for init state")
    horizon = min(horizon, env.horizon)
    m = learned_model.dynamics_net.act_dim
    noise = None if eval_mode is True else draw_rollout_noise(1, int(horizon), int(np.shape(st)[0]), m)
    obs, act = rollout_models([learned_model], policy, st, horizon, noise, s_min, s_max, a_min, a_max, large_value)
    return dict(observations=obs[0], actions=act[0])


# ===========================================================
# Rollout action sequences on the learned model
# ===========================================================

def trajectory_rollout(actions, learned_model, init_states):
    """sampling.py:96-123"""
    actions = np.array(actions) if type(actions) == list else actions
    num_traj, horizon = actions.shape[0], actions.shape[1]
    if len(init_states.shape) == 1:
        init_states = np.tile(init_states, (num_traj, 1))
    obs, _ = rollout_models([learned_model], None, init_states, horizon, actions=actions)
    return dict(observations=obs[0], actions=actions)


# ===========================================================
# Rollout policy (parametric or implicit MPC) on real env
# ===========================================================

def stack_tensor_dict_list(tensor_dict_list):
    """mjrl.utils.tensor_utils.stack_tensor_dict_list: a list of (nested) dicts -> a (nested) dict of np.array(list)"""
    out = dict()
    for k in list(tensor_dict_list[0].keys()):
        vals = [x[k] for x in tensor_dict_list]
        out[k] = stack_tensor_dict_list(vals) if isinstance(tensor_dict_list[0][k], dict) else np.array(vals)
    return out


def sample_paths(num_traj,
                 env,
                 policy,  # mpc policy on fitted model
                 horizon=1e6,
                 eval_mode=True,
                 base_seed=None,
                 noise_level=0.1,
                 ):
    """sampling.py:131-184: num_traj episodes of `policy` on the real environment.  Exploration noise (eval_mode False, array
    actions) is np.random.uniform from NumPy's global stream; a list-valued get_action is [action, {'evaluation': ...}]."""
    env = _as_env(env)
    if base_seed is not None:
        env.set_seed(base_seed)
    horizon = min(horizon, env.horizon)
    paths = []
    for ep in range(num_traj):
        env.reset()
        observations, actions, rewards, env_infos = [], [], [], []
        t, done = 0, False
        while t < horizon and done is False:
            obs = env.get_obs()
            ifo = env.get_env_infos()
            act = policy.get_action(obs)
            if eval_mode is False and type(act) != list:
                act = act + np.random.uniform(low=-noise_level, high=noise_level, size=act.shape[0])
            if type(act) == list:
                act = act[0] if eval_mode is False else act[1]['evaluation']
            next_obs, reward, done, _ = env.step(act)
            t = t + 1
            observations.append(obs)
            actions.append(act)
            rewards.append(reward)
            env_infos.append(ifo)
        paths.append(dict(observations=np.array(observations), actions=np.array(actions), rewards=np.array(rewards),
                          terminated=done, env_infos=stack_tensor_dict_list(env_infos)))
    return paths


# ===========================================================
# Utility functions
# ===========================================================

def discount_sum(x, gamma, discounted_terminal=0.0):
    """sampling.py:191-201: y[t] = x[t] + gamma * y[t + 1], y[T] = discounted_terminal"""
    out, acc = [0.0] * len(x), discounted_terminal
    for t in reversed(range(len(x))):
        acc = x[t] + gamma * acc
        out[t] = acc
    return np.array(out)


def generate_perturbed_actions(base_act, filter_coefs):
    """sampling.py:204-215: base + sigma * N(0, 1) noise (NumPy's global stream), smoothed by a 3-tap recursive filter"""
    sigma, b0, b1, b2 = filter_coefs
    u = base_act + np.random.normal(loc=0, scale=1.0, size=base_act.shape) * sigma
    u[0] = u[0] * (b0 + b1 + b2)
    u[1] = b0 * u[1] + (b1 + b2) * u[0]
    for t in range(2, u.shape[0]):
        u[t] = b0 * u[t] + b1 * u[t - 1] + b2 * u[t - 2]
    return u


def generate_paths(num_traj, learned_model, start_state, base_act, filter_coefs, base_seed=None):
    """sampling.py:218-232"""
    if base_seed is not None:
        np.random.seed(base_seed)
    act = np.array([generate_perturbed_actions(base_act, filter_coefs) for _ in range(num_traj)])
    return trajectory_rollout(act, learned_model, start_state)


def evaluate_policy(e, policy, learned_model, noise_level=0.0,
                    real_step=False, num_episodes=10, visualize=False):
    """sampling.py:235-283: roll `policy` out on e -- on the real simulator (real_step) or by setting the learned model's
    prediction as the simulator's state -- and record the paths.  Noise is e.env.env.np_random.uniform."""
    paths = []
    for ep in range(num_episodes):
        e.reset()
        observations, actions, rewards, env_infos = [], [], [], []
        t, done = 0, False
        while t < e.horizon and done is False:
            o = e.get_obs()
            ifo = e.get_env_infos()
            a = policy.get_action(o)
            if type(a) == list:
                a = a[1]['evaluation']
            if noise_level > 0.0:
                a = a + e.env.env.np_random.uniform(low=-noise_level, high=noise_level, size=a.shape[0])
            if real_step is False:
                next_s = learned_model.predict(o, a)
                r = 0.0                                 # (filled in by compute_path_rewards below)
                e.env.env.set_fitted_state(next_s)
            else:
                next_o, r, done, ifo2 = e.step(a)
                ifo = ifo2 if ifo == {} else ifo
            if visualize:
                e.render()
            t = t + 1
            observations.append(o)
            actions.append(a)
            rewards.append(r)
            env_infos.append(ifo)
        path = dict(observations=np.array(observations), actions=np.array(actions), rewards=np.array(rewards),
                    env_infos=stack_tensor_dict_list(env_infos))
        if real_step is False:
            e.env.env.compute_path_rewards(path)
            try:
                path = e.env.env.truncate_paths([path])[0]
            except Exception:
                pass
        paths.append(path)
        if visualize:
            print("episode score = %f " % np.sum(path['rewards']))
    return paths


def enforce_tensor_bounds(torch_tensor, min_val=None, max_val=None, large_value=float(1e4), device=None):
    """sampling.py:286-315: clamp to Box[min_val, max_val] (scalars or (B,) tensors; None = -/+ large_value)"""
    min_val = -large_value if min_val is None else min_val
    max_val = large_value if max_val is None else max_val
    device = torch_tensor.data.device if device is None else device
    assert type(min_val) == float or type(min_val) == torch.Tensor
    assert type(max_val) == float or type(max_val) == torch.Tensor
    lo = min_val if type(min_val) == torch.Tensor else torch.tensor(min_val)
    hi = max_val if type(max_val) == torch.Tensor else torch.tensor(max_val)
    for b in (lo, hi):
        if len(b.shape) > 0:
            assert b.shape[-1] == torch_tensor.shape[-1]
    return torch.max(torch.min(torch_tensor, hi.to(device)), lo.to(device))
