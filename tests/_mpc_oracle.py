"""fp64 NumPy restatement of one MPCPolicy.get_action (reference model_learning_mpc.py:42-99 over sampling.py:96-123, 204-215),
and the stand-ins the MPC fixtures and tests share (tests/golden/make_golden_mpc.py, tests/test_mpc_cpu.py,
tests/_mpc_worker.py).

What is rounded where: the rollout sees the fp32 parameters, transforms, start state and fp32-rounded actions the reference's
torch code sees (`.float()`), but runs in fp64; rewards, scores, weights and the weighted sequence use the fp64 actions, as in
the reference.  The reference itself computes the rollout, the reward's mean over fp32 observations and np.std of the fp32
predictions in fp32: that is its distance from this restatement."""
import types

import numpy as np

import _dyn_oracle as O


# ---- the planner
def perturbed_actions(num_traj, base_act, filter_coefs):
    """num_traj calls of generate_perturbed_actions (sampling.py:204-215), one after the other, from NumPy's global stream"""
    sigma, b0, b1, b2 = filter_coefs
    out = []
    for _ in range(num_traj):
        eps = np.random.normal(loc=0, scale=1.0, size=base_act.shape) * sigma
        eps = base_act + eps
        eps[0] = eps[0] * (b0 + b1 + b2)
        eps[1] = b0 * eps[1] + (b1 + b2) * eps[0]
        for i in range(2, eps.shape[0]):
            eps[i] = b0 * eps[i] + b1 * eps[i - 1] + b2 * eps[i - 2]
        out.append(eps)
    return np.array(out)


def rollout(s0, actions, thetas, sizes, trs, act, flags):
    """trajectory_rollout for every member -> (K, N, H, n) fp64; s0 (n) or (N, n); actions (N, H, m), rounded to fp32 here"""
    a32 = np.asarray(actions, np.float32).astype(np.float64)
    N, H = a32.shape[:2]
    s0 = np.asarray(s0, np.float32).astype(np.float64)
    if s0.ndim == 1:
        s0 = np.tile(s0, (N, 1))
    obs, _ = O.rollout(s0, H, None, None, None, None, [np.float32(t) for t in thetas], list(sizes), [np.float32(t) for t in trs],
                       act, flags, None, actions=a32)
    return obs


def path_rewards(obs, act):
    """the stand-in environment's reward: -mean(obs^2, -1) - 0.1 mean(act^2, -1)"""
    return -np.mean(np.asarray(obs, np.float64) ** 2, -1) - 0.1 * np.mean(np.asarray(act, np.float64) ** 2, -1)


def disagreement(obs):
    """model_learning_mpc.py:90-92: np.std over the members, summed over (t, j) -> (N,)"""
    return np.sum(np.std(np.asarray(obs, np.float64), axis=0), axis=(1, 2))


def scores(obs, rewards, omega, gamma, reference_indexing=True, ensemble=True):
    """:93-98 (ensemble) or :101-110 -> R (K N,)"""
    K, N, H = rewards.shape
    R = np.zeros(K * N)
    if ensemble:
        dis = disagreement(obs)
        idx = np.arange(K * N) // N if reference_indexing else np.arange(K * N) % N
        R += omega * dis[idx]
    r = np.asarray(rewards, np.float64).reshape(K * N, H)
    for t in range(H):
        R += (gamma ** t) * r[:, t]
    return R


def weights(R, kappa):
    return np.exp(kappa * (R - np.max(R)))


def sequence(S, actions, K):
    """:71-74 with paths['actions'] = the K members' copies of the same actions -> (H, m)"""
    act = np.concatenate([np.asarray(actions, np.float64)] * K, 0)
    return np.sum((S * act.T).T, axis=0) / (np.sum(S) + 1e-6)


def ess(S):
    return float(np.sum(S) ** 2 / np.sum(S ** 2))


def plan(s0, actions, thetas, sizes, trs, act, flags, kappa, gamma, omega, reference_indexing=True, ensemble=True):
    """one get_action given its perturbed actions -> dict(obs, rewards, R, S, seq)"""
    obs = rollout(s0, actions, thetas, sizes, trs, act, flags)
    rew = np.stack([path_rewards(obs[k], actions) for k in range(len(thetas))])
    R = scores(obs, rew, omega, gamma, reference_indexing, ensemble)
    S = weights(R, kappa)
    return dict(obs=obs, rewards=rew, R=R, S=S, seq=sequence(S, actions, len(thetas)))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- the planner's stand-in environment: env.env.env.compute_path_rewards(paths) is all MPCPolicy asks of it
class RewardInner:
    def compute_path_rewards(self, paths):
        paths["rewards"] = -np.mean(paths["observations"] ** 2, -1) - 0.1 * np.mean(paths["actions"] ** 2, -1)


def plan_env(n, m):
    return types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=RewardInner()))


# the cases of the fixture: name -> (n, m, hidden, K, N, H, kappa, omega, filter_coefs, activation, residual, gamma)
CASES = {
    "a": (6, 2, (64, 64), 3, 40, 8, 1.0, 5.0, (0.5, 0.25, 0.8, 0.0), "relu", True, 1.0),
    "b": (6, 2, (64, 64), 3, 256, 16, 5.0, 0.0, (1.0, 1.0, 0.0, 0.0), "relu", True, 0.95),
    "c": (17, 6, (128, 128), 3, 512, 32, 5.0, 5.0, (0.3, 0.25, 0.8, 0.0), "relu", True, 0.95),
    "d": (11, 2, (256, 256), 3, 200, 20, 10.0, 1.0, (0.3, 0.25, 0.8, 0.0), "relu", True, 0.95),
    "e": (39, 28, (64, 64), 3, 333, 12, 20.0, 2.0, (0.2, 0.25, 0.5, 0.25), "relu", True, 0.9),
    "f": (6, 2, (96, 32), 3, 70, 10, 3.0, 1.0, (0.4, 0.5, 0.5, 0.0), "relu", True, 0.95),
    "g": (6, 2, (32, 32), 1, 33, 5, 2.0, 5.0, (0.5, 1.0, 0.0, 0.0), "tanh", False, 0.95),
}
ROUTES = {"a": 1, "b": 1, "c": 1, "d": 0, "e": 1, "f": 1, "g": 1}
FITTED = ("a", "b")
CALLS = 3


def sample_idx(size, count=400):
    """the strided sample of a flat array the fixture keeps"""
    return np.arange(0, size, max(1, size // count))


def fit_data(N, n, m, seed):
    """cases a, b: sp = 0.8 s + 0.3 tanh([s, a] W)"""
    rng = np.random.RandomState(seed)
    s = rng.randn(N, n).astype(np.float32)
    a = rng.randn(N, m).astype(np.float32)
    W = rng.randn(n + m, n).astype(np.float32) * 0.5
    sp = (0.8 * s + 0.3 * np.tanh(np.concatenate([s, a], 1) @ W)).astype(np.float32)
    return s, a, sp


def call_obs(case, call, n):
    """the observation of call `call` of case `case`"""
    return np.random.RandomState(1000 + 10 * sorted(CASES).index(case) + call).randn(n) * 0.5


def init_members(WorldModel, torch, case):
    """cases c - g: the members AS INITIALISED from their seeds, with fixed transforms"""
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = CASES[case]
    out = []
    for k in range(K):
        wm = WorldModel(n, m, hidden_size=hid, seed=70 + k, activation=activation, residual=residual)
        wm.dynamics_net.set_transformations(torch.zeros(n), torch.ones(n), torch.zeros(m), torch.ones(m),
                                            torch.full((n,), -0.02), torch.full((n,), 0.3))
        out.append(wm)
    return out


def flat_params(net):
    return np.concatenate([p.detach().cpu().numpy().ravel() for p in net.parameters()])


def flat_transforms(net):
    return np.concatenate([np.asarray(t.detach().cpu().numpy(), np.float32).ravel() for t in net.get_params()["transforms"]])


def packed(tr, n, m):
    """get_params()['transforms'] order (s_shift, s_scale, a_shift, a_scale, out_shift, out_scale) -> the kernels' and the
    oracle's [in_shift (s, a), in_scale (s, a), out_shift, out_scale]"""
    s_sh, s_sc, a_sh, a_sc, o_sh, o_sc = np.split(np.asarray(tr), np.cumsum([n, n, m, m, n]))
    return np.concatenate([s_sh, a_sh, s_sc, a_sc, o_sh, o_sc])


# ---- sample_paths / evaluate_policy stand-ins: a NumPy point mass and a policy that is a fixed linear map
class PointMassInner:
    def __init__(self, outer):
        self.outer = outer
        self.np_random = np.random.RandomState(5)

    def set_fitted_state(self, s):
        self.outer.x = np.array(s, np.float64).ravel()

    def compute_path_rewards(self, path):
        path["rewards"] = -np.sum(path["observations"] ** 2, -1)


class PointMass:
    """x' = x + 0.1 a, r = -|x|^2, done when |x|_inf > limit; observation_dim = action_dim = 3"""
    def __init__(self, horizon=7, limit=1.2):
        self.horizon, self.limit = horizon, limit
        self.observation_dim = self.action_dim = 3
        self.rng = np.random.RandomState(0)
        self.x = np.zeros(3)
        self.env = types.SimpleNamespace(env=PointMassInner(self))

    def set_seed(self, seed=None):
        self.rng = np.random.RandomState(seed)

    def reset(self):
        self.x = self.rng.randn(3)
        return self.get_obs()

    def get_obs(self):
        return self.x.copy()

    def get_env_infos(self):
        return dict(norm=float(np.linalg.norm(self.x)), state=dict(x=self.x.copy()))

    def step(self, a):
        self.x = self.x + 0.1 * np.asarray(a, np.float64)
        done = bool(np.max(np.abs(self.x)) > self.limit)
        return self.get_obs(), -float(np.sum(self.x ** 2)), done, self.get_env_infos()


class LinearPolicy:
    A = np.array([[-0.5, 0.2, 0.0], [0.1, -0.7, 0.3], [0.4, 0.0, 0.9]])

    def __init__(self, as_list=False):
        self.as_list = as_list

    def get_action(self, o):
        a = self.A @ np.asarray(o, np.float64)
        return [a, dict(evaluation=0.5 * a)] if self.as_list else a


class LinearModel:
    def predict(self, o, a):
        return np.asarray(o) * 0.9 + 0.1 * np.asarray(a)


SAMPLE_RUNS = [("sp_eval_arr", True, False), ("sp_noisy_arr", False, False), ("sp_eval_list", True, True), ("sp_noisy_list", False, True)]
EVAL_RUNS = [("ev_model_noise", False, 0.1, False), ("ev_real", True, 0.0, False), ("ev_model_list", False, 0.0, True)]


def run_sample_paths(sample_paths, name, eval_mode, as_list):
    np.random.seed(300)
    paths = sample_paths(4, lambda: PointMass(), LinearPolicy(as_list), horizon=6, eval_mode=eval_mode, base_seed=11, noise_level=0.3)
    return paths, np.random.rand()


def run_evaluate_policy(evaluate_policy, name, real_step, noise_level, as_list):
    e = PointMass()
    e.set_seed(12)
    paths = evaluate_policy(e, LinearPolicy(as_list), LinearModel(), noise_level=noise_level, real_step=real_step, num_episodes=3)
    return paths, e.env.env.np_random.rand()


def flatten_paths(prefix, paths, after):
    """paths -> fixture entries"""
    out = {prefix + "_count": np.int64(len(paths)), prefix + "_after": np.float64(after)}
    for i, p in enumerate(paths):
        out["%s_%d_keys" % (prefix, i)] = np.array(sorted(p.keys()))
        for key in ("observations", "actions", "rewards"):
            out["%s_%d_%s" % (prefix, i, key)] = np.asarray(p[key])
        if "terminated" in p:
            out["%s_%d_terminated" % (prefix, i)] = np.bool_(p["terminated"])
        out["%s_%d_info_norm" % (prefix, i)] = np.asarray(p["env_infos"]["norm"])
        out["%s_%d_info_x" % (prefix, i)] = np.asarray(p["env_infos"]["state"]["x"])
        out["%s_%d_info_keys" % (prefix, i)] = np.array(sorted(p["env_infos"].keys()) + sorted(p["env_infos"]["state"].keys()))
    return out
