"""fp64 NumPy restatement of the learned-reward chain (reference nn_dynamics.py:65-77, 149-164 over :230-245 and :313-328) and of
one MPCPolicy.get_action that plans on it, on top of tests/_dyn_oracle.py and tests/_mpc_oracle.py; and the cases the fixture
(tests/golden/make_golden_mpc_learned.py -> tests/golden/mpc_learned.npz), the CPU tests (tests/test_mpc_learned_cpu.py) and the
GPU worker (tests/_path_reward_worker.py) share.

What is rounded where, as in _mpc_oracle: the chain sees the fp32 parameters, transforms, observations and fp32-rounded actions
that the reference's torch code sees, but runs in fp64.  The reference computes s', the reward and (under NumPy 2, where a Python
float times an np.float32 stays fp32) each gamma**t * r in fp32: that is its distance from this restatement."""
import types

import numpy as np

import _dyn_oracle as O
import _mpc_oracle as M


def path_rewards(obs, act, dyn_theta, dyn_sizes, dyn_tr, dact, dflags, rew_theta, rew_sizes, rew_tr, ract):
    """one member's compute_path_rewards: obs (..., n), act (..., m) -> r (...) fp64.  s' = DynamicsNet(s, a) recomputed and
    unclamped, r = RewardNet(s, a, s') with its output affine (flags = AFF, no mask, no residual)"""
    obs, act = np.asarray(obs, np.float64), np.asarray(act, np.float64)
    lead = obs.shape[:-1]
    x = np.concatenate([obs.reshape(-1, obs.shape[-1]), act.reshape(-1, act.shape[-1])], 1)
    sp = O.forward(np.float32(dyn_theta), list(dyn_sizes), np.float32(dyn_tr), x, dact, dflags)
    r = O.forward(np.float32(rew_theta), list(rew_sizes), np.float32(rew_tr), np.concatenate([x, sp], 1), ract, O.AFF)
    return r[:, 0].reshape(lead)


def ensemble_rewards(obs, act, mem):
    """every member k on its own obs[k] and on act[k] or the shared act (one dimension less) -> (K, ...) fp64.
    mem: dict(dyn_thetas, dyn_sizes, dyn_trs, dact, dflags, rew_thetas, rew_sizes, rew_trs, ract)"""
    K = len(mem["dyn_thetas"])
    own = np.ndim(act) == np.ndim(obs)
    return np.stack([path_rewards(obs[k], act[k] if own else act, mem["dyn_thetas"][k], mem["dyn_sizes"], mem["dyn_trs"][k], mem["dact"],
                                  mem["dflags"], mem["rew_thetas"][k], mem["rew_sizes"], mem["rew_trs"][k], mem["ract"]) for k in range(K)])


def plan(s0, actions, mem, kappa, gamma, omega, reference_indexing=True, ensemble=True):
    """one get_action on learned rewards given its perturbed actions -> dict(obs, rewards, R, S, seq): _mpc_oracle.plan with the
    stand-in reward replaced by the members' reward nets (on the fp32-rounded actions, the reference's `.float()`)"""
    K = len(mem["dyn_thetas"])
    obs = M.rollout(s0, actions, mem["dyn_thetas"], mem["dyn_sizes"], mem["dyn_trs"], mem["dact"], mem["dflags"])
    a32 = np.asarray(actions, np.float32).astype(np.float64)
    rew = ensemble_rewards(obs, a32, mem)
    R = M.scores(obs, rew, omega, gamma, reference_indexing, ensemble)
    S = M.weights(R, kappa)
    return dict(obs=obs, rewards=rew, R=R, S=S, seq=M.sequence(S, actions, K))


def rel_max(got, ref):
    """the kernel tests' error: the largest absolute error over the rows relative to the largest absolute reward"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


# ---- the planner's stand-in environment on learned rewards: it has NO compute_path_rewards
def plan_env_no_rewards(n, m):
    return types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=types.SimpleNamespace()))


class CyclingInner:
    """the reference's only way to plan on learned rewards: env.env.env.compute_path_rewards hands the k-th call of each get_action
    to members[k % K].compute_path_rewards (MPCPolicy calls it once per member, in member order, model_learning_mpc.py:53-56)"""
    def __init__(self, members):
        self.members, self.calls = members, 0

    def compute_path_rewards(self, paths):
        self.members[self.calls % len(self.members)].compute_path_rewards(paths)
        self.calls += 1


def cycling_env(n, m, members):
    return types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=CyclingInner(members)))


# ---- planner cases of the fixture: name -> (N, H, kappa, omega, filter_coefs, gamma).  All on the same K = 3 fitted members,
# (n, m) = (6, 2), dynamics 64 x 64 ReLU residual, reward 100 x 100 (WorldModel's fixed reward widths).  A conditions cap keeps a
# comparison from being empty: 5 <= ESS <= 0.5 K N on every call (asserted by the generator); case "la" has omega = 0, so only the
# rewards move the weights.
PN, PM, PHID, PK = 6, 2, (64, 64), 3
PLAN_CASES = {
    "la": (256, 16, 8.0, 0.0, (0.5, 0.25, 0.8, 0.0), 0.95),
    "lb": (33, 5, 12.0, 5.0, (0.5, 0.25, 0.8, 0.0), 0.95),
}
CALLS = 3
DYN_SIZES = (PN + PM,) + PHID + (PN,)
REW_SIZES = (2 * PN + PM, 100, 100, 1)


def reward_fit_data(N, seed):
    """_mpc_oracle.fit_data with r = -mean(s'^2) - 0.1 mean(a^2)"""
    s, a, sp = M.fit_data(N, PN, PM, seed)
    r = (-np.mean(sp.astype(np.float64) ** 2, 1) - 0.1 * np.mean(a.astype(np.float64) ** 2, 1)).astype(np.float32).reshape(-1, 1)
    return s, a, sp, r


def call_obs(case, call):
    return np.random.RandomState(2000 + 10 * sorted(PLAN_CASES).index(case) + call).randn(PN) * 0.5


def reward_transforms(net):
    """a RewardNet's transforms in the kernels' layout: [in_shift (s, a, s), in_scale (s, a, s), out_shift, out_scale]"""
    f = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float32).ravel()
    return np.concatenate([f(net.s_shift), f(net.a_shift), f(net.s_shift), f(net.s_scale), f(net.a_scale), f(net.s_scale),
                           f(net.out_shift), f(net.out_scale)])


def fixture_members(G):
    """the oracle's view of the fixture's fitted members"""
    return dict(dyn_thetas=[G["m%d_dyn_params" % k] for k in range(PK)], dyn_sizes=DYN_SIZES,
                dyn_trs=[M.packed(G["m%d_dyn_tr" % k], PN, PM) for k in range(PK)], dact=0, dflags=7,
                rew_thetas=[G["m%d_rew_params" % k] for k in range(PK)], rew_sizes=REW_SIZES,
                rew_trs=[G["m%d_rew_tr" % k] for k in range(PK)], ract=0)


def load_members(WorldModel, torch, G):
    """WorldModel(learn_reward=True) instances carrying the fixture's parameters and transforms (either package's WorldModel)"""
    out = []
    for k in range(PK):
        wm = WorldModel(PN, PM, hidden_size=PHID, seed=70 + k, learn_reward=True)
        for net, th in ((wm.dynamics_net, G["m%d_dyn_params" % k]), (wm.reward_net, G["m%d_rew_params" % k])):
            ws, o = [], 0
            for p in net.parameters():
                ws.append(torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy())); o += p.numel()
            if net is wm.dynamics_net:
                tr = G["m%d_dyn_tr" % k]
                trl = [torch.from_numpy(tr[a:a + l].copy()) for a, l in zip(np.cumsum([0, PN, PN, PM, PM, PN]), [PN, PN, PM, PM, PN, PN])]
                net.set_params(dict(weights=ws, transforms=trl))
            else:
                rt = G["m%d_rew_tr" % k]
                rin = 2 * PN + PM
                for p, w in zip(net.parameters(), ws):
                    p.data = w
                net.set_transformations(torch.from_numpy(rt[:PN].copy()), torch.from_numpy(rt[rin:rin + PN].copy()),
                                        torch.from_numpy(rt[PN:PN + PM].copy()), torch.from_numpy(rt[rin + PN:rin + PN + PM].copy()),
                                        float(rt[2 * rin]), float(rt[2 * rin + 1]))
        out.append(wm)
    return out


# ---- kernel cases: the smallest shapes at which k_path_rewards can go wrong.  name -> (n, m, dynamics hidden, reward hidden,
# activation code, dynamics flags, K).  k1: the planner's shape; k2: padding in n8, m8, HB, both reward widths ragged (36 -> 64,
# 72 -> 96), tanh, not residual, one dynamics out_scale column below 1e-8 (the mask); k3: two state blocks (NB = 2), m8 = 16.
# k1, k2, k3 run the instances <2, 1, 4>, <3, 1, 4>, <1, 2, 4>; k4 .. k7 the other four, <2, 2, 4>, <3, 2, 4>, <4, 1, 2>, <4, 2, 2>,
# at shapes whose image fits (112.6, 133.8, 121.9 and 147.9 KiB), with unequal reward block counts (96 x 40: 3 and 2 blocks).
KCASES = {
    "k1": (6, 2, (64, 64), (100, 100), 0, 7, 3),
    "k2": (17, 6, (96, 32), (36, 72), 1, 3, 2),
    "k3": (33, 9, (32, 32), (100, 100), 0, 7, 1),
    "k4": (40, 5, (64, 64), (96, 40), 0, 7, 1),
    "k5": (33, 9, (96, 64), (64, 33), 0, 7, 1),
    "k6": (6, 2, (128, 128), (64, 64), 1, 7, 1),
    "k7": (33, 2, (128, 128), (32, 32), 0, 7, 1),
}
ROWSETS = ((33, 5), (6, 1))          # (N, H): 165 rows = five tiles and a partial one; 6 rows = under one tile
K2_MASKED = 3                        # k2's dynamics out_scale column that is 0


def _torch_like(rng, sizes):
    """nn.Linear's initial scale: uniform(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for W and b, flat in parameters() order"""
    out = []
    for i in range(len(sizes) - 1):
        b = 1.0 / np.sqrt(sizes[i])
        out += [rng.uniform(-b, b, sizes[i + 1] * sizes[i]), rng.uniform(-b, b, sizes[i + 1])]
    return np.concatenate(out).astype(np.float32)


def kernel_case(name):
    """seeded members and inputs of a kernel case -> (mem as ensemble_rewards takes it, {rowset: (obs (K, N, H, n), shared actions
    (N, H, m), per-member actions (K, N, H, m))}), all fp32"""
    n, m, dh, rh, act, flags, K = KCASES[name]
    rng = np.random.RandomState(700 + sorted(KCASES).index(name))
    ds, rs = (n + m,) + dh + (n,), (2 * n + m,) + rh + (1,)
    mem = dict(dyn_thetas=[], dyn_sizes=ds, dyn_trs=[], dact=act, dflags=flags, rew_thetas=[], rew_sizes=rs, rew_trs=[], ract=act)
    for _ in range(K):
        mem["dyn_thetas"].append(_torch_like(rng, ds))
        mem["rew_thetas"].append(_torch_like(rng, rs))
        dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
        if name == "k2":
            dtr[2 * (n + m) + n + K2_MASKED] = 0.0
        s_sh, s_sc, a_sh, a_sc = rng.randn(n) * 0.2, rng.rand(n) + 0.6, rng.randn(m) * 0.2, rng.rand(m) + 0.6
        rtr = np.concatenate([s_sh, a_sh, s_sh, s_sc, a_sc, s_sc, [rng.randn() * 0.5], [rng.rand() + 0.5]])
        mem["dyn_trs"].append(dtr.astype(np.float32))
        mem["rew_trs"].append(rtr.astype(np.float32))
    data = {}
    for N, H in ROWSETS:
        data[(N, H)] = (rng.randn(K, N, H, n).astype(np.float32), rng.randn(N, H, m).astype(np.float32),
                        rng.randn(K, N, H, m).astype(np.float32))
    return mem, data
