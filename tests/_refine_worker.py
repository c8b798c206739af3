"""GPU worker of tests/test_gpu_refine.py: every check of ModelAccelNPG.get_refined_action in one process; prints one RESULT
line (JSON)."""
import os
import pickle
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build()
from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG  # noqa: E402
from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel  # noqa: E402
from mjrl_amd.algos.model_accel.sampling import draw_rollout_noise  # noqa: E402
from mjrl_amd.baselines.linear_baseline import LinearBaseline  # noqa: E402
from mjrl_amd.policies.gaussian_mlp import MLP  # noqa: E402
import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
import _refine_oracle as F  # noqa: E402
from tests._worker_dev import emit, switch  # noqa: E402

torch.cuda.set_device(0)
G = np.load(os.path.join(ROOT, "tests", "golden", "refine.npz"))
SPEC = types.SimpleNamespace(observation_dim=L.PN, action_dim=L.PM, horizon=6)


def agent_for(case, members, **kw):
    N, H, ph, kappa, omega, gamma = F.RCASES[case]
    pol = MLP(SPEC, hidden_sizes=tuple(ph), seed=F.POL_SEED, init_log_std=F.INIT_LOG_STD)
    pol.set_param_values(G[case + "_pol_params"].copy())
    args = dict(learned_model=members, env=None, policy=pol, baseline=LinearBaseline(SPEC), normalized_step_size=0.05, seed=1, refine=True,
                kappa=kappa, plan_horizon=H, plan_paths=N, refine_gamma=gamma, refine_omega=omega)
    args.update(kw)
    return ModelAccelNPG(**args), pol


def main():
    res = dict(fixture={}, routes={}, after={})
    members = L.load_members(WorldModel, torch, G)
    # ---- against the fixture, call by call, on both routes
    for case in sorted(F.RCASES):
        for mfma in ("1", "0"):
            with switch("MJX_POLICY_ROLLOUT_MFMA", mfma):
                agent, pol = agent_for(case, members)
                for c in range(F.RCALLS):
                    key = "%s_%d_" % (case, c)
                    torch.manual_seed(int(G[key + "seed"]))
                    out = agent.get_action(G[key + "obs"])
                    after = torch.randn(1).item()
                    assert type(out) == list and set(out[1]) == {"mean", "evaluation", "log_std"} and out[0].shape == (L.PM,)
                    R, S = agent.last_scores()
                    res["fixture"]["%s%s_%d" % (case, mfma, c)] = [M.rel_l2(out[0], G[key + "action"]),
                                                                   float(np.max(np.abs(R - G[key + "R"])) / np.max(np.abs(G[key + "R"])))]
                    res["after"]["%s%s_%d" % (case, mfma, c)] = after == float(G[key + "after"])
                    res["routes"]["%s%s_%d" % (case, mfma, c)] = agent.refine_route()
                if case == "ra" and mfma == "1":
                    res["packs_two_calls"] = agent._refine_packs
    # ---- rewards from a host callable: the same rewards (the fp64 chain, member by member) give the same action
    case = "ra"
    N, H, ph, kappa, omega, gamma = F.RCASES[case]
    mem = L.fixture_members(G)
    plain = []
    for k, wm in enumerate(members):
        w2 = WorldModel(L.PN, L.PM, hidden_size=L.PHID, seed=70 + k, learn_reward=False)
        w2.dynamics_net = wm.dynamics_net
        plain.append(w2)
    calls = [0]

    def reward_function(paths):
        k = calls[0] % L.PK
        calls[0] += 1
        paths["rewards"] = L.path_rewards(paths["observations"], paths["actions"], mem["dyn_thetas"][k], mem["dyn_sizes"], mem["dyn_trs"][k],
                                          mem["dact"], mem["dflags"], mem["rew_thetas"][k], mem["rew_sizes"], mem["rew_trs"][k], mem["ract"])
        return paths

    agent, pol = agent_for(case, plain, reward_function=reward_function)
    key = case + "_0_"
    torch.manual_seed(int(G[key + "seed"]))
    out = agent.get_action(G[key + "obs"])
    torch.manual_seed(int(G[key + "seed"]))
    noise = draw_rollout_noise(1, H, N, L.PM)[0].numpy()
    pol_tr = np.concatenate([np.zeros(L.PN), np.ones(L.PN), np.zeros(L.PM), np.ones(L.PM)])
    r64 = F.refined(G[key + "obs"], noise, G[case + "_pol_params"], (L.PN,) + tuple(ph) + (L.PM,), pol_tr, mem, kappa, gamma, omega)
    res["callable"] = [M.rel_l2(out[0], r64["action"]), calls[0]]
    agent, pol = agent_for(case, plain)
    try:
        agent.get_action(G[key + "obs"])
        res["neither"] = "no error"
    except ValueError:
        res["neither"] = "ValueError"
    # ---- pack key: packed again after a member's fit_dynamics and after a fit_reward; the policy is read on every call
    agent, pol = agent_for(case, members)
    torch.manual_seed(3)
    a0 = agent.get_action(G[key + "obs"])[0]
    torch.manual_seed(3)
    a1 = agent.get_action(G[key + "obs"])[0]
    packs = [agent._refine_packs]
    s, a, sp, r = L.reward_fit_data(64, 5)
    np.random.seed(6)
    members[0].fit_dynamics(s, a, sp, 32, 1)
    torch.manual_seed(3)
    a2 = agent.get_action(G[key + "obs"])[0]
    packs.append(agent._refine_packs)
    members[1].fit_reward(s, a, r, 32, 1, set_transformations=False)
    torch.manual_seed(3)
    a3 = agent.get_action(G[key + "obs"])[0]
    packs.append(agent._refine_packs)
    pol.set_param_values(pol.get_param_values() + np.float32(0.05))
    torch.manual_seed(3)
    a4 = agent.get_action(G[key + "obs"])[0]
    packs.append(agent._refine_packs)
    res["packs"] = packs
    res["same_call_same_action"] = bool(np.array_equal(a0, a1))
    res["moved"] = [float(np.max(np.abs(a2 - a1))), float(np.max(np.abs(a3 - a2))), float(np.max(np.abs(a4 - a3)))]
    # ---- unchanged neighbours: refine=False, a train_step after a refined call, a pickle after a call
    agent.refine = False
    np.random.seed(9)
    g = agent.get_action(G[key + "obs"])
    np.random.seed(9)
    w = pol.get_action(G[key + "obs"])
    res["unrefined"] = bool(np.array_equal(g[0], w[0]) and np.array_equal(g[1]["mean"], w[1]["mean"]))
    agent.refine = True
    rng = np.random.RandomState(4)
    env = types.SimpleNamespace(reset=lambda: rng.randn(L.PN) * 0.5, horizon=6, observation_dim=L.PN, action_dim=L.PM)
    torch.manual_seed(12)
    stats = agent.train_step(8, env=env, init_states=[rng.randn(L.PN) * 0.5 for _ in range(8)])
    res["train_step"] = bool(np.all(np.isfinite(np.asarray(stats, np.float64))))
    q = pickle.loads(pickle.dumps(agent))
    res["pickle"] = bool(q._refine_pack is None and q._refine_last is None and q.refine is True)
    torch.manual_seed(3)
    res["pickle_acts"] = bool(np.all(np.isfinite(q.get_action(G[key + "obs"])[0])))
    emit(res)


if __name__ == "__main__":
    main()
