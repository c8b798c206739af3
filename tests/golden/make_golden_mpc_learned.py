#!/usr/bin/env python
"""Fixtures for MPC planning on LEARNED rewards from the UNMODIFIED reference (mjrl/algos/model_accel/model_learning_mpc.py,
nn_dynamics.py), run on the CPU through _ref_import.

The reference's MPCPolicy asks env.env.env.compute_path_rewards for the rewards, once per member in member order; the stand-in
environment behind it hands the k-th call of each get_action to members[k % K].compute_path_rewards (_mpc_learned_oracle.CyclingInner),
which is WorldModel.compute_path_rewards, the learned-reward chain.  Members are reference WorldModel(learn_reward=True)
instances, fitted briefly with fit_dynamics and fit_reward(..., set_transformations=False) (True reads r_shift unbound, as
make_golden_model_accel.py notes; the reward nets' input transforms are set from the data before the fit instead) on
_mpc_oracle.fit_data with r = -mean(s'^2) - 0.1 mean(a^2).  Stored: both nets' parameters and transforms per member; per case of
_mpc_learned_oracle.PLAN_CASES and call (three warm-started calls) seq_in, the observation, the action, seq_out, the scores R, their
effective sample size, each member's (N, H) fp32 rewards, the distance of those rewards from the fp64 chain on the same fp32 rows
("pref") and the next np.random.rand().  The generator asserts 5 <= ESS <= 0.5 K N
on every call.

Also the yardstick of the kernel tests: per case of _mpc_learned_oracle.KCASES the reference's own fp32 result
(DynamicsNet.forward, RewardNet.forward on the CPU) on the seeded inputs against the fp64 restatement, measured as the GPU worker
measures the kernel: per row set and action mode the largest |error| over all members' rows relative to the largest |reward| over
the same rows, and the largest of those ("kref_<case>").
    python tests/golden/make_golden_mpc_learned.py      ->  tests/golden/mpc_learned.npz
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

_ref_import.install()
sys.modules.setdefault("mjrl.envs", types.ModuleType("mjrl.envs"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mjrl.algos.model_accel import nn_dynamics  # noqa: E402
from mjrl.algos.model_accel.model_learning_mpc import MPCPolicy  # noqa: E402

import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402

torch.set_num_threads(1)
MIN_ESS = 5.0


def fitted_members(out):
    members = []
    for k in range(L.PK):
        s, a, sp, r = L.reward_fit_data(2000, 60 + k)
        np.random.seed(61 + k)
        wm = nn_dynamics.WorldModel(L.PN, L.PM, hidden_size=L.PHID, seed=70 + k, learn_reward=True)
        wm.fit_dynamics(s, a, sp, 32, 5)
        st, at, rt = torch.from_numpy(s), torch.from_numpy(a), torch.from_numpy(r)
        s_shift, a_shift = torch.mean(st, dim=0), torch.mean(at, dim=0)
        s_scale, a_scale = torch.mean(torch.abs(st - s_shift), dim=0), torch.mean(torch.abs(at - a_shift), dim=0)
        r_shift = torch.mean(rt, dim=0)
        r_scale = torch.mean(torch.abs(rt - r_shift), dim=0)
        wm.reward_net.set_transformations(s_shift, s_scale, a_shift, a_scale, float(r_shift), float(r_scale))
        wm.fit_reward(s, a, r, 32, 5, set_transformations=False)
        out["m%d_dyn_params" % k] = M.flat_params(wm.dynamics_net)
        out["m%d_dyn_tr" % k] = M.flat_transforms(wm.dynamics_net)
        out["m%d_rew_params" % k] = M.flat_params(wm.reward_net)
        out["m%d_rew_tr" % k] = L.reward_transforms(wm.reward_net)
        members.append(wm)
    return members


def reference_nets(mem, k, n, m, dh, rh, act, flags):
    """member k of a kernel case as the reference's own DynamicsNet and RewardNet"""
    dyn = nn_dynamics.DynamicsNet(n, m, dh, residual=bool(flags & 4))
    rew = nn_dynamics.RewardNet(n, m, hidden_size=rh)
    for net, th in ((dyn, mem["dyn_thetas"][k]), (rew, mem["rew_thetas"][k])):
        o = 0
        for p in net.parameters():
            p.data = torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy()); o += p.numel()
        if act == 1:
            net.nonlinearity = torch.tanh
    dtr, rtr, din, rin = mem["dyn_trs"][k], mem["rew_trs"][k], n + m, 2 * n + m
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    dyn.set_transformations(t(dtr[:n]), t(dtr[din:din + n]), t(dtr[n:din]), t(dtr[din + n:2 * din]), t(dtr[2 * din:2 * din + n]),
                            t(dtr[2 * din + n:]))
    rew.set_transformations(t(rtr[:n]), t(rtr[rin:rin + n]), t(rtr[n:din]), t(rtr[rin + n:rin + din]), float(rtr[2 * rin]),
                            float(rtr[2 * rin + 1]))
    return dyn, rew


def kernel_yardsticks(out):
    """exactly what the GPU worker measures of the kernel, measured of the reference: per row set and action mode the K members'
    fp32 rewards (K, N, H) against _mpc_learned_oracle.ensemble_rewards through _mpc_learned_oracle.rel_max -- the largest error over
    all members' rows relative to the largest |reward| over the same rows -- and the largest of those over the case"""
    for name in sorted(L.KCASES):
        n, m, dh, rh, act, flags, K = L.KCASES[name]
        mem, data = L.kernel_case(name)
        nets = [reference_nets(mem, k, n, m, dh, rh, act, flags) for k in range(K)]
        worst = 0.0
        for (N, H), (obs, shared, own) in data.items():
            for acts in (shared, own):
                r32 = []
                for k, (dyn, rew) in enumerate(nets):
                    s = torch.from_numpy(obs[k].reshape(-1, n))
                    a = torch.from_numpy(np.ascontiguousarray((acts if acts.ndim == 3 else acts[k]).reshape(-1, m)))
                    with torch.no_grad():
                        r32.append(rew.forward(s, a, dyn.forward(s, a).detach().clone()).numpy()[:, 0].reshape(N, H))
                worst = max(worst, L.rel_max(np.stack(r32), L.ensemble_rewards(obs, acts, mem)))
        out["kref_" + name] = np.float64(worst)
        print("kernel case %s: the reference's fp32 chain is %.3e from fp64" % (name, worst))


def main():
    out = {}
    members = fitted_members(out)
    for ci, case in enumerate(sorted(L.PLAN_CASES)):
        N, H, kappa, omega, fc, gamma = L.PLAN_CASES[case]
        env = L.cycling_env(L.PN, L.PM, members)
        pol = MPCPolicy(env=env, plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc), warmstart=True,
                        fitted_model=members, omega=omega)
        cap = {}
        score = pol.score_trajectory_ensemble

        def rec(paths, paths_list, score=score, cap=cap):
            R = score(paths, paths_list)
            cap.update(R=R.copy(), rewards=np.stack([p["rewards"].copy() for p in paths_list]),
                       obs=np.stack([p["observations"].copy() for p in paths_list]), actions=paths_list[0]["actions"].copy())
            return R

        pol.score_trajectory_ensemble = rec
        np.random.seed(900 + ci)
        for c in range(L.CALLS):
            key = "%s_%d_" % (case, c)
            o = L.call_obs(case, c)
            out[key + "seq_in"] = pol.act_sequence.copy()
            out[key + "obs"] = o
            out[key + "action"] = pol.get_action(o)
            out[key + "seq_out"] = pol.act_sequence.copy()
            out[key + "after"] = np.float64(np.random.rand())
            R = cap["R"]
            e = M.ess(M.weights(R, kappa))
            assert env.env.env.calls == L.PK * (c + 1)
            assert cap["rewards"].dtype == np.float32 and cap["rewards"].shape == (L.PK, N, H)
            # neither degenerate nor flat: lower or raise kappa, not these
            assert MIN_ESS <= e <= 0.5 * L.PK * N, (case, c, e)
            out[key + "R"], out[key + "ess"], out[key + "rewards"] = R, np.float64(e), cap["rewards"]
            # the reference's own fp32 reward chain against the fp64 chain on the SAME rows (its own fp32 observations and actions):
            # the yardstick of a kernel-only comparison on this call's inputs, measured as the kernel cases' is
            assert cap["obs"].dtype == np.float32
            a32 = np.asarray(cap["actions"], np.float32)
            out[key + "pref"] = np.float64(L.rel_max(cap["rewards"], L.ensemble_rewards(cap["obs"], a32, L.fixture_members(out))))
            print("     the reference's fp32 rewards are %.3e from fp64 on the same rows" % float(out[key + "pref"]))
            print("case %s call %d: ESS %.1f of %d, R spread %.3g, max |R| %.3g" % (case, c, e, L.PK * N, np.ptp(R), np.max(np.abs(R))))
    kernel_yardsticks(out)
    path = os.path.join(HERE, "mpc_learned.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
