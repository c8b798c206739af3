#!/usr/bin/env python
"""Fixtures for MPC planning from the UNMODIFIED reference (mjrl/algos/model_accel/model_learning_mpc.py, sampling.py), run on
the CPU through _ref_import.  Per case of tests/_mpc_oracle.CASES three consecutive MPCPolicy.get_action calls under warm
start: the input act_sequence, the observation, the returned action, the new act_sequence, the scores R and their effective
sample size, a strided sample and the fp64 sums of the perturbed actions and of each member's observations, and the next
np.random.rand() after the call.  Members of cases a, b are fitted and stored; the others are WorldModels as initialised from
their seeds (a strided sample and the sum of each parameter vector are stored to prove the identity).  Also sample_paths and
evaluate_policy on a NumPy point mass with a linear stub policy.
    python tests/golden/make_golden_mpc.py      ->  tests/golden/mpc.npz
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
from mjrl.algos.model_accel import nn_dynamics, sampling  # noqa: E402
from mjrl.algos.model_accel.model_learning_mpc import MPCPolicy  # noqa: E402

import _mpc_oracle as M  # noqa: E402

torch.set_num_threads(1)
MIN_ESS = 5.0


def fitted_members(out):
    members = []
    for k in range(3):
        s, a, sp = M.fit_data(2000, 6, 2, 60 + k)
        np.random.seed(61 + k)
        wm = nn_dynamics.WorldModel(6, 2, hidden_size=(64, 64), seed=70 + k)
        wm.fit_dynamics(s, a, sp, 32, 5)
        out["fit_%d_params" % k] = M.flat_params(wm.dynamics_net)
        out["fit_%d_tr" % k] = M.flat_transforms(wm.dynamics_net)
        members.append(wm)
    return members


def main():
    out = {}
    fitted = fitted_members(out)
    for ci, case in enumerate(sorted(M.CASES)):
        n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
        members = fitted if case in M.FITTED else M.init_members(nn_dynamics.WorldModel, torch, case)
        if case not in M.FITTED:
            for k, wm in enumerate(members):
                th = M.flat_params(wm.dynamics_net)
                out["%s_m%d_psample" % (case, k)] = th[M.sample_idx(th.size)]
                out["%s_m%d_psum" % (case, k)] = np.float64(np.sum(th.astype(np.float64)))
        pol = MPCPolicy(env=M.plan_env(n, m), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc),
                        warmstart=True, fitted_model=members, omega=omega)
        cap = {}
        score = pol.score_trajectory_ensemble

        def rec(paths, paths_list, score=score, cap=cap):
            R = score(paths, paths_list)
            cap.update(R=R.copy(), actions=paths_list[0]["actions"].copy(), obs=[p["observations"].copy() for p in paths_list])
            return R

        pol.score_trajectory_ensemble = rec
        np.random.seed(500 + ci)
        for c in range(M.CALLS):
            key = "%s_%d_" % (case, c)
            o = M.call_obs(case, c, n)
            out[key + "seq_in"] = pol.act_sequence.copy()
            out[key + "obs"] = o
            out[key + "action"] = pol.get_action(o)
            out[key + "seq_out"] = pol.act_sequence.copy()
            out[key + "after"] = np.float64(np.random.rand())
            R = cap["R"]
            e = M.ess(M.weights(R, kappa))
            assert e >= MIN_ESS, (case, c, e)       # degenerate weights would make the comparison empty: lower kappa, not this
            out[key + "R"], out[key + "ess"] = R, np.float64(e)
            act = cap["actions"].ravel()
            out[key + "act_sample"], out[key + "act_sum"] = act[M.sample_idx(act.size)], np.float64(act.sum())
            obs = np.stack([x.ravel() for x in cap["obs"]])
            out[key + "obs_sample"] = obs[:, M.sample_idx(obs.shape[1])]
            out[key + "obs_sum"] = obs.astype(np.float64).sum(1)
            print("case %s call %d: ESS %.1f of %d, max |R| %.3g" % (case, c, e, K * N, np.max(np.abs(R))))
    for name, eval_mode, as_list in M.SAMPLE_RUNS:
        out.update(M.flatten_paths(name, *M.run_sample_paths(sampling.sample_paths, name, eval_mode, as_list)))
    for name, real_step, noise, as_list in M.EVAL_RUNS:
        out.update(M.flatten_paths(name, *M.run_evaluate_policy(sampling.evaluate_policy, name, real_step, noise, as_list)))
    path = os.path.join(HERE, "mpc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
