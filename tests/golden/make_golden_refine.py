#!/usr/bin/env python
"""Fixtures for the policy rollout on learned models and for ModelAccelNPG.get_refined_action from the UNMODIFIED reference
(mjrl/algos/model_accel/sampling.py, nn_dynamics.py, mjrl/policies/gaussian_mlp.py), run on the CPU through _ref_import.

The reference leaves get_refined_action a stub with its intent in a comment (model_accel_npg.py:191-196).  What it does have is
every piece: per member `policy_rollout(..., init_state=np.tile(obs, (N, 1)), horizon=H, seed=s)` -- the seed argument reseeds
torch for each member, so all members see the same noise -- and `model.compute_path_rewards(rollouts)`.  This generator calls
those and adds its own few NumPy lines: the discounted returns R (plus omega times the per-trajectory disagreement), the softmax
weights S and the weighted first action.  Members are _mpc_learned_oracle's (fitted as make_golden_mpc_learned.py fits them);
cases and calls are _refine_oracle.RCASES.  Stored per call: obs, the members' rollouts and fp32 rewards, R, the effective sample
size of S, the action and torch's next randn after the call; members and policy once.  The generator asserts
5 <= ESS <= 0.5 K N on every call.

Also the yardsticks of the kernel tests: per case of _refine_oracle.KCASES the reference's own fp32 rollout -- policy.model.forward,
+ noise * exp(log_std), enforce_tensor_bounds, learned_model.forward, enforce_tensor_bounds, on the case's seeded nets, start
states and noise -- measured exactly as the GPU worker measures the kernel: _refine_oracle.step_errors on its stored states and
actions ("kya_<case>", "kys_<case>"), and for the free-running case its distance from the fp64 free-running rollout
("kfree_obs", "kfree_act").
    python tests/golden/make_golden_refine.py      ->  tests/golden/refine.npz
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
from mjrl.policies.gaussian_mlp import MLP  # noqa: E402

import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
import _refine_oracle as F  # noqa: E402
from make_golden_model_accel import StandInEnv  # noqa: E402
from make_golden_mpc_learned import fitted_members  # noqa: E402

torch.set_num_threads(1)
MIN_ESS = 5.0


def reference_case(c):
    """a kernel case as the reference's own MLP policy and DynamicsNets"""
    n, m = c["n"], c["m"]
    pol = MLP(types.SimpleNamespace(observation_dim=n, action_dim=m), hidden_sizes=tuple(c["pol_sizes"][1:-1]), seed=1)
    pol.set_param_values(c["pol_theta"].copy())
    ptr = c["pol_tr"]
    pol.model.set_transformations(ptr[:n], ptr[n:2 * n], ptr[2 * n:2 * n + m], ptr[2 * n + m:])
    dyns = []
    for k in range(c["K"]):
        dyn = nn_dynamics.DynamicsNet(n, m, tuple(c["dyn_sizes"][1:-1]), residual=bool(c["flags"] & 4), use_mask=bool(c["flags"] & 2))
        th, o = c["dyn_thetas"][k], 0
        for p in dyn.parameters():
            p.data = torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy()); o += p.numel()
        if c["act"] == 1:
            dyn.nonlinearity = torch.tanh
        dtr, din = c["dyn_trs"][k], n + m
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
        dyn.set_transformations(t(dtr[:n]), t(dtr[din:din + n]), t(dtr[n:din]), t(dtr[din + n:2 * din]), t(dtr[2 * din:2 * din + n]),
                                t(dtr[2 * din + n:]))
        dyn._apply_out_transforms = bool(c["flags"] & 1)
        dyns.append(dyn)
    return pol, dyns


def reference_rollout(c):
    """the reference's fp32 steps (sampling.py:70-80) on the case's inputs -> obs (K, N, H, n), act (K, N, H, m) fp32"""
    pol, dyns = reference_case(c)
    nz, b = F.case_noise_members(c), c["bounds"]
    tb = None if b is None else [torch.from_numpy(v) for v in b]
    obs, act = [], []
    with torch.no_grad():
        for k, dyn in enumerate(dyns):
            st = torch.from_numpy(F.case_s0_rows(c).copy())
            ok, ak = [], []
            for t in range(c["H"]):
                at = pol.model.forward(st)
                if nz is not None:
                    at = at + torch.from_numpy(nz[k, t]) * torch.exp(pol.log_std)
                if tb is not None:
                    at = sampling.enforce_tensor_bounds(at, tb[0], tb[1])
                stp1 = dyn.forward(st, at)
                if tb is not None:
                    stp1 = sampling.enforce_tensor_bounds(stp1, tb[2], tb[3])
                ok.append(st.numpy().copy()); ak.append(at.numpy().copy())
                st = stp1
            obs.append(np.swapaxes(np.array(ok), 0, 1)); act.append(np.swapaxes(np.array(ak), 0, 1))
    return np.stack(obs), np.stack(act)


def kernel_yardsticks(out):
    for name in sorted(F.KCASES):
        c = F.kernel_case(name)
        obs, act = reference_rollout(c)
        out["kya_" + name], out["kys_" + name] = (np.float64(v) for v in F.step_errors(c, obs, act))
        print("kernel case %s: the reference's fp32 steps are %.3e (action) and %.3e (state) from fp64" %
              (name, out["kya_" + name], out["kys_" + name]))
        if c["bounds"] is not None:
            print("     clamped shares of the fp64 rollout: %.2f of the actions, %.2f of the states" % F.clamped_shares(c, *F.free_rollout(c)))
    c = F.kernel_case(F.FREE_CASE, F.FREE_H)
    obs, act = reference_rollout(c)
    o64, a64 = F.free_rollout(c)
    out["kfree_obs"], out["kfree_act"] = np.float64(F.rel_max(obs, o64)), np.float64(F.rel_max(act, a64))
    print("free-running %s at H = %d: the reference's fp32 rollout is %.3e (states) and %.3e (actions) from fp64" %
          (F.FREE_CASE, F.FREE_H, out["kfree_obs"], out["kfree_act"]))


def main():
    out = {}
    members = fitted_members(out)
    for ci, case in enumerate(sorted(F.RCASES)):
        N, H, ph, kappa, omega, gamma = F.RCASES[case]
        env = StandInEnv(L.PN, L.PM, 1000)
        pol = MLP(env.spec, hidden_sizes=ph, seed=F.POL_SEED, init_log_std=F.INIT_LOG_STD)
        out[case + "_pol_params"] = pol.get_param_values()
        for call in range(F.RCALLS):
            key = "%s_%d_" % (case, call)
            o, seed = F.rcall_obs(case, call), F.rcall_seed(case, call)
            rolls = []
            for mdl in members:
                r = sampling.policy_rollout(N, env, pol, mdl, init_state=np.tile(o, (N, 1)), horizon=H, seed=seed)
                mdl.compute_path_rewards(r)
                rolls.append(r)
            after = torch.randn(1).item()
            obs, act = np.stack([r["observations"] for r in rolls]), np.stack([r["actions"] for r in rolls])
            rew = np.stack([np.asarray(r["rewards"]) for r in rolls])
            assert obs.dtype == act.dtype == rew.dtype == np.float32 and rew.shape == (L.PK, N, H)
            assert all(np.array_equal(act[k, :, 0], act[0, :, 0]) for k in range(L.PK))          # shared noise, shared start
            # the generator's own lines: R, S and the weighted first action
            R = np.zeros(L.PK * N)
            if omega != 0.0:
                dis = np.sum(np.std(obs.astype(np.float64), axis=0), axis=(1, 2))
                R += omega * np.tile(dis, L.PK)
            for t in range(H):
                R += (gamma ** t) * rew.reshape(L.PK * N, H)[:, t].astype(np.float64)
            S = np.exp(kappa * (R - np.max(R)))
            w = S.reshape(L.PK, N).sum(0)
            action = (w[:, None] * act[0, :, 0].astype(np.float64)).sum(0) / (np.sum(S) + 1e-6)
            e = M.ess(S)
            assert MIN_ESS <= e <= 0.5 * L.PK * N, (case, call, e)
            out[key + "obs"], out[key + "seed"], out[key + "after"] = o, np.int64(seed), np.float64(after)
            out[key + "roll_obs"], out[key + "roll_act"], out[key + "rewards"] = obs, act, rew
            out[key + "R"], out[key + "ess"], out[key + "action"] = R, np.float64(e), action
            print("case %s call %d: ESS %.1f of %d, R spread %.3g, max |R| %.3g, action %s" %
                  (case, call, e, L.PK * N, np.ptp(R), np.max(np.abs(R)), action))
    kernel_yardsticks(out)
    path = os.path.join(HERE, "refine.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
