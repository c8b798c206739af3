#!/usr/bin/env python
"""Yardsticks of the wide plan rollout's tests (tests/test_gpu_plan_wide.py) from the UNMODIFIED reference, run on the CPU through
_ref_import: per case of _plan_wide_cases.CASES the reference's own fp32 rollout -- its DynamicsNet
(mjrl/algos/model_accel/nn_dynamics.py:166-245) stepped by its trajectory_rollout (sampling.py:96-123), one call per member as
model_learning_mpc.py:53-56 makes them -- on the seeded inputs against the same fp64 oracle, measured with the functions the GPU
worker measures the kernel with (_plan_wide_cases.step_error, free_error):
    pstep_<case>   every case with H > 1 but f1: the per-column one-step error, every state the reference stored against one fp64
                   step (_dyn_oracle.rollout_next) from the state and action IT stored before; the largest over columns, members and
                   the case's s0 modes
    pfree_f1       the same measure against the free-running fp64 rollout (_mpc_oracle.rollout) over 16 steps
and for the end-to-end check the reference's own fp32 planner -- its MPCPolicy on _plan_wide_cases.mpc_members' seeded 256 x 256
members, driven as make_golden_mpc.py / make_golden_mpc_learned.py drive it (the stand-in environment's reward, or
_mpc_learned_oracle.CyclingInner handing the k-th call to member k's compute_path_rewards) -- against the fp64 oracle on the same
perturbed actions (_plan_wide_cases.mpc_oracle):
    mpc_R, mpc_seq           on learned rewards: the scores max-relative, the planned sequence relative L2
    mpc_R_env, mpc_seq_env   on the environment's rewards
The generator asserts an effective sample size of 5 .. 0.5 K N for both.  float64 scalars, nothing else.

The reference expresses every case without a changed line, as make_golden_plan_matrix.py says: the activation is net.nonlinearity,
the flags are DynamicsNet's constructor arguments (7 residual use_mask, 5 residual, 3 use_mask, 1 neither, 0
net._apply_out_transforms = False), and a column whose out_scale is exactly 0 has mask False.

    python tests/golden/make_golden_plan_wide.py      ->  tests/golden/plan_wide.npz
It writes that file alone, and a second run reproduces it bit for bit."""
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

import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
import _plan_wide_cases as C  # noqa: E402

torch.set_num_threads(1)


def reference_net(name, mem, k):
    """member k of a case as the reference's own DynamicsNet"""
    c = C.CASES[name]
    n, m, flags = c["n"], c["m"], c["flags"]
    net = nn_dynamics.DynamicsNet(n, m, c["dh"], residual=bool(flags & C.RES), use_mask=bool(flags & C.MASK))
    th, o = mem["thetas"][k], 0
    for p in net.parameters():
        p.data = torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy()); o += p.numel()
    if c["act"] == C.TANH:
        net.nonlinearity = torch.tanh
    if not flags & C.AFF:
        assert flags == 0
        net._apply_out_transforms = False
    tr, din = mem["trs"][k], n + m
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    net.set_transformations(t(tr[:n]), t(tr[din:din + n]), t(tr[n:din]), t(tr[din + n:2 * din]), t(tr[2 * din:2 * din + n]), t(tr[2 * din + n:]))
    return net


def yardstick(name):
    c = C.CASES[name]
    mem, data = C.cached_case(name)
    nets = [reference_net(name, mem, k) for k in range(c["K"])]
    worst = 0.0
    for mode in c["s0"]:
        s0, actions = data[mode]
        with torch.no_grad():
            obs = np.stack([sampling.trajectory_rollout(actions, net, s0)["observations"] for net in nets])
        assert obs.dtype == np.float32 and obs.shape == (c["K"], c["rows"], c["H"], c["n"])
        e = C.free_error(name, obs, C.free_reference(name, mode)) if name == C.FREE else C.step_error(name, obs, actions, mem)
        worst = max(worst, e)
    return worst


def planner(out, reward):
    """one get_action of the reference's MPCPolicy on the seeded wide members -> its distances from the fp64 oracle"""
    P = C.MPC
    n, m, K, N, H = P["n"], P["m"], P["K"], P["N"], P["H"]
    members = C.mpc_members(nn_dynamics.WorldModel, torch)
    env = L.cycling_env(n, m, members) if reward == "learned" else M.plan_env(n, m)
    pol = MPCPolicy(env=env, plan_horizon=H, plan_paths=N, kappa=P["kappa"], gamma=P["gamma"], filter_coefs=list(P["fc"]), warmstart=True,
                    fitted_model=members, omega=P["omega"])
    cap = {}
    score = pol.score_trajectory_ensemble

    def rec(paths, paths_list):
        cap["R"] = score(paths, paths_list).copy()
        return cap["R"]

    pol.score_trajectory_ensemble = rec
    np.random.seed(P["draw"])
    actions = M.perturbed_actions(N, pol.act_sequence, list(P["fc"]))
    np.random.seed(P["draw"])
    action = pol.get_action(C.mpc_obs())
    seq = np.concatenate([action[None], pol.act_sequence[:-1]])
    plan = C.mpc_oracle(actions, reward)
    e = M.ess(plan["S"])
    assert C.MPC_MIN_ESS <= e <= 0.5 * K * N, (reward, e)          # neither degenerate nor flat: lower or raise kappa, not this
    eR, eq = C.mpc_errors(cap["R"], seq, plan)
    out[C.mpc_key("R", reward)], out[C.mpc_key("seq", reward)] = np.float64(eR), np.float64(eq)
    print("planner on reward=%s: ESS %.1f of %d; the reference's fp32 scores are %.3e and its sequence %.3e from fp64" % (reward, e, K * N, eR, eq))


def main():
    out = {}
    for name in C.ORDER:
        if C.CASES[name]["H"] == 1:
            continue
        key = "pfree_" + name if name == C.FREE else "pstep_" + name
        out[key] = np.float64(yardstick(name))
        print("case %s: the reference's fp32 rollout is %.3e from fp64 (%s)" % (name, out[key], key))
    for reward in ("learned", "env"):
        planner(out, reward)
    path = os.path.join(HERE, "plan_wide.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
