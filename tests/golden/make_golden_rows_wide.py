#!/usr/bin/env python
"""Yardsticks of the wide passes over stored rollouts (tests/_rows_wide_cases.py), on the CPU.  Data only.

r_<case>: per reward case the UNMODIFIED reference's own fp32 chain (mjrl/algos/model_accel/nn_dynamics.py through _ref_import, as
make_golden_path_reward_matrix.py expresses every flag, activation and the s' transform without a changed line) --
RewardNet.forward(s, a, DynamicsNet.forward(s, a)) -- against the fp64 oracle _mpc_learned_oracle.ensemble_rewards, measured as the
GPU worker measures the kernel: _rollout_batch_cases.row_err over every row of every member, the largest over the case's row sets
and action modes.
d_<case>: per disagreement case the existing plain fp32 torch-CPU restatement _rollout_batch_cases.torch_err32 against the fp64
oracle _rollout_batch_cases.oracle_err under the same row_err, as make_golden_rollout_batch.py does.

It asserts, from the oracle alone: every masked case's mask moves the result, every residual case's residual moves it, and each
limited disagreement case has between a quarter and three quarters of its paths truncating, at least one path clamped to min_len
and one path untruncated (tests/test_rows_wide_cpu.py repeats them).
    python tests/golden/make_golden_rows_wide.py      ->  tests/golden/rows_wide.npz
It writes that file alone, and a second run reproduces it bit for bit."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_import  # noqa: E402

_ref_import.install()
sys.modules.setdefault("mjrl.envs", types.ModuleType("mjrl.envs"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from mjrl.algos.model_accel import nn_dynamics  # noqa: E402

import _rollout_batch_cases as B  # noqa: E402
import _rows_wide_cases as W  # noqa: E402

torch.set_num_threads(1)


def reference_nets(name, mem, k):
    """member k of a reward case as the reference's own DynamicsNet and RewardNet"""
    net, rh, ract = W.RCASES[name][:3]
    n, m, dh, dact, flags, _ = W.NETS[net]
    dyn = nn_dynamics.DynamicsNet(n, m, dh, residual=bool(flags & W.RES), use_mask=bool(flags & W.MASK))
    rew = nn_dynamics.RewardNet(n, m, hidden_size=rh)
    for nn_, th, act in ((dyn, mem["dyn_thetas"][k], dact), (rew, mem["rew_thetas"][k], ract)):
        o = 0
        for p in nn_.parameters():
            p.data = torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy()); o += p.numel()
        if act == W.TANH:
            nn_.nonlinearity = torch.tanh
    if not flags & W.AFF:
        assert flags == 0
        dyn._apply_out_transforms = False
    dtr, rtr, din, rin = mem["dyn_trs"][k], mem["rew_trs"][k], n + m, 2 * n + m
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    dyn.set_transformations(t(dtr[:n]), t(dtr[din:din + n]), t(dtr[n:din]), t(dtr[din + n:2 * din]), t(dtr[2 * din:2 * din + n]),
                            t(dtr[2 * din + n:]))
    rew.set_transformations(t(rtr[:n]), t(rtr[rin:rin + n]), t(rtr[n:din]), t(rtr[rin + n:rin + din]), float(rtr[2 * rin]),
                            float(rtr[2 * rin + 1]))
    rew.sp_shift, rew.sp_scale = t(rtr[din:rin]), t(rtr[rin + din:2 * rin])
    return dyn, rew


def reward_yardstick(name):
    _, _, _, K, rowsets, modes = W.RCASES[name]
    mem, data = W.rcase(name)
    ref = W.rreference(name)
    nets = [reference_nets(name, mem, k) for k in range(K)]
    worst = 0.0
    for rows in rowsets:
        obs, shared, own = data[rows]
        for mode in modes:
            r32 = []
            for k, (dyn, rew) in enumerate(nets):
                s = torch.from_numpy(np.ascontiguousarray(obs[k]))
                a = torch.from_numpy(np.ascontiguousarray(shared if mode == "shared" else own[k]))
                r32.append(rew.forward(s, a, dyn.forward(s, a).detach().clone()).numpy()[:, 0])
            worst = max(worst, B.row_err(np.stack(r32), ref[(rows, mode)]))
    return worst


def reward_conditions(name):
    """the mask and the residual move the oracle's result"""
    mem = W.rcase(name)[0]
    for bit in (W.MASK, W.RES):
        if mem["dflags"] & bit:
            for (rows, mode), ref in W.rreference(name).items():
                moved = B.row_err(W.roracle(name, W.without_flag(mem, bit), rows, mode), ref)
                assert moved > W.MOVES, (name, bit, rows, mode, moved)


def dis_conditions(case):
    mem, obs, act = W.dis_data(case)
    ref = B.oracle_err(mem, obs, act)
    for bit in (W.MASK, W.RES):
        if mem["flags"] & bit:
            moved = B.row_err(B.oracle_err(dict(mem, flags=mem["flags"] & ~bit), obs, act), ref)
            assert moved > W.MOVES, (case, bit, moved)
    if case in W.limited():
        cut, clamped, whole, P = W.truncation_shares(ref, B.fix_lim(ref))
        assert P / 4 <= cut <= 3 * P / 4 and clamped >= 1 and whole >= 1, (case, cut, clamped, whole)


def main():
    out = {}
    for name in W.RORDER:
        reward_conditions(name)
        out["r_" + name] = np.float64(reward_yardstick(name))
        print("reward case %s: the reference's fp32 chain is %.3e from fp64" % (name, out["r_" + name]))
    for case in W.dis_cases():
        dis_conditions(case)
        mem, obs, act = W.dis_data(case)
        out["d_" + W.dis_id(case)] = np.float64(B.row_err(B.torch_err32(mem, obs, act), B.oracle_err(mem, obs, act)))
        print("disagreement case %s: fp32 torch is %.3e from fp64" % (W.dis_id(case), out["d_" + W.dis_id(case)]))
    path = os.path.join(HERE, "rows_wide.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    with torch.no_grad():
        main()
