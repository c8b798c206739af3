#!/usr/bin/env python
"""Yardsticks of the path-reward matrix (tests/test_gpu_path_reward_matrix.py) from the UNMODIFIED reference
(mjrl/algos/model_accel/nn_dynamics.py), run on the CPU through _ref_import: per case of _path_reward_cases.CASES the reference's own
fp32 result -- RewardNet.forward(s, a, DynamicsNet.forward(s, a)) -- on the seeded inputs against the fp64 restatement
_mpc_learned_oracle.ensemble_rewards, measured exactly as the GPU worker measures the kernel and as make_golden_mpc_learned.
kernel_yardsticks does: per row set and action mode the largest |error| over all members' compared rows relative to the largest
|reward| over the same rows (_mpc_learned_oracle.rel_max), and the largest of those ("kref_<case>", float64 scalars, nothing else).
For g3 the compared rows are _path_reward_cases.subset_rows of every member, as in the test.

The reference expresses every case without a changed line:
  * the s' transform: RewardNet.set_transformations copies s_shift / s_scale into its separate attributes sp_shift / sp_scale
    (nn_dynamics.py:288, :293), which RewardNet.forward reads (:321); they are set to the case's s' columns after set_transformations.
  * the activations: net.nonlinearity = torch.tanh per net (:188, :278 set the attribute; forward reads it at :239, :325), as the
    existing generator does.
  * the dynamics flags, all through DynamicsNet's own constructor arguments and the attribute its forward reads (:241-244):
      7  affine, mask, residual   DynamicsNet(residual=True,  use_mask=True)            lines 242, 243, 244
      5  affine, residual         DynamicsNet(residual=True,  use_mask=False)           lines 242, 244 (243 passes `out` through)
      3  affine, mask             DynamicsNet(residual=False, use_mask=True)            lines 242, 243
      1  affine                   DynamicsNet(residual=False, use_mask=False)           line 242
      0  none                     net._apply_out_transforms = False (set True at :190)  line 241 skips 242-244
    so no line of the chain had to be restated in torch here.
A masked column has out_scale exactly 0, so the reference's mask (out_scale >= 1e-8, :224) is False there.

    python tests/golden/make_golden_path_reward_matrix.py      ->  tests/golden/path_reward_matrix.npz
It writes that file alone (tests/golden/mpc_learned.npz is not touched), and a second run reproduces it bit for bit."""
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

import _mpc_learned_oracle as L  # noqa: E402
import _path_reward_cases as C  # noqa: E402

torch.set_num_threads(1)


def reference_nets(name, mem, k):
    """member k of a case as the reference's own DynamicsNet and RewardNet"""
    c = C.CASES[name]
    n, m, flags = c["n"], c["m"], c["flags"]
    dyn = nn_dynamics.DynamicsNet(n, m, c["dh"], residual=bool(flags & C.RES), use_mask=bool(flags & C.MASK))
    rew = nn_dynamics.RewardNet(n, m, hidden_size=c["rh"])
    for net, th, act in ((dyn, mem["dyn_thetas"][k], c["dact"]), (rew, mem["rew_thetas"][k], c["ract"])):
        o = 0
        for p in net.parameters():
            p.data = torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy()); o += p.numel()
        if act == C.TANH:
            net.nonlinearity = torch.tanh
    if not flags & C.AFF:
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


def yardstick(name):
    c = C.CASES[name]
    n, m, K = c["n"], c["m"], c["K"]
    mem, data = C.cached_case(name)
    ref = C.reference(name)
    nets = [reference_nets(name, mem, k) for k in range(K)]
    worst = 0.0
    for rows in c["rows"]:
        obs, shared, own = data[rows]
        idx = C.compared_rows(name, rows)
        for mode in c["modes"]:
            r32 = []
            for k, (dyn, rew) in enumerate(nets):
                s = torch.from_numpy(np.ascontiguousarray(obs[k][idx]))
                a = torch.from_numpy(np.ascontiguousarray(shared[idx] if mode == "shared" else own[k][idx]))
                with torch.no_grad():
                    r32.append(rew.forward(s, a, dyn.forward(s, a).detach().clone()).numpy()[:, 0])
            worst = max(worst, L.rel_max(np.stack(r32), ref[(rows, mode)]))
    return worst


def main():
    out = {}
    for name in C.ORDER:
        out["kref_" + name] = np.float64(yardstick(name))
        print("case %s: the reference's fp32 chain is %.3e from fp64" % (name, out["kref_" + name]))
    path = os.path.join(HERE, "path_reward_matrix.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
