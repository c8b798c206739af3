#!/usr/bin/env python
"""Yardsticks of the plan matrix (tests/test_gpu_plan_matrix.py) from the UNMODIFIED reference, run on the CPU through _ref_import: per
case of _plan_cases.CASES that stores a computed state (H > 1) the reference's own fp32 rollout -- its DynamicsNet
(mjrl/algos/model_accel/nn_dynamics.py:166-245) stepped by its trajectory_rollout (sampling.py:96-123), one call per member as
model_learning_mpc.py:53-56 makes them -- on the seeded inputs against the same fp64 oracle, measured exactly as the GPU worker measures
the kernels (_plan_cases.step_error, free_error):
    pstep_<case>   the per-column one-step error: every state the reference stored against one fp64 step (_dyn_oracle.rollout_next)
                   from the state and action IT stored before, per state column of each member relative to that column's largest
                   |reference| over the compared rows, the largest over columns, members and the case's runs
    pfree_<case>   the same measure against the free-running fp64 rollout (_mpc_oracle.rollout)
float64 scalars, nothing else.

The reference expresses every case without a changed line: the activation is net.nonlinearity (:188 sets it, :239 reads it), the flags
are DynamicsNet's own constructor arguments and the attribute its forward reads (:241-244) -- 7 residual=True use_mask=True, 5
residual=True use_mask=False, 3 residual=False use_mask=True, 1 both False, 0 net._apply_out_transforms = False -- and a column whose
out_scale is exactly 0 has mask False (:224).

    python tests/golden/make_golden_plan_matrix.py      ->  tests/golden/plan_matrix.npz
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

import _plan_cases as C  # noqa: E402

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


def yardsticks(name):
    c = C.CASES[name]
    mem, data = C.cached_case(name)
    nets = [reference_net(name, mem, k) for k in range(c["K"])]
    step, free = 0.0, 0.0
    for rows in c["rows"]:
        for mode in c["s0"]:
            s0, actions = data[(rows, mode)]
            with torch.no_grad():
                obs = np.stack([sampling.trajectory_rollout(actions, net, s0)["observations"] for net in nets])
            assert obs.dtype == np.float32 and obs.shape == (c["K"], rows, c["H"], c["n"])
            step = max(step, C.step_error(name, obs, actions, mem)[0])
            free = max(free, C.free_error(name, obs, C.free_reference(name, (rows, mode)))[0])
    return step, free


def main():
    out = {}
    for name in C.STEPPED:
        s, f = yardsticks(name)
        out["pstep_" + name], out["pfree_" + name] = np.float64(s), np.float64(f)
        print("case %s: the reference's fp32 rollout is %.3e per step and %.3e free-running from fp64" % (name, s, f))
    path = os.path.join(HERE, "plan_matrix.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
