#!/usr/bin/env python
"""Yardsticks of the wide policy-rollout tests from the UNMODIFIED reference, run on the CPU: per case of
_rollout_wide_cases.WCASES the reference's own fp32 rollout (make_golden_refine.reference_rollout: policy.model.forward,
+ noise * exp(log_std), enforce_tensor_bounds, learned_model.forward, enforce_tensor_bounds, on the case's seeded nets, start
states and noise) measured exactly as the GPU worker measures the kernel: _refine_oracle.step_errors on its stored states and
actions ("kya_<case>", "kys_<case>"), for the free-running case its distance from the fp64 free-running rollout ("kfree_obs",
"kfree_act"), and for the cases with tight bounds the shares of the fp64 rollout's actions and states that sit on a bound
("share_<case>": [actions, states]; asserted to be at least a tenth each).  Data only.
    python tests/golden/make_golden_rollout_wide.py      ->  tests/golden/rollout_wide.npz
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_refine import reference_rollout  # noqa: E402  (installs the reference's modules)

import numpy as np  # noqa: E402

import _refine_oracle as F  # noqa: E402
import _rollout_wide_cases as W  # noqa: E402

MIN_SHARE = 0.1


def main():
    out = {}
    for name in sorted(W.WCASES):
        c = W.wide_case(name)
        obs, act = reference_rollout(c)
        out["kya_" + name], out["kys_" + name] = (np.float64(v) for v in F.step_errors(c, obs, act))
        print("case %s: the reference's fp32 steps are %.3e (action) and %.3e (state) from fp64" % (name, out["kya_" + name], out["kys_" + name]))
        if c["H"] == 1:
            assert out["kys_" + name] == 0.0 and np.array_equal(obs[:, :, 0], np.stack([F.case_s0_rows(c)] * c["K"]))
        if c["bounds"] is not None:
            sa, ss = F.clamped_shares(c, *F.free_rollout(c))
            print("     clamped shares of the fp64 rollout: %.2f of the actions, %.2f of the states" % (sa, ss))
            assert sa >= MIN_SHARE and ss >= MIN_SHARE, (name, sa, ss)
            out["share_" + name] = np.array([sa, ss])
    assert sorted(k[6:] for k in out if k.startswith("share_")) == sorted(W.TIGHT)
    c = W.wide_case(W.FREE_CASE, W.FREE_H)
    obs, act = reference_rollout(c)
    o64, a64 = F.free_rollout(c)
    out["kfree_obs"], out["kfree_act"] = np.float64(F.rel_max(obs, o64)), np.float64(F.rel_max(act, a64))
    print("free-running %s at H = %d: the reference's fp32 rollout is %.3e (states) and %.3e (actions) from fp64" %
          (W.FREE_CASE, W.FREE_H, out["kfree_obs"], out["kfree_act"]))
    path = os.path.join(HERE, "rollout_wide.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
