"""The cases of the wide policy-rollout tests (csrc/policy_rollout_wide.h, mjx_policy_rollout_wide): _refine_oracle.KCASES's tuple
layout and seeding scheme with seeds of their own; the error measures (step_errors, rel_max, free_rollout, clamped_shares) are
_refine_oracle's.  Used by the fixture generator (tests/golden/make_golden_rollout_wide.py -> tests/golden/rollout_wide.npz), the
CPU tests (tests/test_rollout_wide_cpu.py) and the GPU worker (tests/_rollout_wide_worker.py).

name -> (n, m, dynamics hidden, policy hidden, activation code, dynamics flags, K, N, H, s0 mode, noise mode, bounds mode)
Each case is the smallest shape that has its edge.  Rows 1 (w4), 31 (w3), 32 (w5, w8), 33 (w1, w7: a second workgroup), 64 (w6),
65 (w2: a third); 256 x 256 (one tile per wave per layer), ragged and unequal widths (160 x 96, 100 x 200, 64 x 33, 128 x 100), a
one-unit layer (129 x 1, 1 x 1), n = 64 and m = 32 (w5), a policy wider than the dynamics net (w7), H = 1 (w8); ReLU and tanh;
flags 7, 3, 5, 1, 0; w2 has a masked output column."""
import numpy as np

import _mpc_learned_oracle as L
import _refine_oracle as F  # noqa: F401  (the measures, for the users of this module)

WCASES = {
    "w1": (11, 2, (256, 256), (64, 64), 0, 7, 3, 33, 7, "one", "shared", "tight"),
    "w2": (6, 2, (256, 256), (32, 32), 1, 3, 1, 65, 7, "rows", "member", "none"),
    "w3": (17, 6, (160, 96), (64, 64), 0, 5, 2, 31, 7, "rows", "none", "none"),
    "w4": (1, 1, (129, 1), (1, 1), 1, 1, 1, 1, 7, "one", "shared", "none"),
    "w5": (64, 32, (256, 256), (64, 33), 0, 0, 1, 32, 7, "rows", "member", "none"),
    "w6": (33, 9, (100, 200), (128, 100), 0, 7, 2, 64, 7, "rows", "member", "none"),
    "w7": (17, 6, (64, 64), (128, 128), 1, 7, 1, 33, 7, "one", "shared", "tight"),
    "w8": (6, 2, (256, 256), (32, 32), 0, 7, 1, 32, 1, "rows", "member", "none"),
}
W2_MASKED = 3                        # w2's dynamics out_scale column that is 0
FREE_CASE, FREE_H = "w1", 16         # the free-running comparison: w1's nets and bounds at H = 16
TIGHT = ("w1", "w7")
A_BOUND, S_BOUND = F.A_BOUND, F.S_BOUND


def wide_case(name, H=None):
    """seeded nets and inputs of a case -> the dict of _refine_oracle.kernel_case, all fp32"""
    n, m, dh, ph, act, flags, K, N, H0, s0m, nzm, bdm = WCASES[name]
    H = H0 if H is None else H
    rng = np.random.RandomState(7100 + sorted(WCASES).index(name))
    ds, ps = (n + m,) + dh + (n,), (n,) + ph + (m,)
    c = dict(n=n, m=m, K=K, N=N, H=H, pol_sizes=ps, dyn_sizes=ds, act=act, flags=flags, dyn_thetas=[], dyn_trs=[])
    for _ in range(K):
        c["dyn_thetas"].append(L._torch_like(rng, ds))
        dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
        if name == "w2":
            dtr[2 * (n + m) + n + W2_MASKED] = 0.0
        c["dyn_trs"].append(dtr.astype(np.float32))
    c["pol_theta"] = np.concatenate([L._torch_like(rng, ps), -0.5 + 0.07 * np.arange(m) - 0.3 * rng.rand(m)]).astype(np.float32)
    c["pol_tr"] = np.concatenate([rng.randn(n) * 0.3, rng.rand(n) + 0.5, rng.randn(m) * 0.2, rng.rand(m) + 0.5]).astype(np.float32)
    c["s0"] = (rng.randn(n) if s0m == "one" else rng.randn(N, n)).astype(np.float32)
    hrng = np.random.RandomState(7200 + 17 * sorted(WCASES).index(name) + H)          # (the noise depends on H)
    c["noise"] = None if nzm == "none" else hrng.randn(*((H, N, m) if nzm == "shared" else (K, H, N, m))).astype(np.float32)
    c["bounds"] = None if bdm == "none" else tuple(np.float32(v) for v in (-A_BOUND * (1 + 0.1 * rng.rand(m)), A_BOUND * (1 + 0.1 * rng.rand(m)),
                                                                          -S_BOUND * (1 + 0.1 * rng.rand(n)), S_BOUND * (1 + 0.1 * rng.rand(n))))
    return c
