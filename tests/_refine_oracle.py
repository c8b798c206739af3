"""What the policy-rollout and refinement tests share (csrc/policy_rollout.h, ModelAccelNPG.get_refined_action): the kernel cases
with their seeded nets and inputs, the step-by-step and free-running error measures, and the fp64 restatement of one refined
call, on top of tests/_dyn_oracle.py, tests/_mpc_oracle.py and tests/_mpc_learned_oracle.py.  Used by the fixture generator
(tests/golden/make_golden_refine.py -> tests/golden/refine.npz), the CPU tests (tests/test_refine_cpu.py) and the GPU workers
(tests/_policy_rollout_worker.py, tests/_refine_worker.py).

What is rounded where, as in _mpc_oracle: the restatement sees the fp32 parameters, transforms, start states and noise that the
reference's torch code sees, but runs in fp64."""
import numpy as np

import _dyn_oracle as O
import _mpc_learned_oracle as L
import _mpc_oracle as M

# ---- kernel cases: each puts edges on k_policy_rollout at the smallest shape that has them.
# name -> (n, m, dynamics hidden, policy hidden, activation code, dynamics flags, K, N, H, s0 mode, noise mode, bounds mode)
#   s0 mode "one": one state for all trajectories (s0_stride 0), "rows": (N, n); noise "none" / "shared" / "member"; bounds "none" / "tight".
# Instances <HB, NB>: p1 <2, 1>, p2 <3, 1>, p3 <1, 2>, p4 <1, 1>, p5 <2, 2>, p6 <3, 2>, p7 <4, 1>, p8 <4, 2> -- all eight, each at H = 7, so
# that every instance's dynamics half, every flag set, the mask, m = 32 (four action slot groups into chain_l1_actions) and n = 64 reach a
# STORED state; p9 is the H = 1 case (s0 and the first action only: its edges are the policy's and the one-step loop's).
# Rows 1 (p4), 31 (p3), 32 (p5, p8, p9), 33 (p1, p7), 129 (p2, p6: a second workgroup); H 1 and 7; K 1 and 3; n 1, 17, 33, 64; m 1, 6, 9 (two
# slot groups), 32 (no padding); policy widths (64, 64), (20, 50), (32, 32), (1, 1), (64, 33); ReLU and tanh; flags 7, 3, 5, 1, 0; p2 has a
# masked output column.
KCASES = {
    "p1": (17, 6, (64, 64), (64, 64), 0, 7, 3, 33, 7, "one", "shared", "tight"),
    "p2": (17, 6, (96, 32), (20, 50), 1, 3, 1, 129, 7, "rows", "member", "none"),
    "p3": (33, 9, (32, 32), (32, 32), 0, 5, 1, 31, 7, "rows", "none", "tight"),
    "p4": (1, 1, (32, 32), (1, 1), 1, 1, 1, 1, 7, "one", "shared", "none"),
    "p5": (64, 32, (64, 64), (64, 33), 0, 0, 1, 32, 7, "rows", "member", "none"),
    "p6": (33, 9, (96, 64), (32, 32), 0, 7, 3, 129, 7, "rows", "member", "none"),
    "p7": (6, 2, (128, 128), (64, 64), 1, 7, 1, 33, 7, "one", "shared", "tight"),
    "p8": (33, 2, (128, 128), (32, 32), 0, 7, 1, 32, 7, "one", "none", "none"),
    "p9": (6, 2, (32, 32), (32, 32), 0, 7, 1, 32, 1, "rows", "member", "none"),
}
P2_MASKED = 3                        # p2's dynamics out_scale column that is 0
FREE_CASE, FREE_H = "p1", 16         # the free-running comparison: p1's nets and bounds at H = 16
A_BOUND, S_BOUND = 0.3, 0.5          # the tight bounds (+-): at least a tenth of the actions and of the states sit on them


def kernel_case(name, H=None):
    """seeded nets and inputs of a kernel case -> dict(n, m, K, N, H, pol_theta, pol_sizes, pol_tr, dyn_thetas, dyn_sizes, dyn_trs,
    act, flags, s0 ((n,) or (N, n)), noise (None, (H, N, m) or (K, H, N, m)), bounds (None or 4 arrays)), all fp32"""
    n, m, dh, ph, act, flags, K, N, H0, s0m, nzm, bdm = KCASES[name]
    H = H0 if H is None else H
    rng = np.random.RandomState(4100 + sorted(KCASES).index(name))
    ds, ps = (n + m,) + dh + (n,), (n,) + ph + (m,)
    c = dict(n=n, m=m, K=K, N=N, H=H, pol_sizes=ps, dyn_sizes=ds, act=act, flags=flags, dyn_thetas=[], dyn_trs=[])
    for _ in range(K):
        c["dyn_thetas"].append(L._torch_like(rng, ds))
        dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
        if name == "p2":
            dtr[2 * (n + m) + n + P2_MASKED] = 0.0
        c["dyn_trs"].append(dtr.astype(np.float32))
    # the policy: torch-like weights, a log_std that differs per action, non-trivial transforms on both sides
    c["pol_theta"] = np.concatenate([L._torch_like(rng, ps), -0.5 + 0.07 * np.arange(m) - 0.3 * rng.rand(m)]).astype(np.float32)
    c["pol_tr"] = np.concatenate([rng.randn(n) * 0.3, rng.rand(n) + 0.5, rng.randn(m) * 0.2, rng.rand(m) + 0.5]).astype(np.float32)
    c["s0"] = (rng.randn(n) if s0m == "one" else rng.randn(N, n)).astype(np.float32)
    hrng = np.random.RandomState(4200 + 17 * sorted(KCASES).index(name) + H)          # (the noise depends on H)
    c["noise"] = None if nzm == "none" else hrng.randn(*((H, N, m) if nzm == "shared" else (K, H, N, m))).astype(np.float32)
    c["bounds"] = None if bdm == "none" else tuple(np.float32(v) for v in (-A_BOUND * (1 + 0.1 * rng.rand(m)), A_BOUND * (1 + 0.1 * rng.rand(m)),
                                                                          -S_BOUND * (1 + 0.1 * rng.rand(n)), S_BOUND * (1 + 0.1 * rng.rand(n))))
    return c


def case_s0_rows(c):
    return np.tile(c["s0"], (c["N"], 1)) if c["s0"].ndim == 1 else c["s0"]


def case_noise_members(c):
    """(K, H, N, m) or None"""
    if c["noise"] is None:
        return None
    return np.stack([c["noise"]] * c["K"]) if c["noise"].ndim == 3 else c["noise"]


def free_rollout(c):
    """the fp64 free-running rollout of a case -> obs (K, N, H, n), act (K, N, H, m)"""
    return O.rollout(case_s0_rows(c), c["H"], c["pol_theta"], list(c["pol_sizes"]), c["pol_tr"], case_noise_members(c), c["dyn_thetas"],
                     list(c["dyn_sizes"]), c["dyn_trs"], c["act"], c["flags"], c["bounds"])[:2]


def rel_max(got, ref):
    """the largest absolute error over a block relative to the largest magnitude in the (reference) block"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300)) if ref.size else 0.0


def step_errors(c, obs, act):
    """stored obs (K, N, H, n) and act (K, N, H, m) of ANY implementation, step by step against fp64 -> (action error, state
    error): every stored action against the fp64 action step from the stored state before it, every stored state against the
    fp64 state step from the stored state and stored action before it (the first against s0), each through rel_max over the
    whole block"""
    K, N, H, n, m = c["K"], c["N"], c["H"], c["n"], c["m"]
    nz = case_noise_members(c)
    a_ref, s_ref = np.zeros((K, N, H, m)), np.zeros((K, N, H, n))
    for k in range(K):
        s_ref[k, :, 0] = case_s0_rows(c)
        for t in range(H):
            a_ref[k, :, t] = O.rollout_action(obs[k, :, t], c["pol_theta"], list(c["pol_sizes"]), c["pol_tr"],
                                              None if nz is None else nz[k, t], c["bounds"])
            if t + 1 < H:
                s_ref[k, :, t + 1] = O.rollout_next(obs[k, :, t], act[k, :, t], c["dyn_thetas"][k], list(c["dyn_sizes"]), c["dyn_trs"][k],
                                                    c["act"], c["flags"], c["bounds"])
    return rel_max(act, a_ref), rel_max(obs, s_ref)


def clamped_shares(c, obs, act):
    """the share of the actions, and of the states after the first, that sit on a bound"""
    b = c["bounds"]
    sa = np.mean((act == b[0]) | (act == b[1]))
    ss = np.mean((obs[:, :, 1:] == b[2]) | (obs[:, :, 1:] == b[3])) if obs.shape[2] > 1 else 1.0
    return float(sa), float(ss)


# ---- one refined call.  The cases of the fixture: name -> (N, H, policy hidden, kappa, omega, gamma), on _mpc_learned_oracle's K = 3
# fitted members ((n, m) = (6, 2), dynamics 64 x 64 ReLU residual, reward nets 100 x 100), policy seed and init_log_std -0.5.
# kappa keeps 5 <= ESS <= 0.5 K N on every call (asserted by the generator) and the reference within a third of TOL_STEP of the
# restatement (asserted by tests/test_refine_cpu.py).
RCASES = {
    "ra": (64, 8, (32, 32), 6.0, 0.0, 1.0),
    "rb": (33, 5, (64, 64), 1.5, 5.0, 1.0),
}
RCALLS = 2
POL_SEED, INIT_LOG_STD, LARGE = 11, -0.5, 1e2


def rcall_obs(case, call):
    return np.random.RandomState(5000 + 10 * sorted(RCASES).index(case) + call).randn(L.PN) * 0.5


def rcall_seed(case, call):
    return 600 + 10 * sorted(RCASES).index(case) + call


def refined(obs0, noise, pol_theta, pol_sizes, pol_tr, mem, kappa, gamma, omega, rewards=None):
    """one get_refined_action in fp64 given its noise (H, N, m) -> dict(obs, act, rewards, R, S, action).  rewards: a callable
    (obs, act) -> (K, N, H) in place of the members' reward nets."""
    H, N, m = noise.shape
    K, n = len(mem["dyn_thetas"]), len(obs0)
    s0 = np.tile(np.asarray(obs0, np.float32).astype(np.float64), (N, 1))
    b = (np.full(m, -LARGE), np.full(m, LARGE), np.full(n, -LARGE), np.full(n, LARGE))
    obs, act = O.rollout(s0, H, pol_theta, list(pol_sizes), pol_tr, np.stack([noise] * K), mem["dyn_thetas"], list(mem["dyn_sizes"]),
                         mem["dyn_trs"], mem["dact"], mem["dflags"], b)[:2]
    rew = L.ensemble_rewards(obs, act, mem) if rewards is None else rewards(obs, act)
    R = M.scores(obs, rew, omega, gamma, reference_indexing=False, ensemble=omega != 0.0)
    S = M.weights(R, kappa)
    w = S.reshape(K, N).sum(0)
    return dict(obs=obs, act=act, rewards=rew, R=R, S=S, action=(w[:, None] * act[0, :, 0]).sum(0) / (np.sum(S) + 1e-6))
