"""The cases of tests/test_gpu_fit_matrix.py and their inputs, shared by the GPU worker (tests/_fit_matrix_worker.py) and by
tests/test_fit_checks.py, which shows on CPU, from the fp64 oracle alone, that every case is well posed: few ill-conditioned
parameters, PPO rows on both branches of the clip and none near its boundaries."""
import numpy as np

from oracle import npg_oracle as NO
from tests import _fit_oracle as F
from tests._dyn_check import rand_theta

LR, CLIP = 1e-3, 0.2
LAUNCHES, HALVES, ONEPASS, WIDE = 0, 1, 2, 3          # out6[0] of mjx_mlp_fit_route
N_MLP = 64 * 6 + 37           # 5 steps an epoch at batch 64, e N no multiple of 64, a tail of rows never visited
N_POL, POL_STEPS = 500, 12    # 10 steps against fp64; 3 + 9 for the continuation
MODES = ((0, 1), (1, 1), (2, 1), (2, 0))              # (loss, old_tracks_new)

_REG = ({}, {"MJX_FIT_REGMOM": "0"})
_NONE = (LAUNCHES, 0, 0, 0)


def _mlp_cases():
    """(name, d_in, switches, (kind, NF1, REGMOM, workgroups) the route must report, hidden, batch, wd, seed)"""
    out = [("d_in %d" % d, d, {}, (ONEPASS, 1, 1, 1), (128, 128), 64, 1e-3, 1000 + d) for d in (1, 3, 4, 23)]
    for reg, env in ((1, _REG[0]), (0, _REG[1])):
        for d in (24, 31, 9):
            out.append(("d_in %d regmom %d" % (d, reg), d, dict(env, MJX_FIT_ONEPASS="0") if d == 9 else env, (HALVES, 1, reg, 1),
                        (128, 128), 64, 1e-3, 1100 + d))
        for d in (32, 43, 55):
            out.append(("d_in %d regmom %d" % (d, reg), d, env, (HALVES, 2, reg, 1), (128, 128), 64, 1e-3, 1200 + d))
        for d, G in ((56, 2), (96, 2), (97, 3), (768, 16)):     # last slice: 8 + bias, full, 1 feature; 16 workgroups
            out.append(("d_in %d regmom %d" % (d, reg), d, env, (WIDE, 2, reg, G), (128, 128), 64, 1e-3, 1300 + d))
    out += [("d_in 769", 769, {}, _NONE, (128, 128), 64, 1e-3, 1401),
            ("d_in 43 hidden 64 x 64", 43, {}, _NONE, (64, 64), 64, 1e-3, 1402),
            ("d_in 43 batch 32", 43, {}, _NONE, (128, 128), 32, 1e-3, 1403),
            ("d_in 9 launches", 9, {"MJX_MLP_FIT_LAUNCHES": "1"}, _NONE, (128, 128), 64, 1e-3, 1404)]
    return out


# one shape an instance: without weight decay, and for the continuation (23 inputs on the one-pass trainer: with fewer and no
# weight decay, the dead ReLU units of 128 alone leave 4 .. 7 % of W1 without a gradient)
MLP_INSTANCES = [("d_in 23", 23, {}, (ONEPASS, 1, 1, 1)), ("d_in 24 regmom 1", 24, _REG[0], (HALVES, 1, 1, 1)),
                 ("d_in 24 regmom 0", 24, _REG[1], (HALVES, 1, 0, 1)), ("d_in 43 regmom 1", 43, _REG[0], (HALVES, 2, 1, 1)),
                 ("d_in 43 regmom 0", 43, _REG[1], (HALVES, 2, 0, 1)), ("d_in 97 regmom 1", 97, _REG[0], (WIDE, 2, 1, 3)),
                 ("d_in 97 regmom 0", 97, _REG[1], (WIDE, 2, 0, 3)), ("d_in 769", 769, {}, _NONE)]
# Seeds, from the oracle alone (tests/test_fit_checks.py): the first minibatch's residuals keep |mean e| >= 0.1 mean |e|.  b3 is a
# block of ONE entry, its moments are compared over their own size, and its gradient is 2 mean e: where the residuals cancel (to
# 0.3 % at one of the seeds replaced here) any fp32 forward pass shows its rounding multiplied by as much.
_RESEED = {1003: 3003, 1124: 2124, 1131: 2131, 1232: 2232, 1255: 2255, 1356: 2356, 1501: 2501, 1502: 5502, 1504: 2504, 1507: 2507}
MLP_CASES = [c[:7] + (_RESEED.get(c[7], c[7]),) for c in
             _mlp_cases() + [(name + " wd 0", d, env, expect, (128, 128), 64, 0.0, 1500 + i)
                             for i, (name, d, env, expect) in enumerate(MLP_INSTANCES)]]
B3_CANCEL_FLOOR = 0.1
MLP_CONT_SEED = 1600


def mlp_data(d_in, hidden, batch, seed):
    """-> theta (nn.Linear scale), features, targets, two permutations of N_MLP rows, one of 2 batches (the single-step fit)"""
    rng = np.random.RandomState(seed)
    th = rand_theta(rng, F.mlp_sizes(d_in, hidden))
    x = rng.randn(N_MLP, d_in).astype(np.float32)
    y = rng.randn(N_MLP).astype(np.float32)
    perm = np.concatenate([rng.permutation(N_MLP) for _ in range(2)])
    return th, x, y, perm, rng.permutation(2 * batch)


# (n, m, hidden, B, switches, H the route must report (0: per-step launches), seed)
POL_CASES = [(17, 6, (64, 64), 64, {}, 64, 2000), (63, 16, (64, 64), 32, {}, 64, 2001), (16, 4, (64, 64), 12, {}, 64, 2002),
             (17, 5, (64, 64), 20, {}, 64, 2003),
             (1, 1, (32, 32), 8, {}, 32, 2100), (5, 2, (32, 32), 8, {}, 32, 2101), (32, 16, (32, 32), 64, {}, 32, 2102),
             (17, 6, (64, 64), 68, {}, 0, 2200), (17, 6, (64, 64), 10, {}, 0, 2211), (11, 17, (32, 32), 32, {}, 0, 2202),
             (17, 6, (64, 32), 32, {}, 0, 2203), (64, 6, (64, 64), 64, {}, 0, 2214),
             (17, 6, (64, 64), 64, {"MJX_NO_POLICY_FIT": "1"}, 0, 2320)]


def pol_name(n, m, hid, B, env):
    return "(%d, %d, %s, %d)%s" % (n, m, " x ".join(map(str, hid)), B, " no fit" if env else "")


def pol_data(n, m, hid, B, seed):
    """theta and a theta_old that differs from it (log_std by more: with old_tracks_new the ratio moves through it alone),
    non-trivial transforms of each, actions as the old policy draws them, idx with replacement and a row twice in a minibatch"""
    rng = np.random.RandomState(seed)
    th = np.concatenate([rand_theta(rng, [n] + list(hid) + [m]), rng.randn(m) * 0.3 - 0.5]).astype(np.float32)
    tho = th + np.concatenate([0.02 * rng.randn(th.size - m), 0.15 * rng.randn(m)]).astype(np.float32)
    mk_tr = lambda: np.concatenate([0.1 * rng.randn(n), 1 + 0.2 * rng.rand(n), 0.1 * rng.randn(m), 1 + 0.2 * rng.rand(m)]).astype(np.float32)
    tr, tro = mk_tr(), mk_tr()
    obs = rng.randn(N_POL, n).astype(np.float32)
    mu_old = NO.forward(tho.astype(np.float64), obs.astype(np.float64), n, m, hid, F.transforms(n, m, tro))
    act = (mu_old + np.exp(tho[-m:].astype(np.float64)) * rng.randn(N_POL, m)).astype(np.float32)
    adv = rng.randn(N_POL).astype(np.float32)
    idx = rng.randint(0, N_POL, size=(POL_STEPS, B))
    idx[0, 1], idx[4, B - 1] = idx[0, 0], idx[4, 2]
    # under MSE log_std and ITS moments must come back untouched: moments with values there, not zeros
    am_ls, av_ls = (0.25 * rng.randn(m)).astype(np.float32), (0.1 + rng.rand(m)).astype(np.float32)
    return {"theta": th, "theta_old": tho, "tr": tr, "tr_old": tro, "obs": obs, "act": act, "adv": adv, "idx": idx.ravel(),
            "am_ls": am_ls, "av_ls": av_ls}


def pol_moments(D, m, loss):
    am, av = np.zeros(D["theta"].size, np.float32), np.zeros(D["theta"].size, np.float32)
    if loss == 0:
        am[-m:], av[-m:] = D["am_ls"], D["av_ls"]
    return am, av
