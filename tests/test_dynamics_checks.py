"""The checks of tests/test_gpu_dynamics_matrix.py can fail: fp64 results with the defects a wrong learned-dynamics kernel would
leave behind are flagged at the bars that module uses, and the same results rounded to fp32 pass.  CPU only."""
import numpy as np
import pytest

from tests import _dyn_check as C
from tests import _dyn_oracle as O
from tests.test_gpu_dynamics_matrix import BARS

n, m, K, N, H = 11, 2, 3, 250, 8              # N = 250: the last 8-trajectory tile holds 2 rows
DSZ, PSZ = [n + m, 48, 48, n], [n, 32, 32, m]


def _setup():
    rng = np.random.RandomState(7)
    dth = C.rand_theta(rng, DSZ, K).astype(np.float64)
    dtr = np.stack([C.rand_tr(rng, n + m, n, zero_col=1) for _ in range(K)]).astype(np.float64)
    pth = np.concatenate([C.rand_theta(rng, PSZ, gain=1.5), rng.randn(m) * 0.3 - 0.5])
    ptr_ = np.concatenate([rng.randn(n) * 0.2, rng.rand(n) + 0.5, rng.randn(m) * 0.3 + 0.2, rng.rand(m) + 0.5])
    s0 = rng.randn(N, n).astype(np.float32)                        # the device's inputs are fp32
    nz = rng.randn(K, H, N, m).astype(np.float32)
    bnd = [np.full(m, -0.8, np.float32), np.full(m, 0.8, np.float32), np.full(n, -1.2, np.float32), np.full(n, 1.2, np.float32)]
    return dth, dtr, pth, ptr_, s0, nz, bnd


def _rollout(s0, pth, ptr_, nz, dth, dtr, bnd, skip_state_clamp_at=None):
    """O.rollout, with the state clamp optionally left out after one step"""
    obs, act = np.zeros((K, N, H, n)), np.zeros((K, N, H, m))
    for k in range(K):
        s = s0.copy()
        for t in range(H):
            a = O.rollout_action(s, pth, PSZ, ptr_, nz[k, t], bnd)
            obs[k, :, t], act[k, :, t] = s, a
            b = bnd if t != skip_state_clamp_at else bnd[:2] + [-np.inf, np.inf]
            s = O.rollout_next(s, a, dth[k], DSZ, dtr[k], 0, 7, b)
    return obs, act


def _rollout_flags(obs, act, setup):
    """the rollout checks of the GPU module that fail for (obs, act)"""
    dth, dtr, pth, ptr_, s0, nz, bnd = setup
    bad = []
    if C.unwritten(obs) + C.unwritten(act):
        bad.append("unwritten")
    if np.any(obs[:, :, 0] != s0[None]):
        bad.append("s0")
    tf = C.teacher_forced(obs, act, (pth, PSZ, ptr_), nz, (dth, DSZ, dtr, 0, 7), bnd)
    for key in ("act", "obs"):
        if not tf[key][0] < BARS["roll_tf_" + key]:
            bad.append(("tf", key, tf[key]))
    return bad


def _rounded(a):
    return np.asarray(a, np.float32).astype(np.float64)


def test_rollout_defects_are_flagged():
    setup = _setup()
    dth, dtr, pth, ptr_, s0, nz, bnd = setup
    obs, act = _rollout(s0, pth, ptr_, nz, dth, dtr, bnd)
    assert not _rollout_flags(_rounded(obs), _rounded(act), setup)

    o, a = obs.copy(), act.copy()                                  # the last partial tile never written (NaN sentinel)
    o[:, 248:], a[:, 248:] = np.nan, np.nan
    assert _rollout_flags(o, a, setup)

    o, a = _rollout(s0, pth, ptr_, nz[[1, 0, 2]], dth, dtr, bnd)   # members 0 and 1 read each other's noise
    assert _rollout_flags(o, a, setup)

    o, a = _rollout(s0, pth, ptr_, nz, dth, dtr, bnd, skip_state_clamp_at=3)
    assert np.any(o != obs)                                        # the clamp acts at that step
    assert _rollout_flags(o, a, setup)

    p = ptr_.copy()                                                # the policy's out_shift dropped
    p[2 * n:2 * n + m] = 0.0
    o, a = _rollout(s0, pth, p, nz, dth, dtr, bnd)
    assert _rollout_flags(o, a, setup)


def _fit_setup(sizes, batch, seed):
    rng = np.random.RandomState(seed)
    th = C.rand_theta(rng, sizes).astype(np.float64)
    tr = C.rand_tr(rng, sizes[0], sizes[-1]).astype(np.float64)
    x = rng.randn(300, sizes[0])
    y = x[:, :sizes[-1]] * 0.8 + 0.3 * rng.randn(300, sizes[-1])
    idx = np.concatenate([rng.permutation(300)[:(300 // batch) * batch] for _ in range(3)])
    return th, tr, x, y, idx


@pytest.mark.parametrize("sizes", [[10, 64, 64, 8], [13, 256, 256, 11]])
def test_adam_bias_correction_off_by_one_is_flagged(sizes):
    """continuation at t0 = 3: a call that numbers its steps from 2 (or from 4) instead"""
    batch, lr, s1, s2 = 32, 1e-3, 3, 7
    th, tr, x, y, idx = _fit_setup(sizes, batch, 3)
    p1, m1, v1, _ = O.adam_steps(th, sizes, tr, x, y, idx[:s1 * batch], batch, 0, 2, lr, 1e-5)
    rest = idx[s1 * batch:(s1 + s2) * batch]
    ref = O.adam_steps(p1, sizes, tr, x, y, rest, batch, 0, 2, lr, 1e-5, m=m1, v=v1, t0=s1)[0]
    ok = O.adam_steps(_rounded(p1), sizes, tr, x, y, rest, batch, 0, 2, lr, 1e-5, m=_rounded(m1), v=_rounded(v1), t0=s1)[0]
    assert C.over_lr(_rounded(ok), ref, lr) < BARS["fit_cont_over_lr"]
    for t0 in (s1 - 1, s1 + 1):
        bad = O.adam_steps(p1, sizes, tr, x, y, rest, batch, 0, 2, lr, 1e-5, m=m1, v=v1, t0=t0)[0]
        assert not C.over_lr(bad, ref, lr) < BARS["fit_cont_over_lr"], t0
        assert not C.over_lr(bad, ref, lr) < BARS["fit_params_over_lr"], t0


def test_fit_rounded_to_fp32_passes():
    sizes, batch, lr = [13, 256, 256, 11], 16, 1e-3
    th, tr, x, y, idx = _fit_setup(sizes, batch, 4)
    p, _, _, losses = O.adam_steps(th, sizes, tr, x, y, idx[:10 * batch], batch, 0, 2, lr, 1e-5)
    assert C.over_lr(_rounded(p), p, lr) < BARS["fit_params_over_lr"]
    assert C.rel_max(_rounded(losses), losses) < BARS["fit_loss"]


def test_forward_masked_column_and_rounding():
    rng = np.random.RandomState(5)
    sizes = [13, 64, 64, 11]
    th = C.rand_theta(rng, sizes, 2).astype(np.float64)
    trs = np.stack([C.rand_tr(rng, 13, 11, zero_col=2) for _ in range(2)]).astype(np.float64)
    x = rng.randn(77, 13).astype(np.float32)
    for flags in (3, 7, 2, 6):
        ref = np.stack([O.forward(th[k], sizes, trs[k], x, 0, flags) for k in range(2)])
        out = _rounded(ref)
        assert C.col_err(out, ref)[0] < BARS["fwd"]
        assert all(C.masked_bad(out[k], x, 2, flags & O.RES) == 0 for k in range(2))
        bad = out.copy()
        bad[1, 40, 2] += 1e-6                                      # one masked entry not exactly 0 (or x)
        assert C.masked_bad(bad[1], x, 2, flags & O.RES) == 1
        bad = out.copy()
        bad[:, 64:] = np.nan                                       # the last 13 rows (a partial 32-row tile) never written
        assert C.unwritten(bad) and not C.col_err(bad, ref)[0] < BARS["fwd"]


def test_truncation_first_off_by_one_and_nan_member_are_flagged():
    rng = np.random.RandomState(6)
    sn = (rng.randn(700, 5) * 0.3).astype(np.float32)
    pred = (sn[None] + rng.randn(3, 700, 5) * 0.01).astype(np.float32)
    pred[1, [300, 520]] += 1.0
    pred[0, 100, 0] = np.nan
    pred[2, 100] += 1.0                       # a NaN member next to one over the limit: not a violation
    off, lim = np.array([0, 700]), 0.05
    err, first = O.pred_error(pred, sn, off, lim)
    assert first.tolist() == [300] and np.isnan(err[100])
    r = C.pred_err_errors(_rounded(err), first, err, first)
    assert r["err"] < BARS["trunc_err"] and r["nan"] == 0 and r["first"] == 0
    assert C.pred_err_errors(err, first + 1, err, first)["first"] == 1
    fmax = err.copy()                         # fmaxf: the NaN member dropped, the row truncated
    fmax[100] = np.max(np.mean((sn[100] - pred[:, 100].astype(np.float64)) ** 2, -1)[[1, 2]])
    assert C.pred_err_errors(fmax, np.array([100]), err, first)["nan"] == 1
    left = err.copy()
    left[650] = C.ERR_SENTINEL
    assert C.pred_err_errors(left, first, err, first)["unwritten"] == 1
