"""Comparison helpers of the learned-dynamics fp64 tests (tests/test_gpu_dynamics_matrix.py): column-wise errors of a device
result against tests/_dyn_oracle.py, the teacher-forced rollout check, the fit's error in units of lr, the truncation's
comparison with the reference expression, and the sentinel counts that show every output element was written.

tests/test_dynamics_checks.py shows on CPU that each defect a wrong kernel would leave (an unwritten tile, swapped noise, a
skipped clamp, a dropped shift, an off-by-one bias correction, a masked column that is not zero, an off-by-one first violation)
is flagged at the bars the GPU module uses."""
import numpy as np

from tests import _dyn_oracle as O


def rand_theta(rng, sizes, K=None, gain=1.0):
    """flat parameters ([W1, b1, ..., W_out, b_out]; K x that with K) at torch.nn.Linear's scale (~1 / sqrt(fan_in)) per layer,
    so that deep and wide nets keep O(1) activations"""
    def one():
        parts = []
        for i in range(len(sizes) - 1):
            s = gain / np.sqrt(sizes[i])
            parts += [rng.uniform(-s, s, sizes[i] * sizes[i + 1]) * 1.7, rng.uniform(-s, s, sizes[i + 1])]
        return np.concatenate(parts)
    return (np.stack([one() for _ in range(K)]) if K else one()).astype(np.float32)


def rand_tr(rng, din, dout, zero_col=None):
    """transforms [in_shift, in_scale, out_shift, out_scale]; zero_col: that output's out_scale = 0 (a masked column)"""
    tr = np.concatenate([rng.randn(din) * 0.3, rng.rand(din) + 0.5, rng.randn(dout) * 0.2, rng.rand(dout) + 0.3])
    if zero_col is not None:
        tr[2 * din + dout + zero_col] = 0.0
    return tr.astype(np.float32)


def col_err(dev, ref):
    """dev, ref: (groups, rows, cols) -> (worst error, (group, col)).  Each column of each group on its own:
    max_i |dev - ref| over the larger of the column's max |ref| and the group's rms -- a column that is small or zero (a masked
    one) carries the rounding of the group's typical size, not a larger relative one.  A NaN or inf where the reference is
    finite (a sentinel left in place) is an infinite error."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    if dev.size == 0:
        return 0.0, None
    rms = np.sqrt(np.mean(ref * ref, axis=(1, 2), keepdims=True))
    scale = np.maximum(np.max(np.abs(ref), axis=1, keepdims=True), np.maximum(rms, 1e-30))
    with np.errstate(invalid="ignore"):
        e = np.abs(dev - ref) / scale
    e = np.where(np.isfinite(e), e, np.inf)
    e = e.max(axis=1)
    g, j = np.unravel_index(int(np.argmax(e)), e.shape)
    return float(e[g, j]), (int(g), int(j))


def unwritten(a):
    """NaN-sentinel entries left in a device result"""
    return int(np.isnan(np.asarray(a, np.float64)).sum())


def masked_bad(out, x, col, residual):
    """entries of a masked output column that are not exactly 0 (or exactly x[:, col] with the residual): out (K, rows, d_out)"""
    want = np.asarray(x, np.float32)[..., col] if residual else 0.0
    return int(np.sum(np.asarray(out)[..., col] != want))


def by_step(a):
    """(K, N, H, c) -> (K, H, N, c): groups per member and step"""
    return np.asarray(a).transpose(0, 2, 1, 3)


def teacher_forced(obs, act, pol, noise, dyn, bounds, actions=None):
    """the device's own trajectories, one step at a time, in fp64:
        act[k, i, t]     = clamp(policy_mean(obs[k, i, t]) + noise[k, t, i] * exp(log_std))   (or clamp(actions[i, t]))
        obs[k, i, t + 1] = clamp(f_k(obs[k, i, t], act[k, i, t]))
    obs (K, N, H, n), act (K, N, H, m); pol = (theta, sizes, tr) or None with actions; noise (K, H, N, m) or None;
    dyn = (thetas, sizes, trs, act, flags); bounds = (a_lo, a_hi, s_lo, s_hi) or None.
    -> {"act": (err, (member, step, col)), "obs": (err, (member, step, col))}, each per member, per step and per column"""
    K, N, H, n = obs.shape
    m = act.shape[-1]
    dth, dsz, dtr, da, dfl = dyn
    res = {"act": (0.0, None), "obs": (0.0, None)}
    for k in range(K):
        S = by_step(obs[k:k + 1])[0].reshape(H * N, n).astype(np.float64)
        A = by_step(act[k:k + 1])[0].reshape(H * N, m).astype(np.float64)
        if actions is None:
            nz = None if noise is None else np.asarray(noise[k], np.float64).reshape(H * N, m)
            a_ref = O.rollout_action(S, pol[0], pol[1], pol[2], nz, bounds)
        else:
            a_ref = np.asarray(actions, np.float64).transpose(1, 0, 2).reshape(H * N, m)
            if bounds is not None:
                a_ref = O.clamp(a_ref, bounds[0], bounds[1])
        s_ref = O.rollout_next(S[:(H - 1) * N], A[:(H - 1) * N], dth[k], dsz, dtr[k], da, dfl, bounds)
        for key, dev, ref, steps in (("act", A, a_ref, H), ("obs", S[N:], s_ref, H - 1)):
            e, where = col_err(dev.reshape(steps, N, -1), ref.reshape(steps, N, -1))
            if e > res[key][0] or res[key][1] is None:
                res[key] = (e, None if where is None else (k, where[0] + (key == "obs"), where[1]))
    return res


def over_lr(p, ref, lr):
    """parameters after Adam steps: max |p - ref| in units of the step size lr"""
    return float(np.max(np.abs(np.asarray(p, np.float64) - np.asarray(ref, np.float64)))) / lr


def rel_max(a, b):
    """max |a - b| over max(1, max |b|): the losses, as tests/test_gpu_model_accel.py measures them"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


ERR_SENTINEL = -1.0      # truncation errors are >= 0 or NaN: a row left at -1 was not written, even where NaN is expected
FIRST_SENTINEL = -7


def pred_err_errors(err, first, err_ref, first_ref):
    """the truncation against O.pred_error -> {"err": worst |err - ref| / |ref| over the finite rows, "nan": rows whose NaN-ness
    (equal_nan) or infinity differs, "first": segments whose first violation differs, "unwritten": sentinels left}"""
    err, err_ref = np.asarray(err, np.float64), np.asarray(err_ref, np.float64)
    first, first_ref = np.asarray(first), np.asarray(first_ref)
    fin = np.isfinite(err_ref) & np.isfinite(err)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(err[fin] - err_ref[fin]) / np.maximum(np.abs(err_ref[fin]), 1e-30)
    nan_bad = np.sum(np.isnan(err) != np.isnan(err_ref)) + np.sum(np.isinf(err_ref) & ~(err == err_ref)) + \
        np.sum(np.isfinite(err_ref) & ~np.isfinite(err))
    return {"err": float(rel.max()) if rel.size else 0.0, "nan": int(nan_bad), "first": int(np.sum(first != first_ref)),
            "unwritten": int(np.sum(err == ERR_SENTINEL) + np.sum(first == FIRST_SENTINEL))}
