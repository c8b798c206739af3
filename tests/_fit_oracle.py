"""fp64 oracle and comparison helpers of the minibatch-Adam trainers (tests/test_gpu_fit_matrix.py): the MLP value baseline
(csrc/mlp_fit.h, mjx_mlp_fit_adam) and the policy fit of BC and PPO (csrc/policy_fit.h, mjx_policy_minibatch_adam).

The oracle follows torch, not the kernels: Adam's coefficients are 0.9f, 0.1f, 0.999f, 0.001f (each the double rounded once to
fp32: what torch.optim.Adam hands its fp32 kernels), the bias corrections come from the double betas, eps is 1e-8 and weight
decay is folded into the gradient (tests/_dyn_oracle.ADAM_TORCH, adam_update).  The policy's losses are the three that
k_minibatch_head documents (csrc/layerwise.h): MSE as the mean over B m elements of the post-affine mean against the action,
MLE as -mean log-likelihood, and the clipped surrogate -mean min(LR adv, clamp(LR, 1 - c, 1 + c) adv) with LR = exp(LL - LL_old),
LL_old a constant.  tests/test_fit_checks.py shows on CPU that the comparisons below flag the defects a wrong trainer leaves."""
import numpy as np

from oracle import npg_oracle as N
from tests import _dyn_oracle as O
from tests._dyn_check import col_err

GRAD_FLOOR = 3e-7        # a parameter whose first fp64 gradient is below this is ill-conditioned for any fp32 Adam: only counted
FS = 48                  # the feature slice one workgroup of the wide baseline trainer owns (MLPFIT_FS)


# ---------------------------------------------------------------- MLP baseline
def mlp_sizes(d_in, hidden=(128, 128)):
    return [d_in] + list(hidden) + [1]


def mlp_fit(theta, d_in, x, y, perm, N_, epochs, lr, wd, hidden=(128, 128), batch=64, m=None, v=None, t0=0, g_first=None,
            coef=O.ADAM_TORCH):
    """mjx_mlp_fit_adam in fp64: `epochs` x (N / batch - 1) steps over perm[e N + s batch ...] (optimize_model.py:7-36), the exact
    identity for the transforms -> (theta, m, v, epoch losses = sum of the epoch's minibatch mean squared errors)"""
    steps = N_ // batch - 1
    idx = np.concatenate([np.asarray(perm)[e * N_:e * N_ + steps * batch] for e in range(epochs)])
    th, m, v, losses = O.adam_steps(theta, mlp_sizes(d_in, hidden), None, x, y, idx, batch, 0, 0, lr, wd, m=m, v=v, t0=t0,
                                    g_first=g_first, coef=coef)
    return th, m, v, losses.reshape(epochs, steps).sum(1)


def mlp_blocks(d_in, hidden=(128, 128)):
    """[(name, flat indices)]: W1 per 48-feature slice (the workgroup that owns it in the wide trainer), b1, W2, b2, W3, b3"""
    h1, h2 = hidden
    W1 = np.arange(h1 * d_in).reshape(h1, d_in)
    out = [("W1[:, %d:%d]" % (f, min(f + FS, d_in)), W1[:, f:f + FS].ravel()) for f in range(0, d_in, FS)]
    k = h1 * d_in
    for name, cnt in (("b1", h1), ("W2", h1 * h2), ("b2", h2), ("W3", h2), ("b3", 1)):
        out.append((name, np.arange(k, k + cnt)))
        k += cnt
    return out


# ---------------------------------------------------------------- policy
def policy_blocks(n, m, hidden):
    ls = N.layer_sizes(n, m, hidden)
    out, k = [], 0
    for i in range(len(ls) - 1):
        for name, cnt in (("W%d" % (i + 1), ls[i] * ls[i + 1]), ("b%d" % (i + 1), ls[i + 1])):
            out.append((name, np.arange(k, k + cnt)))
            k += cnt
    out.append(("log_std", np.arange(k, k + m)))
    return out


def transforms(n, m, tr):
    """packed [in_shift n, in_scale n, out_shift m, out_scale m] -> oracle.npg_oracle.Transforms, in fp64"""
    tr = np.asarray(tr, np.float64)
    t = N.Transforms(n, m)
    t.in_shift, t.in_scale, t.out_shift, t.out_scale = tr[:n], tr[n:2 * n], tr[2 * n:2 * n + m], tr[2 * n + m:]
    return t


def policy_loss_grad(theta, n, m, hidden, tr, theta_old, tr_old, obs, act, adv, loss, track, clip, defect=None):
    """one minibatch -> (loss, gradient, PPO row statistics or None).  track 1: the old network runs on the CURRENT weights and
    transforms with the old log_std; 0: the old policy is theta_old / tr_old.  defect (tests/test_fit_checks.py only):
    "mse_over_B", "no_log_std_grad", "no_clip_mask" """
    B = obs.shape[0]
    Ws, bs, ls = N.unflatten(theta, n, m, hidden)
    mu, acts = N.forward(theta, obs, n, m, hidden, tr, keep=True)
    stats = None
    if loss == 0:
        e = mu - act
        val = np.mean(e * e)
        dmu = 2.0 * e / (B if defect == "mse_over_B" else B * m)
        g_s = np.zeros(m)
    else:
        sig = np.exp(ls)
        z = (act - mu) / sig
        ll = -0.5 * np.sum(z * z, axis=1) - np.sum(ls) - 0.5 * m * N.LOG_2PI
        if loss == 1:
            val, w = -np.mean(ll), np.full(B, -1.0 / B)
        else:
            ls_old = N.unflatten(theta_old, n, m, hidden)[2]
            mu_old = mu if track else N.forward(theta_old, obs, n, m, hidden, tr_old)
            zo = (act - mu_old) / np.exp(ls_old)
            ll_old = -0.5 * np.sum(zo * zo, axis=1) - np.sum(ls_old) - 0.5 * m * N.LOG_2PI
            LR = np.exp(ll - ll_old)
            s1, s2 = LR * adv, np.clip(LR, 1.0 - clip, 1.0 + clip) * adv
            val = -np.mean(np.minimum(s1, s2))
            live = ((LR >= 1.0 - clip) & (LR <= 1.0 + clip)) | (s1 < s2)        # the unclipped branch is (co-)active
            stats = {"unclipped": int(live.sum()), "clipped": int((~live).sum()), "adv_pos": int((adv > 0).sum()),
                     "adv_neg": int((adv < 0).sum()),
                     "near": int(np.sum(np.minimum(np.abs(LR - (1.0 - clip)), np.abs(LR - (1.0 + clip))) < 1e-4))}
            if defect == "no_clip_mask":
                live = np.ones(B, bool)
            w = -adv * LR * live / B
        dmu = w[:, None] * z / sig
        g_s = np.zeros(m) if defect == "no_log_std_grad" else (w[:, None] * (z * z - 1.0)).sum(0)
    grads = N._backprop(Ws, acts, dmu, tr.out_scale)
    return val, N.flatten([g[0] for g in grads], [g[1] for g in grads], g_s), stats


def policy_fit(theta, n, m, hidden, tr, theta_old, tr_old, obs, act, adv, idx, B, loss, track, lr, clip, am=None, av=None, t0=0,
               g_first=None, coef=O.ADAM_TORCH, defect=None):
    """mjx_policy_minibatch_adam in fp64 (no weight decay; MSE leaves log_std and its moments alone: no gradient there)
    -> (theta, m, v, per-step losses, PPO statistics summed over the steps or None)"""
    theta, theta_old = np.array(theta, np.float64), np.asarray(theta_old, np.float64)
    obs, act, adv = (np.asarray(a, np.float64) for a in (obs, act, adv))
    tr, tr_old = transforms(n, m, tr), transforms(n, m, tr_old)
    am = np.zeros_like(theta) if am is None else np.array(am, np.float64)
    av = np.zeros_like(theta) if av is None else np.array(av, np.float64)
    d = theta.size
    live = slice(0, d - m if loss == 0 else d)
    losses, total = [], None
    for s in range(len(idx) // B):
        rows = np.asarray(idx[s * B:(s + 1) * B])
        val, g, st = policy_loss_grad(theta, n, m, hidden, tr, theta_old, tr_old, obs[rows], act[rows], adv[rows], loss, track, clip,
                                      defect)
        losses.append(val)
        if st is not None:
            total = st if total is None else {k: total[k] + st[k] for k in st}
        if g_first is not None and s == 0:
            g_first[...] = np.abs(g)
        theta[live], am[live], av[live] = O.adam_update(theta[live], g[live], am[live], av[live], t0 + s + 1, lr, coef)
    return theta, am, av, np.array(losses), total


# ---------------------------------------------------------------- comparisons
def param_errors(p, ref, blocks, lr, well=None):
    """per block: (worst |p - ref| / lr over the well-conditioned parameters, its flat index); a NaN counts as infinite"""
    p, ref = np.asarray(p, np.float64), np.asarray(ref, np.float64)
    out = {}
    for name, ix in blocks:
        if well is not None:
            ix = ix[well[ix]]
        if ix.size == 0:
            continue
        e = np.abs(p[ix] - ref[ix]) / lr
        e = np.where(np.isfinite(e), e, np.inf)
        k = int(np.argmax(e))
        out[name] = (float(e[k]), int(ix[k]))
    return out


def moment_errors(q, ref, blocks):
    """per block: (worst |q - ref| over the block's own largest |ref|, its flat index) -- element-wise, not a norm.  A block
    whose reference is all zero (log_std under MSE) is compared exactly elsewhere"""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    out = {}
    for name, ix in blocks:
        if not np.any(ref[ix]):
            continue
        e, _ = col_err(q[ix].reshape(1, -1, 1), ref[ix].reshape(1, -1, 1))
        with np.errstate(invalid="ignore"):
            d = np.abs(q[ix] - ref[ix])
        k = int(np.argmax(np.where(np.isfinite(d), d, np.inf)))
        out[name] = (e, int(ix[k]))
    return out


def moment_bias(q, ref, blocks, min_entries=64):
    """per block of at least min_entries: (|sum (q - ref)| / sum |ref|, the block's first index).  For the second moment after
    ONE step, v = (1 - beta2) g^2: every entry has one sign, rounding averages out of the sums, and a coefficient that is off
    (1.0f - 0.999f is 1.3e-5 low) does not -- element by element the same 1.3e-5 can hide under the rounding of a gradient.
    (Later steps compound through the parameters, and a few entries do not average.)"""
    q, ref = np.asarray(q, np.float64), np.asarray(ref, np.float64)
    out = {}
    for name, ix in blocks:
        if ix.size >= min_entries and np.any(ref[ix]):
            e = abs(np.sum(q[ix] - ref[ix])) / np.sum(np.abs(ref[ix]))
            out[name] = (float(e) if np.isfinite(e) else np.inf, int(ix[0]))
    return out


def worst(errs):
    """{block: (err, index)} -> (err, block, index) of the worst block"""
    name = max(errs, key=lambda k: errs[k][0])
    return errs[name][0], name, errs[name][1]


def rel_losses(l, ref):
    """worst |l - ref| / max(1, |ref|) entry by entry (a PPO minibatch loss is a sum of cancelling O(1) terms)"""
    l, ref = np.asarray(l, np.float64), np.asarray(ref, np.float64)
    e = np.abs(l - ref) / np.maximum(1.0, np.abs(ref))
    return float(np.max(np.where(np.isfinite(e), e, np.inf)))


def tail_intact(buf, used):
    """the NaN guard behind the first `used` entries of a device buffer is still all NaN, and every real entry is finite"""
    buf = np.asarray(buf)
    return bool(np.all(np.isnan(buf[used:])) and np.all(np.isfinite(buf[:used])))
