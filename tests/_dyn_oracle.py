"""fp64 NumPy oracle for the model-based NPG operations (csrc/dynamics.h): DynamicsNet / RewardNet forward
(reference nn_dynamics.py:230-245, 313-328), torch.optim.Adam steps of fit_model (:344-385), a learned-model rollout given
its noise (sampling.py:16-89, enforce_tensor_bounds :286-315), its single steps for a teacher-forced check, and the
ensemble-disagreement truncation (model_accel_npg.py:139-150)."""
import numpy as np

AFF, MASK, RES = 1, 2, 4
# Adam's coefficients (beta1, 1 - beta1, beta2, 1 - beta2) and the betas of the bias corrections.  ADAM_F64: the Python scalars;
# ADAM_TORCH: what torch.optim.Adam hands its fp32 kernels -- each double rounded ONCE to fp32 -- with the corrections still
# from the double betas (tests/_fit_oracle.py)
ADAM_F64 = (0.9, 0.1, 0.999, 0.001, 0.9, 0.999)
ADAM_TORCH = tuple(float(np.float32(c)) for c in (0.9, 0.1, 0.999, 0.001)) + (0.9, 0.999)


def unflatten(theta, sizes):
    Ws, bs, k = [], [], 0
    for i in range(len(sizes) - 1):
        Ws.append(theta[k:k + sizes[i] * sizes[i + 1]].reshape(sizes[i + 1], sizes[i])); k += sizes[i] * sizes[i + 1]
        bs.append(theta[k:k + sizes[i + 1]]); k += sizes[i + 1]
    return Ws, bs


def act_fn(x, act):
    return np.tanh(x) if act == 1 else np.maximum(x, 0.0)


def forward(theta, sizes, tr, x, act, flags, keep=False):
    """tr = [in_shift, in_scale, out_shift, out_scale] over the concatenated input; None: the exact identity (no 1e-8), flags 0"""
    theta, x = np.asarray(theta, np.float64), np.asarray(x, np.float64)
    din, dout = sizes[0], sizes[-1]
    Ws, bs = unflatten(theta, sizes)
    if tr is None:
        assert flags == 0
        tr = np.zeros(2 * (din + dout))
        h = x
    else:
        tr = np.asarray(tr, np.float64)
        h = (x - tr[:din]) / (tr[din:2 * din] + 1e-8)
    hs = [h]
    for i, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W.T + b
        if i < len(Ws) - 1:
            h = act_fn(h, act)
        hs.append(h)
    osh, osc = tr[2 * din:2 * din + dout], tr[2 * din + dout:]
    if flags & AFF:
        h = h * (osc + 1e-8) + osh
    if flags & MASK:
        h = h * (osc >= 1e-8)
    if flags & RES:
        h = h + x[:, :dout]
    return (h, hs) if keep else h


def adam_steps(theta, sizes, tr, x, y, idx, batch, act, tmode, lr, wd, m=None, v=None, t0=0, g_first=None, coef=ADAM_F64):
    """fit_model's Adam steps in fp64: tmode 0 = loss through the output affine on raw y, 1 = (y - out_shift) /
    (out_scale + 1e-8), 2 = residual targets.  -> (theta, m, v, per-step losses).  g_first: an array that takes |gradient|
    (weight decay included) of the first step.  tr None (tmode 0): no transforms at all, the plain MSE of the net's output"""
    theta = np.array(theta, np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64).reshape(len(x), -1)
    din, dout = sizes[0], sizes[-1]
    if tr is None:
        assert tmode == 0
        osh, osc = np.zeros(dout), None
    else:
        tr = np.asarray(tr, np.float64)
        osh, osc = tr[2 * din:2 * din + dout], tr[2 * din + dout:]
    if tmode == 2:
        tg = (y - x[:, :dout] - osh) / (osc + 1e-8)
    elif tmode == 1:
        tg = (y - osh) / (osc + 1e-8)
    else:
        tg = y
    m = np.zeros_like(theta) if m is None else np.array(m, np.float64)
    v = np.zeros_like(theta) if v is None else np.array(v, np.float64)
    losses = []
    steps = len(idx) // batch
    for s in range(steps):
        rows = idx[s * batch:(s + 1) * batch]
        _, hs = forward(theta, sizes, tr, x[rows], act, 0, keep=True)
        z = hs[-1]
        sc = (osc + 1e-8) if tmode == 0 and osc is not None else 1.0
        yh = z * sc + (osh if tmode == 0 else 0.0)
        err = yh - tg[rows]
        losses.append(np.mean(err ** 2))
        dz = 2.0 * err * sc / err.size
        Ws, _ = unflatten(theta, sizes)
        g = np.zeros_like(theta)
        gW, gb = unflatten(g, sizes)
        for l in range(len(Ws) - 1, -1, -1):
            gW[l][...] = dz.T @ hs[l]
            gb[l][...] = dz.sum(0)
            if l > 0:
                da = dz @ Ws[l]
                dz = da * ((1.0 - hs[l] ** 2) if act == 1 else (hs[l] > 0))
        t = t0 + s + 1
        g = g + wd * theta
        if g_first is not None and s == 0:
            g_first[...] = np.abs(g)
        theta, m, v = adam_update(theta, g, m, v, t, lr, coef)
    return theta, m, v, np.array(losses)


def adam_update(theta, g, m, v, t, lr, coef=ADAM_F64):
    """step t (1-based) of torch.optim.Adam (eps 1e-8; weight decay already in g) -> (theta, m, v)"""
    b1, c1, b2, c2, bb1, bb2 = coef
    m = b1 * m + c1 * g
    v = b2 * v + c2 * g * g
    return theta - lr / (1 - bb1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - bb2 ** t) + 1e-8), m, v


def policy_mean(pol_theta, pol_sizes, pol_tr, s):
    """the tanh FCNetwork's mean (fc_network.py:39-52) of states s (rows x n) -> (mean (rows x m), log_std (m));
    pol_theta = [W1, b1, ..., W_out, b_out, log_std], pol_tr = [in_shift n, in_scale n, out_shift m, out_scale m]"""
    n, m = pol_sizes[0], pol_sizes[-1]
    pt, ptr = np.asarray(pol_theta, np.float64), np.asarray(pol_tr, np.float64)
    P = pt.size - m
    Ws, bs = unflatten(pt[:P], pol_sizes)
    h = (np.asarray(s, np.float64) - ptr[:n]) / (ptr[n:2 * n] + 1e-8)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W.T + b
        if i < len(Ws) - 1:
            h = np.tanh(h)
    return h * ptr[2 * n + m:] + ptr[2 * n:2 * n + m], pt[P:]


def clamp(x, lo, hi):
    """torch.max(torch.min(x, hi), lo) (sampling.py:315)"""
    return np.maximum(np.minimum(x, hi), lo)


def rollout_action(s, pol_theta, pol_sizes, pol_tr, noise=None, bounds=None):
    """one step's action from the states s: clamp(policy_mean(s) + noise * exp(log_std))"""
    a, ls = policy_mean(pol_theta, pol_sizes, pol_tr, s)
    if noise is not None:
        a = a + np.asarray(noise, np.float64) * np.exp(ls)
    return clamp(a, bounds[0], bounds[1]) if bounds is not None else a


def rollout_next(s, a, dyn_theta, dyn_sizes, dyn_tr, act, flags, bounds=None):
    """one step's next states: clamp(f([s, a]))"""
    x = np.concatenate([np.asarray(s, np.float64), np.asarray(a, np.float64)], -1)
    s = forward(dyn_theta, dyn_sizes, dyn_tr, x, act, flags)
    return clamp(s, bounds[2], bounds[3]) if bounds is not None else s


def pred_error(pred, s_next, off, lim):
    """model_accel_npg.py:139-150 as written, per segment [off[g], off[g+1]) of rows: pred_err starts from zeros and takes
    np.maximum with each model's mean squared error in model order; -> (pred_err per row, first violating row per segment or
    -1).  pred: K x rows x n, s_next: rows x n, both taken as they are (fp32 values in fp64)."""
    pred, s_next = np.asarray(pred, np.float64), np.asarray(s_next, np.float64)
    errs, first = np.zeros(s_next.shape[0]), []
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(len(off) - 1):
            a0, a1 = int(off[g]), int(off[g + 1])
            pred_err = np.zeros(a1 - a0)
            for k in range(pred.shape[0]):
                model_err = np.mean((s_next[a0:a1] - pred[k, a0:a1]) ** 2, axis=-1)
                pred_err = np.maximum(pred_err, model_err)
            violations = np.where(pred_err > lim)[0]
            errs[a0:a1] = pred_err
            first.append(int(violations[0]) if len(violations) else -1)
    return errs, np.array(first, np.int64)


def rollout(s0, H, pol_theta, pol_sizes, pol_tr, noise, dyn_thetas, dyn_sizes, dyn_trs, act, flags, bounds=None, actions=None):
    """-> obs (K, N, H, n), act (K, N, H, m); bounds = (a_lo, a_hi, s_lo, s_hi) arrays or None; noise (K, H, N, m) or None"""
    s0 = np.asarray(s0, np.float64)
    K, (N, n) = len(dyn_thetas), s0.shape
    m = dyn_sizes[0] - n
    obs, acts = np.zeros((K, N, H, n)), np.zeros((K, N, H, m))
    if pol_theta is not None:
        pt = np.asarray(pol_theta, np.float64)
        P = pt.size - m
        Ws, bs = unflatten(pt[:P], pol_sizes)
        ls = pt[P:]
        ptr = np.asarray(pol_tr, np.float64)
    for k in range(K):
        s = s0.copy()
        for t in range(H):
            if pol_theta is not None:
                h = (s - ptr[:n]) / (ptr[n:2 * n] + 1e-8)
                for i, (W, b) in enumerate(zip(Ws, bs)):
                    h = h @ W.T + b
                    if i < len(Ws) - 1:
                        h = np.tanh(h)
                a = h * ptr[2 * n + m:] + ptr[2 * n:2 * n + m]
                if noise is not None:
                    a = a + np.asarray(noise[k, t], np.float64) * np.exp(ls)
            else:
                a = np.asarray(actions[:, t], np.float64)
            if bounds is not None:
                a = np.maximum(np.minimum(a, bounds[1]), bounds[0])
            obs[k, :, t], acts[k, :, t] = s, a
            s = forward(dyn_thetas[k], dyn_sizes, dyn_trs[k], np.concatenate([s, a], 1), act, flags)
            if bounds is not None:
                s = np.maximum(np.minimum(s, bounds[3]), bounds[2])
    return obs, acts
