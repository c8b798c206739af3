"""fp64 NumPy oracle for the model-based NPG operations (csrc/dynamics.h): DynamicsNet / RewardNet forward
(reference nn_dynamics.py:230-245, 313-328), torch.optim.Adam steps of fit_model (:344-385) and a learned-model rollout given
its noise (sampling.py:16-89, enforce_tensor_bounds :286-315)."""
import numpy as np

AFF, MASK, RES = 1, 2, 4


def unflatten(theta, sizes):
    Ws, bs, k = [], [], 0
    for i in range(len(sizes) - 1):
        Ws.append(theta[k:k + sizes[i] * sizes[i + 1]].reshape(sizes[i + 1], sizes[i])); k += sizes[i] * sizes[i + 1]
        bs.append(theta[k:k + sizes[i + 1]]); k += sizes[i + 1]
    return Ws, bs


def act_fn(x, act):
    return np.tanh(x) if act == 1 else np.maximum(x, 0.0)


def forward(theta, sizes, tr, x, act, flags, keep=False):
    """tr = [in_shift, in_scale, out_shift, out_scale] over the concatenated input"""
    theta, tr, x = (np.asarray(v, np.float64) for v in (theta, tr, x))
    din, dout = sizes[0], sizes[-1]
    Ws, bs = unflatten(theta, sizes)
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


def adam_steps(theta, sizes, tr, x, y, idx, batch, act, tmode, lr, wd, m=None, v=None, t0=0):
    """fit_model's Adam steps in fp64: tmode 0 = loss through the output affine on raw y, 1 = (y - out_shift) /
    (out_scale + 1e-8), 2 = residual targets.  -> (theta, m, v, per-step losses)"""
    theta = np.array(theta, np.float64)
    x, y, tr = np.asarray(x, np.float64), np.asarray(y, np.float64).reshape(len(x), -1), np.asarray(tr, np.float64)
    din, dout = sizes[0], sizes[-1]
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
        sc = (osc + 1e-8) if tmode == 0 else 1.0
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
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        theta = theta - lr / (1 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8)
    return theta, m, v, np.array(losses)


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
