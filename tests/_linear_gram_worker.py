"""GPU worker of tests/test_gpu_linear_gram.py: every case of the Gram route (csrc/linear_policy.h) against oracle/npg_oracle.py in
fp64, in one process.  Prints one RESULT line: per case the errors of mjx_linear_moments and mjx_npg_update_linear (and, beside
them, of mjx_npg_update on the same case: the yardstick), then the checks that run once."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mjrl_amd import _lib  # noqa: E402
from mjrl_amd._lib import check, ptr  # noqa: E402
from oracle import npg_oracle as O  # noqa: E402
from tests._worker_dev import emit, ints, nan_block, checked_block, same_bits, stream, switch, up  # noqa: E402

CASES = [(1, 1, 33, True), (31, 32, 1500, True), (32, 1, 1025, True), (63, 17, 3000, True), (17, 6, 4099, False), (17, 6, 70001, True)]
ITERS, DAMPING, DELTA, TOL = 10, float(np.float32(1e-4)), 0.05, 1e-10
lib = _lib.load()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


class Case:
    """inputs as the device sees them (fp32), the oracle's view of them (the same values in fp64), and a context bound to them"""

    def __init__(self, n, m, N, transforms, seed=0, n_global=None):
        rng = np.random.RandomState(1000 * n + m + seed)
        self.n, self.m, self.N, self.d = n, m, N, m * n + 2 * m
        self.obs = (rng.randn(N, n) * (1 + 2 * rng.rand(n)) + rng.randn(n)).astype(np.float32)
        self.act = (0.7 * rng.randn(N, m)).astype(np.float32)
        self.adv = O.whiten(rng.randn(N) * 2.0 + 0.3).astype(np.float32)
        self.theta = np.concatenate([0.3 * rng.randn(m * n) / np.sqrt(n), 0.1 * rng.randn(m), -0.5 + 0.2 * rng.randn(m)]).astype(np.float32)
        tr = [0.3 * rng.randn(n), 0.5 + rng.rand(n), 0.2 * rng.randn(m), 0.5 + rng.rand(m)] if transforms else \
            [np.zeros(n), np.ones(n), np.zeros(m), np.ones(m)]
        self.tr = np.concatenate(tr).astype(np.float32)
        self.otr = O.Transforms(n, m, *np.split(self.tr, [n, 2 * n, 2 * n + m]))
        self.o64 = [x.astype(np.float64) for x in (self.theta, self.obs, self.act, self.adv)]
        self.ctx = ctypes.c_void_p()
        check(lib.mjx_create(ctypes.byref(self.ctx), 0, n, m, ints([]), 0))
        self.dev = [up(x) for x in (self.obs, self.act, self.adv, self.theta, self.theta, self.tr)]
        o, a, w, tn, to, t = self.dev
        check(lib.mjx_bind_batch(self.ctx, ptr(o), ptr(a), ptr(w), N, n_global or N))
        check(lib.mjx_bind_policy(self.ctx, ptr(tn), ptr(to), ptr(t), ptr(t), 1))

    def oracle(self, **kw):
        th, o, a, w = self.o64
        return O.npg_update(th.copy(), o, a, w, self.n, self.m, (), self.otr, cg_iters=ITERS, damping=DAMPING, delta=DELTA, **kw)

    def update(self, linear=True, tol=TOL, const_alpha=None, min_log_std=-3.0):
        """one update from the bound state -> dict(route, grad, x, theta, res); the context is bound again afterwards"""
        g, x, th, res = nan_block(self.d), nan_block(self.d), nan_block(self.d), torch.full((16,), -7.0, dtype=torch.float64, device="cuda:0")
        route = ctypes.c_int32(-1)
        args = [self.ctx, ITERS, DAMPING, tol, DELTA, float("nan") if const_alpha is None else const_alpha, min_log_std, ptr(g), ptr(x), ptr(th),
                ptr(res), stream()]
        check(lib.mjx_npg_update_linear(*args, ctypes.byref(route)) if linear else lib.mjx_npg_update(*args))
        out = dict(route=route.value, grad=checked_block(g, self.d, "grad"), x=checked_block(x, self.d, "x"),
                   theta=checked_block(th, self.d, "theta"), res=res.cpu().numpy())
        check(lib.mjx_bind_policy(self.ctx, ptr(self.dev[3]), ptr(self.dev[4]), ptr(self.dev[5]), ptr(self.dev[5]), 1))
        return out

    def errors(self, u, ref):
        """an update against the oracle's: the quantities tests/test_gpu_parity.py puts bars on"""
        r, N = u["res"], self.N
        return dict(x=rel(u["x"], ref["npg"]), step=rel(u["theta"].astype(np.float64) - self.o64[0], ref["new_params"] - self.o64[0]),
                    grad=rel(u["grad"], ref["vpg"]), surr_after=abs(r[0] / N - ref["surr_after"]), kl=abs(r[1] / N - ref["kl"]) / ref["kl"],
                    surr_before=abs(r[4] / N - ref["surr_before"]), count=r[5], gx=abs(r[8] - ref["vpg"].dot(ref["npg"])) / abs(r[8]),
                    alpha=abs(r[9] - ref["alpha"]) / ref["alpha"])

    def moments(self):
        L = 32 if self.n < 32 else 64
        cnt = L * L + self.m * L + self.m + 4
        blk = nan_block(cnt, torch.float64)
        check(lib.mjx_linear_moments(self.ctx, ptr(blk), stream()))
        return checked_block(blk, cnt, "moment block"), L

    def close(self):
        torch.cuda.synchronize(); lib.mjx_destroy(self.ctx)


def fisher_from_G(c, G, L, v):
    """the closed form of the issue, NumPy fp64: (F v)_[W|b] = diag(c) P G, (F v)_log_std = s .* v_log_std"""
    n, m = c.n, c.m
    u, eps, osc = np.exp(c.o64[0][-m:]) ** 2, 1e-8, c.otr.out_scale
    P = np.zeros((m, L)); P[:, :n] = v[:m * n].reshape(m, n); P[:, n] = v[m * n:m * n + m]
    FP = (2.0 / (2.0 * u + eps) * osc ** 2)[:, None] * (P @ G)
    return np.concatenate([FP[:, :n].ravel(), FP[:, n], 4 * u * (2 * u - eps) / (2 * u + eps) ** 2 * v[-m:]])


def run_case(n, m, N, transforms):
    c = Case(n, m, N, transforms)
    th, o, a, w = c.o64
    blk, L = c.moments()
    blk2, _ = c.moments()
    G, gWb, rest = blk[:L * L].reshape(L, L) / N, blk[L * L:L * L + m * L].reshape(m, L) / N, blk[L * L + m * L:]
    v = np.random.RandomState(7).randn(c.d)
    g = np.concatenate([gWb[:, :n].ravel(), gWb[:, n], rest[:m] / N])
    out = dict(fvp=rel(fisher_from_G(c, G, L, v), O.fvp(th, o, v, n, m, (), c.otr)), vpg=rel(g, O.vpg(th, th, o, a, w, n, m, (), c.otr, c.otr)),
               surr=abs(rest[m] / N - O.surrogate(th, th, o, a, w, n, m, (), c.otr, c.otr)), rows=rest[m + 1], tail=[rest[m + 2], rest[m + 3]],
               same_bits=same_bits(blk, blk2), pad=float(np.abs(G[n + 1:]).max(initial=0.0) + np.abs(gWb[:, n + 1:]).max(initial=0.0)))
    ref = c.oracle()
    u1, u0 = c.update(True), c.update(False)
    out.update(route=u1["route"], gram=c.errors(u1, ref), layerwise=c.errors(u0, ref))
    c.close()
    return out


def cg_residuals(c, g):
    """r.r after each iteration of the reference's CG in fp64 (oracle/npg_oracle.py cg_solve, without the break)"""
    th, o = c.o64[:2]
    res = []
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rr = r.dot(r)
    for _ in range(ITERS):
        z = O.fvp(th, o, p, c.n, c.m, (), c.otr, DAMPING)
        al = rr / p.dot(z)
        x += al * p; r -= al * z
        nw = r.dot(r); p = r + (nw / rr) * p; rr = nw
        res.append(rr)
    return res


def run_once():
    out = {}
    c = Case(17, 6, 4099, True, seed=1)
    th, o, a, w = c.o64
    # the clamp: min_log_std above every stepped log_std
    ref = c.oracle(min_log_std=0.25)
    u = c.update(min_log_std=0.25)
    out["clamp"] = dict(step=rel(u["theta"] - th, ref["new_params"] - th), log_std=u["theta"][-6:].tolist())
    # a constant step length: results[9] keeps what it held
    ref = c.oracle(const_alpha=0.125)
    u = c.update(const_alpha=0.125)
    out["const_alpha"] = dict(step=rel(u["theta"] - th, ref["new_params"] - th), slot9=u["res"][9])
    # the early break, on the one-feature case (d = 3): tol between the first two consecutive fp64 residuals that lie 100x apart
    b = Case(1, 1, 33, True)
    bt, bo, ba, bw = b.o64
    g = O.vpg(bt, bt, bo, ba, bw, 1, 1, (), b.otr, b.otr)
    res = cg_residuals(b, g)
    k = next(i for i in range(ITERS - 1) if res[i] >= 100 * res[i + 1])
    tol = float(np.sqrt(res[k] * res[k + 1]))
    f = lambda p: O.fvp(bt, bo, p, 1, 1, (), b.otr, DAMPING)
    x_break = O.cg_solve(f, g, ITERS, tol)
    out["break"] = dict(k=k, above=res[k] / tol, below=tol / res[k + 1], oracle_is_k=rel(O.cg_solve(f, g, k + 2, 0.0), x_break),
                        one_less=rel(O.cg_solve(f, g, k + 1, 0.0), x_break), one_more=rel(O.cg_solve(f, g, k + 3, 0.0), x_break),
                        x=rel(b.update(tol=tol)["x"], x_break))
    b.close()
    # the switch: route 0, the bits of mjx_npg_update
    with switch("MJX_LINEAR_GRAM", "0"):
        off = c.update(True)
    on = c.update(False)
    out["switch"] = dict(route=off["route"], same=all(same_bits(off[k], on[k]) for k in ("grad", "x", "theta", "res")))
    # a twin rank: world 2 through the transport hook, which doubles every buffer it is handed
    one = c.update(True)
    c.close()
    c2 = Case(17, 6, 4099, True, seed=1, n_global=2 * 4099)
    calls = []

    def hook(user, buf, count, dtype, st):
        h = np.empty(count, np.float64 if dtype else np.float32)
        check(lib.mjx_memcpy_d2h(h.ctypes.data_as(ctypes.c_void_p), buf, h.nbytes, st)); check(lib.mjx_stream_sync(st))
        h *= 2
        check(lib.mjx_memcpy_h2d(buf, h.ctypes.data_as(ctypes.c_void_p), h.nbytes, st)); check(lib.mjx_stream_sync(st))
        calls.append((int(count), int(dtype)))
        return 0
    fn = _lib.REDUCE_FN(hook)
    check(lib.mjx_comm_set_callback(c2.ctx, fn, None, 2))
    two = c2.update(True)
    L = 32
    out["twin"] = dict(calls=calls, want=[[L * L + 6 * L + 6 + 4, 1], [4, 1]], route=two["route"], theta=rel(two["theta"], one["theta"].astype(np.float64)),
                       x=rel(two["x"], one["x"].astype(np.float64)), res=float(np.abs(two["res"][[0, 1, 4, 5]] / 2 - one["res"][[0, 1, 4, 5]]).max()
                                                                               / np.abs(one["res"][[0, 1, 4, 5]]).max()))
    c2.close()
    return out


if __name__ == "__main__":
    payload = {"%d_%d_%d" % cs[:3]: run_case(*cs) for cs in CASES}
    payload["once"] = run_once()
    emit(payload)
