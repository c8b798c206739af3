"""GPU worker of tests/test_gpu_linear_gram_trpo_dapg.py: TRPO and DAPG on the Gram route (mjx_trpo_update_linear,
mjx_dapg_update_linear, mjx_linear_moments_segments) against oracle/npg_oracle.py in fp64, every case once, one RESULT line."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mjrl_amd import _lib  # noqa: E402
from mjrl_amd._lib import check, ptr  # noqa: E402
from oracle import npg_oracle as O  # noqa: E402
from tests._linear_gram_worker import DAMPING, ITERS, TOL, Case, lib, rel  # noqa: E402
from tests._worker_dev import checked_block, emit, nan_block, same_bits, stream, switch, up  # noqa: E402

DAPG_CASES = [(1, 1, 33, 1), (31, 32, 1024, 40), (32, 1, 1025, 31), (63, 17, 3000, 1056), (17, 6, 4099, 200)]
TRPO_CASES = [(1, 1, 33, 1), (32, 1, 1025, 0), (63, 17, 3000, 0), (17, 6, 4099, 1)]          # (n, m, N, seed): seeds fixed on the CPU oracle
KL = 0.025


def rebind(c, N, n_global=None):
    o, a, w, tn, to, t = c.dev
    check(lib.mjx_bind_batch(c.ctx, ptr(o), ptr(a), ptr(w), N, n_global or N))
    check(lib.mjx_bind_policy(c.ctx, ptr(tn), ptr(to), ptr(t), ptr(t), 1))


def call(c, fn, head, n_global=None, routed=True):
    """fn(*head, grad, x, theta, results, stream[, &route]) on NaN-prefilled outputs -> dict; the whole batch is bound again behind it"""
    g, x, th, res = nan_block(c.d), nan_block(c.d), nan_block(c.d), torch.full((64,), -7.0, dtype=torch.float64, device="cuda:0")
    route = ctypes.c_int32(-1)
    check(fn(*head, ptr(g), ptr(x), ptr(th), ptr(res), stream(), *([ctypes.byref(route)] if routed else [])))
    u = dict(route=route.value, grad=checked_block(g, c.d, "grad"), x=checked_block(x, c.d, "x"), theta=checked_block(th, c.d, "theta"),
             res=res.cpu().numpy())
    rebind(c, c.N, n_global)
    return u


class Dapg(Case):
    """[N_on on-policy ; N_demo demonstration] rows with the advantages of dapg.py:62-70 bound, adv_on apart"""

    def __init__(self, n, m, N_on, N_demo, world=1):
        super().__init__(n, m, N_on + N_demo, True, seed=1)
        self.N_on, self.world = N_on, world
        self.adv_on = O.whiten(np.random.RandomState(5).randn(N_on) * 2.0 + 0.3).astype(np.float32)
        a64 = self.adv_on.astype(np.float64)
        self.dev[2] = up(1e-2 * np.concatenate([a64 / (np.std(a64) + 1e-8), np.ones(N_demo)]))
        self.adv_on_dev = up(self.adv_on)
        rebind(self, self.N, world * self.N)

    def update(self, linear=True):
        head = [self.ctx, ITERS, DAMPING, TOL, 2 * KL, -3.0, self.N_on, self.world * self.N_on, ptr(self.adv_on_dev)]
        return call(self, lib.mjx_dapg_update_linear if linear else lib.mjx_dapg_update, head, self.world * self.N, routed=linear)

    def block(self, segments):
        L = 32 if self.n < 32 else 64
        cnt = L * L + self.m * L + self.m + 4
        blk = nan_block(cnt, torch.float64)
        check(lib.mjx_linear_moments_segments(self.ctx, self.N_on, ptr(self.adv_on_dev), ptr(blk), stream()) if segments
              else lib.mjx_linear_moments(self.ctx, ptr(blk), stream()))
        return checked_block(blk, cnt, "moment block"), L


def run_dapg(n, m, N_on, N_demo):
    c = Dapg(n, m, N_on, N_demo)
    th, o, a, _ = c.o64
    ref = O.dapg_update(th.copy(), o[:N_on], a[:N_on], c.adv_on.astype(np.float64), o[N_on:], a[N_on:], n, m, (), c.otr, cg_iters=ITERS,
                        damping=DAMPING, kl_dist=KL)
    u, u2 = c.update(), c.update()
    blk, L = c.block(True)
    rebind(c, N_on)                                    # the on-policy prefix alone
    alone, _ = c.block(False)
    G, gWb, r = blk[:L * L].reshape(L, L), blk[L * L:L * L + m * L].reshape(m, L), u["res"]
    out = dict(route=u["route"], x=rel(u["x"], ref["npg"]), step=rel(u["theta"].astype(np.float64) - th, ref["new_params"] - th),
               grad=rel(u["grad"], ref["vpg"]), kl=abs(r[1] / N_on - ref["kl"]) / ref["kl"], surr_before=abs(r[4] / N_on - ref["surr_before"]),
               rows=r[5], G_bits=same_bits(blk[:L * L], alone[:L * L]), pad=float(np.abs(G[n + 1:]).max(initial=0.0) + np.abs(gWb[:, n + 1:]).max(initial=0.0)),
               same_bits=all(same_bits(u[k], u2[k]) for k in ("grad", "x", "theta", "res")))
    c.close()
    return out


def trpo(c, kl_dist, step_size):
    return call(c, lib.mjx_trpo_update_linear, [c.ctx, ITERS, DAMPING, TOL, step_size, kl_dist, 100, -3.0])


def run_trpo(n, m, N, seed):
    c = Case(n, m, N, True, seed=seed)
    th, o, a, w = c.o64
    ref = O.trpo_update(th.copy(), o, a, w, n, m, (), c.otr, cg_iters=ITERS, damping=DAMPING, kl_dist=KL)
    a0 = np.sqrt(abs(2 * KL / (ref["vpg"].dot(ref["npg"]) + 1e-20)))
    kls = [O.mean_kl(th + a0 * 0.9 ** k * ref["npg"], th, o, n, m, (), c.otr, c.otr) for k in range(ref["tries"])]      # (no log_std reaches the clamp)
    u = trpo(c, KL, 2 * KL)
    r = u["res"]
    out = dict(route=u["route"], trials=r[11], want_trials=ref["tries"], accepted=r[10], margin=min(abs(k - KL) / KL for k in kls),
               alpha=abs(r[9] - ref["alpha"]) / ref["alpha"], x=rel(u["x"], ref["npg"]), step=rel(u["theta"].astype(np.float64) - th, ref["new_params"] - th),
               ring=max(abs(r[17 + 2 * k] / N - kl) / kl for k, kl in enumerate(kls)), surr_slots_nan=bool(np.isnan(r[16:16 + 2 * len(kls):2]).all()),
               kl=abs(r[1] / N - ref["kl"]) / ref["kl"])
    c.close()
    return out


def run_once():
    out = {}
    c = Case(17, 6, 4099, True, seed=1)
    z = trpo(c, 0.0, 0.02)                             # no step length can be accepted
    out["zero"] = dict(route=z["route"], theta_same=same_bits(z["theta"], c.theta), accepted=z["res"][10], trials=z["res"][11])
    with switch("MJX_LINEAR_GRAM", "0"):               # TRPO: nothing is enqueued, the outputs keep their NaN
        g, x, th, res, route = nan_block(c.d), nan_block(c.d), nan_block(c.d), torch.full((64,), -7.0, dtype=torch.float64, device="cuda:0"), ctypes.c_int32(-1)
        check(lib.mjx_trpo_update_linear(c.ctx, ITERS, DAMPING, TOL, 2 * KL, KL, 100, -3.0, ptr(g), ptr(x), ptr(th), ptr(res), stream(), ctypes.byref(route)))
        torch.cuda.synchronize()
        out["trpo_off"] = dict(route=route.value, untouched=bool(torch.isnan(th).all().item() and (res == -7.0).all().item()))
    c.close()
    d = Dapg(17, 6, 4099, 200)
    with switch("MJX_LINEAR_GRAM", "0"):
        off = d.update(True)
    on, one = d.update(False), d.update(True)
    out["dapg_off"] = dict(route=off["route"], same=all(same_bits(off[k], on[k]) for k in ("grad", "x", "theta", "res")))
    d.close()
    # a twin rank: world 2 through the transport hook, which doubles every buffer it is handed
    d2, calls = Dapg(17, 6, 4099, 200, world=2), []

    def hook(user, buf, count, dtype, st):
        h = np.empty(count, np.float64 if dtype else np.float32)
        check(lib.mjx_memcpy_d2h(h.ctypes.data_as(ctypes.c_void_p), buf, h.nbytes, st)); check(lib.mjx_stream_sync(st))
        h *= 2
        check(lib.mjx_memcpy_h2d(buf, h.ctypes.data_as(ctypes.c_void_p), h.nbytes, st)); check(lib.mjx_stream_sync(st))
        calls.append([int(count), int(dtype)])
        return 0
    fn = _lib.REDUCE_FN(hook)
    check(lib.mjx_comm_set_callback(d2.ctx, fn, None, 2))
    two = d2.update(True)
    out["twin"] = dict(calls=calls, want=[[32 * 32 + 6 * 32 + 6 + 4, 1], [4, 1]], route=two["route"], theta=rel(two["theta"], one["theta"].astype(np.float64)),
                       x=rel(two["x"], one["x"].astype(np.float64)), res=float(np.abs(two["res"][[0, 1, 4, 5]] / 2 - one["res"][[0, 1, 4, 5]]).max()
                                                                               / np.abs(one["res"][[0, 1, 4, 5]]).max()))
    d2.close()
    return out


if __name__ == "__main__":
    payload = {"dapg_%d_%d_%d_%d" % cs: run_dapg(*cs) for cs in DAPG_CASES}
    payload.update({"trpo_%d_%d_%d" % cs[:3]: run_trpo(*cs) for cs in TRPO_CASES})
    payload["once"] = run_once()
    emit(payload)
