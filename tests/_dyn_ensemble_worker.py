"""GPU worker for tests/test_gpu_dynamics_ensemble.py: every mjx_dyn_fit_ensemble / fit_ensemble check in ONE fresh process;
prints one RESULT JSON line of measured errors and counts (the test module compares them with its bars).
python tests/_dyn_ensemble_worker.py"""
import copy
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _dyn_check as C  # noqa: E402
from tests import _dyn_oracle as O  # noqa: E402
from tests._dyn_check import rand_theta, rand_tr  # noqa: E402
from tests._dyn_ensemble_cases import CASES, GRAD_FLOOR, K, LR, NF, ROUTE0, WD, XSCR_CASE, member_data  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import KEEP, emit, ints, stream, switch  # noqa: E402

dev = W.device()
lib = load()
ERR, CNT, INFO = {}, {}, {}
t32 = functools.partial(W.up, keep=True)


def put(key, val, case):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]


def count(key, n):
    CNT[key] = CNT.get(key, 0) + int(n)


def ens_fit(th, sizes, trs, xs, ys, idxs, steps, batch, act, tmode, m=None, v=None, step0=None, env=None, shared=False):
    """one mjx_dyn_fit_ensemble call over the members th (K x P): -> (params, losses, m, v, route).  xs / ys: K x N x d (or one
    member's N x d with shared: strides 0); idxs: K x (>= steps * batch).  Losses are prefilled with NaN."""
    k = th.shape[0]
    din, dout = sizes[0], sizes[-1]
    P = t32(th)
    mm = torch.zeros_like(P) if m is None else t32(m)
    vv = torch.zeros_like(P) if v is None else t32(v)
    loss = torch.full((k, steps), float("nan"), device=dev)
    ix = torch.as_tensor(np.ascontiguousarray(np.stack([i[:steps * batch] for i in idxs]), np.int32)).to(dev)
    KEEP.extend([loss, ix])
    s0 = (ctypes.c_int64 * k)(*([0] * k if step0 is None else [int(t) for t in step0]))
    route = ctypes.c_int(-9)
    n = xs.shape[-2]
    with switch("MJX_DYN_FIT_ENS", env):
        check(lib.mjx_dyn_fit_ensemble(ptr(t32(xs)), 0 if shared else n * din, ptr(t32(ys)), 0 if shared else n * dout, n, k, ints(sizes),
                                       len(sizes), ptr(t32(trs[:, :2 * din])), ptr(t32(trs[:, 2 * din:])), tmode, act, ptr(P), ptr(mm), ptr(vv),
                                       s0, ptr(ix), steps, batch, LR, WD, ptr(loss), ctypes.byref(route), stream()))
    p, l = P.cpu().numpy(), loss.cpu().numpy()
    count("unwritten", C.unwritten(l) + C.unwritten(p))
    return p, l, mm.cpu().numpy(), vv.cpu().numpy(), route.value


def one_fit(th, sizes, tr, x, y, idx, steps, batch, act, tmode, m=None, v=None, step0=0):
    """one mjx_dyn_fit_adam call (the parent commit's path) -> (params, losses, m, v)"""
    din = sizes[0]
    P = t32(th)
    mm = torch.zeros_like(P) if m is None else t32(m)
    vv = torch.zeros_like(P) if v is None else t32(v)
    loss = torch.full((steps,), float("nan"), device=dev)
    ix = torch.as_tensor(np.ascontiguousarray(idx[:steps * batch], np.int32)).to(dev)
    KEEP.extend([loss, ix])
    check(lib.mjx_dyn_fit_adam(ptr(t32(x)), ptr(t32(y)), x.shape[0], ints(sizes), len(sizes), ptr(t32(tr[:2 * din])), ptr(t32(tr[2 * din:])),
                               tmode, act, ptr(P), ptr(mm), ptr(vv), step0, ptr(ix), steps, batch, LR, WD, ptr(loss), stream()))
    return P.cpu().numpy(), loss.cpu().numpy(), mm.cpu().numpy(), vv.cpu().numpy()


def members(name, sizes, batch, k=K, epochs=12):
    d = [member_data(name, sizes, batch, i, epochs=epochs) for i in range(k)]
    return tuple(np.stack([m[q] for m in d]) for q in range(5))        # th, tr, x, y, idx


def bits(*pairs):
    return int(sum(np.sum(np.asarray(a) != np.asarray(b)) for a, b in pairs))


# ================================================================ 1. against fp64, per member; member k of K = 4 against K = 1
RUN10 = {}
for name, sizes, batch, act, tmode in CASES + [XSCR_CASE]:
    pre = "xscr_" if name == XSCR_CASE[0] else ""
    th, tr, x, y, idx = members(name, sizes, batch)
    for steps in (1, 10):
        p, l, m, v, route = ens_fit(th, sizes, tr, x, y, idx, steps, batch, act, tmode)
        INFO.setdefault("route", {})[name] = route
        for k in range(K):
            g1 = np.zeros(th.shape[1])
            ref, _, _, rl = O.adam_steps(th[k], sizes, tr[k], x[k], y[k], idx[k][:steps * batch], batch, act, tmode, LR, WD, g_first=g1)
            well = g1 >= GRAD_FLOOR
            if steps == 10:
                count(pre + "ill_conditioned", np.sum(~well))
                count(pre + "params", th.shape[1])
                put(pre + "ill_share_member", float(np.mean(~well)), "%s member %d" % (name, k))
            count("ill_not_finite", np.sum(~np.isfinite(p[k][~well])))
            e = C.over_lr(p[k][well], ref[well], LR)
            put(pre + "params_over_lr", e, "%s steps %d member %d" % (name, steps, k))
            INFO.setdefault("params_over_lr_by_case", {})[name] = max(e, INFO.get("params_over_lr_by_case", {}).get(name, 0.0))
            if steps == 10:          # for the record: the member-by-member path (the existing fp32 routes) on the same member
                ps, _, _, _ = one_fit(th[k], sizes, tr[k], x[k], y[k], idx[k], steps, batch, act, tmode)
                put(pre + "seq_params_over_lr", C.over_lr(ps[well], ref[well], LR), "%s steps %d member %d" % (name, steps, k))
            put(pre + "loss", C.rel_max(l[k], rl), "%s steps %d member %d" % (name, steps, k))
        if steps == 10:
            RUN10[name] = (p, l, m, v)
    # member k of the K = 4 call against the K = 1 call of that member alone
    p, l, m, v = RUN10[name]
    for k in range(K):
        p1, l1, m1, v1, r1 = ens_fit(th[k:k + 1], sizes, tr[k:k + 1], x[k:k + 1], y[k:k + 1], idx[k:k + 1], 10, batch, act, tmode)
        count("k4_vs_k1_not_bitwise", bits((p1[0], p[k]), (l1[0], l[k]), (m1[0], m[k]), (v1[0], v[k])) + (r1 != 1))

# ================================================================ 2. route 0: bit for bit K mjx_dyn_fit_adam calls
for name, sizes, batch, act, tmode, env in ROUTE0:
    th, tr, x, y, idx = members(name, sizes, batch)
    steps = 3
    p, l, m, v, route = ens_fit(th, sizes, tr, x, y, idx, steps, batch, act, tmode, env=env)
    INFO.setdefault("route0", {})[name] = route
    for k in range(K):
        p1, l1, m1, v1 = one_fit(th[k], sizes, tr[k], x[k], y[k], idx[k], steps, batch, act, tmode)
        count("route0_not_bitwise", bits((p1, p[k]), (l1, l[k]), (m1, m[k]), (v1, v[k])))

# ================================================================ 3. bit-for-bit properties of route 1
by_name = {c[0]: c for c in CASES}
# K = 7, members 0 and 5 with identical inputs
for name in ("w256_b16", "w32_b33"):
    _, sizes, batch, act, tmode = by_name[name]
    th, tr, x, y, idx = members(name, sizes, batch, k=7)
    for a in (th, tr, x, y, idx):
        a[5] = a[0]
    p, l, m, v, route = ens_fit(th, sizes, tr, x, y, idx, 10, batch, act, tmode)
    count("k7_twins_differ", bits((p[0], p[5]), (l[0], l[5]), (m[0], m[5]), (v[0], v[5])) + (route != 1))
    count("k7_members_equal", int(np.array_equal(p[0], p[1])))        # (distinct members must differ: the check above is no tautology)
# 3 steps, then 9 with the moments carried and step0 + 3: one 12-step call, and the fp64 chain from the device's state after 3
for name in ("w256_b64", "w64_b32", "h64_96_tanh"):
    _, sizes, batch, act, tmode = by_name[name]
    th, tr, x, y, idx = members(name, sizes, batch, epochs=30)
    for s0 in ((0, 0, 0, 0), (0, 3, 12, 40)):
        p1, l1, m1, v1, _ = ens_fit(th, sizes, tr, x, y, idx, 3, batch, act, tmode, step0=s0)
        p2, l2, m2, v2, _ = ens_fit(p1, sizes, tr, x, y, idx[:, 3 * batch:], 9, batch, act, tmode, m=m1, v=v1, step0=[t + 3 for t in s0])
        pa, la, ma, va, _ = ens_fit(th, sizes, tr, x, y, idx, 12, batch, act, tmode, step0=s0)
        count("cont_not_bitwise", bits((p2, pa), (np.concatenate([l1, l2], 1), la), (m2, ma), (v2, va)))
        for k in range(K):
            ref, _, _, _ = O.adam_steps(p1[k], sizes, tr[k], x[k], y[k], idx[k][3 * batch:12 * batch], batch, act, tmode, LR, WD, m=m1[k],
                                        v=v1[k], t0=s0[k] + 3)
            put("cont_over_lr", C.over_lr(p2[k], ref, LR), "%s step0 %d member %d" % (name, s0[k], k))
# shared rows (strides 0) against the same rows replicated per member
for name in ("w256_b16", "w64_b32"):
    _, sizes, batch, act, tmode = by_name[name]
    th, tr, x, y, idx = members(name, sizes, batch)
    xr, yr = np.stack([x[0]] * K), np.stack([y[0]] * K)
    ps, ls, ms, vs, _ = ens_fit(th, sizes, tr, x[0], y[0], idx, 10, batch, act, tmode, shared=True)
    pr, lr_, mr, vr, _ = ens_fit(th, sizes, tr, xr, yr, idx, 10, batch, act, tmode)
    count("shared_rows_not_bitwise", bits((ps, pr), (ls, lr_), (ms, mr), (vs, vr)))

# ================================================================ 4. fit_ensemble against the fit_dynamics loop
from mjrl_amd.algos.model_accel import nn_dynamics as D  # noqa: E402
from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy  # noqa: E402

n_, m_ = 13, 4
rng = np.random.RandomState(77)
s = rng.randn(NF, n_).astype(np.float32)
a = rng.randn(NF, m_).astype(np.float32)
sp = (s + 0.1 * np.tanh(s * 0.7 + a.sum(1, keepdims=True) * 0.2) + 0.02 * rng.randn(NF, n_)).astype(np.float32)
ens = [D.WorldModel(n_, m_, hidden_size=(256, 256), seed=100 + i, fit_lr=LR, fit_wd=WD) for i in range(3)]
loop = copy.deepcopy(ens)


class _Env:
    observation_dim, action_dim, horizon = n_, m_, 10
    env_id = "none"


planner = MPCPolicy(env=_Env(), fitted_model=ens, plan_horizon=4, plan_paths=8, seed=3)
key0 = planner._pack_key(dev)[0]
theta0 = [np.concatenate([p.detach().cpu().numpy().ravel() for p in w.dynamics_net.parameters()]) for w in ens]
np.random.seed(1234)
ref_losses = [w.fit_dynamics(s, a, sp, 64, 2) for w in loop]
state_loop = np.random.get_state()
np.random.seed(1234)
ens_losses = D.fit_ensemble(ens, s, a, sp, 64, 2)
state_ens = np.random.get_state()
count("wm_rng_state_differs", int(not all(np.array_equal(u, w) for u, w in zip(state_loop, state_ens))))
for k, (we, wl) in enumerate(zip(ens, loop)):
    pe = np.concatenate([p.detach().cpu().numpy().ravel() for p in we.dynamics_net.parameters()])
    pl = np.concatenate([p.detach().cpu().numpy().ravel() for p in wl.dynamics_net.parameters()])
    put("wm_params_over_lr", C.over_lr(pe, pl, LR), "member %d" % k)
    put("wm_loss", C.rel_max(np.array(ens_losses[k], np.float64), np.array(ref_losses[k], np.float64)), "member %d" % k)
    count("wm_unchanged", int(np.array_equal(pe, theta0[k])))
    count("wm_not_finite", np.sum(~np.isfinite(pe)))
    count("wm_state_differs", int(we.dynamics_opt.step_count != wl.dynamics_opt.step_count or we.dynamics_opt.step_count != 12) +
          int(we.dynamics_net._generation != wl.dynamics_net._generation))
    put("wm_moments", max(C.rel_max(we.dynamics_opt.exp_avg.cpu().numpy(), wl.dynamics_opt.exp_avg.cpu().numpy()),
                          C.rel_max(we.dynamics_opt.exp_avg_sq.cpu().numpy(), wl.dynamics_opt.exp_avg_sq.cpu().numpy())), "member %d" % k)
count("wm_epochs_bad", int(any(len(l) != 2 for l in ens_losses)))
count("wm_pack_key_unchanged", int(planner._pack_key(dev)[0] == key0))

torch.cuda.synchronize()
emit({"err": ERR, "count": CNT, "info": INFO})
