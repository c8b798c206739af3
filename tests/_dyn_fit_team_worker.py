"""GPU worker for tests/test_gpu_dyn_fit_team.py: every mjx_dyn_fit_ensemble_team / fit_ensemble(team=True) check in ONE fresh
process; prints one RESULT JSON line of measured errors and counts.    python tests/_dyn_fit_team_worker.py"""
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
from tests._dyn_fit_team_cases import CASES, FALL_THROUGH, GRAD_FLOOR, LR, WD, members  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import KEEP, emit, ints, stream, switch  # noqa: E402

dev = W.device()
lib = load()
ERR, CNT, INFO = {}, {}, {"route": {}, "G": {}, "fall": {}}
t32 = functools.partial(W.up, keep=True)


def put(key, val, case):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]


def count(key, n):
    CNT[key] = CNT.get(key, 0) + int(n)


def fit(entry, th, sizes, trs, xs, ys, idxs, steps, batch, act, tmode, m=None, v=None, step0=None, env=None):
    """one call of lib.<entry> over the members th (K x P): -> (params, losses, m, v, route); losses are prefilled with NaN"""
    k, din, dout, n = th.shape[0], sizes[0], sizes[-1], xs.shape[-2]
    P = t32(th)
    mm = torch.zeros_like(P) if m is None else t32(m)
    vv = torch.zeros_like(P) if v is None else t32(v)
    loss = torch.full((k, steps), float("nan"), device=dev)
    ix = torch.as_tensor(np.ascontiguousarray(np.stack([i[:steps * batch] for i in idxs]), np.int32)).to(dev)
    KEEP.extend([loss, ix])
    s0 = (ctypes.c_int64 * k)(*([0] * k if step0 is None else [int(t) for t in step0]))
    route = ctypes.c_int(-9)
    with switch("MJX_DYN_FIT_TEAM", env):
        check(getattr(lib, entry)(ptr(t32(xs)), n * din, ptr(t32(ys)), n * dout, n, k, ints(sizes), len(sizes), ptr(t32(trs[:, :2 * din])),
                                  ptr(t32(trs[:, 2 * din:])), tmode, act, ptr(P), ptr(mm), ptr(vv), s0, ptr(ix), steps, batch, LR, WD,
                                  ptr(loss), ctypes.byref(route), stream()))
    p, l = P.cpu().numpy(), loss.cpu().numpy()
    count("unwritten", C.unwritten(l) + C.unwritten(p))
    return p, l, mm.cpu().numpy(), vv.cpu().numpy(), route.value


team = functools.partial(fit, "mjx_dyn_fit_ensemble_team")


def bits(*pairs):
    return int(sum(np.sum(np.asarray(a) != np.asarray(b)) for a, b in pairs))


def blocks(sizes):
    """(name, slice) of W1, b1, W2, b2, W3, b3 in the flat parameter vector"""
    cut = np.cumsum([0] + [c for l in range(3) for c in (sizes[l] * sizes[l + 1], sizes[l + 1])])
    return [("W1 b1 W2 b2 W3 b3".split()[i], slice(cut[i], cut[i + 1])) for i in range(6)]


# ================================================================ 1. against fp64, per member and block; member 1 of K = 3 alone
RUN10 = {}
for name, sizes, batch, act, tmode, K, G in CASES:
    th, tr, x, y, idx = members(name, sizes, batch, K)
    INFO["G"][name] = lib.mjx_dyn_fit_team_route(ints(sizes), len(sizes), batch, tmode, K)
    for steps in (1, 10):
        p, l, m, v, route = team(th, sizes, tr, x, y, idx, steps, batch, act, tmode)
        INFO["route"][name] = route
        for k in range(K):
            g1 = np.zeros(th.shape[1])
            ref, rm, rv, rl = O.adam_steps(th[k], sizes, tr[k], x[k], y[k], idx[k][:steps * batch], batch, act, tmode, LR, WD, g_first=g1)
            well, case = g1 >= GRAD_FLOOR, "%s steps %d member %d" % (name, steps, k)
            put("ill_share", float(np.mean(~well)), case)
            count("ill_not_finite", np.sum(~np.isfinite(p[k][~well])))
            for nm, sl in blocks(sizes):
                put("params_over_lr", C.over_lr(p[k][sl][well[sl]], ref[sl][well[sl]], LR), case + " " + nm)
                for key, got, want in (("m", m[k][sl], rm[sl]), ("v", v[k][sl], rv[sl])):     # element-wise, over the block's largest entry
                    put(key, float(np.max(np.abs(got - want)) / np.max(np.abs(want))), case + " " + nm)
            put("loss", C.rel_max(l[k], rl), case)
        RUN10[name] = (th, tr, x, y, idx, p, l, m, v)
    if K > 1:
        p1, l1, m1, v1, r1 = team(th[1:2], sizes, tr[1:2], x[1:2], y[1:2], idx[1:2], 10, batch, act, tmode)
        count("alone_not_bitwise", bits((p1[0], p[1]), (l1[0], l[1]), (m1[0], m[1]), (v1[0], v[1])) + (r1 != 2))

# ================================================================ 2. 4 steps, then 6 with the moments carried = one 10-step call
for name, sizes, batch, act, tmode, K, G in CASES[:3]:
    th, tr, x, y, idx = RUN10[name][:5]
    s0 = (0, 3, 12)
    p1, l1, m1, v1, _ = team(th, sizes, tr, x, y, idx, 4, batch, act, tmode, step0=s0)
    p2, l2, m2, v2, _ = team(p1, sizes, tr, x, y, idx[:, 4 * batch:], 6, batch, act, tmode, m=m1, v=v1, step0=[t + 4 for t in s0])
    pa, la, ma, va, _ = team(th, sizes, tr, x, y, idx, 10, batch, act, tmode, step0=s0)
    count("cont_not_bitwise", bits((p2, pa), (np.concatenate([l1, l2], 1), la), (m2, ma), (v2, va)))

# ================================================================ 3. fall-through: the bits and the route of mjx_dyn_fit_ensemble
for name, sizes, batch, env in FALL_THROUGH:
    th, tr, x, y, idx = members(name, sizes, batch, 3)
    got = team(th, sizes, tr, x, y, idx, 3, batch, 0, 2, env=env)
    want = fit("mjx_dyn_fit_ensemble", th, sizes, tr, x, y, idx, 3, batch, 0, 2)
    INFO["fall"][name] = [got[4], want[4]]
    count("fall_not_bitwise", bits(*zip(got[:4], want[:4])) + (got[4] != want[4]))

# ================================================================ 4. fit_ensemble(team=True) = the direct call, bit for bit
from mjrl_amd.algos.model_accel import nn_dynamics as D  # noqa: E402

n_, m_, NF = 13, 4, 135
rng = np.random.RandomState(77)
s, a = rng.randn(NF, n_).astype(np.float32), rng.randn(NF, m_).astype(np.float32)
sp = (s + 0.1 * np.tanh(s * 0.7 + a.sum(1, keepdims=True) * 0.2) + 0.02 * rng.randn(NF, n_)).astype(np.float32)
ens = [D.WorldModel(n_, m_, hidden_size=(128, 128), seed=100 + i, fit_lr=LR, fit_wd=WD) for i in range(3)]
plain = copy.deepcopy(ens)
th0 = np.stack([np.concatenate([q.detach().cpu().numpy().ravel() for q in w.dynamics_net.parameters()]) for w in ens])
np.random.seed(1234)
D.fit_ensemble(ens, s, a, sp, 32, 2, team=True)
np.random.seed(1234)
D.fit_ensemble(plain, s, a, sp, 32, 2)
pk = D.pack_members([w.dynamics_net for w in plain], dev, one_kind=False)       # (the transforms the fit left; the parameters below)
np.random.seed(1234)
idx, num_steps, ran = D.ensemble_fit_indices(3, NF, 32, 2)
p, l, m, v, route = team(th0, [int(q) for q in pk["sizes"]], pk["tr"].cpu().numpy(), np.stack([np.concatenate([s, a], -1)] * 3), np.stack([sp] * 3),
                         idx, ran * num_steps, 32, pk["act"], D.TGT_RESIDUAL)
for k, (we, wp) in enumerate(zip(ens, plain)):
    pe = np.concatenate([q.detach().cpu().numpy().ravel() for q in we.dynamics_net.parameters()])
    count("public_not_bitwise", bits((pe, p[k]), (we.dynamics_opt.exp_avg.cpu().numpy(), m[k]), (we.dynamics_opt.exp_avg_sq.cpu().numpy(), v[k])))
    count("public_state_differs", int(we.dynamics_opt.step_count != wp.dynamics_opt.step_count or we.dynamics_opt.step_count != ran * num_steps) +
          int(we.dynamics_net._generation != wp.dynamics_net._generation) + int(route != 2))

torch.cuda.synchronize()
emit({"err": ERR, "count": CNT, "info": INFO})
