"""GPU worker for tests/test_gpu_reward_fit.py: every mjx_reward_fit_ensemble / fit_reward_ensemble / fit_world_models /
ensemble_path_rewards check in ONE fresh process; prints one RESULT JSON line of measured errors and counts (the test module
compares them with its bars).
python tests/_reward_fit_worker.py"""
import copy
import ctypes
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _dyn_check as C  # noqa: E402
from tests import _dyn_oracle as O  # noqa: E402
from tests._reward_fit_cases import (BLOCKS, CASES, GRAD_FLOOR, K, LR, MAX_CASE, ROUTE0, WD, compare_losses, compare_params,  # noqa: E402
                                     fixture_data, member_data)
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


def ens_fit(th, sizes, trs, xs, ys, idxs, steps, batch, act, m=None, v=None, step0=None, env=None, shared_y=False):
    """one mjx_reward_fit_ensemble call over the members th (K x P): -> (params, losses, m, v, route).  xs: K x N x d_in; ys:
    K x N x d_out, or one member's N x d_out with shared_y (stride 0); idxs: K x (>= steps * batch).  Losses are prefilled with
    NaN."""
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
    with switch("MJX_REWARD_FIT_ENS", env):
        check(lib.mjx_reward_fit_ensemble(ptr(t32(xs)), n * din, ptr(t32(ys)), 0 if shared_y else n * dout, n, k, ints(sizes), len(sizes),
                                          ptr(t32(trs[:, :2 * din])), ptr(t32(trs[:, 2 * din:])), act, ptr(P), ptr(mm), ptr(vv), s0, ptr(ix),
                                          steps, batch, LR, WD, ptr(loss), ctypes.byref(route), stream()))
    p, l = P.cpu().numpy(), loss.cpu().numpy()
    count("unwritten", C.unwritten(l) + C.unwritten(p))
    return p, l, mm.cpu().numpy(), vv.cpu().numpy(), route.value


def one_fit(th, sizes, tr, x, y, idx, steps, batch, act):
    """one mjx_dyn_fit_adam call in target mode 0 (the member-by-member path) -> (params, losses, m, v)"""
    din = sizes[0]
    P = t32(th)
    mm, vv = torch.zeros_like(P), torch.zeros_like(P)
    loss = torch.full((steps,), float("nan"), device=dev)
    ix = torch.as_tensor(np.ascontiguousarray(idx[:steps * batch], np.int32)).to(dev)
    KEEP.extend([loss, ix])
    check(lib.mjx_dyn_fit_adam(ptr(t32(x)), ptr(t32(y)), x.shape[0], ints(sizes), len(sizes), ptr(t32(tr[:2 * din])), ptr(t32(tr[2 * din:])),
                               0, act, ptr(P), ptr(mm), ptr(vv), 0, ptr(ix), steps, batch, LR, WD, ptr(loss), stream()))
    return P.cpu().numpy(), loss.cpu().numpy(), mm.cpu().numpy(), vv.cpu().numpy()


def members(name, sizes, batch, k=K, epochs=12):
    d = [member_data(name, sizes, batch, i, epochs=epochs) for i in range(k)]
    return tuple(np.stack([m[q] for m in d]) for q in range(5))        # th, tr, x, y, idx


def bits(*pairs):
    return int(sum(np.sum(np.asarray(a) != np.asarray(b)) for a, b in pairs))


# ================================================================ 1. against fp64, per member; member k of K = 4 against K = 1
for name, sizes, batch, act in CASES + [MAX_CASE]:
    pre = "max_" if name == MAX_CASE[0] else ""
    th, tr, x, y, idx = members(name, sizes, batch)
    run10 = None
    for steps in (1, 10):
        p, l, m, v, route = ens_fit(th, sizes, tr, x, y, idx, steps, batch, act)
        INFO.setdefault("route", {})[name] = route
        for k in range(K):
            g1 = np.zeros(th.shape[1])
            ref, _, _, rl = O.adam_steps(th[k], sizes, tr[k], x[k], y[k], idx[k][:steps * batch], batch, act, 0, LR, WD, g_first=g1)
            well = g1 >= GRAD_FLOOR
            where = "%s steps %d member %d" % (name, steps, k)
            if steps == 10:
                count(pre + "ill_conditioned", np.sum(~well))
                count(pre + "params", th.shape[1])
                put(pre + "ill_share_member", float(np.mean(~well)), "%s member %d" % (name, k))
            count("ill_not_finite", np.sum(~np.isfinite(p[k][~well])))
            e = compare_params(p[k], ref, well, sizes)
            put(pre + "params_over_lr", e["all"], where)
            put(pre + "edge_over_lr", e["edge"], where)
            for b in BLOCKS:
                put(pre + "block_" + b, e[b], where)
            by = INFO.setdefault("params_over_lr_by_case", {})
            by[name] = max(e["all"], by.get(name, 0.0))
            put(pre + "loss", compare_losses(l[k], rl), where)
        if steps == 10:
            run10 = (p, l, m, v)
    # member k of the K = 4 call against the K = 1 call of that member alone
    p, l, m, v = run10
    for k in range(K):
        p1, l1, m1, v1, r1 = ens_fit(th[k:k + 1], sizes, tr[k:k + 1], x[k:k + 1], y[k:k + 1], idx[k:k + 1], 10, batch, act)
        count("k4_vs_k1_not_bitwise", bits((p1[0], p[k]), (l1[0], l[k]), (m1[0], m[k]), (v1[0], v[k])) + (r1 != 1))
    count("k4_members_equal", int(np.array_equal(p[0], p[1])))          # (distinct members must differ)

# ================================================================ 2. route 0: bit for bit K mjx_dyn_fit_adam calls in mode 0
for name, sizes, batch, act, env in ROUTE0:
    th, tr, x, y, idx = members(name, sizes, batch)
    steps = 3
    p, l, m, v, route = ens_fit(th, sizes, tr, x, y, idx, steps, batch, act, env=env)
    INFO.setdefault("route0", {})[name] = route
    for k in range(K):
        p1, l1, m1, v1 = one_fit(th[k], sizes, tr[k], x[k], y[k], idx[k], steps, batch, act)
        count("route0_not_bitwise", bits((p1, p[k]), (l1, l[k]), (m1, m[k]), (v1, v[k])))

# ================================================================ 3. bit-for-bit properties of route 1
by_name = {c[0]: c for c in CASES}
# 3 steps, then 9 with the moments carried and per-member step0: one 12-step call, and the fp64 chain from the device's state
for name in ("rw_ref_b64", "rw_tanh_b33", "rw_w33_36"):
    _, sizes, batch, act = by_name[name]
    th, tr, x, y, idx = members(name, sizes, batch, epochs=30)
    for s0 in ((0, 0, 0, 0), (0, 3, 12, 40)):
        p1, l1, m1, v1, _ = ens_fit(th, sizes, tr, x, y, idx, 3, batch, act, step0=s0)
        p2, l2, m2, v2, _ = ens_fit(p1, sizes, tr, x, y, idx[:, 3 * batch:], 9, batch, act, m=m1, v=v1, step0=[t + 3 for t in s0])
        pa, la, ma, va, _ = ens_fit(th, sizes, tr, x, y, idx, 12, batch, act, step0=s0)
        count("cont_not_bitwise", bits((p2, pa), (np.concatenate([l1, l2], 1), la), (m2, ma), (v2, va)))
        for k in range(K):
            ref, _, _, _ = O.adam_steps(p1[k], sizes, tr[k], x[k], y[k], idx[k][3 * batch:12 * batch], batch, act, 0, LR, WD, m=m1[k],
                                        v=v1[k], t0=s0[k] + 3)
            put("cont_over_lr", C.over_lr(p2[k], ref, LR), "%s step0 %d member %d" % (name, s0[k], k))
# shared y (stride 0) against y replicated per member
for name in ("rw_ref_b16", "rw_dout3"):
    _, sizes, batch, act = by_name[name]
    th, tr, x, y, idx = members(name, sizes, batch)
    ps, ls, ms, vs, _ = ens_fit(th, sizes, tr, x, y[0], idx, 10, batch, act, shared_y=True)
    pr, lr_, mr, vr, _ = ens_fit(th, sizes, tr, x, np.stack([y[0]] * K), idx, 10, batch, act)
    count("shared_y_not_bitwise", bits((ps, pr), (ls, lr_), (ms, mr), (vs, vr)))

print("PARTIAL " + json.dumps({"err": ERR, "count": CNT, "info": INFO}), flush=True)

# ================================================================ 4. fit_reward_ensemble against the fit_reward loop
from mjrl_amd.algos.model_accel import nn_dynamics as D  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "model_accel.npz"))
n_, m_ = 11, 2
rng = np.random.RandomState(78)
s = rng.randn(400, n_).astype(np.float32)
a = rng.randn(400, m_).astype(np.float32)
sp = (s + 0.1 * np.tanh(s * 0.7 + a.sum(1, keepdims=True) * 0.2) + 0.02 * rng.randn(400, n_)).astype(np.float32)
r = (-np.sum(s ** 2, 1, keepdims=True) * 0.1 + 0.1 * a[:, :1]).astype(np.float32)


def params(net):
    return np.concatenate([p.detach().cpu().numpy().ravel() for p in net.parameters()])


def fresh(k=3, **kw):
    return [D.WorldModel(n_, m_, learn_reward=True, hidden_size=(64, 64), seed=100 + i, fit_lr=LR, fit_wd=WD, **kw) for i in range(k)]


def set_transforms(models):
    """fit_dynamics' and fit_reward's transform expressions, set by hand with a per-member factor on the scales (the members'
    transforms differ; the fits below run with set_transformations=False, as the reference's fit_reward fixture does)"""
    S, A, SP, R = (torch.from_numpy(q) for q in (s, a, sp, r))
    for i, w in enumerate(models):
        f = 1.0 + 0.1 * i
        s_shift, a_shift = torch.mean(S, dim=0), torch.mean(A, dim=0)
        s_scale, a_scale = torch.mean(torch.abs(S - s_shift), dim=0) * f, torch.mean(torch.abs(A - a_shift), dim=0) * f
        out_shift = torch.mean(SP - S, dim=0)
        out_scale = torch.mean(torch.abs(SP - S - out_shift), dim=0) * f
        w.dynamics_net.set_transformations(s_shift, s_scale, a_shift, a_scale, out_shift, out_scale)
        if w.learn_reward:
            r_shift = torch.mean(R, dim=0)
            r_scale = torch.mean(torch.abs(R - r_shift), dim=0) * f
            w.reward_net.set_transformations(s_shift, s_scale, a_shift, a_scale, r_shift, r_scale)


def same_state(u, w):
    return all(np.array_equal(p, q) for p, q in zip(u, w))


ens = fresh()
np.random.seed(4321)
D.fit_ensemble(ens, s, a, sp, 64, 2)                      # the dynamics are fitted first
set_transforms(ens)
loop = copy.deepcopy(ens)
theta0 = [params(w.reward_net) for w in ens]
for call in (1, 2):                                       # the second call carries the moments and the step count
    np.random.seed(1234 + call)
    ref_losses = [w.fit_reward(s, a, r, 64, 2, set_transformations=False) for w in loop]
    state_loop = np.random.get_state()
    np.random.seed(1234 + call)
    ens_losses = D.fit_reward_ensemble(ens, s, a, r, 64, 2, set_transformations=False)
    state_ens = np.random.get_state()
    count("wm_rng_state_differs", int(not same_state(state_loop, state_ens)))
    for k, (we, wl) in enumerate(zip(ens, loop)):
        pe, pl = params(we.reward_net), params(wl.reward_net)
        put("wm_params_over_lr", C.over_lr(pe, pl, LR), "call %d member %d" % (call, k))
        put("wm_loss", C.rel_max(np.array(ens_losses[k], np.float64), np.array(ref_losses[k], np.float64)), "call %d member %d" % (call, k))
        count("wm_unchanged", int(np.array_equal(pe, theta0[k])))
        count("wm_not_finite", np.sum(~np.isfinite(pe)))
        count("wm_state_differs", int(we.reward_opt.step_count != wl.reward_opt.step_count or we.reward_opt.step_count != 12 * call) +
              int(we.reward_net._generation != wl.reward_net._generation))
        put("wm_moments", max(C.rel_max(we.reward_opt.exp_avg.cpu().numpy(), wl.reward_opt.exp_avg.cpu().numpy()),
                              C.rel_max(we.reward_opt.exp_avg_sq.cpu().numpy(), wl.reward_opt.exp_avg_sq.cpu().numpy())), "call %d member %d" % (call, k))
    count("wm_epochs_bad", int(any(len(l) != 2 for l in ens_losses) or [len(l) for l in ens_losses] != [len(l) for l in ref_losses]))
# a member with learn_reward=False sends the call to the plain loop (which answers None for it, as fit_reward does)
mixed = fresh(2) + [D.WorldModel(n_, m_, learn_reward=False, hidden_size=(64, 64), seed=7)]
set_transforms(mixed)
mixed_loop = copy.deepcopy(mixed)
np.random.seed(99)
want = [w.fit_reward(s, a, r, 64, 1, set_transformations=False) for w in mixed_loop]
np.random.seed(99)
got = D.fit_reward_ensemble(mixed, s, a, r, 64, 1, set_transformations=False)
count("wm_mixed_differs", int(got[2] is not None or want[2] is not None) +
      bits(*[(params(u.reward_net), params(w.reward_net)) for u, w in zip(mixed[:2], mixed_loop[:2])]) +
      bits(*[(np.array(u), np.array(w)) for u, w in zip(got[:2], want[:2])]))

# ================================================================ 5. fit_world_models against the driver's interleaved loop
ens = fresh()
set_transforms(ens)
loop = copy.deepcopy(ens)
np.random.seed(555)
ref_d, ref_r = [], []
for w in loop:
    ref_d.append(w.fit_dynamics(s, a, sp, 64, 2, set_transformations=False))
    ref_r.append(w.fit_reward(s, a, r, 64, 2, set_transformations=False))
state_loop = np.random.get_state()
np.random.seed(555)
got_d, got_r = D.fit_world_models(ens, s, a, sp, r, 64, 2, set_transformations=False)
state_ens = np.random.get_state()
count("fwm_rng_state_differs", int(not same_state(state_loop, state_ens)))
count("fwm_epochs_bad", int([len(l) for l in got_d] != [len(l) for l in ref_d] or [len(l) for l in got_r] != [len(l) for l in ref_r]))
for k, (we, wl) in enumerate(zip(ens, loop)):
    put("fwm_dyn_params_over_lr", C.over_lr(params(we.dynamics_net), params(wl.dynamics_net), LR), "member %d" % k)
    put("fwm_rew_params_over_lr", C.over_lr(params(we.reward_net), params(wl.reward_net), LR), "member %d" % k)
    put("fwm_dyn_loss", C.rel_max(np.array(got_d[k], np.float64), np.array(ref_d[k], np.float64)), "member %d" % k)
    put("fwm_rew_loss", C.rel_max(np.array(got_r[k], np.float64), np.array(ref_r[k], np.float64)), "member %d" % k)
    count("fwm_state_differs", int(we.reward_opt.step_count != wl.reward_opt.step_count) + int(we.dynamics_opt.step_count != wl.dynamics_opt.step_count))
nolearn = [D.WorldModel(n_, m_, hidden_size=(64, 64), seed=100 + i, fit_lr=LR, fit_wd=WD) for i in range(2)]
nolearn2 = copy.deepcopy(nolearn)
np.random.seed(8)
w_d = D.fit_ensemble(nolearn2, s, a, sp, 64, 1)
np.random.seed(8)
g_d, g_r = D.fit_world_models(nolearn, s, a, sp, None, 64, 1)
count("fwm_nolearn_differs", int(g_r is not None) + bits(*[(params(u.dynamics_net), params(w.dynamics_net)) for u, w in zip(nolearn, nolearn2)]) +
      bits((np.array(g_d), np.array(w_d))))

# ================================================================ 6. the reference fixture through fit_reward_ensemble([wm])
n, m = 6, 2
s6, a6, sp6 = fixture_data(300, n, m, 40, zero_col=False)
r6 = (-np.sum(s6 ** 2, 1, keepdims=True) + 0.1 * a6[:, :1]).astype(np.float32)
np.random.seed(41)
wm = D.WorldModel(n, m, learn_reward=True, hidden_size=(32, 32), seed=5)
p0 = params(wm.reward_net)
wm.fit_dynamics(s6, a6, sp6, 32, 1)
rl = D.fit_reward_ensemble([wm], s6, a6, r6, 32, 2, set_transformations=False)[0]
put("fixture_reward", max(C.rel_max(np.array(rl), G["rew_losses"]), C.rel_max(wm.reward(s6[:40], a6[:40]).detach().cpu().numpy(), G["rew_pred"]),
                          float(np.linalg.norm(params(wm.reward_net) - G["rew_params"]) / np.linalg.norm(G["rew_params"] - p0))), "fixture")
INFO["fixture_route"] = int(lib.mjx_reward_fit_route(ints(list(wm.reward_net.layer_sizes)), 4, 32))

# ================================================================ 7. ensemble_path_rewards against K compute_path_rewards calls
ens = fresh(2) + fresh(1, activation='tanh')
set_transforms(ens)
np.random.seed(31)
D.fit_world_models(ens, s, a, sp, r, 64, 1, set_transformations=False)
Kp, Np, Hp = 3, 5, 7
obs = rng.randn(Kp, Np, Hp, n_).astype(np.float32)
act_ = rng.randn(Kp, Np, Hp, m_).astype(np.float32)
got = D.ensemble_path_rewards(ens, obs, act_)
got_l = D.ensemble_path_rewards(ens, [o for o in obs], [o for o in act_])
bad = int(got.shape != (Kp, Np, Hp) or got.dtype != np.float32) + bits((got, got_l))
for k, w in enumerate(ens):
    paths = dict(observations=obs[k], actions=act_[k])
    w.compute_path_rewards(paths)
    bad += bits((paths["rewards"], got[k]))
count("path_rewards_not_bitwise", bad)
count("path_rewards_members_equal", int(np.array_equal(got[0], got[1])))

torch.cuda.synchronize()
emit({"err": ERR, "count": CNT, "info": INFO})
