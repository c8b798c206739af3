"""GPU worker for tests/test_gpu_fit_matrix.py: every case of the two minibatch-Adam trainers (mjx_mlp_fit_adam,
mjx_policy_minibatch_adam) in ONE fresh process against the fp64 oracle (tests/_fit_oracle.py); prints one RESULT JSON line of
measured errors, counts and routes (the test module compares them with its bars).  Every ctypes call goes through check(): the
first HIP error ends the process.
python tests/_fit_matrix_worker.py"""
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from mjrl_amd.engine import UpdateEngine  # noqa: E402
from tests import _fit_cases as K  # noqa: E402
from tests import _fit_oracle as F  # noqa: E402
from tests._fit_cases import CLIP, HALVES, LAUNCHES, LR, N_MLP, ONEPASS  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import ints  # noqa: E402

TAIL = 64                     # NaN floats behind params / theta and both moments
SENTINEL = -7.0               # behind the last loss entry (an MSE is >= 0; a PPO loss of exactly -7 does not occur)
SWITCHES = ("MJX_MLP_FIT_LAUNCHES", "MJX_FIT_WIDE", "MJX_FIT_REGMOM", "MJX_FIT_ONEPASS", "MJX_NO_POLICY_FIT")

dev = W.device()
lib = load()
ERR, ROUTES, BY_ROUTE, PPO, CASES = {}, {}, {}, {}, {}     # CASES: every figure of every case, for reading a failure
CNT = {k: 0 for k in ("route_mismatch", "mlp_guard_bad", "mlp_cont_not_bitwise", "pol_guard_bad", "pol_cont_not_bitwise",
                      "pol_log_std_touched")}
up = functools.partial(W.up, keep=True)      # every uploaded block stays alive until the process ends


def put(key, val, case, route=None):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]
    CASES.setdefault(key, {})[case] = float(val)
    if route is not None:
        k = key + " / " + route
        BY_ROUTE[k] = max(BY_ROUTE.get(k, 0.0), float(val))


def count(key, n):
    CNT[key] = CNT.get(key, 0) + int(n)


def guarded(a):
    """fp32 device copy of a with TAIL NaNs behind it"""
    return up(np.concatenate([np.asarray(a, np.float32), np.full(TAIL, np.nan, np.float32)]))


def loss_buf(entries):
    return up(np.concatenate([np.full(entries, np.nan), [SENTINEL]]), np.float64)


def set_env(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


def report(kind, key, errs, case, route):
    e, block, index = F.worst(errs)
    put(kind + "_" + key, e, "%s %s[%d]" % (case, block, index), route)


# ================================================================ 1. MLP baseline
def mlp_route(d_in, hidden, batch, N, epochs):
    out = (ctypes.c_int32 * 6)()
    check(lib.mjx_mlp_fit_route(d_in, ints(hidden), len(hidden), batch, N, epochs, out))
    kind, nf1, regmom, G = out[0], out[1], out[2], out[3]
    name = ("launches" if kind == LAUNCHES else "k_mlp_fit1p" if kind == ONEPASS else
            "k_mlp_fit<NF1=%d,REGMOM=%d>" % (nf1, regmom) if kind == HALVES else "k_mlp_fit<wide,REGMOM=%d>" % regmom)
    return (kind, nf1, regmom, G), name


def gpu_mlp_fit(theta, d_in, hidden, batch, x, y, N, perm, epochs, wd, m=None, v=None, step0=0):
    """-> params, m, v (each with its guard tail), losses (with the sentinel)"""
    P = theta.size
    p = guarded(theta)
    mm, vv = guarded(np.zeros(P) if m is None else m), guarded(np.zeros(P) if v is None else v)
    loss = loss_buf(epochs)
    check(lib.mjx_mlp_fit_adam(ptr(up(x[:N])), ptr(up(y[:N])), N, d_in, ints(hidden), len(hidden), ptr(p), ptr(mm), ptr(vv), step0,
                               ptr(up(perm, np.int32)), epochs, batch, LR, wd, ptr(loss), None))
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (p, mm, vv, loss)]
    count("mlp_guard_bad", sum(not F.tail_intact(a, P) for a in out[:3]) + (out[3][epochs] != SENTINEL) +
          (not np.all(np.isfinite(out[3][:epochs]))))
    return out


def mlp_case(name, d_in, env, expect, hidden=(128, 128), batch=64, wd=1e-3, seed=0):
    """1 step (N = 2 batches: the single-step fit) and 2 epochs of N_MLP rows against fp64, block by block"""
    th, x, y, perm, perm1 = K.mlp_data(d_in, hidden, batch, seed)
    blocks = F.mlp_blocks(d_in, hidden)
    P = th.size
    set_env(env)
    for tag, N, epochs, pm in (("1 step", 2 * batch, 1, perm1), ("2 epochs", N_MLP, 2, perm)):
        route, rname = mlp_route(d_in, hidden, batch, N, epochs)
        case = "%s %s" % (name, tag)
        ROUTES["mlp " + case] = rname
        if route != expect:
            count("route_mismatch", 1)
            ROUTES["mlp " + case] += " (expected %r)" % (expect,)
        g1 = np.zeros(P)
        rp, rm, rv, rl = F.mlp_fit(th, d_in, x[:N], y[:N], pm, N, epochs, LR, wd, hidden, batch, g_first=g1)
        well = g1 >= F.GRAD_FLOOR
        put("mlp_ill_share", np.mean(~well), case)
        p, m, v, l = gpu_mlp_fit(th, d_in, hidden, batch, x, y, N, pm, epochs, wd)
        report("mlp", "params_over_lr", F.param_errors(p[:P], rp, blocks, LR, well), case, rname)
        report("mlp", "m", F.moment_errors(m[:P], rm, blocks), case, rname)
        report("mlp", "v", F.moment_errors(v[:P], rv, blocks), case, rname)
        if epochs == 1:
            report("mlp", "v_bias", F.moment_bias(v[:P], rv, blocks), case, rname)
        put("mlp_loss", F.rel_losses(l[:epochs], rl), case, rname)
    set_env({})


def mlp_continuation(name, d_in, env, expect, s0, seed):
    """epochs = 1, then perm + N with the moments carried and step0 = s0 + 5: the bits of one epochs = 2 call, and the fp64 chain
    from the device's own state after the first call (t0 = s0 + 5; the first call itself against fp64 from t0 = s0)"""
    hidden, batch, wd, N = (128, 128), 64, 1e-3, N_MLP
    th, x, y, perm, _ = K.mlp_data(d_in, hidden, batch, seed)
    blocks, P = F.mlp_blocks(d_in, hidden), th.size
    set_env(env)
    route, rname = mlp_route(d_in, hidden, batch, N, 1)
    case = "%s step0 %d" % (name, s0)
    ROUTES["mlp continuation " + case] = rname
    count("route_mismatch", route != expect)
    pa, ma, va, la = gpu_mlp_fit(th, d_in, hidden, batch, x, y, N, perm[:N], 1, wd, step0=s0)
    pb, mb, vb, lb = gpu_mlp_fit(pa[:P], d_in, hidden, batch, x, y, N, perm[N:], 1, wd, ma[:P], va[:P], step0=s0 + 5)
    pc, mc, vc, lc = gpu_mlp_fit(th, d_in, hidden, batch, x, y, N, perm, 2, wd, step0=s0)
    set_env({})
    count("mlp_cont_not_bitwise", np.sum(pb[:P] != pc[:P]) + np.sum(mb[:P] != mc[:P]) + np.sum(vb[:P] != vc[:P]) +
          (la[0] != lc[0]) + (lb[0] != lc[1]))
    for start, t0, pm, (dp, dm, dv) in ((th, s0, perm[:N], (None, None, None)), (pa[:P], s0 + 5, perm[N:], (pa, ma, va))):
        g1 = np.zeros(P)
        got = pa if dp is None else pb
        ref = F.mlp_fit(start, d_in, x, y, pm, N, 1, LR, wd, hidden, batch, m=None if dm is None else dm[:P],
                        v=None if dv is None else dv[:P], t0=t0, g_first=g1)[0]
        report("mlp", "cont_over_lr", F.param_errors(got[:P], ref, blocks, LR, g1 >= F.GRAD_FLOOR), "%s t0 %d" % (case, t0), rname)


for name, d, env, expect, hidden, batch, wd, seed in K.MLP_CASES:
    mlp_case(name, d, env, expect, hidden, batch, wd, seed)
for i, (name, d, env, expect) in enumerate(K.MLP_INSTANCES):
    for s0 in (0, 12):
        mlp_continuation(name, d, env, expect, s0, K.MLP_CONT_SEED + i)


# ================================================================ 2. policy
def pol_route(n, m, hid, B, loss, track):
    out = (ctypes.c_int32 * 2)()
    check(lib.mjx_policy_fit_route(n, m, ints(hid), len(hid), B, loss, track, out))
    return int(out[0])


def gpu_pol_fit(eng, D, loss, track, idx, steps, B, theta, am, av, step0=0):
    d = theta.size
    th, m_, v_ = guarded(theta), guarded(am), guarded(av)
    lt = loss_buf(steps)
    check(lib.mjx_policy_minibatch_adam(eng.ctx, loss, ptr(D["obs"]), ptr(D["act"]), ptr(D["adv"]), ptr(up(idx[:steps * B], np.int32)), steps, B,
                                        ptr(th), ptr(D["tr"]), ptr(D["tho"]), ptr(D["tro"]), track, ptr(m_), ptr(v_), step0, LR, CLIP,
                                        ptr(lt), eng.stream()))
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in (th, m_, v_, lt)]
    count("pol_guard_bad", sum(not F.tail_intact(a, d) for a in out[:3]) + (out[3][steps] != SENTINEL) +
          (not np.all(np.isfinite(out[3][:steps]))))
    return out


def pol_case(n, m, hid, B, env, expect, seed):
    name = K.pol_name(n, m, hid, B, env)
    P = K.pol_data(n, m, hid, B, seed)
    th0, tho, tr, tro, obs, act, adv, idx = (P[k] for k in ("theta", "theta_old", "tr", "tr_old", "obs", "act", "adv", "idx"))
    D = {"obs": up(obs), "act": up(act), "adv": up(adv), "tr": up(tr), "tho": up(tho), "tro": up(tro)}
    blocks, d = F.policy_blocks(n, m, hid), th0.size
    eng = UpdateEngine(n, m, hid)
    set_env(env)
    for loss, track in K.MODES:
        H = pol_route(n, m, hid, B, loss, track)
        rname = "k_policy_fit<%d>" % H if H else "launches"
        mode = "%s loss %d track %d" % (name, loss, track)
        ROUTES["policy " + mode] = rname
        if H != expect and not (loss == 2 and not track and H == 0):     # an old network of its own may no longer fit LDS
            count("route_mismatch", 1)
            ROUTES["policy " + mode] += " (expected %d)" % expect
        am0, av0 = K.pol_moments(P, m, loss)
        args = (n, m, hid, tr, tho, tro, obs, act, adv)
        for steps in (1, 10):
            case = "%s %d step%s" % (mode, steps, "s" * (steps > 1))
            g1 = np.zeros(d)
            rp, rm, rv, rl, st = F.policy_fit(th0, *args, idx[:steps * B], B, loss, track, LR, CLIP, am0, av0, g_first=g1)
            well = g1 >= F.GRAD_FLOOR
            if loss == 0:
                well[-m:] = True                                         # no gradient there by construction: compared exactly below
                g1[-m:] = 1.0
            put("pol_ill_share", np.mean(g1 < F.GRAD_FLOOR), case)
            p, am, av, lt = gpu_pol_fit(eng, D, loss, track, idx, steps, B, th0, am0, av0)
            report("pol", "params_over_lr", F.param_errors(p[:d], rp, blocks, LR, well), case, rname)
            report("pol", "m", F.moment_errors(am[:d], rm, blocks[:-1] if loss == 0 else blocks), case, rname)
            report("pol", "v", F.moment_errors(av[:d], rv, blocks[:-1] if loss == 0 else blocks), case, rname)
            if steps == 1:
                report("pol", "v_bias", F.moment_bias(av[:d], rv, blocks), case, rname)
            put("pol_loss", F.rel_losses(lt[:steps], rl), case, rname)
            if loss == 0:
                count("pol_log_std_touched", np.sum(p[d - m:d] != th0[-m:]) + np.sum(am[d - m:d] != am0[-m:]) + np.sum(av[d - m:d] != av0[-m:]))
        if loss == 2:                                                    # the branch statistics of every step any check runs
            PPO[mode] = F.policy_fit(th0, *args, idx, B, loss, track, LR, CLIP, am0, av0)[4]
        # continuation: 3 steps, then 9 with the moments carried and step0 = 3, against one 12-step call and against fp64
        pa, ma, va, la = gpu_pol_fit(eng, D, loss, track, idx, 3, B, th0, am0, av0)
        pb, mb, vb, lb = gpu_pol_fit(eng, D, loss, track, idx[3 * B:], 9, B, pa[:d], ma[:d], va[:d], step0=3)
        pc, mc, vc, lc = gpu_pol_fit(eng, D, loss, track, idx, 12, B, th0, am0, av0)
        count("pol_cont_not_bitwise", np.sum(pb[:d] != pc[:d]) + np.sum(mb[:d] != mc[:d]) + np.sum(vb[:d] != vc[:d]) +
              np.sum(np.concatenate([la[:3], lb[:9]]) != lc[:12]))
        g1 = np.zeros(d)
        ref = F.policy_fit(pa[:d], *args, idx[3 * B:], B, loss, track, LR, CLIP, ma[:d], va[:d], t0=3, g_first=g1)[0]
        well = g1 >= F.GRAD_FLOOR
        if loss == 0:
            well[-m:] = True
        report("pol", "cont_over_lr", F.param_errors(pb[:d], ref, blocks, LR, well), mode + " t0 3", rname)
    set_env({})
    eng.close()


for n, m, hid, B, env, expect, seed in K.POL_CASES:
    pol_case(n, m, hid, B, env, expect, seed)

W.emit({"err": ERR, "count": CNT, "routes": ROUTES, "by_route": BY_ROUTE, "ppo": PPO, "cases": CASES})
