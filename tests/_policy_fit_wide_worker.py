"""GPU worker of tests/test_gpu_policy_fit_wide.py: every case on route 2 of mjx_policy_minibatch_adam_wide and on the existing entry
(the per-step launches for these shapes), both against the fp64 oracle; then BC / PPO with wide_fit=True.  One RESULT JSON line."""
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
from tests import _worker_dev as W  # noqa: E402
from tests._fit_cases import CLIP, LR  # noqa: E402
from tests._worker_dev import ints  # noqa: E402

# (n, m, H, B, seed)
CASES = [(33, 17, 32, 8, 3110), (46, 30, 32, 64, 3101), (64, 32, 32, 12, 3102), (39, 28, 32, 32, 3103), (17, 17, 64, 20, 3104),
         (48, 32, 64, 32, 3105), (45, 24, 64, 32, 3106)]
TAIL, SENTINEL = 64, -7.0

os.environ.pop("MJX_NO_POLICY_FIT", None), os.environ.pop("MJX_POLICY_FIT_WIDE", None)
lib = load()
up = functools.partial(W.up, keep=True)
OUT = {}                      # "(n, m, H, B) loss l track t": every figure of the case


def guarded(a):
    return up(np.concatenate([np.asarray(a, np.float32), np.full(TAIL, np.nan, np.float32)]))


def gpu_fit(eng, D, wide, loss, track, idx, steps, B, theta, am, av, step0=0):
    """-> theta, m, v, losses (host), guards intact, route the wide entry reports (None: the existing entry)"""
    d = theta.size
    th, m_, v_ = guarded(theta), guarded(am), guarded(av)
    lt = up(np.concatenate([np.full(steps, np.nan), [SENTINEL]]), np.float64)
    args = (eng.ctx, loss, ptr(D["obs"]), ptr(D["act"]), ptr(D["adv"]), ptr(up(idx[:steps * B], np.int32)), steps, B, ptr(th), ptr(D["tr"]),
            ptr(D["tho"]), ptr(D["tro"]), track, ptr(m_), ptr(v_), step0, LR, CLIP, ptr(lt), eng.stream())
    route = ctypes.c_int(-1)
    check(lib.mjx_policy_minibatch_adam_wide(*args, ctypes.byref(route)) if wide else lib.mjx_policy_minibatch_adam(*args))
    torch.cuda.synchronize()
    p, a, v, l = (t.cpu().numpy() for t in (th, m_, v_, lt))
    ok = all(F.tail_intact(x, d) for x in (p, a, v)) and l[steps] == SENTINEL and bool(np.all(np.isfinite(l[:steps])))
    return p[:d], a[:d], v[:d], l[:steps], ok, (int(route.value) if wide else None)


def pol_case(n, m, H, B, seed):
    hid = (H, H)
    P = K.pol_data(n, m, hid, B, seed)
    th0, tho, tr, tro, obs, act, adv, idx = (P[k] for k in ("theta", "theta_old", "tr", "tr_old", "obs", "act", "adv", "idx"))
    D = {"obs": up(obs), "act": up(act), "adv": up(adv), "tr": up(tr), "tho": up(tho), "tro": up(tro)}
    blocks, d = F.policy_blocks(n, m, hid), th0.size
    eng = UpdateEngine(n, m, hid)
    for loss, track in K.MODES:
        r = OUT["(%d, %d, %d, %d) loss %d track %d" % (n, m, H, B, loss, track)] = {"wide": {}, "base": {}, "ill": 0.0, "guards_ok": True, "log_std_touched": 0}
        out3 = (ctypes.c_int32 * 3)()
        check(lib.mjx_policy_fit_wide_route(n, m, ints(hid), 2, B, loss, track, out3))
        r["route"], r["ran"] = int(out3[0]), []
        am0, av0 = K.pol_moments(P, m, loss)
        mom_blocks = blocks[:-1] if loss == 0 else blocks
        for steps in (1, 10):
            g1 = np.zeros(d)
            rp, rm, rv, rl, _ = F.policy_fit(th0, n, m, hid, tr, tho, tro, obs, act, adv, idx[:steps * B], B, loss, track, LR, CLIP, am0, av0,
                                             g_first=g1)
            well = g1 >= F.GRAD_FLOOR
            if loss == 0:
                well[-m:] = True                                         # no gradient there by construction: compared exactly below
                g1[-m:] = 1.0
            r["ill"] = max(r["ill"], float(np.mean(g1 < F.GRAD_FLOOR)))
            for which in ("wide", "base"):
                p, a, v, l, ok, route = gpu_fit(eng, D, which == "wide", loss, track, idx, steps, B, th0, am0, av0)
                e = r[which]
                for key, val in (("params_over_lr", F.worst(F.param_errors(p, rp, blocks, LR, well))[0]), ("m", F.worst(F.moment_errors(a, rm, mom_blocks))[0]),
                                 ("v", F.worst(F.moment_errors(v, rv, mom_blocks))[0]), ("loss", F.rel_losses(l, rl))):
                    e[key] = max(e.get(key, 0.0), float(val))
                if which == "wide":
                    r["ran"].append(route)
                    r["guards_ok"] = r["guards_ok"] and ok
                    if loss == 0:
                        r["log_std_touched"] += int(np.sum(p[-m:] != th0[-m:]) + np.sum(a[-m:] != am0[-m:]) + np.sum(v[-m:] != av0[-m:]))
        # continuation: 3 steps, then 9 with the moments carried and step0 = 3, against one 12-step call
        pa, ma, va, la, _, _ = gpu_fit(eng, D, True, loss, track, idx, 3, B, th0, am0, av0)
        pb, mb, vb, lb, _, _ = gpu_fit(eng, D, True, loss, track, idx[3 * B:], 9, B, pa, ma, va, step0=3)
        pc, mc, vc, lc, _, _ = gpu_fit(eng, D, True, loss, track, idx, 12, B, th0, am0, av0)
        r["cont_not_bitwise"] = int(np.sum(pb != pc) + np.sum(mb != mc) + np.sum(vb != vc) + np.sum(np.concatenate([la, lb]) != lc))
    eng.close()


def host_classes():
    """BC(wide_fit=True / False).fit on a (39, 28, 32 x 32) policy at mb 32 against the oracle on the same draws; one PPO step"""
    from mjrl_amd.algos.behavior_cloning import BC
    from mjrl_amd.algos.ppo_clip import PPO
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils.ingest import minibatch_indices
    from oracle import synth
    n, m, hid, mb = 39, 28, (32, 32), 32
    spec = type("Spec", (), dict(observation_dim=n, action_dim=m, horizon=40))
    paths = synth.make_paths(6, 40, n, m, seed=3)
    obs = np.float32(np.concatenate([p["observations"] for p in paths]))
    act = np.float32(np.concatenate([p["actions"] for p in paths]))
    steps = obs.shape[0] // mb
    res = {}
    for wide in (False, True):
        pol = MLP(spec, hidden_sizes=hid, seed=1, init_log_std=-0.5)
        th0 = np.float32(pol.get_param_values())
        tr = np.float32(pol.model.packed_transforms())
        bc = BC(paths, pol, epochs=1, batch_size=mb, lr=LR, loss_type="MSE", save_logs=False, wide_fit=wide)
        np.random.seed(5)
        idx = minibatch_indices(None, obs.shape[0], steps, mb).ravel()
        np.random.seed(5)
        bc.fit(dict(observations=obs, expert_actions=act))
        g1 = np.zeros(th0.size)
        ref = F.policy_fit(th0, n, m, hid, tr, th0, tr, obs, act, np.zeros(obs.shape[0]), idx, mb, 0, 0, LR, CLIP, g_first=g1)[0]
        well = g1 >= F.GRAD_FLOOR
        well[-m:] = True
        res["bc_wide" if wide else "bc_base"] = F.worst(F.param_errors(pol.get_param_values(), ref, F.policy_blocks(n, m, hid), LR, well))[0]
        res["bc_route_wide" if wide else "bc_route_base"] = bc.last_fit_route
    rng = np.random.RandomState(7)
    for p in paths:
        p["advantages"] = rng.randn(len(p["rewards"]))
    pol = MLP(spec, hidden_sizes=hid, seed=1, init_log_std=-0.5)
    agent = PPO(None, pol, None, epochs=1, mb_size=mb, learn_rate=3e-4, reference_aliasing=False, wide_fit=True)
    np.random.seed(5)
    agent.train_from_paths(paths)
    res["ppo_route_wide"] = agent.last_fit_route
    res["ppo_finite"] = bool(np.all(np.isfinite(pol.get_param_values())))
    return res


if __name__ == "__main__":
    for c in CASES:
        pol_case(*c)
    W.emit({"cases": OUT, "host": host_classes()})
