"""One small case per trainer route -> an .npz of every output array (parameters, both moments, losses; predictions): the MLP-baseline
fit on kinds 0 .. 4 and its predict (fused, chunked), the dynamics fit of one member (persistent, launches), the ensemble and the reward
fit on routes 0 and 1, the policy minibatch fit (H 64, H 32, launches; MSE and PPO).  A refactor's evidence: run once per build (MJX_LIB
selects it) and compare the two files byte for byte (tools/_dbg_npz_diff.py prints them side by side).
    python tools/bits_fit.py OUT.npz"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from mjrl_amd.engine import UpdateEngine  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._dyn_check import rand_theta, rand_tr  # noqa: E402
from tests._fit_cases import pol_data  # noqa: E402

lib = load()
dev = W.device()
OUT = {}
up = lambda x, dt=np.float32: W.up(x, dt, keep=True)


def save(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        OUT["%s/%d" % (name, i)] = t.cpu().numpy()


# ---- MLP baseline fit, kinds 0 .. 4, two steps, two epochs; and predict, fused and chunked
HID = (128, 128)
for name, d_in, batch, env, kind in (("mlp_k2_d9", 9, 64, {}, 2), ("mlp_k1_d24", 24, 64, {}, 1), ("mlp_k1_d43", 43, 64, {}, 1), ("mlp_k1_d49", 49, 64, {}, 1), ("mlp_k3_d56", 56, 64, {}, 3),
                                     ("mlp_k4_d9_b128", 9, 128, {}, 4), ("mlp_k4_d43_b128", 43, 128, {}, 4), ("mlp_k0_d24", 24, 64, {"MJX_MLP_FIT_LAUNCHES": "1"}, 0),
                                     ("mlp_k0_d9_b128", 9, 128, {"MJX_FIT_TEAM": "0"}, 0), ("mlp_k1_d9_noregmom", 9, 64, {"MJX_FIT_REGMOM": "0"}, 1)):
    rng = np.random.RandomState(100 + d_in + batch)
    N = 3 * batch
    th = up(rand_theta(rng, [d_in, 128, 128, 1]))
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    x, y = up(rng.randn(N, d_in)), up(1.0 + rng.randn(N))
    perm = up(np.concatenate([rng.permutation(N) for _ in range(2)]), np.int32)
    loss = up(np.full(2, np.nan), np.float64)
    os.environ.update(env)
    r = (ctypes.c_int32 * 6)()
    check(lib.mjx_mlp_fit_route(d_in, W.ints(HID), 2, batch, N, 2, r))
    assert r[0] == kind, (name, list(r))
    check(lib.mjx_mlp_fit_adam(ptr(x), ptr(y), N, d_in, W.ints(HID), 2, ptr(th), ptr(m), ptr(v), 3, ptr(perm), 2, batch, 1e-3, 1e-3, ptr(loss), W.stream()))
    for k in env:
        del os.environ[k]
    save(name, th, m, v, loss)
    if name in ("mlp_k1_d24", "mlp_k3_d56"):
        for fused in ("1", "0"):
            out = torch.full((N,), float("nan"), device=dev)
            os.environ["MJX_MLP_PREDICT_FUSED"] = fused
            check(lib.mjx_mlp_predict(ptr(x), N, d_in, W.ints(HID), 2, ptr(th), ptr(out), W.stream()))
            del os.environ["MJX_MLP_PREDICT_FUSED"]
            save("%s_predict_fused%s" % (name, fused), out)

# ---- dynamics: one member (persistent, launches), the ensemble (routes 0 and 1), the reward nets (routes 0 and 1)
sizes, B, steps, K, N = [7, 64, 64, 5], 32, 3, 3, 200
din, dout = sizes[0], sizes[-1]
rng = np.random.RandomState(7)
th0 = rand_theta(rng, sizes, K=K)
trs = np.stack([rand_tr(rng, din, dout) for _ in range(K)])
xs, ys = rng.randn(K, N, din).astype(np.float32), rng.randn(K, N, dout).astype(np.float32)
idx = rng.randint(0, N, size=(K, steps * B))
for env in ("0", "1"):
    os.environ["MJX_DYN_FIT_LAUNCHES"] = env
    P = up(th0[0]); m, v = torch.zeros_like(P), torch.zeros_like(P)
    loss = torch.full((steps,), float("nan"), device=dev)
    check(lib.mjx_dyn_fit_adam(ptr(up(xs[0])), ptr(up(ys[0])), N, W.ints(sizes), len(sizes), ptr(up(trs[0, :2 * din])), ptr(up(trs[0, 2 * din:])), 1, 1,
                               ptr(P), ptr(m), ptr(v), 2, ptr(up(idx[0], np.int32)), steps, B, 1e-3, 1e-4, ptr(loss), W.stream()))
    del os.environ["MJX_DYN_FIT_LAUNCHES"]
    save("dyn_one_launches%s" % env, P, m, v, loss)
rsizes = [7, 100, 100, 1]
rth0 = rand_theta(rng, rsizes, K=K)
rtrs = np.stack([rand_tr(rng, 7, 1) for _ in range(K)])
rys = rng.randn(K, N, 1).astype(np.float32)
for which, sw, fn, szs, t0, tr_, y_, extra in (("ens", "MJX_DYN_FIT_ENS", lib.mjx_dyn_fit_ensemble, sizes, th0, trs, ys, (1,)),
                                               ("reward", "MJX_REWARD_FIT_ENS", lib.mjx_reward_fit_ensemble, rsizes, rth0, rtrs, rys, ())):
    di, do = szs[0], szs[-1]
    for env in ("0", "1"):
        os.environ[sw] = env
        P = up(t0); m, v = torch.zeros_like(P), torch.zeros_like(P)
        loss = torch.full((K, steps), float("nan"), device=dev)
        s0 = (ctypes.c_int64 * K)(0, 2, 5)
        route = ctypes.c_int(-9)
        check(fn(ptr(up(xs)), N * di, ptr(up(y_)), N * do, N, K, W.ints(szs), len(szs), ptr(up(tr_[:, :2 * di])), ptr(up(tr_[:, 2 * di:])), *extra, 1,
                 ptr(P), ptr(m), ptr(v), s0, ptr(up(idx, np.int32)), steps, B, 1e-3, 1e-4, ptr(loss), ctypes.byref(route), W.stream()))
        del os.environ[sw]
        assert route.value == int(env), (which, env, route.value)
        save("%s_route%s" % (which, env), P, m, v, loss)

# ---- the team ensemble fit (route 2), the smallest shape of each team size: G = 2 with one 32-unit tile a slice and padded d_in / d_out;
# G = 4 with Bp 64 and 31 padded sample columns
for name, tsizes, tB, G, mode, act in (("team_g2", [13, 64, 64, 11], 16, 2, 1, 1), ("team_g4", [13, 128, 128, 11], 33, 4, 2, 0)):
    tK, tsteps, tN = 2, 5, 200
    rng = np.random.RandomState(11 + G)
    P = up(rand_theta(rng, tsizes, K=tK)); m, v = torch.zeros_like(P), torch.zeros_like(P)
    ttr = np.stack([rand_tr(rng, 13, 11) for _ in range(tK)])
    tx, ty = up(rng.randn(tK, tN, 13)), up(rng.randn(tK, tN, 11))
    tidx = up(rng.randint(0, tN, size=(tK, tsteps * tB)), np.int32)
    loss = torch.full((tK, tsteps), float("nan"), device=dev)
    s0 = (ctypes.c_int64 * tK)(0, 3)
    route = ctypes.c_int(-9)
    assert lib.mjx_dyn_fit_team_route(W.ints(tsizes), 4, tB, mode, tK) == G, name
    check(lib.mjx_dyn_fit_ensemble_team(ptr(tx), tN * 13, ptr(ty), tN * 11, tN, tK, W.ints(tsizes), 4, ptr(up(ttr[:, :26])), ptr(up(ttr[:, 26:])), mode, act,
                                        ptr(P), ptr(m), ptr(v), s0, ptr(tidx), tsteps, tB, 1e-3, 1e-4, ptr(loss), ctypes.byref(route), W.stream()))
    assert route.value == 2, (name, route.value)
    save(name, P, m, v, loss)

# ---- policy minibatch fit: H 64, H 32, the launch route; MSE, and PPO with an old net of its own
for name, n, mm, hid, env in (("pol_h64", 11, 3, (64, 64), {}), ("pol_h32", 11, 3, (32, 32), {}), ("pol_launches", 11, 3, (64, 64), {"MJX_NO_POLICY_FIT": "1"})):
    Bp, st = 16, 3
    D = pol_data(n, mm, hid, Bp, 55)
    eng = UpdateEngine(n, mm, hid)
    os.environ.update(env)
    for loss_kind, track in ((0, 0), (2, 0)):
        r = (ctypes.c_int32 * 2)()
        check(lib.mjx_policy_fit_route(n, mm, W.ints(hid), 2, Bp, loss_kind, track, r))
        assert (r[0] == 0) == bool(env) and (env or r[0] == hid[0]), (name, list(r))
        th = up(D["theta"]); am, av = torch.zeros_like(th), torch.zeros_like(th)
        lt = up(np.full(st, np.nan), np.float64)
        check(lib.mjx_policy_minibatch_adam(eng.ctx, loss_kind, ptr(up(D["obs"])), ptr(up(D["act"])), ptr(up(D["adv"])), ptr(up(D["idx"][:st * Bp], np.int32)),
                                            st, Bp, ptr(th), ptr(up(D["tr"])), ptr(up(D["theta_old"])), ptr(up(D["tr_old"])), track, ptr(am), ptr(av), 1,
                                            1e-3, 0.2, ptr(lt), eng.stream()))
        save("%s_loss%d" % (name, loss_kind), th, am, av, lt)
    for k in env:
        del os.environ[k]
    eng.close()

np.savez(sys.argv[1], **OUT)
print("dumped %d arrays to %s" % (len(OUT), sys.argv[1]))
