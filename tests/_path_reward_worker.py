"""GPU worker for tests/test_gpu_path_rewards.py: every learned-path-reward check in ONE fresh process; prints one JSON line of
measured errors (the test module compares them with its bars).  python tests/_path_reward_worker.py"""
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
from mjrl_amd._lib import check, load, ptr  # noqa: E402
from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy, perturbed_action_batch  # noqa: E402
from mjrl_amd.algos.model_accel.nn_dynamics import (WorldModel, ensemble_path_rewards, ensemble_path_rewards_device,  # noqa: E402
                                                    pack_reward_members)
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import emit, ints, stream, switch  # noqa: E402

R = {}
dev = W.device()
lib = load()
G = np.load(os.path.join(ROOT, "tests", "golden", "mpc_learned.npz"))
G0 = np.load(os.path.join(ROOT, "tests", "golden", "mpc.npz"))
SWITCH = "MJX_PATH_REWARDS_MFMA"
up = functools.partial(W.up, keep=True)          # every uploaded block stays alive until the process ends


def gpu_rewards(obs, act, mem, mfma, want32=True, want64=True):
    """mjx_path_rewards -> (r32 (K, N, H) or None, r64 or None, route taken); act (N, H, m): shared, (K, N, H, m): per member"""
    K, N, H, n = obs.shape
    m = act.shape[-1]
    rows = N * H
    r32 = torch.full((K, N, H), float("nan"), device=dev) if want32 else None
    r64 = torch.full((K, N, H), float("nan"), dtype=torch.float64, device=dev) if want64 else None
    route = ctypes.c_int(-1)
    ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
    with switch(SWITCH, "1" if mfma else "0"):
        check(lib.mjx_path_rewards(ptr(up(obs)), ptr(up(act)), 0 if act.ndim == 3 else rows * m, rows, K, ints(ds), len(ds),
                                   ptr(up(np.stack(mem["dyn_thetas"]))), ptr(up(np.stack(mem["dyn_trs"]))), mem["dact"], mem["dflags"],
                                   ints(rs), len(rs), ptr(up(np.stack(mem["rew_thetas"]))), ptr(up(np.stack(mem["rew_trs"]))), mem["ract"],
                                   ptr(r32), ptr(r64), ctypes.byref(route), stream()))
    return (None if r32 is None else r32.cpu().numpy(), None if r64 is None else r64.cpu().numpy(), route.value)


def world_models(mem, n, m):
    """this package's WorldModels carrying a kernel case's members (reward widths 100 x 100 only: WorldModel's own)"""
    out = []
    din, rin = n + m, 2 * n + m
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    for k in range(len(mem["dyn_thetas"])):
        wm = WorldModel(n, m, hidden_size=tuple(mem["dyn_sizes"][1:-1]), seed=k, learn_reward=True, residual=bool(mem["dflags"] & 4),
                        activation="tanh" if mem["dact"] == 1 else "relu")
        for net, th in ((wm.dynamics_net, mem["dyn_thetas"][k]), (wm.reward_net, mem["rew_thetas"][k])):
            o = 0
            for p in net.parameters():
                p.data = t(th[o:o + p.numel()].reshape(p.shape).copy()); o += p.numel()
        d, r = mem["dyn_trs"][k], mem["rew_trs"][k]
        wm.dynamics_net.set_transformations(t(d[:n]), t(d[din:din + n]), t(d[n:din]), t(d[din + n:2 * din]), t(d[2 * din:2 * din + n]),
                                            t(d[2 * din + n:]))
        wm.reward_net.set_transformations(t(r[:n]), t(r[rin:rin + n]), t(r[n:din]), t(r[rin + n:rin + din]), float(r[2 * rin]),
                                          float(r[2 * rin + 1]))
        out.append(wm)
    return out


# ---- (1) mjx_path_rewards on both routes against the fp64 oracle, per member: every kernel case, both row sets, shared and
# per-member actions; route_out against mjx_path_rewards_route; r64 == r32 widened; one output pointer at a time
err = {1: {}, 0: {}}
routes, same_bits, route_ok, widened, single_ok = {}, [], True, True, True
for name in sorted(L.KCASES):
    mem, data = L.kernel_case(name)
    ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
    served = lib.mjx_path_rewards_route(ints(ds), len(ds), ints(rs), len(rs))
    assert served == 1, name
    for (N, H), (obs, shared, own) in data.items():
        for mode, act in (("shared", shared), ("own", own)):
            ref = L.ensemble_rewards(obs, act, mem)
            outs = {}
            for mfma in (1, 0):
                r32, r64, route = gpu_rewards(obs, act, mem, mfma)
                outs[mfma] = r32
                e = L.rel_max(r32, ref)
                print("kernel %s rows %d %s route %d: %.3e" % (name, N * H, mode, mfma, e), flush=True)
                err[mfma][name] = max(err[mfma].get(name, 0.0), e)
                route_ok = route_ok and route == (served if mfma else 0)
                widened = widened and np.array_equal(r64, r32.astype(np.float64)) and not np.isnan(r32).any()
            routes[name] = max(routes.get(name, 0.0), L.rel_max(outs[1], outs[0]))
            if N * H > 32 and np.array_equal(outs[1], outs[0]):     # two kernels with different summation orders never agree to the bit
                same_bits.append("%s %d %s" % (name, N * H, mode))  # over hundreds of values: equal bits mean a quiet fallback
    (N, H), (obs, shared, own) = next(iter(data.items()))
    for mfma in (1, 0):
        both = gpu_rewards(obs, shared, mem, mfma)
        only32, only64 = gpu_rewards(obs, shared, mem, mfma, want64=False), gpu_rewards(obs, shared, mem, mfma, want32=False)
        single_ok = single_ok and np.array_equal(only32[0], both[0]) and np.array_equal(only64[1], both[1])
R["kernel_mfma"], R["kernel_generic"], R["routes"], R["routes_same_bits"] = err[1], err[0], routes, same_bits
R["route_out_ok"], R["widened_exact"], R["single_output_ok"] = bool(route_ok), bool(widened), bool(single_ok)
R["kref"] = {name: float(G["kref_" + name]) for name in L.KCASES}
z = torch.zeros(8, device=dev)
rt = ctypes.c_int(-1)
R["empty_ok"] = [lib.mjx_path_rewards(ptr(z), ptr(z), 0, 0, 2, ints((8, 64, 64, 6)), 4, ptr(z), ptr(z), 0, 7, ints((14, 100, 100, 1)), 4, ptr(z),
                                      ptr(z), 0, ptr(z), None, ctypes.byref(rt), stream()), rt.value]

# ---- (2) route 0 is ensemble_path_rewards bit for bit: forced by the switch on a served shape (k1's members as WorldModels), and by
# the shape itself (dynamics 256 x 256)
bits = {}
mem, data = L.kernel_case("k1")
models = world_models(mem, 6, 2)
(N, H), (obs, shared, own) = next(iter(data.items()))
want = ensemble_path_rewards(models, obs, own)
with switch(SWITCH, "0"):
    got = ensemble_path_rewards_device(models, up(obs), up(own)).cpu().numpy()
bits["forced"] = bool(np.array_equal(got, want) and got.dtype == np.float32 and got.shape == (3, N, H))
got1, got1_64 = ensemble_path_rewards_device(models, up(obs), up(own), want64=True)
bits["mfma_differs"] = bool(not np.array_equal(got1.cpu().numpy(), want))        # (... and the default route is the other kernel)
bits["want64"] = bool(np.array_equal(got1_64.cpu().numpy(), got1.cpu().numpy().astype(np.float64)))
packed = pack_reward_members(models, dev)           # (... and blocks packed once serve later calls)
bits["packed"] = bool(np.array_equal(ensemble_path_rewards_device(models, up(obs), up(own), packed=packed).cpu().numpy(), got1.cpu().numpy()))
wide = [WorldModel(6, 2, hidden_size=(256, 256), seed=40 + k, learn_reward=True) for k in range(2)]
rng = np.random.RandomState(11)
obs_w, act_w = rng.randn(2, 33, 5, 6).astype(np.float32), rng.randn(2, 33, 5, 2).astype(np.float32)
assert lib.mjx_path_rewards_route(ints((8, 256, 256, 6)), 4, ints((14, 100, 100, 1)), 4) == 0
bits["unserved"] = bool(np.array_equal(ensemble_path_rewards_device(wide, up(obs_w), up(act_w)).cpu().numpy(),
                                       ensemble_path_rewards(wide, obs_w, act_w)))
shared_w = np.ascontiguousarray(act_w[0])
bits["unserved_shared"] = bool(np.array_equal(ensemble_path_rewards_device(wide, up(obs_w), up(shared_w)).cpu().numpy(),
                                              ensemble_path_rewards(wide, obs_w, np.stack([shared_w, shared_w]))))
R["route0_bits"] = bits

# ---- (3) MPCPolicy(reward='learned') on an env with NO compute_path_rewards against the reference's fixture, call by call (each
# from the fixture's input sequence), then the three calls chained under warm start; both reward routes
pol_seq, pol_R, pol_rew, chain_seq, streams, shapes_ok = {}, {}, {}, {}, True, True
members = L.load_members(WorldModel, torch, G)
for ci, case in enumerate(sorted(L.PLAN_CASES)):
    N, H, kappa, omega, fc, gamma = L.PLAN_CASES[case]
    for mfma in (1, 0):
        with switch(SWITCH, mfma):
            name = case if mfma else case + "_generic"
            for chained in (False, True):
                env = L.plan_env_no_rewards(L.PN, L.PM)
                assert not hasattr(env.env.env, "compute_path_rewards")
                pol = MPCPolicy(env=env, plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc), warmstart=True,
                                fitted_model=members, omega=omega, reward='learned')
                assert pol.route() == 1 and pol.reward_route() == 1
                np.random.seed(900 + ci)
                for c in range(L.CALLS):
                    key = "%s_%d_" % (case, c)
                    if not chained:
                        pol.act_sequence = G[key + "seq_in"].copy()
                    action = pol.get_action(G[key + "obs"])
                    streams = streams and np.random.rand() == float(G[key + "after"])
                    ref_seq = np.concatenate([G[key + "action"][None], G[key + "seq_out"][:-1]])
                    got_seq = np.concatenate([action[None], pol.act_sequence[:-1]])
                    if chained:
                        chain_seq[name] = max(chain_seq.get(name, 0.0), M.rel_l2(got_seq, ref_seq))
                    else:
                        Rg, rg = pol.last_scores()[0], pol.last_rewards()
                        shapes_ok = shapes_ok and rg.shape == (L.PK, N, H) and rg.dtype == np.float64
                        e_seq, e_R = M.rel_l2(got_seq, ref_seq), float(np.max(np.abs(Rg - G[key + "R"])) / np.ptp(G[key + "R"]))
                        e_rew = L.rel_max(rg, G[key + "rewards"])
                        print("planner %s call %d: sequence %.3e  R/spread %.3e  rewards %.3e" % (name, c, e_seq, e_R, e_rew), flush=True)
                        pol_seq[name], pol_R[name] = max(pol_seq.get(name, 0.0), e_seq), max(pol_R.get(name, 0.0), e_R)
                        pol_rew[name] = max(pol_rew.get(name, 0.0), e_rew)
R["policy_seq"], R["policy_R"], R["policy_rewards"], R["chained_seq"] = pol_seq, pol_R, pol_rew, chain_seq
R["streams_equal"], R["last_rewards_ok"] = bool(streams), bool(shapes_ok)

# ---- (4) a bare WorldModel on learned rewards (K = 1, no disagreement term; the reference raises there) against the fp64
# restatement, and the re-pack after a reward refit by the package's own trainer
N, H, kappa, omega, fc, gamma = L.PLAN_CASES["lb"]
mem = L.fixture_members(G)
mem1 = dict(mem, dyn_thetas=mem["dyn_thetas"][:1], dyn_trs=mem["dyn_trs"][:1], rew_thetas=mem["rew_thetas"][:1], rew_trs=mem["rew_trs"][:1])
pol = MPCPolicy(env=L.plan_env_no_rewards(L.PN, L.PM), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc),
                fitted_model=members[0], omega=omega, reward='learned', warmstart=False)
np.random.seed(77)
actions = perturbed_action_batch(N, pol.act_sequence, list(fc))
np.random.seed(77)
action = pol.get_action(G["lb_0_obs"])
r = L.plan(G["lb_0_obs"], actions, mem1, kappa, gamma, omega, ensemble=False)
R["bare"] = dict(action=M.rel_l2(action, r["seq"][0]), R=float(np.max(np.abs(pol.last_scores()[0] - r["R"])) / np.max(np.abs(r["R"]))),
                 ess=M.ess(r["S"]), rewards=L.rel_max(pol.last_rewards(), r["rewards"]))

pol = MPCPolicy(env=L.plan_env_no_rewards(L.PN, L.PM), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc),
                fitted_model=members, omega=omega, reward='learned', warmstart=False)
np.random.seed(1); pol.get_action(G["lb_0_obs"]); pack0 = pol._pack[1]["rew"]["rew_P"]; rew0 = pol.last_rewards()
np.random.seed(1); pol.get_action(G["lb_0_obs"]); same = pol._pack[1]["rew"]["rew_P"] is pack0
old = M.flat_params(members[2].reward_net)
fs, fa, fsp, fr = L.reward_fit_data(400, 90)
members[2].fit_reward(fs, fa, fr, 32, 10, set_transformations=False)
new = M.flat_params(members[2].reward_net)
np.random.seed(1); actions = perturbed_action_batch(N, pol.act_sequence, list(fc))
np.random.seed(1); a3 = pol.get_action(G["lb_0_obs"]); rew3 = pol.last_rewards()
mem_new = dict(mem, rew_thetas=mem["rew_thetas"][:2] + [new])
plan_new = L.plan(G["lb_0_obs"], actions, mem_new, kappa, gamma, omega)
# the rewards against the fp64 chain on the observations the planner's own rollout produced (the same launch on the same packed
# members and fp32 inputs gives the same bits): the kernel's error alone, the quantity the kernel cases bound
pk = pol._packed(dev)
a32 = np.asarray(actions, np.float32)
obs_d = torch.empty((L.PK, N, H, L.PN), dtype=torch.float32, device=dev)
check(lib.mjx_plan_rollout(ptr(up(G["lb_0_obs"])), 0, N, H, L.PK, ptr(up(a32)), ints(pk["sizes"]), len(pk["sizes"]), ptr(pk["P"]), ptr(pk["tr"]),
                           pk["act"], pk["flags"], ptr(obs_d), stream()))
obs_g = obs_d.cpu().numpy()
own_new, own_old = L.ensemble_rewards(obs_g, a32, mem_new), L.ensemble_rewards(obs_g, a32, mem)
R["refit"] = dict(same_before=bool(same), repacked=bool(pol._pack[1]["rew"]["rew_P"] is not pack0), moved=float(np.max(np.abs(new - old))),
                  others_unchanged=bool(np.array_equal(rew3[:2], rew0[:2])), rewards_vs_new=L.rel_max(rew3, own_new),
                  rewards_before=L.rel_max(rew0, own_old), pref=float(G["lb_0_pref"]),
                  rewards_vs_old=L.rel_max(rew3, own_old), action_vs_new=M.rel_l2(a3, plan_new["seq"][0]))

# ---- (5) reward='env' is today's planner: case a of the existing fixture, call by call
case = "a"
n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
env_models = []
for k in range(K):
    wm = WorldModel(n, m, hidden_size=hid, seed=70 + k)
    th, tr = G0["fit_%d_params" % k], G0["fit_%d_tr" % k]
    ws, o = [], 0
    for p in wm.dynamics_net.parameters():
        ws.append(torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy())); o += p.numel()
    trl = [torch.from_numpy(tr[a:a + l].copy()) for a, l in zip(np.cumsum([0, n, n, m, m, n]), [n, n, m, m, n, n])]
    wm.dynamics_net.set_params(dict(weights=ws, transforms=trl))
    env_models.append(wm)
pol = MPCPolicy(env=M.plan_env(n, m), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc), warmstart=True,
                fitted_model=env_models, omega=omega)
assert pol.reward == 'env'
np.random.seed(500 + sorted(M.CASES).index(case))
e_seq = e_R = 0.0
env_streams = True
for c in range(M.CALLS):
    key = "%s_%d_" % (case, c)
    pol.act_sequence = G0[key + "seq_in"].copy()
    action = pol.get_action(G0[key + "obs"])
    env_streams = env_streams and np.random.rand() == float(G0[key + "after"])
    e_seq = max(e_seq, M.rel_l2(np.concatenate([action[None], pol.act_sequence[:-1]]), np.concatenate([G0[key + "action"][None], G0[key + "seq_out"][:-1]])))
    e_R = max(e_R, float(np.max(np.abs(pol.last_scores()[0] - G0[key + "R"])) / np.max(np.abs(G0[key + "R"]))))
R["env_mode"] = dict(seq=e_seq, R=e_R, streams=bool(env_streams), no_rewards=pol.last_rewards() is None)
emit(R)
