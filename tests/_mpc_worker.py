"""GPU worker for tests/test_gpu_mpc.py: every MPC planning check in ONE fresh process; prints one JSON line of measured
errors (the test module compares them with its bars).  python tests/_mpc_worker.py"""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _dyn_oracle as O  # noqa: E402
import _mpc_oracle as M  # noqa: E402
from mjrl_amd._lib import check, load, ptr  # noqa: E402
from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy, perturbed_action_batch  # noqa: E402
from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import emit, ints, stream, switch  # noqa: E402

R = {}
dev = W.device()
lib = load()
G = np.load(os.path.join(ROOT, "tests", "golden", "mpc.npz"))
up = functools.partial(W.up, keep=True)          # every uploaded block stays alive until the process ends


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def gpu_rollout(s0, actions, thetas, sizes, trs, act, flags, mfma):
    K, (N, H) = len(thetas), actions.shape[:2]
    n = sizes[-1]
    obs = torch.full((K, N, H, n), float("nan"), device=dev)
    with switch("MJX_PLAN_MFMA", "1" if mfma else "0"):
        check(lib.mjx_plan_rollout(ptr(up(s0)), 0 if np.ndim(s0) == 1 else n, N, H, K, ptr(up(actions)), ints(sizes), len(sizes),
                                   ptr(up(np.stack(thetas))), ptr(up(np.stack(trs))), act, flags, ptr(obs), stream()))
    return obs.cpu().numpy()


def step_errors(got, s0, actions, thetas, sizes, trs, act, flags):
    """step by step: the first stored state against s0, then every stored state against the fp64 step from the stored state
    before it (teacher forcing: the error of ONE step, whatever the horizon); and the free-running fp64 rollout"""
    a32 = np.asarray(actions, np.float32)
    N = a32.shape[0]
    s0 = np.asarray(s0, np.float32)
    s0 = np.tile(s0, (N, 1)) if s0.ndim == 1 else s0
    err = 0.0
    for k in range(len(thetas)):
        assert np.array_equal(got[k][:, 0], s0), "observations[:, 0] is the start state"
        for t in range(a32.shape[1] - 1):
            ref = O.rollout_next(got[k][:, t], a32[:, t], np.float32(thetas[k]), list(sizes), np.float32(trs[k]), act, flags)
            err = max(err, rel(got[k][:, t + 1], ref))
    free = rel(got, M.rollout(s0, a32, thetas, sizes, trs, act, flags))
    return err, free


def case_setup(case):
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
    if case in M.FITTED:
        models = []
        for k in range(K):
            wm = WorldModel(n, m, hidden_size=hid, seed=70 + k)
            th, tr = G["fit_%d_params" % k], G["fit_%d_tr" % k]
            ws, o = [], 0
            for p in wm.dynamics_net.parameters():
                ws.append(torch.from_numpy(th[o:o + p.numel()].reshape(p.shape).copy())); o += p.numel()
            trl = [torch.from_numpy(tr[a:a + l].copy()) for a, l in zip(np.cumsum([0, n, n, m, m, n]), [n, n, m, m, n, n])]
            wm.dynamics_net.set_params(dict(weights=ws, transforms=trl))
            models.append(wm)
    else:
        models = M.init_members(WorldModel, torch, case)
    ths = [M.flat_params(w.dynamics_net) for w in models]
    trs = [M.packed(M.flat_transforms(w.dynamics_net), n, m) for w in models]
    return models, ths, trs, (n + m,) + tuple(hid) + (n,), (1 if activation == "tanh" else 0), (7 if residual else 3)


# ---- (1) mjx_plan_rollout on both routes against fp64: the fixture cases ...
step = {1: {}, 0: {}}
free = {1: {}, 0: {}}
routes = {}
same_bits = []
for ci, case in enumerate(sorted(M.CASES)):
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
    models, ths, trs, sizes, act, flags = case_setup(case)
    np.random.seed(500 + ci)
    actions = perturbed_action_batch(N, G["%s_0_seq_in" % case], list(fc))
    s0 = G["%s_0_obs" % case]
    assert lib.mjx_plan_route(ints(sizes), len(sizes), m) == M.ROUTES[case]
    outs = {}
    for mfma in (1, 0):
        outs[mfma] = gpu_rollout(s0, actions, ths, sizes, trs, act, flags, mfma)
        step[mfma][case], free[mfma][case] = step_errors(outs[mfma], s0, actions, ths, sizes, trs, act, flags)
    if M.ROUTES[case]:
        routes[case] = rel(outs[1], outs[0])
        if np.array_equal(outs[1], outs[0]):            # two kernels with different summation orders never agree to the bit:
            same_bits.append(case)                      # equal bits mean the MFMA kernel did not run (a quiet fallback)
# ... and the edge shapes: N around the 32-trajectory tile and the 128-trajectory workgroup, H = 1, s0 as one state and per
# trajectory, a masked output column, ReLU and tanh, every flag combination the nets use
masked_exact = True
for N in (1, 31, 32, 33, 129):
    for H in (1, 7):
        for per_traj in (False, True):
            rng = np.random.RandomState(1000 * N + 10 * H + per_traj)
            n, m, K = 6, 3, 2
            sizes = (n + m, 64, 32, n)
            act, flags = (N + H) % 2, (7, 3, 1, 5)[(N + H + per_traj) % 4]
            P = sum(sizes[i] * sizes[i + 1] + sizes[i + 1] for i in range(3))
            ths = [(rng.randn(P) * 0.2).astype(np.float32) for _ in range(K)]
            trs = []
            for _ in range(K):
                tr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
                tr[2 * (n + m) + n + 2] = 0.0           # out_scale of state column 2
                trs.append(tr.astype(np.float32))
            s0 = (rng.randn(N, n) if per_traj else rng.randn(n)).astype(np.float32)
            actions = rng.randn(N, H, m)
            outs = {}
            for mfma in (1, 0):
                got = outs[mfma] = gpu_rollout(s0, actions, ths, sizes, trs, act, flags, mfma)
                e, f = step_errors(got, s0, actions, ths, sizes, trs, act, flags)
                step[mfma]["edge"] = max(step[mfma].get("edge", 0.0), e)
                free[mfma]["edge"] = max(free[mfma].get("edge", 0.0), f)
                if flags & 2:                           # masked: the column is 0 (+ the start state under the residual), exactly
                    col0 = (np.tile(s0, (N, 1)) if s0.ndim == 1 else s0)[:, 2]
                    want = np.where(np.arange(H)[None, :] == 0, col0[:, None], (col0[:, None] if flags & 4 else 0.0))
                    masked_exact = masked_exact and all(np.array_equal(got[k][:, :, 2], np.broadcast_to(want, (N, H))) for k in range(K))
            routes["edge"] = max(routes.get("edge", 0.0), rel(outs[1], outs[0]))
# ... and the instances no fixture case reaches: two state blocks with one, three and four hidden blocks -- <4, 2> at the largest
# LDS image the route admits ([96, 128, 128, 64], m = 32) -- with random weights, N across a tile boundary
for n, m, hid in ((64, 32, (128, 128)), (40, 5, (32, 32)), (33, 9, (96, 64))):
    rng = np.random.RandomState(n + m)
    K, N, H = 2, 70, 4
    sizes = (n + m,) + hid + (n,)
    assert lib.mjx_plan_route(ints(sizes), len(sizes), m) == 1
    P = sum(sizes[i] * sizes[i + 1] + sizes[i + 1] for i in range(3))
    ths = [(rng.randn(P) * 0.1).astype(np.float32) for _ in range(K)]
    trs = [np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1]).astype(np.float32)
           for _ in range(K)]
    s0 = rng.randn(N, n).astype(np.float32)
    actions = rng.randn(N, H, m)
    act, flags = n % 2, 7
    outs = {}
    for mfma in (1, 0):
        outs[mfma] = gpu_rollout(s0, actions, ths, sizes, trs, act, flags, mfma)
        e, f = step_errors(outs[mfma], s0, actions, ths, sizes, trs, act, flags)
        step[mfma]["wide"] = max(step[mfma].get("wide", 0.0), e)
        free[mfma]["wide"] = max(free[mfma].get("wide", 0.0), f)
    routes["wide"] = max(routes.get("wide", 0.0), rel(outs[1], outs[0]))
    if np.array_equal(outs[1], outs[0]):
        same_bits.append("wide %d" % n)
R["routes_same_bits"] = same_bits
R["rollout_step_mfma"], R["rollout_step_generic"] = step[1], step[0]
R["rollout_free_mfma"], R["rollout_free_generic"] = free[1], free[0]
R["routes"] = routes
R["masked_exact"] = bool(masked_exact)
# N = 0 and H = 0 return without a launch
z = torch.zeros(8, device=dev)
R["empty_ok"] = [lib.mjx_plan_rollout(ptr(z), 0, 0, 3, 1, ptr(z), ints((9, 64, 32, 6)), 4, ptr(z), ptr(z), 0, 7, ptr(z), stream()),
                 lib.mjx_plan_rollout(ptr(z), 0, 3, 0, 1, ptr(z), ints((9, 64, 32, 6)), 4, ptr(z), ptr(z), 0, 7, ptr(z), stream())]

# ---- (2) mjx_plan_score against NumPy fp64: both index settings, K = 1, no disagreement term
err_score = 0.0
for K, N, H, n, m, kappa, gamma, omega in [(3, 40, 8, 6, 2, 1.0, 1.0, 5.0), (4, 1024, 32, 17, 6, 5.0, 0.95, 2.0), (1, 33, 5, 6, 2, 2.0, 0.9, 5.0),
                                           (2, 2, 3, 65, 33, 0.5, 0.99, 1.0), (3, 300, 12, 5, 1, 3.0, 0.5, 0.0)]:
    rng = np.random.RandomState(K * 100 + H)
    obs = rng.randn(K, N, H, n).astype(np.float32)
    rew = rng.randn(K, N, H) * 0.3
    acts = rng.randn(N, H, m)
    for mode in ("reference", "trajectory", "none"):
        Rd = torch.empty(K * N, dtype=torch.float64, device=dev); Sd = torch.empty_like(Rd)
        qd = torch.empty(H * m, dtype=torch.float64, device=dev)
        check(lib.mjx_plan_score(None if mode == "none" else ptr(up(obs)), ptr(up(rew, np.float64)), ptr(up(acts, np.float64)), K, N, H, n, m,
                                 kappa, gamma, omega, 1 if mode == "trajectory" else 0, ptr(Rd), ptr(Sd), ptr(qd), stream()))
        Rr = M.scores(obs, rew, omega, gamma, mode == "reference", mode != "none")
        Sr = M.weights(Rr, kappa)
        err_score = max(err_score, float(np.max(np.abs(Rd.cpu().numpy() - Rr)) / np.max(np.abs(Rr))),
                        float(np.max(np.abs(Sd.cpu().numpy() - Sr))), M.rel_l2(qd.cpu().numpy(), M.sequence(Sr, acts, K)))
R["score"] = err_score

# ---- (3) MPCPolicy.get_action against the reference's fixture, call by call (each from the fixture's input sequence), then the
# three calls chained under warm start; both routes where the MFMA route serves the case
pol_seq, pol_act, pol_R, chain_seq, streams = {}, {}, {}, {}, True
for ci, case in enumerate(sorted(M.CASES)):
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
    models = case_setup(case)[0]
    for mfma in ((1, 0) if M.ROUTES[case] else (1,)):
        with switch("MJX_PLAN_MFMA", mfma):
            name = case if mfma else case + "_generic"
            for chained in (False, True):
                pol = MPCPolicy(env=M.plan_env(n, m), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc),
                                warmstart=True, fitted_model=models, omega=omega)
                assert pol.route() == M.ROUTES[case]
                np.random.seed(500 + ci)
                for c in range(M.CALLS):
                    key = "%s_%d_" % (case, c)
                    if not chained:
                        pol.act_sequence = G[key + "seq_in"].copy()
                    action = pol.get_action(G[key + "obs"])
                    streams = streams and np.random.rand() == float(G[key + "after"])
                    ref_seq = np.concatenate([G[key + "action"][None], G[key + "seq_out"][:-1]])
                    got_seq = np.concatenate([action[None], pol.act_sequence[:-1]])
                    assert np.array_equal(pol.act_sequence[-1], np.zeros(m))
                    if chained:
                        chain_seq[name] = max(chain_seq.get(name, 0.0), M.rel_l2(got_seq, ref_seq))
                    else:
                        pol_seq[name] = max(pol_seq.get(name, 0.0), M.rel_l2(got_seq, ref_seq))
                        pol_act[name] = max(pol_act.get(name, 0.0), M.rel_l2(action, G[key + "action"]))
                        Rg = pol.last_scores()[0]
                        pol_R[name] = max(pol_R.get(name, 0.0), float(np.max(np.abs(Rg - G[key + "R"])) / np.max(np.abs(G[key + "R"]))))
R["policy_seq"], R["policy_action"], R["policy_R"], R["chained_seq"], R["streams_equal"] = pol_seq, pol_act, pol_R, chain_seq, bool(streams)

# ---- (4) the packed members are re-packed when a parameter changes, and only then
models = M.init_members(WorldModel, torch, "f")
n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES["f"]
pol = MPCPolicy(env=M.plan_env(n, m), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc), fitted_model=models, omega=omega)
np.random.seed(1); pol.get_action(G["f_0_obs"]); pack0 = pol._pack[1]["P"]
pol.act_sequence = pol.init_act_sequence.copy()
np.random.seed(1); a1 = pol.get_action(G["f_0_obs"]); same = pol._pack[1]["P"] is pack0
with torch.no_grad():
    next(models[1].dynamics_net.parameters()).mul_(1.5)
pol.act_sequence = pol.init_act_sequence.copy()
np.random.seed(1); a2 = pol.get_action(G["f_0_obs"])
R["repack"] = [bool(same), bool(pol._pack[1]["P"] is not pack0), bool(not np.array_equal(a1, a2))]

# ... and after a member is refitted by the package's own trainer with the transforms kept (the write-back goes through p.data,
# which leaves p._version alone): the next call must plan on the NEW weights
pol.act_sequence = pol.init_act_sequence.copy()
np.random.seed(1); pol.get_action(G["f_0_obs"]); pack1 = pol._pack[1]["P"]
old = [M.flat_params(w.dynamics_net) for w in models]
fs, fa, fsp = M.fit_data(400, n, m, 90)
models[2].fit_dynamics(fs, fa, fsp, 32, 20, set_transformations=False)
new = [M.flat_params(w.dynamics_net) for w in models]
trs_f = [M.packed(M.flat_transforms(w.dynamics_net), n, m) for w in models]
pol.act_sequence = pol.init_act_sequence.copy()
np.random.seed(1); acts_f = perturbed_action_batch(N, pol.act_sequence, list(fc))
np.random.seed(1); a3 = pol.get_action(G["f_0_obs"])
sizes_f = (n + m,) + tuple(hid) + (n,)
plans = [M.plan(G["f_0_obs"], acts_f, th, sizes_f, trs_f, 0, 7, kappa, gamma, omega) for th in (new, old)]
R["refit"] = dict(repacked=bool(pol._pack[1]["P"] is not pack1), moved=float(np.max(np.abs(new[2] - old[2]))),
                  action_vs_new=M.rel_l2(a3, plans[0]["seq"][0]), action_vs_old=M.rel_l2(a3, plans[1]["seq"][0]),
                  R_vs_new=float(np.max(np.abs(pol.last_scores()[0] - plans[0]["R"])) / np.max(np.abs(plans[0]["R"]))),
                  ess=M.ess(plans[0]["S"]))

# ---- (5) a bare WorldModel (the reference raises there): the same draws, one rollout, score_trajectory; and the per-trajectory
# disagreement index on an ensemble -- both against the fp64 restatement
err_bare, err_bare_R, min_ess = 0.0, 0.0, 1e30
# (case a's kappa = 1 leaves an effective sample size of 4.6 of 120 under the per-trajectory index: 0.25 there, 32.8)
for case, bare, ref_idx, kap in (("f", True, True, None), ("a", False, False, 0.25), ("g", True, True, None)):
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
    kappa = kappa if kap is None else kap
    models, ths, trs, sizes, act, flags = case_setup(case)
    fm = models[0] if bare else models
    pol = MPCPolicy(env=M.plan_env(n, m), plan_horizon=H, plan_paths=N, kappa=kappa, gamma=gamma, filter_coefs=list(fc), fitted_model=fm,
                    omega=omega, reference_indexing=ref_idx, warmstart=False)
    np.random.seed(77)
    actions = perturbed_action_batch(N, pol.act_sequence, list(fc))
    np.random.seed(77)
    action = pol.get_action(G[case + "_0_obs"])
    r = M.plan(G[case + "_0_obs"], actions, ths[:1] if bare else ths, sizes, trs[:1] if bare else trs, act, flags, kappa, gamma, omega,
               reference_indexing=ref_idx, ensemble=not bare)
    min_ess = min(min_ess, M.ess(r["S"]))
    assert np.array_equal(pol.act_sequence, pol.init_act_sequence)          # warmstart off
    err_bare = max(err_bare, M.rel_l2(action, r["seq"][0]))
    err_bare_R = max(err_bare_R, float(np.max(np.abs(pol.last_scores()[0] - r["R"])) / np.max(np.abs(r["R"]))))
R["bare_action"], R["bare_R"], R["bare_min_ess"] = err_bare, err_bare_R, min_ess
emit(R)
