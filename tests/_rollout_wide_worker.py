"""GPU worker of tests/test_gpu_rollout_wide.py: every check of mjx_policy_rollout_wide in one process; prints one RESULT line (JSON).
Every output block starts as NaN with 64 NaN guard elements behind it; after a call no NaN may stay inside and nothing behind it
may be touched (asserted here, per call).  "Route 0" is the same entry under MJX_POLICY_ROLLOUT_WIDE=0."""
import ctypes
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build()
from mjrl_amd import _lib  # noqa: E402
from mjrl_amd._lib import ptr  # noqa: E402
import _refine_oracle as F  # noqa: E402
import _rollout_wide_cases as W  # noqa: E402
from tests._worker_dev import checked_block, device, emit, ints, nan_block as guarded, same_bits as bits, switch, up  # noqa: E402

lib = _lib.load()
dev = device()
SWITCHES = ("MJX_POLICY_ROLLOUT_WIDE", "MJX_POLICY_ROLLOUT_MFMA")


def unguard(buf, shape, what, nan_rows=()):
    """the block behind its guard; nan_rows: trajectories (axis 1) that may hold NaN"""
    numel = int(np.prod(shape))
    if not nan_rows:
        return checked_block(buf, numel, what).reshape(shape).copy()
    h = buf.cpu().numpy()
    assert np.isnan(h[numel:]).all(), what + ": the guard behind the block was touched"
    out = h[:numel].reshape(shape).copy()
    keep = np.ones(shape[1], bool)
    keep[list(nan_rows)] = False
    assert not np.isnan(out[:, keep]).any(), what + ": NaN left inside the block"
    return out


def blocks(c):
    return dict(P=up(np.stack(c["dyn_thetas"])), tr=up(np.stack(c["dyn_trs"])), pP=up(c["pol_theta"]), ptr=up(c["pol_tr"]),
                b=[None] * 4 if c["bounds"] is None else [up(v) for v in c["bounds"]])


def rollout(c, wide="1", mfma=None, entry="mjx_policy_rollout_wide", s0=None, nan_rows=(), d=None):
    """one call of `entry` under MJX_POLICY_ROLLOUT_WIDE = wide (and MJX_POLICY_ROLLOUT_MFMA = mfma if given) -> (obs, act, route)"""
    K, N, H, n, m = c["K"], c["N"], c["H"], c["n"], c["m"]
    d = blocks(c) if d is None else d
    s0 = c["s0"] if s0 is None else s0
    nz = c["noise"]
    s0_d, nz_d = up(s0), up(nz)
    ob, ab = guarded(K * N * H * n), guarded(K * N * H * m)
    route = ctypes.c_int(-9)
    with switch(SWITCHES[0], wide), switch(SWITCHES[1], mfma):
        rc = getattr(lib, entry)(ptr(s0_d), n if s0.ndim == 2 else 0, N, H, K, ints(c["pol_sizes"]), len(c["pol_sizes"]), ptr(d["pP"]),
                                 ptr(d["ptr"]), ptr(nz_d), H * N * m if (nz is not None and nz.ndim == 4) else 0, ints(c["dyn_sizes"]),
                                 len(c["dyn_sizes"]), ptr(d["P"]), ptr(d["tr"]), c["act"], c["flags"], ptr(d["b"][0]), ptr(d["b"][1]),
                                 ptr(d["b"][2]), ptr(d["b"][3]), ptr(ob), ptr(ab), ctypes.byref(route), None)
    _lib.check(rc)
    torch.cuda.synchronize()
    return unguard(ob, (K, N, H, n), "obs", nan_rows), unguard(ab, (K, N, H, m), "act", nan_rows), route.value


def kernel_checks(res):
    res.update(step={"2": {}, "0": {}}, routes={}, route_out={}, route_fn={}, differ={}, switch_bits={}, free={}, chained={})
    for name in sorted(W.WCASES):
        c = W.wide_case(name)
        res["route_fn"][name] = lib.mjx_policy_rollout_wide_route(ints(c["pol_sizes"]), len(c["pol_sizes"]), ints(c["dyn_sizes"]), len(c["dyn_sizes"]))
        o2, a2, r2 = rollout(c)
        o0, a0, r0 = rollout(c, wide="0")
        _, _, rm = rollout(c, mfma="0")
        ob, ab, rb = rollout(c, wide="0", entry="mjx_policy_rollout")
        res["route_out"][name] = [r2, r0, rm, rb]
        res["switch_bits"][name] = bits(o0, ob) and bits(a0, ab)
        res["step"]["2"][name] = list(F.step_errors(c, o2, a2))
        res["step"]["0"][name] = list(F.step_errors(c, o0, a0))
        res["routes"][name] = [F.rel_max(a2, a0), F.rel_max(o2, o0)]
        res["differ"][name] = not (bits(o2, o0) and bits(a2, a0))
        if name == "w1":
            res["shared"] = all(bits(a2[k, :, 0], a2[0, :, 0]) for k in range(c["K"]))
            o2b, a2b, _ = rollout(c)
            res["repeat"] = bits(o2, o2b) and bits(a2, a2b)
        if name == "w2":                                  # flags 3: a masked output column is exactly 0 in every stored next state
            res["masked_zero"] = bool(np.all(o2[:, :, 1:, W.W2_MASKED] == 0.0) and np.all(o0[:, :, 1:, W.W2_MASKED] == 0.0))
            bad, s0 = 40, c["s0"].copy()
            s0[bad] = np.nan
            on, an, _ = rollout(c, s0=s0, nan_rows=(bad,))
            others = np.arange(c["N"]) != bad
            res["nan"] = dict(others=bits(on[:, others], o2[:, others]) and bits(an[:, others], a2[:, others]),
                              s0_nan=bool(np.isnan(on[:, bad, 0]).all()))
        if name == "w8":
            res["h1_s0_exact"] = bits(o2[:, :, 0], np.stack([F.case_s0_rows(c)] * c["K"]))
        print(name, res["step"]["2"][name], res["step"]["0"][name], res["routes"][name], flush=True)
    # free-running, one case, both routes
    c = W.wide_case(W.FREE_CASE, W.FREE_H)
    o64, a64 = F.free_rollout(c)
    for wide in "10":
        o, a, r = rollout(c, wide=wide)
        assert r == (2 if wide == "1" else 0), r
        res["free"]["2" if wide == "1" else "0"] = [F.rel_max(a, a64), F.rel_max(o, o64)]
    # shapes the register-resident route serves too: the wide kernel on _refine_oracle's p1 and p7, called directly
    for name in ("p1", "p7"):
        c = F.kernel_case(name)
        o, a, r = rollout(c)
        res["chained"][name] = list(F.step_errors(c, o, a)) + [r]


def python_checks(res):
    from mjrl_amd.algos.model_accel import model_accel_npg as A
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    from mjrl_amd.algos.model_accel import sampling as S
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils import ingest

    n, m, K = 6, 2, 2
    spec = types.SimpleNamespace(observation_dim=n, action_dim=m, horizon=8)

    class Env:
        horizon, observation_dim, action_dim = spec.horizon, n, m

        def __init__(self):
            self.spec = spec

        def reset(self):
            return np.zeros(n)

        def set_seed(self, seed=None):
            pass

    def reward_function(paths):
        paths["rewards"] = -np.sum(paths["observations"] ** 2, -1) - 0.1 * np.sum(paths["actions"] ** 2, -1)
        return paths

    models = [D.WorldModel(n, m, hidden_size=(256, 256), seed=50 + k) for k in range(K)]
    pol = MLP(spec, hidden_sizes=(32, 32), seed=3, init_log_std=-0.5)
    rng = np.random.RandomState(12)
    py = {}
    # rollout_models_device against a direct entry call on the same device blocks
    N, H = 33, 5
    s0, noise = rng.randn(N, n).astype(np.float32), rng.randn(K, H, N, m).astype(np.float32)
    pk = D.pack_dynamics_members(models, dev)
    info = {}
    obs_d, act_d = S.rollout_models_device(models, pol, s0, H, noise, packed=pk, info=info)
    torch.cuda.synchronize()
    ps = (n,) + tuple(pol.hidden_sizes) + (m,)
    c = dict(K=K, N=N, H=H, n=n, m=m, pol_sizes=ps, dyn_sizes=tuple(pk["sizes"]), act=pk["act"], flags=pk["flags"], s0=s0, noise=noise)
    bnd = S.rollout_bounds(n, m, dev)
    d = dict(P=pk["P"], tr=pk["tr"], pP=up(pol.get_param_values()), ptr=up(pol.model.packed_transforms()), b=bnd)
    o, a, r = rollout(c, d=d)
    py["device"] = [info["route"], r, bits(obs_d.cpu().numpy(), o) and bits(act_d.cpu().numpy(), a)]
    # get_refined_action with a host reward_function
    agent = A.ModelAccelNPG(learned_model=models, env=Env(), policy=pol, baseline=LinearBaseline(spec), normalized_step_size=0.05, seed=1,
                            refine=True, kappa=2.0, plan_horizon=5, plan_paths=33, reward_function=reward_function)
    before = agent.refine_route()
    act = agent.get_refined_action(rng.randn(n))
    py["refine"] = [before, agent.refine_route(), bool(np.all(np.isfinite(act[0])))]
    # one resident train_step without truncation: the paths are the rollout's rows
    N, H = 40, 8
    init = [x for x in rng.randn(N, n)]
    torch.manual_seed(77)
    noise = S.draw_rollout_noise(K, H, N, m)
    obs_d, act_d = S.rollout_models_device(models, pol, np.array(init), H, noise, large_value=A.TRAIN_LARGE_VALUE)
    want_o, want_a = obs_d.cpu().numpy(), act_d.cpu().numpy()
    got, tfp0 = [], agent.train_from_paths

    def train_from_paths(paths):
        got.extend((np.array(p["observations"]), np.array(p["actions"])) for p in paths)
        return tfp0(paths)

    agent.train_from_paths = train_from_paths
    torch.manual_seed(77)
    agent.train_step(N, env=Env(), init_states=init, horizon=H, resident=True)
    tinfo = agent.train_step_info()
    py["train"] = [tinfo["resident"], tinfo["routes"]["rollout"], len(got), sorted(set(len(g[0]) for g in got)),
                   all(bits(g[0].astype(np.float32), want_o.reshape(K * N, H, n)[i]) and bits(g[1].astype(np.float32), want_a.reshape(K * N, H, m)[i])
                       for i, g in enumerate(got)) and got[0][0].dtype == np.float32]
    ingest.drop_shared_batch()
    res["python"] = py


def main():
    res = {}
    kernel_checks(res)
    python_checks(res)
    emit(res)


if __name__ == "__main__":
    main()
