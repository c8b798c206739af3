"""GPU worker of tests/test_gpu_rows_wide.py: every check of mjx_path_rewards_wide and mjx_rollout_disagreement_wide in one process;
prints one RESULT line (JSON).  Every output block starts as NaN with 64 NaN guard elements behind it; after a call no NaN may stay
inside (but where a test put one into the inputs) and nothing behind it may be touched (asserted here, per call).  "Route 0" is
the same _wide entry under its MJX_..._WIDE=0 switch."""
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
import _mpc_learned_oracle as L  # noqa: E402
import _rollout_batch_cases as B  # noqa: E402
import _rows_wide_cases as W  # noqa: E402
from tests._worker_dev import device, emit, ints, nan_block, same_bits as bits, switch, up  # noqa: E402

lib = _lib.load()
dev = device()
RSW = ("MJX_PATH_REWARDS_WIDE", "MJX_PATH_REWARDS_MFMA")
DSW = ("MJX_ROLLOUT_DISAGREE_WIDE", "MJX_ROLLOUT_DISAGREE_MFMA")


def unguard(buf, count, what, nan_ok=None):
    """the block behind its guard; nan_ok: a mask of the elements that may hold NaN"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[count:]).all(), what + ": the guard behind the block was touched"
    out = h[:count].copy()
    bad = np.isnan(out) if nan_ok is None else np.isnan(out) & ~nan_ok.ravel()
    assert not bad.any(), "%s: %d elements never written" % (what, int(bad.sum()))
    return out


def worse(a, b):
    return float("nan") if (a != a or b != b) else float(max(a, b))


# ---- rewards
def rew_blocks(mem):
    return dict(dP=up(np.stack(mem["dyn_thetas"])), dtr=up(np.stack(mem["dyn_trs"])), rP=up(np.stack(mem["rew_thetas"])),
                rtr=up(np.stack(mem["rew_trs"])))


def rewards(mem, d, obs, act, wide=None, mfma=None, entry="mjx_path_rewards_wide", outs="both", nan_ok=None):
    """one call -> (r32 (K, rows) or None, r64 or None, route); obs (K, rows, n), act (rows, m) shared or (K, rows, m)"""
    K, rows, n = obs.shape
    m = act.shape[-1]
    obs_d, act_d = up(obs), up(act)
    b32 = nan_block(K * rows) if outs in ("both", "r32") else None
    b64 = nan_block(K * rows, torch.float64) if outs in ("both", "r64") else None
    route = ctypes.c_int(-9)
    ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
    with switch(RSW[0], wide), switch(RSW[1], mfma):
        rc = getattr(lib, entry)(ptr(obs_d), ptr(act_d), 0 if act.ndim == 2 else rows * m, rows, K, ints(ds), len(ds), ptr(d["dP"]), ptr(d["dtr"]),
                                 mem["dact"], mem["dflags"], ints(rs), len(rs), ptr(d["rP"]), ptr(d["rtr"]), mem["ract"], ptr(b32), ptr(b64),
                                 ctypes.byref(route), None)
    _lib.check(rc)
    r32 = None if b32 is None else unguard(b32, K * rows, "r32", nan_ok).reshape(K, rows)
    r64 = None if b64 is None else unguard(b64, K * rows, "r64", nan_ok).reshape(K, rows)
    if r32 is not None and r64 is not None:
        assert bits(r64, r32.astype(np.float64)), "r64 is not r32 widened"
    return r32, r64, route.value


def reward_checks(res):
    out = dict(err={"2": {}, "0": {}}, routes={}, route_out={}, route_fn={}, switch_bits={}, differ={})
    for name in W.RORDER:
        mem, data = W.rcase(name)
        ref = W.rreference(name)
        d = rew_blocks(mem)
        ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
        out["route_fn"][name] = [lib.mjx_path_rewards_wide_route(ints(ds), len(ds), ints(rs), len(rs)),
                                 lib.mjx_path_rewards_route(ints(ds), len(ds), ints(rs), len(rs))]
        e2 = e0 = er = 0.0
        routes, same, differ = set(), True, False
        for (rows, mode), want in sorted(ref.items()):
            obs, shared, own = data[rows]
            act = shared if mode == "shared" else own
            r2, _, t2 = rewards(mem, d, obs, act)
            r0, _, t0 = rewards(mem, d, obs, act, wide="0")
            rm, _, tm = rewards(mem, d, obs, act, mfma="0")
            rn, _, tn = rewards(mem, d, obs, act, entry="mjx_path_rewards")
            routes.add((t2, t0, tm, tn))
            same = same and bits(r0, rn) and bits(rm, rn)
            differ = differ or not bits(r2, r0)
            e2, e0, er = worse(e2, B.row_err(r2, want)), worse(e0, B.row_err(r0, want)), worse(er, B.row_err(r2, r0))
            print("rewards", name, rows, mode, B.row_err(r2, want), B.row_err(r0, want), B.row_err(r2, r0), "bar", W.MARGIN * W.ryard(name), flush=True)
        out["err"]["2"][name], out["err"]["0"][name], out["routes"][name] = e2, e0, er
        out["route_out"][name] = sorted(list(r) for r in routes)
        out["switch_bits"][name], out["differ"][name] = same, differ
        if name == "r1":
            obs, shared, own = data[129]
            r2, w2, _ = rewards(mem, d, obs, own)
            rb, wb, _ = rewards(mem, d, obs, own)
            out["repeat"] = bits(r2, rb) and bits(w2, wb)
            a32, _, _ = rewards(mem, d, obs, own, outs="r32")
            _, a64, _ = rewards(mem, d, obs, own, outs="r64")
            out["alone"] = bits(a32, r2) and bits(a64, w2)
            # the masked column: s' there is exactly s (flags 7) whatever its out_shift is -- the oracle's bits and the kernel's
            col, n, m = W.masked_column(W.RCASES[name][0]), ds[-1], ds[0] - ds[-1]
            moved = dict(mem, dyn_trs=[t.copy() for t in mem["dyn_trs"]])
            for t in moved["dyn_trs"]:
                t[2 * (n + m) + col] = np.float32(-0.7)
            rmv, _, _ = rewards(moved, rew_blocks(moved), obs, own)
            out["masked"] = dict(kernel=bits(rmv, r2), oracle=bits(L.ensemble_rewards(obs, own, moved), ref[(129, "own")]))
    # a NaN in one stored row of member 1 of r4 (tanh in both nets: the library's ReLU is fmaxf, which drops a NaN): every other row's
    # bits stay, that row is NaN
    mem, data = W.rcase("r4")
    obs, shared, own = data[64]
    d = rew_blocks(mem)
    r2, _, _ = rewards(mem, d, obs, own)
    k_bad, row_bad = 1, 40
    bad = obs.copy()
    bad[k_bad, row_bad, 0] = np.nan
    ok = np.zeros(r2.shape, bool)
    ok[k_bad, row_bad] = True
    rn, _, _ = rewards(mem, d, bad, own, nan_ok=ok)
    out["nan"] = dict(others=bits(rn[~ok], r2[~ok]), row_nan=bool(np.isnan(rn[k_bad, row_bad])))
    # a shape the register-resident route serves too (_mpc_learned_oracle's k1: 64 x 64 beside 100 x 100), called directly
    mem, data = L.kernel_case("k1")
    obs, shared, own = data[(33, 5)]
    K, n, m = obs.shape[0], obs.shape[-1], own.shape[-1]
    obs, own = obs.reshape(K, -1, n), own.reshape(K, -1, m)
    d = rew_blocks(mem)
    r2, _, t2 = rewards(mem, d, obs, own)
    r0, _, t0 = rewards(mem, d, obs, own, wide="0")
    rn, _, tn = rewards(mem, d, obs, own, entry="mjx_path_rewards")
    want = L.ensemble_rewards(obs, own, mem)
    out["chained"] = dict(routes=[t2, t0, tn], bits=bits(r0, rn), rel=[L.rel_max(r2, want), L.rel_max(rn, want)])
    res["rew"] = out


# ---- disagreement
def dis_blocks(mem):
    return dict(P=up(np.stack(mem["thetas"])), tr=up(np.stack(mem["trs"])))


def disagreement(mem, d, obs, act, wide=None, mfma=None, entry="mjx_rollout_disagreement_wide", nan_ok=None):
    """one call -> (err (P, H - 1), route): the block holds P (H - 1) elements, so nothing may be stored for t = H - 1"""
    P, H, n = obs.shape
    obs_d, act_d = up(obs), up(act)
    eb = nan_block(P * (H - 1))
    route = ctypes.c_int(-9)
    ds = mem["sizes"]
    with switch(DSW[0], wide), switch(DSW[1], mfma):
        rc = getattr(lib, entry)(ptr(obs_d), ptr(act_d), P, H, len(mem["thetas"]), ints(ds), len(ds), ptr(d["P"]), ptr(d["tr"]), mem["act"],
                                 mem["flags"], ptr(eb), ctypes.byref(route), None)
    _lib.check(rc)
    return unguard(eb, P * (H - 1), "err", nan_ok).reshape(P, H - 1), route.value


def dis_checks(res):
    out = dict(err={"2": {}, "0": {}}, routes={}, route_out={}, route_fn={}, switch_bits={}, differ={}, first={})
    for case in W.dis_cases():
        cid = W.dis_id(case)
        mem, obs, act = W.dis_data(case)
        want = B.oracle_err(mem, obs, act)
        d = dis_blocks(mem)
        ds = mem["sizes"]
        out["route_fn"][cid] = [lib.mjx_rollout_disagreement_wide_route(ints(ds), len(ds)), lib.mjx_rollout_disagreement_route(ints(ds), len(ds))]
        e2, t2 = disagreement(mem, d, obs, act)
        e0, t0 = disagreement(mem, d, obs, act, wide="0")
        em, tm = disagreement(mem, d, obs, act, mfma="0")
        en, tn = disagreement(mem, d, obs, act, entry="mjx_rollout_disagreement")
        out["route_out"][cid] = [t2, t0, tm, tn]
        out["switch_bits"][cid] = bits(e0, en) and bits(em, en)
        out["differ"][cid] = not bits(e2, e0)
        out["err"]["2"][cid], out["err"]["0"][cid], out["routes"][cid] = B.row_err(e2, want), B.row_err(e0, want), B.row_err(e2, e0)
        print("disagreement", cid, out["err"]["2"][cid], out["err"]["0"][cid], out["routes"][cid], "bar", W.MARGIN * W.dyard(case), flush=True)
        if case in W.limited():
            lim = B.fix_lim(want)
            v = B.first_violation(want, lim)
            out["first"][cid] = [bool(np.array_equal(B.first_violation(e2, lim), v)), bool(np.array_equal(B.first_violation(e0, lim), v))]
        if case == ("n1", 13, 5, 3):
            eb, _ = disagreement(mem, d, obs, act)
            out["repeat"] = bits(e2, eb)
        if case == ("n2", 16, 4, 1):
            # a NaN action in stored row (6, 2) of a tanh net (the library's ReLU is fmaxf, which drops a NaN): that row's error alone
            # is NaN, every other row's bits stay
            bad = act.copy()
            bad[6, 2, 0] = np.nan
            ok = np.zeros(e2.shape, bool)
            ok[6, 2] = True
            en_, _ = disagreement(mem, d, obs, bad, nan_ok=ok)
            out["nan"] = dict(others=bits(en_[~ok], e2[~ok]), row_nan=bool(np.isnan(en_[6, 2])))
        if case == ("n2", 1, 65, 2):
            # the masked column (flags 3: s' there is exactly 0) whatever its out_shift is
            col, n, m = W.masked_column("n2"), ds[-1], ds[0] - ds[-1]
            moved = dict(mem, trs=[t.copy() for t in mem["trs"]])
            for t in moved["trs"]:
                t[2 * (n + m) + col] = np.float32(-0.7)
            ev, _ = disagreement(moved, dis_blocks(moved), obs, act)
            out["masked"] = dict(kernel=bits(ev, e2), oracle=bits(B.oracle_err(moved, obs, act), want))
    res["dis"] = out


# ---- Python, end to end
def python_checks(res):
    from mjrl_amd.algos.model_accel import model_accel_npg as A
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    from mjrl_amd.algos.model_accel import sampling as S
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    from mjrl_amd.utils import ingest

    n, m, K, N, H = 6, 2, 2, 40, 8
    spec = types.SimpleNamespace(observation_dim=n, action_dim=m, horizon=H)

    class Env:
        horizon, observation_dim, action_dim = H, n, m

        def __init__(self):
            self.spec = spec

        def reset(self):
            return np.zeros(n)

        def set_seed(self, seed=None):
            pass

    def setup():
        models = [D.WorldModel(n, m, hidden_size=(256, 256), learn_reward=True, seed=60 + k) for k in range(K)]
        pol = MLP(spec, hidden_sizes=(32, 32), seed=3, init_log_std=-0.5)
        rng = np.random.RandomState(21)
        init = rng.randn(N, n) * np.exp(rng.uniform(np.log(0.1), np.log(30.0), (N, 1)))       # (errors over decades: fix_lim finds its gap)
        return models, pol, init

    py = {}
    models, pol, init = setup()
    assert tuple(models[0].reward_net.layer_sizes) == (2 * n + m, 100, 100, 1)
    # the limit: B.fix_lim on route 0's errors of the step's own rollout
    torch.manual_seed(77)
    noise = S.draw_rollout_noise(K, H, N, m)
    obs_d, act_d = S.rollout_models_device(models, pol, init, H, noise, large_value=A.TRAIN_LARGE_VALUE)
    info = {}
    with switch(DSW[0], "0"):
        err0 = D.rollout_disagreement_device(models, obs_d, act_d, info=info, wide=True).cpu().numpy()
    lim = B.fix_lim(err0.astype(np.float64))
    py["lim_route"] = info["route"]
    # ensemble_path_rewards_device without wide=True: still the generic route's bits; with it: route 2's, within the bar of them
    plain = D.ensemble_path_rewards_device(models, obs_d, act_d).cpu().numpy()
    with switch(RSW[0], "0"):
        narrow = D.ensemble_path_rewards_device(models, obs_d, act_d, wide=True).cpu().numpy()
    with switch(RSW[1], "0"):
        generic = D.ensemble_path_rewards_device(models, obs_d, act_d).cpu().numpy()
    wide = D.ensemble_path_rewards_device(models, obs_d, act_d, wide=True).cpu().numpy()
    py["plain_is_generic"] = bits(plain, generic) and bits(plain, narrow)
    # the yardstick of this step's rewards: the package's own fp32 torch forward on the CPU against the fp64 oracle on the stored rows
    mem = dict(dyn_thetas=[D._flat_params(mdl.dynamics_net, "cpu").numpy() for mdl in models], dyn_sizes=tuple(models[0].dynamics_net.layer_sizes),
               dyn_trs=[D._packed_transforms(mdl.dynamics_net, "cpu").numpy() for mdl in models], dact=D._act_code(models[0].dynamics_net),
               dflags=D._flags(models[0].dynamics_net), rew_thetas=[D._flat_params(mdl.reward_net, "cpu").numpy() for mdl in models],
               rew_sizes=tuple(models[0].reward_net.layer_sizes), rew_trs=[L.reward_transforms(mdl.reward_net) for mdl in models],
               ract=D._act_code(models[0].reward_net))
    o_h, a_h = obs_d.cpu().numpy(), act_d.cpu().numpy()
    want = L.ensemble_rewards(o_h, a_h, mem)
    yard = B.row_err(W.torch_rewards32(mem, o_h, a_h), want)
    py["rewards"] = dict(yard=yard, wide=B.row_err(wide, want), narrow=B.row_err(plain, want), between=B.row_err(wide, plain))

    def step(off):
        models, pol, init = setup()
        agent = A.ModelAccelNPG(learned_model=models, env=Env(), policy=pol, baseline=LinearBaseline(spec), normalized_step_size=0.05, seed=1)
        got, rp0 = [], agent._resident_paths

        def resident_paths(*a, **kw):
            paths = rp0(*a, **kw)
            got.extend((len(p["rewards"]), bool(p["terminated"]), np.array(p["rewards"], np.float64)) for p in paths)
            return paths

        agent._resident_paths = resident_paths
        torch.manual_seed(77)
        with switch(RSW[0], "0" if off else None), switch(DSW[0], "0" if off else None):
            try:
                agent.train_step(N, env=Env(), init_states=[x for x in init], horizon=H, truncate_lim=lim, truncate_reward=-1.0, resident=True)
            finally:
                ingest.drop_shared_batch()
        return got, agent.train_step_info()

    gw, iw = step(False)
    gn, inn = step(True)
    py["routes"] = [iw["routes"], inn["routes"], iw["resident"], inn["resident"]]
    py["lens"] = [[g[0] for g in gw] == [g[0] for g in gn], [g[1] for g in gw] == [g[1] for g in gn], int(sum(g[1] for g in gw)), len(gw)]
    if py["lens"][0]:
        py["step_rewards"] = B.row_err(np.concatenate([g[2] for g in gw]), np.concatenate([g[2] for g in gn]))
    res["python"] = py


def main():
    res = {}
    reward_checks(res)
    dis_checks(res)
    python_checks(res)
    emit(res)


if __name__ == "__main__":
    main()
