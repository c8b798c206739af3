"""GPU worker of tests/test_gpu_plan_wide.py: every check of mjx_plan_rollout_wide in one process; prints one RESULT line (JSON).
Every output block starts as NaN with 64 NaN guard elements behind it (_worker_dev.nan_block); the records count what stayed NaN
inside and what was touched behind, and the calls outside the records go through _worker_dev.checked_block.  "Route 0" is the same
entry under MJX_PLAN_WIDE=0."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build()
from mjrl_amd import _lib  # noqa: E402
from mjrl_amd._lib import ptr  # noqa: E402
import _mpc_oracle as M  # noqa: E402
import _plan_wide_cases as C  # noqa: E402
from tests._worker_dev import checked_block, device, emit, ints, nan_block, same_bits as bits, switch, up  # noqa: E402

lib = _lib.load()
dev = device()
ROUTES = {}                  # (case, what) -> route_out of the record's calls


def call(name, mem, s0, actions, wide=None, mfma=None, entry="mjx_plan_rollout_wide"):
    """one call of `entry` under MJX_PLAN_WIDE = wide and MJX_PLAN_MFMA = mfma (None: left alone) -> (the guarded block on the host,
    route_out)"""
    c = C.CASES[name]
    K, n, m = len(mem["thetas"]), c["n"], c["m"]
    N, H = actions.shape[:2]
    ds = mem["sizes"]
    s0_d, a_d, P_d, tr_d = up(s0), up(actions), up(np.stack(mem["thetas"])), up(np.stack(mem["trs"]))
    ob = nan_block(K * N * H * n)
    route = ctypes.c_int(-9)
    args = [ptr(s0_d), n if s0.ndim == 2 else 0, N, H, K, ptr(a_d), ints(ds), len(ds), ptr(P_d), ptr(tr_d), mem["act"], mem["flags"], ptr(ob)]
    with switch("MJX_PLAN_WIDE", wide), switch("MJX_PLAN_MFMA", mfma):
        if entry == "mjx_plan_rollout_wide":
            rc = lib.mjx_plan_rollout_wide(*args, ctypes.byref(route), None)
        else:
            rc = lib.mjx_plan_rollout(*args, None)
    _lib.check(rc)
    torch.cuda.synchronize()
    return ob.cpu().numpy(), route.value


def runner(rt, name, mem, s0, actions):
    buf, route = call(name, mem, s0, actions, wide=None if rt == "2" else "0")
    ROUTES.setdefault((name, rt), set()).add(route)
    return buf


def block(buf, name, rows, nan_rows=()):
    """a guarded block of a case -> (K, rows, H, n) after the written / guard checks; nan_rows: trajectories that may hold NaN"""
    c = C.CASES[name]
    shape = (c["K"], rows, c["H"], c["n"])
    numel = int(np.prod(shape))
    if not nan_rows:
        return checked_block(torch.from_numpy(buf), numel, name).reshape(shape).copy()
    assert np.isnan(buf[numel:]).all(), name + ": the guard behind the block was touched"
    out = buf[:numel].reshape(shape).copy()
    keep = np.ones(rows, bool)
    keep[list(nan_rows)] = False
    assert not np.isnan(out[:, keep]).any(), name + ": NaN left inside the block"
    return out


def kernel_checks(res):
    res.update(rec={}, route_fn={}, route_out={}, narrow_fn={}, switch_bits={})
    for name in C.ORDER:
        c = C.CASES[name]
        mem, data = C.cached_case(name)
        ds = mem["sizes"]
        rec = C.measure(name, runner)
        rec["runs"] = rec["runs"][:8]
        res["rec"][name] = rec
        res["route_fn"][name] = lib.mjx_plan_rollout_wide_route(ints(ds), len(ds), c["m"])
        res["narrow_fn"][name] = lib.mjx_plan_route(ints(ds), len(ds), c["m"])
        # the switches: under MJX_PLAN_WIDE=0 the entry is mjx_plan_rollout bit for bit; under MJX_PLAN_MFMA=0 the route is 0
        s0, actions = data[c["s0"][-1]]
        b0, r0 = call(name, mem, s0, actions, wide="0")
        bn, _ = call(name, mem, s0, actions, entry="mjx_plan_rollout")
        _, rm = call(name, mem, s0, actions, mfma="0")
        res["switch_bits"][name] = bits(b0, bn)
        res["route_out"][name] = [sorted(ROUTES[(name, "2")]), sorted(ROUTES[(name, "0")]), r0, rm]
        print(name, rec["err"], rec["routes"], res["route_out"][name], flush=True)
        if name == "q1":
            o2 = block(call(name, mem, s0, actions)[0], name, c["rows"])
            res["repeat"] = bits(o2, block(call(name, mem, s0, actions)[0], name, c["rows"]))
            one, a1 = data["one"]
            tiled = np.ascontiguousarray(np.tile(one, (c["rows"], 1)))
            res["s0_tiled"] = bits(block(call(name, mem, one, a1)[0], name, c["rows"]), block(call(name, mem, tiled, a1)[0], name, c["rows"]))
        if name == C.NAN_CASE:
            clean = block(call(name, mem, s0, actions)[0], name, c["rows"])
            bad = s0.copy()
            bad[C.NAN_ROW] = np.nan
            dirty = block(call(name, mem, bad, actions)[0], name, c["rows"], nan_rows=(C.NAN_ROW,))
            others = np.arange(c["rows"]) != C.NAN_ROW
            res["nan"] = dict(others=bits(dirty[:, others], clean[:, others]), s0_nan=bool(np.isnan(dirty[:, C.NAN_ROW, 0]).all()))
        if name == "q8":
            res["h1_s0_exact"] = bits(block(call(name, mem, s0, actions)[0], name, c["rows"])[:, :, 0], np.stack([s0] * c["K"]))


def python_checks(res):
    """MPCPolicy on the seeded 256 x 256 members, one get_action per setting: the routes it reports and its distance from fp64"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy, perturbed_action_batch
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    import _mpc_learned_oracle as L

    P = C.MPC
    n, m, N, H = P["n"], P["m"], P["N"], P["H"]
    members = C.mpc_members(WorldModel, torch)
    py = {}
    for reward in ("learned", "env"):
        np.random.seed(P["draw"])
        actions = perturbed_action_batch(N, np.ones((H, m)) * np.zeros(m), list(P["fc"]))
        plan = C.mpc_oracle(actions, reward)
        for setting, off in (("wide", None), ("narrow", "0")):
            env = L.plan_env_no_rewards(n, m) if reward == "learned" else M.plan_env(n, m)
            pol = MPCPolicy(env=env, plan_horizon=H, plan_paths=N, kappa=P["kappa"], gamma=P["gamma"], filter_coefs=list(P["fc"]),
                            warmstart=True, fitted_model=members, omega=P["omega"], reward=reward, wide=True)
            np.random.seed(P["draw"])
            with switch("MJX_PLAN_WIDE", off), switch("MJX_PATH_REWARDS_WIDE", off):
                action = pol.get_action(C.mpc_obs())
                asked = (pol.route(), pol.reward_route())
            seq = np.concatenate([action[None], pol.act_sequence[:-1]])
            eR, eq = C.mpc_errors(pol.last_scores()[0], seq, plan)
            py["%s_%s" % (reward, setting)] = dict(route=asked[0], reward_route=asked[1], last=pol.last_routes(), R=eR, seq=eq,
                                                   ess=M.ess(plan["S"]))
            print(reward, setting, py["%s_%s" % (reward, setting)], flush=True)
    res["python"] = py


def main():
    res = {}
    kernel_checks(res)
    python_checks(res)
    emit(res)


if __name__ == "__main__":
    main()
