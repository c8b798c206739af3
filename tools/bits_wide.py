"""Every output array of the four _wide entries over the cases of tests/_rows_wide_cases.py, tests/_rollout_wide_cases.py and
tests/_plan_wide_cases.py, for comparing two builds bit by bit (a refactor's evidence; needs the GPU):
    MJX_LIB=<libmjx.so> python tools/bits_wide.py dump out.npz      one fresh process per library
    python tools/bits_wide.py compare a.npz b.npz [out.json]         array_equal on the raw bytes of every array
Each case runs through its wide entry on every route: the default, MJX_..._WIDE=0 and MJX_..._MFMA=0.  Rewards: both action modes
the case has, r32 and r64; the policy rollout: the case's noise and the other layout (shared by the members / per member) too; the
plan rollout: every start-state mode the case has."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ROUTES = (("default", None, None), ("wide0", "0", None), ("mfma0", None, "0"))


def dump(path):
    import torch
    from mjrl_amd import _lib
    from mjrl_amd._lib import ptr
    import _plan_wide_cases as Q
    import _rollout_wide_cases as R
    import _rows_wide_cases as W
    from tests._worker_dev import ints, nan_block, switch, up
    lib = _lib.load()
    out = {}

    def take(key, buf, count, route):
        torch.cuda.synchronize()
        out[key] = buf.cpu().numpy()[:count].copy()
        out[key + "/route"] = np.int32(route.value)

    for name in W.RORDER:
        mem, data = W.rcase(name)
        d = [up(np.stack(mem[k])) for k in ("dyn_thetas", "dyn_trs", "rew_thetas", "rew_trs")]
        ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
        for rows, (obs, shared, own) in sorted(data.items()):
            K, m = obs.shape[0], ds[0] - ds[-1]
            for mode, act in (("shared", shared), ("own", own)):
                if act is None:
                    continue
                obs_d, act_d = up(obs), up(act)
                for tag, wide, mfma in ROUTES:
                    b32, b64, route = nan_block(K * rows), nan_block(K * rows, torch.float64), ctypes.c_int(-9)
                    with switch("MJX_PATH_REWARDS_WIDE", wide), switch("MJX_PATH_REWARDS_MFMA", mfma):
                        _lib.check(lib.mjx_path_rewards_wide(ptr(obs_d), ptr(act_d), 0 if act.ndim == 2 else rows * m, rows, K, ints(ds), len(ds),
                                                             ptr(d[0]), ptr(d[1]), mem["dact"], mem["dflags"], ints(rs), len(rs), ptr(d[2]), ptr(d[3]),
                                                             mem["ract"], ptr(b32), ptr(b64), ctypes.byref(route), None))
                    key = "rewards/%s/%d/%s/%s" % (name, rows, mode, tag)
                    take(key + "/r32", b32, K * rows, route)
                    take(key + "/r64", b64, K * rows, route)
    for case in W.dis_cases():
        mem, obs, act = W.dis_data(case)
        P, H, _ = obs.shape
        d = [up(np.stack(mem[k])) for k in ("thetas", "trs")]
        ds, obs_d, act_d = mem["sizes"], up(obs), up(act)
        for tag, wide, mfma in ROUTES:
            eb, route = nan_block(P * (H - 1)), ctypes.c_int(-9)
            with switch("MJX_ROLLOUT_DISAGREE_WIDE", wide), switch("MJX_ROLLOUT_DISAGREE_MFMA", mfma):
                _lib.check(lib.mjx_rollout_disagreement_wide(ptr(obs_d), ptr(act_d), P, H, len(mem["thetas"]), ints(ds), len(ds), ptr(d[0]), ptr(d[1]),
                                                             mem["act"], mem["flags"], ptr(eb), ctypes.byref(route), None))
            take("disagree/%s/%s/err" % (W.dis_id(case), tag), eb, P * (H - 1), route)
    for name in sorted(R.WCASES):
        c = R.wide_case(name)
        K, N, H, n, m = c["K"], c["N"], c["H"], c["n"], c["m"]
        other = np.random.RandomState(9100 + sorted(R.WCASES).index(name)).randn(K, H, N, m).astype(np.float32)
        noises = {"case": c["noise"], "shared": other[0], "member": other}
        d = [up(np.stack(c["dyn_thetas"])), up(np.stack(c["dyn_trs"])), up(c["pol_theta"]), up(c["pol_tr"])]
        b = [None] * 4 if c["bounds"] is None else [up(v) for v in c["bounds"]]
        s0_d = up(c["s0"])
        for nzname, nz in sorted(noises.items()):
            nz_d = up(nz)
            for tag, wide, mfma in ROUTES:
                ob, ab, route = nan_block(K * N * H * n), nan_block(K * N * H * m), ctypes.c_int(-9)
                with switch("MJX_POLICY_ROLLOUT_WIDE", wide), switch("MJX_POLICY_ROLLOUT_MFMA", mfma):
                    _lib.check(lib.mjx_policy_rollout_wide(ptr(s0_d), n if c["s0"].ndim == 2 else 0, N, H, K, ints(c["pol_sizes"]), len(c["pol_sizes"]),
                                                           ptr(d[2]), ptr(d[3]), ptr(nz_d), H * N * m if (nz is not None and nz.ndim == 4) else 0,
                                                           ints(c["dyn_sizes"]), len(c["dyn_sizes"]), ptr(d[0]), ptr(d[1]), c["act"], c["flags"],
                                                           ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), ptr(ob), ptr(ab), ctypes.byref(route), None))
                key = "rollout/%s/noise_%s/%s" % (name, nzname, tag)
                take(key + "/obs", ob, K * N * H * n, route)
                take(key + "/act", ab, K * N * H * m, route)
    for name in Q.ORDER:
        mem, data = Q.cached_case(name)
        c, ds = Q.CASES[name], mem["sizes"]
        K, N, H, n = c["K"], c["rows"], c["H"], c["n"]
        d = [up(np.stack(mem[k])) for k in ("thetas", "trs")]
        for mode, (s0, actions) in sorted(data.items()):
            s0_d, act_d = up(s0), up(actions)
            for tag, wide, mfma in ROUTES:
                ob, route = nan_block(K * N * H * n), ctypes.c_int(-9)
                with switch("MJX_PLAN_WIDE", wide), switch("MJX_PLAN_MFMA", mfma):
                    _lib.check(lib.mjx_plan_rollout_wide(ptr(s0_d), n if s0.ndim == 2 else 0, N, H, K, ptr(act_d), ints(ds), len(ds), ptr(d[0]),
                                                         ptr(d[1]), mem["act"], mem["flags"], ptr(ob), ctypes.byref(route), None))
                take("plan/%s/s0_%s/%s/obs" % (name, mode, tag), ob, K * N * H * n, route)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print("dumped", len(out) // 2, "arrays from", _lib.LIB_PATH)


def compare(pa, pb, out_json=None):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    arrays = [k for k in a.files if not k.endswith("/route")]
    differ = [k for k in a.files if not (a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes())]
    routes = {}
    for k in arrays:
        op, tag = k.split("/")[0], k.split("/")[-2]
        routes.setdefault(op + " " + tag, set()).add(int(a[k + "/route"]))
    res = dict(cases=len({k.rsplit("/", 1)[0] for k in arrays}), arrays=len(arrays), elements=int(sum(a[k].size for k in arrays)),
               nan_left=int(sum(int(np.isnan(a[k]).sum()) for k in arrays)), differ=differ, identical=not differ,
               routes_taken={k: sorted(v) for k, v in sorted(routes.items())})
    print(json.dumps(res, indent=1))
    if out_json:
        json.dump(res, open(out_json, "w"), indent=1)
    return 0 if not differ else 1


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(*sys.argv[2:]))
