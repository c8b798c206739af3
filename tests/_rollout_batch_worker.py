"""GPU worker for tests/test_gpu_rollout_batch.py: every case of tests/_rollout_batch_cases.py through mjx_rollout_disagreement on both
routes and through mjx_rollout_pack, in ONE fresh process; prints one JSON line of what it measured (the test module holds the bars).
python tests/_rollout_batch_worker.py"""
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _rollout_batch_cases as B  # noqa: E402
from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import emit, ints, stream, switch  # noqa: E402

R = dict(dis={}, pack={})
dev = W.device()
lib = load()
SWITCH = "MJX_ROLLOUT_DISAGREE_MFMA"
up = functools.partial(W.up, dtype=None, keep=True)          # in its own dtype; every uploaded block stays alive until the process ends


def disagreement(mem, obs, act, forced0, P=None, H=None):
    """-> (err block of P (H - 1) + GUARD floats, NaN where nothing was written; the route reported)"""
    P = obs.shape[0] if P is None else P
    H = obs.shape[1] if H is None else H
    K, ds = len(mem["thetas"]), mem["sizes"]
    out = up(np.full(max(P * (H - 1), 0) + B.GUARD, np.nan, np.float32))
    route = ctypes.c_int(-1)
    with switch(SWITCH, "0" if forced0 else None):
        check(lib.mjx_rollout_disagreement(ptr(up(obs)), ptr(up(act)), P, H, K, ints(ds), len(ds), ptr(up(np.stack(mem["thetas"]))),
                                           ptr(up(np.stack(mem["trs"]))), mem["act"], mem["flags"], ptr(out), ctypes.byref(route), stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), route.value


def host_gathered(mem, obs, act):
    """mjx_dyn_forward + mjx_dyn_pred_error on host-gathered rows, as truncation_points runs them -> err (P (H - 1))"""
    P, H, n = obs.shape
    K, ds, rows = len(mem["thetas"]), mem["sizes"], P * (H - 1)
    x = up(np.concatenate([obs[:, :-1].reshape(rows, n), act[:, :-1].reshape(rows, -1)], -1))
    pred = torch.empty((K, rows, n), dtype=torch.float32, device=dev)
    check(lib.mjx_dyn_forward(ptr(x), 0, rows, K, ints(ds), len(ds), ptr(up(np.stack(mem["thetas"]))), ptr(up(np.stack(mem["trs"]))), mem["act"],
                              mem["flags"], ptr(pred), stream()))
    off = up(np.arange(P + 1, dtype=np.int64) * (H - 1))
    err, first = torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    check(lib.mjx_dyn_pred_error(ptr(pred), K, rows, n, ptr(up(obs[:, 1:].reshape(rows, n))), ptr(off), P, 1e30, ptr(err), ptr(first), stream()))
    return err.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- (1) the disagreement matrix
for case in B.dis_cases():
    mem, obs, act = B.dis_data(case)
    ref = B.oracle_err(mem, obs, act).ravel()
    rows = ref.size
    e1, r1 = disagreement(mem, obs, act, False)
    e0, r0 = disagreement(mem, obs, act, True)
    ds = mem["sizes"]
    R["dis"][B.dis_id(case)] = dict(
        err1=B.row_err(e1[:rows], ref), err0=B.row_err(e0[:rows], ref), routes=[r1, r0, lib.mjx_rollout_disagreement_route(ints(ds), len(ds))],
        guards=bool(np.isnan(e1[rows:]).all() and np.isnan(e0[rows:]).all()), differ=int(np.sum(bits(e1[:rows]) != bits(e0[:rows]))),
        host_equal=bool(np.array_equal(bits(e0[:rows]), bits(host_gathered(mem, obs, act)))), rows=rows)
    if case in B.limited():           # the truncation decisions at the case's limit are the oracle's, on both routes
        P, H = case[1], case[2]
        lim = B.fix_lim(ref.reshape(P, H - 1))
        want = B.first_violation(ref.reshape(P, H - 1), lim)
        R["dis"][B.dis_id(case)]["first"] = [bool(np.array_equal(B.first_violation(e[:rows].reshape(P, H - 1), lim), want)) for e in (e1, e0)]

# ---- (2) a NaN in the middle member's prediction (its output bias): every row is NaN on both routes
case = ("r3", 33, 6, 3)
mem, obs, act = B.dis_data(case)
bad = dict(mem, thetas=[t.copy() for t in mem["thetas"]])
bad["thetas"][1][-1] = np.nan
R["nan"] = [bool(np.isnan(disagreement(bad, obs, act, f)[0][:33 * 5]).all()) for f in (False, True)]
R["nan_clean"] = bool(not np.isnan(disagreement(mem, obs, act, False)[0][:33 * 5]).any())

# ---- (3) H = 1 and P = 0 touch nothing and report the route
e, r = disagreement(mem, obs[:, :1], act[:, :1], False)
R["h1"] = [bool(np.isnan(e).all()), r]
e, r = disagreement(mem, obs, act, True, P=0)
R["p0"] = [bool(np.isnan(e).all()), r]


# ---- (4) the pack matrix: every output exactly the emulation's, nothing at or behind row off[P]
def filled(count, dtype):
    fill = np.nan if np.dtype(dtype).kind == "f" else 113
    return up(np.full(count, fill, dtype))


def untouched(a, dtype):
    return bool(np.isnan(a).all()) if np.dtype(dtype).kind == "f" else bool((a == 113).all())


for name in B.PACK_CASES:
    c = B.pack_case(name)
    P, H, n = c["obs"].shape
    m = c["act"].shape[-1]
    emu = B.emu_pack(c["obs"], c["act"], c["rew"], c["err"], c["lim"], c["min_len"], c["truncate_reward"])
    cap = P * H + B.GUARD
    spec = dict(off=(P + 1 + B.GUARD, np.int64, 1), first=(P + B.GUARD, np.int32, 1), term=(P + B.GUARD, np.uint8, 1), obs=(cap, np.float32, n),
                act=(cap, np.float32, m), rew=(cap, np.float64, 1), obs64=(cap, np.float64, n), tpos=(cap, np.int32, 1))
    out = {k: filled(cnt * w, dt) for k, (cnt, dt, w) in spec.items()}
    opt = c["optional"]
    r32 = c["rew"].dtype == np.float32
    rew = up(c["rew"])
    check(lib.mjx_rollout_pack(ptr(up(c["obs"])), ptr(up(c["act"])), ptr(rew) if r32 else None, None if r32 else ptr(rew),
                               None if c["err"] is None else ptr(up(c["err"])), P, H, n, m, c["lim"], c["min_len"], c["truncate_reward"],
                               ptr(out["off"]), ptr(out["first"]), ptr(out["term"]), ptr(out["obs"]), ptr(out["act"]), ptr(out["rew"]),
                               ptr(out["obs64"]) if opt else None, ptr(out["tpos"]) if opt else None, stream()))
    torch.cuda.synchronize()
    res, rows = {}, emu["rows"]
    for k, (cnt, dt, w) in spec.items():
        got = out[k].cpu().numpy()
        used = dict(off=P + 1, first=P, term=P).get(k, rows) * w
        if k in ("obs64", "tpos") and not opt:
            used = 0
        want = emu[k].reshape(-1)[:used] if used else np.zeros(0, dt)
        same = np.array_equal(got[:used].view(np.uint8), np.ascontiguousarray(want, dt).view(np.uint8))
        res[k] = [bool(same), untouched(got[used:], dt)]
    res["rows"] = [rows, int(np.sum(emu["term"]))]
    R["pack"][name] = res

emit(R)
