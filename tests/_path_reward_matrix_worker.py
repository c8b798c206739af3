"""GPU worker for tests/test_gpu_path_reward_matrix.py: every case of tests/_path_reward_cases.py through mjx_path_rewards on both
routes in ONE fresh process; prints one JSON line of measurements (the test module compares them with its bars).
python tests/_path_reward_matrix_worker.py"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _path_reward_cases as C  # noqa: E402
from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import emit, ints, stream, switch  # noqa: E402

T0 = time.time()
dev = W.device()
lib = load()
SWITCH = "MJX_PATH_REWARDS_MFMA"
CUS = int(torch.cuda.get_device_properties(0).multi_processor_count)
_UP, LAST = {}, {}
assert C.GUARD == W.GUARD


def up(x):
    """one upload per host array (the arrays of a case stay alive in _path_reward_cases' cache, and the device copies here)"""
    if id(x) not in _UP:
        _UP[id(x)] = (x, W.up(x))
    return _UP[id(x)][1]


def members(name, mem):
    key = "members " + name
    if key not in _UP:
        _UP[key] = tuple(torch.as_tensor(np.stack(mem[f])).to(dev) for f in ("dyn_thetas", "dyn_trs", "rew_thetas", "rew_trs"))
    return _UP[key]


def run(route, name, mem, obs, act):
    """mjx_path_rewards into NaN-prefilled blocks of K x rows + GUARD elements -> (r32 block, r64 block, route taken)"""
    K, rows, n = obs.shape
    m = act.shape[-1]
    dP, dtr, rP, rtr = members(name, mem)
    ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
    r32, r64 = W.nan_block(K * rows), W.nan_block(K * rows, torch.float64)
    taken = ctypes.c_int(-1)
    with switch(SWITCH, route):
        check(lib.mjx_path_rewards(ptr(up(obs)), ptr(up(act)), 0 if act.ndim == 2 else rows * m, rows, K, ints(ds), len(ds), ptr(dP), ptr(dtr),
                                   mem["dact"], mem["dflags"], ints(rs), len(rs), ptr(rP), ptr(rtr), mem["ract"], ptr(r32), ptr(r64),
                                   ctypes.byref(taken), stream()))
    torch.cuda.synchronize()
    LAST[(name, route)] = r32
    return r32.cpu().numpy(), r64.cpu().numpy(), taken.value


R = dict(cus=CUS, cases={}, served={})
for name in C.ORDER:
    ds, rs = C.sizes(name)
    R["served"][name] = lib.mjx_path_rewards_route(ints(ds), len(ds), ints(rs), len(rs))
    rec = C.measure(name, run, CUS)
    print("\n".join(rec.pop("runs")), flush=True)
    print("%s routes against each other %.3e  unwritten %d guard %d  walk (grid, most, fewest, rows of the last tile) %s  [%.1f s]"
          % (name, rec["routes"], rec["unwritten"], rec["guard"], rec["walk"], time.time() - T0), flush=True)
    R["cases"][name] = rec

# ---- g3: route 0's fp32 output is two mjx_dyn_forward calls over [s, a] and [s, a, s'] rows assembled by torch, bit for bit
name = "g3"
c = C.CASES[name]
mem, data = C.cached_case(name)
rows = c["rows"][0]
obs, shared, own = data[rows]
K, n, m = c["K"], c["n"], c["m"]
ds, rs = C.sizes(name)
dP, dtr, rP, rtr = members(name, mem)
X1 = torch.cat([up(obs), up(shared)[None].expand(K, rows, m)], 2).contiguous()
sp = torch.full((K, rows, n), float("nan"), device=dev)
check(lib.mjx_dyn_forward(ptr(X1), rows * (n + m), rows, K, ints(ds), len(ds), ptr(dP), ptr(dtr), mem["dact"], mem["dflags"], ptr(sp), stream()))
X2 = torch.cat([X1, sp], 2).contiguous()
two = torch.full((K * rows,), float("nan"), device=dev)
check(lib.mjx_dyn_forward(ptr(X2), rows * (2 * n + m), rows, K, ints(rs), len(rs), ptr(rP), ptr(rtr), mem["ract"], C.AFF, ptr(two), stream()))
torch.cuda.synchronize()
R["g3_two_forwards_same_bits"] = bool(torch.equal(two.view(torch.int32), LAST[(name, 0)][:K * rows].view(torch.int32)))
R["seconds"] = time.time() - T0
print("g3 against two mjx_dyn_forward calls: same bits %s; %d CUs; %.1f s in all" % (R["g3_two_forwards_same_bits"], CUS, R["seconds"]), flush=True)
emit(R)
