"""Host time of one call of the trainer entries (the enqueue alone: a synchronise follows each call, outside the clock; 300 calls
of a three-minibatch fit per route), and of the host permutation draw that makes up most of MLPBaseline.fit_async's time on its
caller (1M rows x 2 epochs, 12 draws).  MJX_LIB selects the build; run once per build in alternation.  Prints one line, "MICRO " +
JSON: per entry [lower quartile, median, upper quartile] in microseconds.
    python tools/bench_fit_enqueue.py"""
import ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from mjrl_amd._lib import check, load, ptr
from tests import _worker_dev as W
from tests._dyn_check import rand_theta, rand_tr
lib = load(); dev = W.device()
up = lambda x, dt=np.float32: W.up(x, dt, keep=True)
res = {}
def clock(name, call, reps=300):
    for _ in range(20): call(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter_ns(); call(); ts.append(time.perf_counter_ns() - t0); torch.cuda.synchronize()
    ts.sort(); res[name] = [round(ts[len(ts) // 4] / 1e3, 2), round(ts[len(ts) // 2] / 1e3, 2), round(ts[3 * len(ts) // 4] / 1e3, 2)]
HID = W.ints((128, 128)); st = W.stream()
for name, d_in, batch in (("mlp_fit_onepass_d21", 21, 64), ("mlp_fit_halves_d43", 43, 64), ("mlp_fit_wide_d56", 56, 64), ("mlp_fit_team_d21_b256", 21, 256), ("mlp_fit_launches_d21_b96", 21, 96)):
    rng = np.random.RandomState(1); N = 3 * batch
    th = up(rand_theta(rng, [d_in, 128, 128, 1])); m, v = torch.zeros_like(th), torch.zeros_like(th)
    x, y, perm, loss = up(rng.randn(N, d_in)), up(rng.randn(N)), up(rng.permutation(N), np.int32), up(np.zeros(1), np.float64)
    clock(name, lambda: check(lib.mjx_mlp_fit_adam(ptr(x), ptr(y), N, d_in, HID, 2, ptr(th), ptr(m), ptr(v), 0, ptr(perm), 1, batch, 1e-4, 0.0, ptr(loss), st)))
    if batch == 64:
        out = torch.zeros(N, device=dev)
        clock(name.replace("fit", "predict"), lambda: check(lib.mjx_mlp_predict(ptr(x), N, d_in, HID, 2, ptr(th), ptr(out), st)))
sizes, B, steps, K, N = [7, 64, 64, 5], 32, 2, 4, 200
rng = np.random.RandomState(7)
P = up(rand_theta(rng, sizes, K=K)); m, v = torch.zeros_like(P), torch.zeros_like(P)
trs = np.stack([rand_tr(rng, 7, 5) for _ in range(K)]); ti, to = up(trs[:, :14]), up(trs[:, 14:])
xs, ys, idx = up(rng.randn(K, N, 7)), up(rng.randn(K, N, 5)), up(rng.randint(0, N, size=(K, steps * B)), np.int32)
loss = torch.zeros(K, steps, device=dev); s0 = (ctypes.c_int64 * K)(); route = ctypes.c_int(0)
for env in ("0", "1"):
    os.environ["MJX_DYN_FIT_ENS"] = env
    clock("dyn_fit_ensemble_route" + env, lambda: check(lib.mjx_dyn_fit_ensemble(ptr(xs), N * 7, ptr(ys), N * 5, N, K, W.ints(sizes), 4, ptr(ti), ptr(to), 1, 1, ptr(P), ptr(m), ptr(v), s0,
                                                                                 ptr(idx), steps, B, 1e-4, 0.0, ptr(loss), ctypes.byref(route), st)))
del os.environ["MJX_DYN_FIT_ENS"]
clock("dyn_fit_ensemble_team_route2", lambda: check(lib.mjx_dyn_fit_ensemble_team(ptr(xs), N * 7, ptr(ys), N * 5, N, K, W.ints(sizes), 4, ptr(ti), ptr(to), 1, 1, ptr(P), ptr(m), ptr(v), s0,
                                                                                  ptr(idx), steps, B, 1e-4, 0.0, ptr(loss), ctypes.byref(route), st)))
assert route.value == 2, route.value
rsizes = [7, 100, 100, 1]
rP = up(rand_theta(rng, rsizes, K=K)); rm, rv = torch.zeros_like(rP), torch.zeros_like(rP)
rtrs = np.stack([rand_tr(rng, 7, 1) for _ in range(K)]); rti, rto, rys = up(rtrs[:, :14]), up(rtrs[:, 14:]), up(rng.randn(K, N, 1))
clock("reward_fit_ensemble_route1", lambda: check(lib.mjx_reward_fit_ensemble(ptr(xs), N * 7, ptr(rys), N, N, K, W.ints(rsizes), 4, ptr(rti), ptr(rto), 1, ptr(rP), ptr(rm), ptr(rv), s0,
                                                                              ptr(idx), steps, B, 1e-4, 0.0, ptr(loss), ctypes.byref(route), st)))
assert route.value == 1, route.value
n, ep = 1000000, 2
out = np.empty(n * ep, np.int32); rs = np.random.RandomState(0).get_state(); ts = []
for r in range(14):
    key = np.ascontiguousarray(rs[1], dtype=np.uint32).copy(); pos = ctypes.c_int32(int(rs[2]))
    t0 = time.perf_counter_ns(); check(lib.mjx_host_mt19937_permutations(ctypes.c_void_p(key.ctypes.data), ctypes.byref(pos), n, ep, ctypes.c_void_p(out.ctypes.data))); ts.append(time.perf_counter_ns() - t0)
ts = sorted(ts[2:]); res["host_permutations_1M_x2"] = [round(ts[3] / 1e3, 1), round(ts[6] / 1e3, 1), round(ts[9] / 1e3, 1)]
print("MICRO " + json.dumps(res), flush=True)
