"""GPU worker for tests/test_gpu_fit_team.py: the team trainer of the MLP baseline (csrc/mlp_fit_team.h, minibatches of 128 .. 512
rows) in ONE fresh process against the fp64 oracle (tests/_fit_oracle.py); prints one RESULT JSON line of measured errors, counts
and routes.  Run under MJX_FIT_TEAM=0 the same cases measure the launch route (the yardstick of the bars).
python tests/_fit_team_worker.py"""
import ctypes
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _fit_oracle as F  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._fit_cases import LR, rand_theta  # noqa: E402

TAIL, SENTINEL, HID, TEAM = 64, -7.0, (128, 128), 4
# (d_in, B, seed): G 2 / NF1 1; G 3, last NF1 = 1 width; G 5, first NF1 = 2 width; G 8, last width that fits LDS; the driver's batch
CASES = [(9, 128, 7001), (31, 192, 7002), (32, 320, 7003), (55, 512, 7004), (24, 256, 7005)]

lib = load()
up = functools.partial(W.up, keep=True)
ERR, CNT, ROUTES = {}, {"route_mismatch": 0, "guard_bad": 0, "not_bitwise": 0}, {}


def put(key, val, case):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]


def worst(key, errs, case):
    e, block, index = F.worst(errs)
    put(key, e, "%s %s[%d]" % (case, block, index))


def route(d_in, B, N, epochs, case):
    out = (ctypes.c_int32 * 6)()
    check(lib.mjx_mlp_fit_route(d_in, W.ints(HID), 2, B, N, epochs, out))
    ROUTES[case] = list(out)[:4]
    CNT["route_mismatch"] += ROUTES[case] != [TEAM, 1 if d_in <= 31 else 2, 1, B // 64]


def gpu_fit(theta, d_in, B, x, y, N, perm, epochs, wd, m=None, v=None, step0=0):
    """-> params, m, v (each with its NaN tail checked), losses (the sentinel behind them checked)"""
    P = theta.size
    guarded = lambda a: up(np.concatenate([np.asarray(a, np.float32), np.full(TAIL, np.nan, np.float32)]))
    bufs = [guarded(theta), guarded(np.zeros(P) if m is None else m), guarded(np.zeros(P) if v is None else v),
            up(np.concatenate([np.full(epochs, np.nan), [SENTINEL]]), np.float64)]
    check(lib.mjx_mlp_fit_adam(ptr(up(x[:N])), ptr(up(y[:N])), N, d_in, W.ints(HID), 2, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), step0,
                               ptr(up(perm, np.int32)), epochs, B, LR, wd, ptr(bufs[3]), None))
    torch.cuda.synchronize()
    out = [t.cpu().numpy() for t in bufs]
    CNT["guard_bad"] += sum(not F.tail_intact(a, P) for a in out[:3]) + (out[3][epochs] != SENTINEL) + (not np.all(np.isfinite(out[3][:epochs])))
    return [a[:P] for a in out[:3]] + [out[3][:epochs]]


def data(d_in, B, seed):
    """y = 1 + N(0, 1): zero-mean targets let the first minibatch's residuals cancel at these batch sizes (an ill-conditioned b3)"""
    rng, N = np.random.RandomState(seed), 6 * B + 37
    th = rand_theta(rng, F.mlp_sizes(d_in, HID))
    x, y = rng.randn(N, d_in).astype(np.float32), (1.0 + rng.randn(N)).astype(np.float32)
    return th, x, y, np.concatenate([rng.permutation(N) for _ in range(2)]), N


def compare(case, d_in, B, th, x, y, perm, N, epochs, wd):
    blocks, g1 = F.mlp_blocks(d_in, HID), np.zeros(th.size)
    rp, rm, rv, rl = F.mlp_fit(th, d_in, x[:N], y[:N], perm, N, epochs, LR, wd, HID, B, g_first=g1)
    well = g1 >= F.GRAD_FLOOR
    put("ill_share", np.mean(~well), case)
    route(d_in, B, N, epochs, case)
    p, m, v, l = gpu_fit(th, d_in, B, x, y, N, perm, epochs, wd)
    worst("params_over_lr", F.param_errors(p, rp, blocks, LR, well), case)
    worst("m", F.moment_errors(m, rm, blocks), case)
    worst("v", F.moment_errors(v, rv, blocks), case)
    if epochs == 1:
        worst("v_bias", F.moment_bias(v, rv, blocks), case)
    put("loss", F.rel_losses(l, rl), case)


for d_in, B, seed in CASES:
    th, x, y, perm, N = data(d_in, B, seed)
    for wd in (1e-3, 0.0) if (d_in, B) == (24, 256) else (1e-3,):
        name = "(%d, %d) wd %g" % (d_in, B, wd)
        compare(name + " 1 step", d_in, B, th, x, y, np.argsort(perm[:2 * B]), 2 * B, 1, wd)      # (a permutation of 2 B rows: the single-step fit)
        compare(name + " 2 epochs", d_in, B, th, x, y, perm, N, 2, wd)

# continuation at the driver's batch: epochs = 1, then the second permutation with the moments carried and step0 + 5 -- the bits of
# one epochs = 2 call; the same call again gives the same bits (no dependence on workgroup timing)
d_in, B, seed = CASES[-1]
th, x, y, perm, N = data(d_in, B, seed)
for s0 in (0, 12):
    pa, ma, va, la = gpu_fit(th, d_in, B, x, y, N, perm[:N], 1, 1e-3, step0=s0)
    pb, mb, vb, lb = gpu_fit(pa, d_in, B, x, y, N, perm[N:], 1, 1e-3, ma, va, step0=s0 + 5)
    two = [gpu_fit(th, d_in, B, x, y, N, perm, 2, 1e-3, step0=s0) for _ in range(2)]
    for got in two:
        CNT["not_bitwise"] += int(sum(np.sum(a != b) for a, b in zip((pb, mb, vb), got[:3])) + (la[0] != got[3][0]) + (lb[0] != got[3][1]))

# the public interface: MLPBaseline(batch_size=256) on four synthetic 200-row paths against the oracle chain on its own features
from mjrl_amd.baselines._features import DeviceBlock  # noqa: E402
from mjrl_amd.baselines.mlp_baseline import MLPBaseline  # noqa: E402

Spec = type("Spec", (), {"observation_dim": 20, "action_dim": 6, "horizon": 200})
s = 7006
rng = np.random.RandomState(s)
paths = [{"observations": rng.randn(200, 20), "rewards": np.zeros(200), "returns": 1.0 + rng.randn(200)} for _ in range(4)]
bl = MLPBaseline(Spec, batch_size=256, epochs=1, reg_coef=1e-3)
th0 = bl.params.copy()
feat = DeviceBlock(paths, "obs", shared=False).mlp_features().cpu().numpy()
yb = np.concatenate([p["returns"] for p in paths]).astype(np.float32)
np.random.seed(s)
bl.fit(paths)
g1 = np.zeros(th0.size)
ref = F.mlp_fit(th0, 24, feat, yb, np.random.RandomState(s).permutation(800), 800, 1, LR, 1e-3, HID, 256, g_first=g1)[0]
route(24, 256, 800, 1, "MLPBaseline")
worst("params_over_lr", F.param_errors(bl.params, ref, F.mlp_blocks(24, HID), LR, g1 >= F.GRAD_FLOOR), "MLPBaseline(batch_size=256)")
CNT["baseline_steps"] = int(bl.adam_steps)

W.emit({"err": ERR, "count": {k: int(n) for k, n in CNT.items()}, "routes": ROUTES})
