"""GPU worker for tests/test_gpu_ridge_matrix.py: every case of mjx_bl_gram, mjx_bl_predict and mjx_bl_features_f32 in ONE fresh
process against the long-double references of tests/_ridge_cases.py; prints one RESULT JSON line of measured ratios, counts and
routes (the test module compares them with its bars).  Every ctypes call that must succeed goes through check(): the first HIP
error ends the process.  The device calls run on the main thread, one after the other; the long-double references, which take
longer than all of them, are formed by a few host threads beside them and judged at the end, in case order.
python tests/_ridge_matrix_worker.py"""
import ctypes
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _ridge_cases as K  # noqa: E402
from tests import _worker_dev as W  # noqa: E402

assert np.finfo(np.longdouble).nmant >= 63, "the references need a long double wider than fp64"
SENTINEL = -7.25              # fills an output that a refused call must leave alone
TAIL = 64                     # NaNs behind every output

lib = load()
ERR, ROUTES, CASES = {}, {}, {}
CNT = {k: 0 for k in ("route_mismatch", "gram_not_symmetric", "gram_not_finite", "gram_tail_touched", "gram_refusal_bad",
                      "predict_not_finite", "predict_tail_touched", "predict_refusal_bad", "feat_obs_bad", "feat_time_bad",
                      "feat_exact_bad", "feat_tail_touched")}


POOL, JOBS = ThreadPoolExecutor(8), []   # (NumPy's long-double loops release the interpreter lock)


def later(fn, *args):
    """fn(*args) on a host thread; fn returns a list of ("put", key, value, case) / ("count", key, n), applied at the end"""
    JOBS.append(POOL.submit(fn, *args))


def put(key, val, case):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]
    CASES.setdefault(key, {})[case] = float(val)


def count(key, n):
    CNT[key] += int(n)


def up(a, dtype=np.float64):
    return W.up(a, dtype)


def out_buf(entries, dtype=np.float64, fill=np.nan):
    return up(np.concatenate([np.full(entries, fill), np.full(TAIL, np.nan)]), dtype)


def tail_intact(a, entries):
    return a.size == entries + TAIL and bool(np.all(np.isnan(a[entries:])))


def set_env(env):
    os.environ.pop("MJX_GRAM_FMA", None)
    os.environ.update(env)


def gram_route(kind, n, N):
    out = (ctypes.c_int32 * 6)()
    check(lib.mjx_bl_gram_route(kind, n, N, out))
    return [int(x) for x in out]


def gpu_gram(kind, n, obs, tpos, y):
    N, FA = len(y), K.num_features(kind, n) + 1
    G = out_buf(FA * FA)
    o, t, yy = up(obs), up(tpos, np.int32), up(y)
    check(lib.mjx_bl_gram(kind, ptr(o), ptr(t), ptr(yy), N, n, ptr(G), None))
    torch.cuda.synchronize()
    g = G.cpu().numpy()
    count("gram_tail_touched", not tail_intact(g, FA * FA))
    return g[:FA * FA].reshape(FA, FA)


def judge_gram(case, arm, kind, n, N, obs, tpos, y, G):
    R, B, b = K.gram_reference(kind, n, obs, tpos, y)
    res = K.gram_check(G, R, B, N, b, K.TILE[arm])
    return [("put", "gram_" + ("mfma", "blk", "fma")[arm], res["ratio"], "%s tile %s at %s" % (case, res["tile"], res["at"])),
            ("count", "gram_not_symmetric", not res["symmetric"]), ("count", "gram_not_finite", not res["finite"])]


def judge_predict(case, kind, n, N, obs, tpos, coef, out):
    ref, S = K.predict_reference(kind, n, obs, tpos, coef)
    res = K.predict_check(out, ref, S, K.num_features(kind, n))
    return [("put", "predict", res["ratio"], "%s row %d" % (case, res["row"])), ("count", "predict_not_finite", not res["finite"])]


def judge_features(case, n, obs, tpos, out):
    res = K.features_check(out, obs, tpos, n)
    return [("put", "feat_time_ulps", res["time_ulps"], case), ("count", "feat_obs_bad", res["obs_bad"]),
            ("count", "feat_time_bad", res["time_bad"]), ("count", "feat_exact_bad", res["exact_bad"])]


# ================================================================ 1. Gram
for arm, kind, n, N, env, Z, yscale in K.GRAM_CASES:
    case = K.case_name(arm, kind, n, N, env)
    set_env(env)
    r = gram_route(kind, n, N)
    want = K.route_expect(kind, n, N, bool(env))
    ROUTES[case] = "%s Z %d" % (K.ARMS[r[0]], r[1])
    if r[0] != arm or r[1] != want[1] or (Z is not None and r[1] != Z) or r[4] != K.TILE[arm]:
        count("route_mismatch", 1)
        ROUTES[case] += " (expected %s Z %s)" % (K.ARMS[arm], want[1] if Z is None else Z)
    seed = K.case_seed(kind, n, N)
    if arm == K.BLK:
        # this arm's partial-sum block is not cleared between calls: first a call of the same shape (as many partials, as large)
        # with other inputs and y scaled by 1e6 -- a partial the case does not rewrite then shows up in the y row and column
        o2, t2, y2 = K.make_inputs(n, N, seed + 1, yscale * 1e6)
        gpu_gram(kind, n, o2, t2, y2)
    obs, tpos, y = K.make_inputs(n, N, seed, yscale)
    G = gpu_gram(kind, n, obs, tpos, y)
    set_env({})
    later(judge_gram, case, arm, kind, n, N, obs, tpos, y, G)

# refused: 127 observations need more than 64 KiB of LDS on the only arm that would serve them; N = 0
for kind, n, N, want_rc in ((1, 127, 33, K.ERR_UNSUPPORTED), (1, 5, 0, K.ERR_ARG)):
    FA = K.num_features(kind, n) + 1
    obs, tpos, y = K.make_inputs(n, max(N, 1), 1)
    G = out_buf(FA * FA, fill=SENTINEL)
    o, t, yy = up(obs), up(tpos, np.int32), up(y)
    rc = lib.mjx_bl_gram(kind, ptr(o), ptr(t), ptr(yy), N, n, ptr(G), None)
    torch.cuda.synchronize()
    g = G.cpu().numpy()
    count("gram_refusal_bad", (rc != want_rc) + (not np.all(g[:FA * FA] == SENTINEL)) + (not tail_intact(g, FA * FA)))
    ROUTES["refused kind %d n %d N %d" % (kind, n, N)] = "rc %d" % rc

# ================================================================ 2. predict
for kind, n, N in K.PREDICT_CASES:
    case = "predict kind %d n %d N %d" % (kind, n, N)
    obs, tpos, _ = K.make_inputs(n, N, K.case_seed(kind, n, N) + 5)
    coef = K.make_coef(kind, n, 9000 + 10 * n + kind)
    out = out_buf(N)
    o, t, c = up(obs), up(tpos, np.int32), up(coef)
    check(lib.mjx_bl_predict(kind, ptr(o), ptr(t), N, n, ptr(c), ptr(out), None))
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    count("predict_tail_touched", not tail_intact(a, N))
    later(judge_predict, case, kind, n, N, obs, tpos, coef, a[:N])

for kind in (1, 2):                                          # 129 observations: 64 rows of them exceed 64 KiB of LDS
    n, N = 129, 65
    obs, tpos, _ = K.make_inputs(n, N, 3)
    out = out_buf(N, fill=SENTINEL)
    o, t, c = up(obs), up(tpos, np.int32), up(K.make_coef(kind, n, 4))
    rc = lib.mjx_bl_predict(kind, ptr(o), ptr(t), N, n, ptr(c), ptr(out), None)
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    count("predict_refusal_bad", (rc != K.ERR_UNSUPPORTED) + (not np.all(a[:N] == SENTINEL)) + (not tail_intact(a, N)))

# ================================================================ 3. fp32 features of the MLP baseline
for n, N in K.FEATURE_CASES:
    case = "features n %d N %d" % (n, N)
    obs, tpos, _ = K.make_inputs(n, N, K.case_seed(0, n, N) + 9)
    out = out_buf(N * (n + 4), np.float32)
    o, t = up(obs), up(tpos, np.int32)
    check(lib.mjx_bl_features_f32(ptr(o), ptr(t), N, n, ptr(out), None))
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    count("feat_tail_touched", not tail_intact(a, N * (n + 4)))
    later(judge_features, case, n, obs, tpos, a[:N * (n + 4)])

for job in JOBS:
    for what, key, *rest in job.result():
        (put if what == "put" else count)(key, *rest)

W.emit({"err": ERR, "count": CNT, "routes": ROUTES, "cases": CASES})
