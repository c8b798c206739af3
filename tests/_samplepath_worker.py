"""GPU worker for tests/test_gpu_samplepath_matrix.py: every case of mjx_discount_scan, mjx_gae, mjx_sum_stats, mjx_whiten_cast,
mjx_cast_f64_f32, mjx_apply_step and mjx_apply_npg_step in ONE fresh process, through the C entries (mjrl_amd._lib), against the
long-double references and NumPy expressions of tests/_samplepath_cases.py; prints one RESULT JSON line of measured ratios and
counts (the test module compares them with its bars).  Every ctypes call that must succeed goes through check(): the first HIP
error ends the process.  The device calls come first, one after the other; the references are formed and the results judged
after the last of them.
python tests/_samplepath_worker.py"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load  # noqa: E402
from mjrl_amd._lib import ptr as p  # noqa: E402
from tests import _samplepath_cases as K  # noqa: E402
from tests import _worker_dev as W  # noqa: E402

assert np.finfo(np.longdouble).nmant >= 63, "the references need a long double wider than fp64"

T0 = time.time()
lib = load()
ERR, CASES = {}, {}
CNT = {k: 0 for k in ("scan_unwritten", "scan_outside_touched", "scan_guard_touched", "scan2_bits_bad", "scan_rc_bad",
                      "stats_n_bad", "stats_guard_touched", "whiten_bad", "whiten_guard_touched", "cast_bad", "cast_guard_touched",
                      "cast_rc_bad", "step_d_bad", "step_bad", "step_guard_touched", "npg_bad", "npg_alpha_bad", "npg_guard_touched")}
FIRST = {}                                                   # the first few mismatching elements per bit-equality key
_INT = {8: np.int64, 4: np.int32}
_UINT = {8: np.uint64, 4: np.uint32}


def put(key, val, case):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]
    CASES[key] = CASES.get(key, 0) + 1


def count(key, n, case=None, first=None):
    CNT[key] += int(n)
    CASES[key] = CASES.get(key, 0) + 1
    if n and case is not None and len(FIRST.setdefault(key, [])) < 4:
        FIRST[key].append([case, first])


def up(a):
    """host array -> device tensor; an empty array as one element, so that its pointer is not NULL"""
    a = np.asarray(a)
    return W.up(np.zeros(1, a.dtype) if a.size == 0 else a, None)


def up_out(buf):
    return up(buf.view(_INT[buf.itemsize]))


def down(t):
    a = t.cpu().numpy()
    return a.view(_UINT[a.itemsize])


def pb(t):
    """the body of a guarded device buffer"""
    return ctypes.c_void_p(t.data_ptr() + K.GUARD * t.element_size())


# ================================================================ 1. scans (device)
def dev_scan(mode, x, b, off, term, gamma, lam):
    """one mjx_discount_scan (mode 0) or mjx_gae call -> the guarded output buffer on the host"""
    out = up_out(K.new_out(int(off[-1])))
    xd, od = up(x), up(np.asarray(off, np.int64))
    if mode == 0:
        check(lib.mjx_discount_scan(p(xd), p(od), len(off) - 1, gamma, pb(out), None))
    else:
        bd, td = up(b), (None if term is None else up(term))
        check(lib.mjx_gae(p(xd), p(bd), p(od), p(td), len(off) - 1, gamma, lam, pb(out), None))
    torch.cuda.synchronize()
    return down(out)


def singles(off):
    """(trajectory index, length) of the first trajectory of every length"""
    lens = np.diff(off)
    return [(int(np.nonzero(lens == T)[0][0]), int(T)) for T in sorted(set(lens.tolist()))]


EDGE = K.offsets_of(K.EDGE_LENS)
NE, NT = int(EDGE[-1]), len(K.EDGE_LENS)
SCAN0, SCAN1, SCAN2, EXTRA = [], [], [], []                 # what the judging below needs

for ci, (g, dist) in enumerate(K.SCAN0_CONFIGS):
    x = K.scan_input(dist, NE, 1000 + ci)
    runs = [("batch", EDGE, slice(0, NE), dev_scan(0, x, None, EDGE, None, g, None))]
    for i, T in singles(EDGE):
        sl = slice(int(EDGE[i]), int(EDGE[i + 1]))
        runs.append(("single T %d" % T, K.offsets_of((T,)), sl, dev_scan(0, x[sl], None, K.offsets_of((T,)), None, g, None)))
    SCAN0.append(("g %g %s" % (g, dist), x, g, runs))

for ci, (gamma, lam, fl, scale, dist) in enumerate(K.SCAN1_CONFIGS):
    r, b, term = K.scan_input(dist, NE, 2000 + ci), K.baseline_input(NE, scale, 2000 + ci), K.flags_for(fl, NT)
    runs = [("batch", EDGE, slice(0, NE), dev_scan(1, r, b, EDGE, term, gamma, lam))]
    for i, T in singles(EDGE):
        sl = slice(int(EDGE[i]), int(EDGE[i + 1]))
        t1 = None if term is None else term[i:i + 1]
        runs.append(("single T %d" % T, K.offsets_of((T,)), sl, dev_scan(1, r[sl], b[sl], K.offsets_of((T,)), t1, gamma, lam)))
    SCAN1.append(("gamma %g lambda %g flags %s baseline x %g %s" % (gamma, lam, fl, scale, dist), r, b, term, gamma, lam, runs))
    if ci < len(K.SCAN2_LAMBDAS):                            # the same inputs through k_traj_scan<2>
        lam2 = K.SCAN2_LAMBDAS[ci]
        SCAN2.append(("lambda %g batch" % lam2, EDGE, r, b, dev_scan(1, r, b, EDGE, term, gamma, lam2)))
        for i, T in singles(EDGE):
            sl = slice(int(EDGE[i]), int(EDGE[i + 1]))
            t1 = None if term is None else term[i:i + 1]
            SCAN2.append(("lambda %g single T %d" % (lam2, T), K.offsets_of((T,)), r[sl], b[sl],
                          dev_scan(1, r[sl], b[sl], K.offsets_of((T,)), t1, gamma, lam2)))

# offsets[0] = 1000 (what lies before it is poison and must be neither read nor written); 70 000 trajectories of 0 to 3 steps
for name, off in (("offsets[0] 1000", K.offsets_of(K.SHIFTED_LENS, K.SHIFTED_START)), ("70000 trajectories", K.offsets_of(K.many_lens()))):
    n, nt = int(off[-1]), len(off) - 1
    x, b, term = K.scan_input("mixed", n, 3000 + nt), K.baseline_input(n, 1.0, 3000 + nt), K.flags_for("pattern", nt)
    x[:off[0]] = 1e30
    b[:off[0]] = -1e30
    EXTRA.append((name, off, x, b, term, 0.995 if off[0] else 0.9, dev_scan(0, x, None, off, None, 0.995 if off[0] else 0.9, None),
                  dev_scan(1, x, b, off, term, 0.995, 0.97), dev_scan(1, x, b, off, term, 0.995, -1.0 if off[0] else 1.5)))

# host-side refusals and the empty batch: nothing is launched, nothing written
buf = K.new_out(8)
o8, x8, off8 = up_out(buf), up(np.ones(8)), up(np.array([0, 8], np.int64))
rcs = [(lib.mjx_discount_scan(None, None, 0, 0.9, None, None), K.OK),
       (lib.mjx_gae(None, None, None, None, 0, 0.9, 0.5, None, None), K.OK),
       (lib.mjx_discount_scan(p(x8), p(off8), -1, 0.9, pb(o8), None), K.ERR_ARG),
       (lib.mjx_gae(p(x8), p(x8), p(off8), None, -1, 0.9, 0.5, pb(o8), None), K.ERR_ARG),
       (lib.mjx_discount_scan(None, p(off8), 1, 0.9, pb(o8), None), K.ERR_ARG),
       (lib.mjx_gae(None, p(x8), p(off8), None, 1, 0.9, 0.5, pb(o8), None), K.ERR_ARG)]
torch.cuda.synchronize()
count("scan_rc_bad", sum(rc != want for rc, want in rcs) + (not np.array_equal(down(o8), buf)), "return codes", [rc for rc, _ in rcs])

# ================================================================ 2. statistics (device)
STATS = []


def dev_stats(xd, N, shift):
    out = up_out(K.new_out(3))
    check(lib.mjx_sum_stats(p(xd), N, shift, pb(out), None))
    torch.cuda.synchronize()
    return down(out)


for mu in K.STATS_MU:
    for N in K.STATS_N:
        x = K.stats_input(N, mu)
        xd = up(x)
        first = dev_stats(xd, N, 0.0)
        s = K.body(first)
        mean = float(s[0] / s[2]) if N else 1.5              # engine.whitened_advantages: the second pass about the first's mean
        STATS.append((mu, N, x, mean, first, dev_stats(xd, N, mean)))

# ================================================================ 3. casts (device)
WHITEN, CAST = [], []
for size in K.WHITEN_SIZES:
    for variant in K.WHITEN_VARIANTS:
        a, mean, std, eps = K.whiten_input(size, variant)
        out = up_out(K.new_out(size, 4))
        ad = up(a)
        check(lib.mjx_whiten_cast(p(ad), size, mean, std, eps, pb(out), None))
        torch.cuda.synchronize()
        WHITEN.append((size, variant, a, mean, std, eps, down(out)))
for size in K.CAST_SIZES:
    a = K.cast_input(size)
    out = up_out(K.new_out(size, 4))
    ad = up(a)
    check(lib.mjx_cast_f64_f32(p(ad), size, pb(out), None))
    torch.cuda.synchronize()
    CAST.append((size, a, down(out)))
buf = K.new_out(8, 4)
o8 = up_out(buf)
rcs = [lib.mjx_whiten_cast(p(x8), 0, 0.0, 1.0, 1e-6, pb(o8), None), lib.mjx_cast_f64_f32(p(x8), 0, pb(o8), None)]
torch.cuda.synchronize()
count("cast_rc_bad", sum(rc != K.OK for rc in rcs) + (not np.array_equal(down(o8), buf)), "count 0", rcs)

# ================================================================ 4. steps (device; judged at once, the expectation is NumPy float32)
POLICIES = {}
mls = K.MIN_LOG_STD
for m in K.STEP_M:
    for residue in K.STEP_RESIDUES:
        n, h, d = K.step_policy(m, residue)
        ctx, hid = ctypes.c_void_p(), (ctypes.c_int * 1)(h)
        check(lib.mjx_create(ctypes.byref(ctx), 0, n, m, hid, 1))
        d_dev = int(lib.mjx_num_params(ctx))
        POLICIES["m %d d %% 256 = %d" % (m, residue)] = "n %d hidden %d d %d" % (n, h, d_dev)
        count("step_d_bad", d_dev != d or d_dev % 256 != residue, "m %d residue %d" % (m, residue), d_dev)
        if d_dev != d:
            continue
        oS = d - m
        for variant in range(K.STEP_VARIANTS):
            theta, x = K.step_input(d, m, variant, 10 * d + variant)
            td, xd = up(theta), up(x)
            for alpha in K.STEP_ALPHAS:
                case = "m %d d %d alpha %g variant %d" % (m, d, alpha, variant)
                out = up_out(K.new_out(d, 4))
                check(lib.mjx_apply_step(ctx, p(td), p(xd), alpha, mls, pb(out), None))
                torch.cuda.synchronize()
                res = K.bits_check(down(out), K.step_expect(theta, x, alpha, oS))
                count("step_bad", res["bad"], case, res["first"])
                count("step_guard_touched", res["guard_touched"], case)
            for gi, gdotx in enumerate(K.NPG_GDOTX):
                case = "m %d d %d g.x %g variant %d" % (m, d, gdotx, variant)
                out, aout, gd = up_out(K.new_out(d, 4)), up_out(K.new_out(1)), up(np.array([gdotx]))
                no_alpha = variant == gi                     # alpha_out = NULL is accepted
                check(lib.mjx_apply_npg_step(ctx, p(td), p(xd), p(gd), K.NPG_STEP_SIZE, mls, pb(out), None if no_alpha else pb(aout), None))
                torch.cuda.synchronize()
                alpha, ab = K.npg_alpha(gdotx), down(aout)
                res = K.bits_check(down(out), K.step_expect(theta, x, np.float32(alpha), oS))
                count("npg_bad", res["bad"], case, res["first"])
                want = K.new_out(1)
                if not no_alpha:
                    K.body(want)[0] = alpha
                count("npg_alpha_bad", not np.array_equal(ab, want), case, [float(K.body(ab)[0]), float(alpha)])
                count("npg_guard_touched", res["guard_touched"] + K.guard_touched(ab), case)
        lib.mjx_destroy(ctx)

T_DEVICE = time.time() - T0

# ================================================================ judging
for name, x, g, runs in SCAN0:
    ref, A = K.scan0_reference(x, EDGE, g)
    for what, off, sl, buf in runs:
        res = K.scan_check(buf, off, ref[sl], A[sl], 4)
        case = "%s %s" % (name, what)
        put("scan0", res["ratio"], "%s: trajectory %d step %d" % (case, res["traj"], res["t"]))
        put("scan0_edge", res["ratio"], "%s: trajectory %d step %d" % (case, res["traj"], res["t"]))
        for k in ("unwritten", "outside_touched", "guard_touched"):
            count("scan_" + k, res[k], case)

for (name, r, b, term, gamma, lam, runs), (ref, A) in zip(SCAN1, K.scan1_references([s[1:6] for s in SCAN1], EDGE)):
    for what, off, sl, buf in runs:
        res = K.scan_check(buf, off, ref[sl], A[sl], 6)
        case = "%s %s" % (name, what)
        put("scan1", res["ratio"], "%s: trajectory %d step %d" % (case, res["traj"], res["t"]))
        put("scan1_edge", res["ratio"], "%s: trajectory %d step %d" % (case, res["traj"], res["t"]))
        for k in ("unwritten", "outside_touched", "guard_touched"):
            count("scan_" + k, res[k], case)


def judge_diff(case, buf, off, x, b):
    res = K.diff_check(buf, off, x, b)
    count("scan2_bits_bad", res["bad"], case)
    for k in ("unwritten", "outside_touched", "guard_touched"):
        count("scan_" + k, res[k], case)


for case, off, r, b, buf in SCAN2:
    judge_diff(case, buf, off, r, b)

for name, off, x, b, term, g0, buf0, buf1, buf2 in EXTRA:
    for key, slack, buf, (ref, A) in (("scan0", 4, buf0, K.scan0_reference(x, off, g0)),
                                      ("scan1", 6, buf1, K.scan1_reference(x, b, off, term, 0.995, 0.97))):
        res = K.scan_check(buf, off, ref, A, slack)
        put(key, res["ratio"], "%s: trajectory %d step %d" % (name, res["traj"], res["t"]))
        for k in ("unwritten", "outside_touched", "guard_touched"):
            count("scan_" + k, res[k], name)
    judge_diff(name, buf2, off, x, b)

for mu, N, x, mean, first, second in STATS:
    for shift, buf in ((0.0, first), (mean, second)):
        case = "N %d mu %g shift %.17g" % (N, mu, shift)
        res = K.stats_check(K.body(buf), x, shift)
        put("stats_s", res["s"], case)
        put("stats_q", res["q"], case)
        count("stats_n_bad", not res["n_ok"], case, float(K.body(buf)[2]))
        count("stats_guard_touched", K.guard_touched(buf), case)
    if N:
        put("std_rel_mu_%g" % mu, K.std_rel_error(K.body(second)[1], x), "N %d" % N)

for size, variant, a, mean, std, eps, buf in WHITEN:
    res = K.bits_check(buf, K.whiten_expect(a, mean, std, eps))
    case = "whiten %s N %d" % (variant, size)
    count("whiten_bad", res["bad"], case, res["first"])
    count("whiten_guard_touched", res["guard_touched"], case)
for size, a, buf in CAST:
    res = K.bits_check(buf, K.cast_expect(a))
    if res["bad"]:
        idx = np.nonzero(K.body(buf).view(np.uint32) != K.cast_expect(a).view(np.uint32))[0][:8]
        res["first"] = [[int(i), repr(float(a[i])), float(K.body(buf)[i])] for i in idx]
    count("cast_bad", res["bad"], "cast N %d" % size, res["first"])
    count("cast_guard_touched", res["guard_touched"], "cast N %d" % size)

W.emit({"err": ERR, "count": CNT, "cases": CASES, "first": FIRST, "policies": POLICIES,
        "seconds": {"device": round(T_DEVICE, 2), "all": round(time.time() - T0, 2)}})
