"""The cases of tests/test_gpu_samplepath_matrix.py, their inputs, the long-double references and the checks, shared by the GPU
worker (tests/_samplepath_worker.py) and by tests/test_samplepath_checks.py, which runs the same checks on NumPy emulations of the
sample-path kernels (csrc/vecops.h: k_traj_scan<0/1/2>, k_sum_stats_partial / _final, k_whiten_cast, k_cast_f64_f32, k_apply_step,
k_apply_npg_step) with and without planted defects.  No GPU here.

Every output lives in a guarded buffer: GUARD elements of a recognisable bit pattern, the body prefilled with another (a NaN with a
payload), GUARD elements again.  The buffers are handled as unsigned integers, so "untouched" and "bit-equal" are integer
comparisons."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
OK, ERR_ARG = 0, -1
GUARD = 64
_PAT = {8: (np.uint64, 0x7FF8C0DEC0DEC0DE, 0x7FF8000000000BAD), 4: (np.uint32, 0x7FC0C0DE, 0x7FC00BAD)}   # size: type, guard, prefill
_FLT = {8: np.float64, 4: np.float32}


# ---------------------------------------------------------------- guarded output buffers
def new_out(n, size=8):
    """GUARD | n prefilled elements | GUARD as unsigned integers of `size` bytes"""
    t, g, f = _PAT[size]
    return np.concatenate([np.full(GUARD, g, t), np.full(n, f, t), np.full(GUARD, g, t)])


def body(buf):
    """the written range of a guarded buffer, as floats (a view)"""
    return buf[GUARD:len(buf) - GUARD].view(_FLT[buf.itemsize])


def guard_touched(buf):
    g = _PAT[buf.itemsize][1]
    return int(np.sum(buf[:GUARD] != g) + np.sum(buf[len(buf) - GUARD:] != g))


def prefilled(buf):
    """mask over the body: the element still holds the prefill pattern"""
    return buf[GUARD:len(buf) - GUARD] == _PAT[buf.itemsize][2]


def _ratio(err, bound):
    """err / bound, an exact zero allowed where the bound is zero; anything not finite is inf"""
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    r = np.asarray(r, np.float64)
    return np.where(np.isfinite(r), r, np.inf)


# ================================================================ 1. scans
SCAN_LENGTHS = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1000, 4099, 65537)
# every length once, in one ragged batch with empty trajectories at the start, in the middle and at the end
EDGE_LENS = (0, 1, 2, 3, 0, 255, 256, 257, 511, 0, 512, 513, 1000, 4099, 65537, 0)
SHIFTED_LENS, SHIFTED_START = (0, 257, 3, 0, 513, 2), 1000             # the call whose offsets[0] is not 0
MANY = 70000                                                            # trajectories of lengths 0 to 3 in one call
DISTS = ("normal", "positive", "mixed")
FLAGS = ("pattern", "zeros", "ones", "null")
SCAN0_CONFIGS = [(0.0, "mixed"), (0.5, "positive"), (0.9, "normal"), (0.995, "mixed"), (1.0, "positive"), (1.0, "mixed")]
# (gamma, lambda, terminated flags, baseline scale, reward distribution)
SCAN1_CONFIGS = [(0.995, 0.97, "pattern", 1.0, "normal"), (1.0, 1.0, "zeros", 1e6, "mixed"), (0.9, 0.0, "ones", 1.0, "positive"),
                 (0.0, 0.5, "null", 1e6, "normal"), (0.99, 1.0, "pattern", 1e6, "mixed"), (0.995, 0.97, "null", 1.0, "mixed")]
SCAN2_LAMBDAS = (-1.0, 1.5, float("nan"))                               # outside [0, 1]: k_traj_scan<2>


def offsets_of(lens, start=0):
    off = np.empty(len(lens) + 1, np.int64)
    off[0] = start
    np.cumsum(np.asarray(lens, np.int64), out=off[1:])
    off[1:] += start
    return off


def many_lens(seed=70):
    lens = np.random.RandomState(seed).randint(0, 4, size=MANY)
    lens[[0, 1, MANY - 2, MANY - 1]] = (0, 3, 3, 0)
    return lens


def scan_input(dist, N, seed):
    """standard normal; all positive; standard normal times 10**randint(-8, 9) per element, so small values sit behind large ones"""
    rng = np.random.RandomState(seed)
    x = rng.randn(N)
    if dist == "positive":
        x = np.abs(x) + 0.01
    elif dist == "mixed":
        x = x * 10.0 ** rng.randint(-8, 9, size=N)
    else:
        assert dist == "normal", dist
    return x


def baseline_input(N, scale, seed):
    return np.random.RandomState(seed + 5000).randn(N) * scale


def flags_for(kind, n):
    """uint8 per trajectory, None for the NULL pointer ("none terminated"); the pattern is not periodic in 2"""
    i = np.arange(n)
    if kind == "null":
        return None
    return {"pattern": ((i % 3 == 0) | (i % 7 == 2)), "zeros": i < 0, "ones": i >= 0}[kind].astype(np.uint8)


def scan_ld(X, off, g):
    """y[t] = x[t] + g y[t + 1] inside every trajectory [off[i], off[i + 1]), sequentially in long double, for the columns of X
    (N x C) at once with a factor per column: the loop runs over the steps of the longest trajectory only"""
    X = np.asarray(X, LD)
    g = np.asarray(g, LD).reshape(1, -1)
    lens, ends = np.diff(off), off[1:]
    Y = np.zeros_like(X)
    run = np.zeros((len(lens), X.shape[1]), LD)
    order = np.argsort(-lens, kind="stable")                # trajectories by falling length: the active ones are a prefix
    sl = lens[order]
    for k in range(int(lens.max()) if len(lens) else 0):
        act = order[:int(np.searchsorted(-sl, -k, side="left"))]         # lens > k
        idx = ends[act] - 1 - k
        r = X[idx] + g * run[act]
        run[act] = r
        Y[idx] = r
    return Y


def next_baseline(b, off, term, dtype=LD):
    """b1[t + 1] of process_samples.py:21-29 per element: the next baseline value, at a trajectory's last step 0 when it is
    terminated and the last value itself otherwise"""
    b = np.asarray(b, dtype)
    bn = np.roll(b, -1)
    lens = np.diff(off)
    last = off[1:][lens > 0] - 1
    t = np.zeros(len(lens), bool) if term is None else np.asarray(term).astype(bool)
    bn[last] = np.where(t[lens > 0], dtype(0), b[last])
    return bn


def scan0_references(items, off):
    """items: (x, g) sharing the offsets -> [(ref, A)] in long double: the recurrence over x and over |x|, all in one loop"""
    cols = [c for x, g in items for c in (np.asarray(x, LD), np.abs(np.asarray(x, LD)))]
    Y = scan_ld(np.stack(cols, axis=1), off, [g for x, g in items for _ in (0, 1)])
    return [(Y[:, 2 * i], Y[:, 2 * i + 1]) for i in range(len(items))]


def scan0_reference(x, off, g):
    return scan0_references([(x, g)], off)[0]


def gae_columns(r, b, off, term, gamma):
    """-> td = r + gamma b_next - b and V = |r| + gamma |b_next| + |b| in long double"""
    r, b, G = np.asarray(r, LD), np.asarray(b, LD), LD(gamma)
    bn = next_baseline(b, off, term)
    return r + G * bn - b, np.abs(r) + G * np.abs(bn) + np.abs(b)


def scan1_references(items, off):
    """items: (r, b, term, gamma, lam) sharing the offsets -> [(ref, A_V)] in long double.  The scan's factor is the fp64 product
    gamma * lam, as include/mjx.h defines the operation (discount_scan(td, gamma*lam)) and as the host forms it; everything else
    is long double"""
    cols, gs = [], []
    for r, b, term, gamma, lam in items:
        cols += list(gae_columns(r, b, off, term, gamma))
        gs += [np.float64(gamma) * np.float64(lam)] * 2
    Y = scan_ld(np.stack(cols, axis=1), off, gs)
    return [(Y[:, 2 * i], Y[:, 2 * i + 1]) for i in range(len(items))]


def scan1_reference(r, b, off, term, gamma, lam):
    return scan1_references([(r, b, term, gamma, lam)], off)[0]


def _rem(off, n):
    """steps left in its trajectory, per element of the body [0, off[-1]) (0 before off[0])"""
    lens = np.diff(off)
    rem = np.zeros(n, np.int64)
    rem[off[0]:] = np.repeat(off[1:], lens) - np.arange(off[0], off[-1])
    return rem


def scan_check(buf, off, ref, A, slack):
    """buf: guarded fp64 buffer whose body is [0, off[-1]).  |y - ref| <= (2 rem + slack) 2^-53 A per element (slack 4: mode 0,
    6: mode 1) -> worst ratio with its index, trajectory and step; elements of a trajectory still prefilled; elements before
    off[0] that changed; guard elements that changed"""
    n = int(off[-1])
    assert len(buf) == n + 2 * GUARD and len(ref) == n and len(A) == n
    y, pre = body(buf), prefilled(buf)
    w = np.arange(n) >= off[0]
    res = {"ratio": 0.0, "at": -1, "traj": -1, "t": -1, "unwritten": int(np.sum(pre & w)), "outside_touched": int(np.sum(~pre & ~w)),
           "guard_touched": guard_touched(buf)}
    if np.any(w):
        bound = (2 * _rem(off, n) + slack).astype(LD) * LD(U) * np.asarray(A, LD)
        with np.errstate(invalid="ignore"):
            ratio = np.where(w, _ratio(np.abs(y.astype(LD) - np.asarray(ref, LD)), bound), 0.0)
        i = int(np.argmax(ratio))
        tr = int(np.searchsorted(off, i, side="right") - 1)
        res.update(ratio=float(ratio[i]), at=i, traj=tr, t=int(i - off[tr]))
    return res


def scan_ok(res):
    return res["ratio"] <= 1.0 and res["unwritten"] == 0 and res["outside_touched"] == 0 and res["guard_touched"] == 0


def diff_check(buf, off, x, b):
    """mode 2: the body from off[0] on bit-equal to NumPy's x - b -> mismatches, and the placement counts of scan_check"""
    n = int(off[-1])
    pre = prefilled(buf)
    w = np.arange(n) >= off[0]
    want = (np.asarray(x, np.float64) - np.asarray(b, np.float64)).view(np.uint64)
    got = buf[GUARD:GUARD + n]
    return {"bad": int(np.sum((got != want) & w)), "unwritten": int(np.sum(pre & w)), "outside_touched": int(np.sum(~pre & ~w)),
            "guard_touched": guard_touched(buf)}


def diff_ok(res):
    return not any(res.values())


# ---- fp64 emulation of k_traj_scan: 256 threads, segments of ceil(T / 256), thread 0 chains the carries
def emulate_scan(buf, mode, x, bl, off, term, gamma, lam, defect=None):
    """One mjx_discount_scan (mode 0, lam unused) or mjx_gae call into the guarded buffer `buf`, in fp64 and in the kernel's
    order (a fused multiply-add on the device only removes roundings).  defect: carry_dropped, pw_short, bootstrap_swapped,
    flag_neighbour, gamma_for_gl, mode2_for_lam0, empty_shifts or offset0_ignored."""
    out = buf.view(np.float64)                               # (indices below include the leading guard)
    x = np.asarray(x, np.float64)
    g = gamma
    if mode != 0:
        bl = np.asarray(bl, np.float64)
        if lam < 0.0 or lam > 1.0 or np.isnan(lam) or (defect == "mode2_for_lam0" and lam == 0.0):
            mode = 2
        else:
            g = gamma * (1.0 if defect == "gamma_for_gl" else lam)
    n_traj = len(off) - 1
    shift = 0
    for i in range(n_traj):
        o, T = int(off[i]), int(off[i + 1] - off[i])
        if defect == "offset0_ignored":
            o -= int(off[0])
        if T <= 0:
            if defect == "empty_shifts":
                shift = 1
            continue
        xr = x[o:o + T]
        if mode == 2:
            v = xr - bl[o:o + T]
        else:
            if mode == 1:
                br = bl[o:o + T]
                fl = term[(i + 1) % n_traj if defect == "flag_neighbour" else i] if term is not None else 0
                if defect == "bootstrap_swapped":
                    fl = not fl
                bn = np.append(br[1:], 0.0 if fl else br[T - 1])
                val = xr + gamma * bn - br
            else:
                val = xr
            seg = (T + 255) // 256
            lo = np.minimum(T, np.arange(256) * seg)
            hi = np.minimum(T, lo + seg)
            run, f = np.zeros(256), np.ones(256)
            for j in range(seg):                             # pass 1: every segment from a zero carry, and g^length
                t = hi - 1 - j
                m = t >= lo
                tc = np.where(m, t, 0)
                run = np.where(m, val[tc] + g * run, run)
                f = np.where(m & ((j > 0) | (defect != "pw_short")), f * g, f)
            cin, c = np.zeros(256), 0.0
            for k in range(255, -1, -1):
                cin[k] = c
                c = run[k] + f[k] * c
            if defect == "carry_dropped":
                cin[:] = 0.0
            run, v = cin.copy(), np.empty(T)
            for j in range(seg):                             # pass 2: every segment again from its carry
                t = hi - 1 - j
                m = t >= lo
                tc = np.where(m, t, 0)
                run = np.where(m, val[tc] + g * run, run)
                v[tc[m]] = run[m]
        a = GUARD + o + shift
        e = min(a + T, len(out))
        out[a:e] = v[:e - a]
        shift = 0
    return buf


# ================================================================ 2. statistics
STATS_N = (0, 1, 255, 256, 257, 131071, 131072, 131073, 300001)
STATS_MU = (0.0, 1e8)
STATS_GRID, STATS_BLOCK = 512, 256


def stats_input(N, mu, seed=None):
    return np.random.RandomState(4000 + N % 9973 if seed is None else seed).randn(N) + mu


def stats_reference(x, shift):
    """-> sum v, sum v^2, sum |v| in long double, v = longdouble(x) - longdouble(shift)"""
    v = np.asarray(x, LD) - LD(shift)
    return v.sum(dtype=LD), (v * v).sum(dtype=LD), np.abs(v).sum(dtype=LD)


def stats_check(out3, x, shift):
    """|s - ref| <= (N + 2) 2^-53 sum |v|, |q - ref| <= (N + 4) 2^-53 sum v^2: forward bounds of an N-term sum in any order plus
    the roundings of v and v^2; out[2] == N exactly -> the two ratios and the count check"""
    N = len(x)
    s, q, a = stats_reference(x, shift)
    out3 = np.asarray(out3, np.float64)
    rs = _ratio(np.abs(LD(out3[0]) - s), LD(N + 2) * LD(U) * a)
    rq = _ratio(np.abs(LD(out3[1]) - q), LD(N + 4) * LD(U) * q)
    return {"s": float(rs), "q": float(rq), "n_ok": bool(out3[2] == N)}


def stats_ok(res):
    return res["s"] <= 1.0 and res["q"] <= 1.0 and res["n_ok"]


def std_rel_error(q_dev, x):
    """relative error of the two-pass population standard deviation sqrt(q / N), as engine.whitened_advantages forms it, against
    the long-double value about the long-double mean; a zero reference asks for exactly zero"""
    N = len(x)
    xl = np.asarray(x, LD)
    dv = xl - xl.sum(dtype=LD) / LD(N)
    ref = np.sqrt((dv * dv).sum(dtype=LD) / LD(N))
    got = LD(np.sqrt(np.float64(q_dev) / np.float64(N)))
    return float(_ratio(np.abs(got - ref), ref))


def emulate_stats(x, shift, defect=None):
    """NumPy's fp64 sums over what the grid of 512 x 256 threads reads.  defect: partial0_dropped, partial511_dropped, tail_dropped
    (what lies beyond one grid pass) or q_unshifted."""
    x = np.asarray(x, np.float64)
    N = len(x)
    i = np.arange(N)
    keep = np.ones(N, bool)
    if defect == "partial0_dropped":
        keep = (i // STATS_BLOCK) % STATS_GRID != 0
    if defect == "partial511_dropped":
        keep = (i // STATS_BLOCK) % STATS_GRID != STATS_GRID - 1
    if defect == "tail_dropped":
        keep = i < STATS_GRID * STATS_BLOCK
    v = x[keep] - shift
    w = x[keep] if defect == "q_unshifted" else v
    return np.array([np.sum(v), np.sum(w * w), float(N)])


# ================================================================ 3. casts
SMALL_SIZES = (1, 255, 256, 257)
WHITEN_SIZES = SMALL_SIZES + (4096 * 256, 4096 * 256 + 1)               # the grid is capped at 4096 workgroups
CAST_SIZES = SMALL_SIZES + (8192 * 256, 8192 * 256 + 1)                 # ... at 8192
WHITEN_VARIANTS = ("plain", "std0", "mean1e8")
_POS = (0.0, np.inf, float(np.finfo(np.float32).max), 3.4028235677973366e38, 1e39,          # FLT_MAX + half an ulp: the first inf
        1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52,             # ties to even (down, up); the first fp64 value
                                                                                            # above a tie (2^-53 more is the tie again)
        1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -52), 1e-46)
CAST_PLANTS = np.array([v for p in _POS for v in (p, -p)] + [np.nan])


def cast_input(size, seed=None):
    """randn times 10**uniform(-50, 42) (so some overflow and some vanish), CAST_PLANTS at the front and again at the very end;
    a buffer too short for them holds the first tie"""
    rng = np.random.RandomState(300 + size % 9973 if seed is None else seed)
    a = rng.randn(size) * 10.0 ** rng.uniform(-50, 42, size=size)
    k = len(CAST_PLANTS)
    if size >= 2 * k:
        a[:k] = CAST_PLANTS
        a[size - k:] = CAST_PLANTS[::-1]
    else:
        a[:] = (1.0 + 2.0 ** -24)
    return a


def whiten_input(size, variant, seed=None):
    """-> a, mean, std, eps"""
    rng = np.random.RandomState(900 + size % 9973 if seed is None else seed)
    a = rng.randn(size) * 3.0 + 0.7
    if variant == "std0":                                    # eps alone is the denominator
        return a, float(np.mean(a)), 0.0, 1e-6
    if variant == "mean1e8":
        return a / 3.0 + 1e8, 1e8, 1.0, 1e-6
    return a, float(np.mean(a)), float(np.std(a)), 1e-6


def bits_check(buf, want):
    """the body of a guarded fp32 buffer against `want` (float32) as uint32, NaN against NaN by NaN-ness only -> mismatches, the
    first few of them, guard elements that changed"""
    got = buf[GUARD:len(buf) - GUARD]
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    gf = got.view(np.float32)
    bad = (got != want.view(np.uint32)) & ~(np.isnan(gf) & np.isnan(want) & (got != _PAT[4][2]))
    idx = np.nonzero(bad)[0]
    return {"bad": int(len(idx)), "first": [[int(i), float(gf[i]), float(want[i])] for i in idx[:4]], "guard_touched": guard_touched(buf)}


def bits_ok(res):
    return res["bad"] == 0 and res["guard_touched"] == 0


def whiten_expect(a, mean, std, eps):
    with np.errstate(all="ignore"):
        return ((a - mean) / (std + eps)).astype(np.float32)


def cast_expect(a):
    with np.errstate(all="ignore"):
        return np.asarray(a, np.float64).astype(np.float32)


def emulate_cast(a, defect=None):
    """a.astype(float32); defect: truncate (round toward zero) or flush (fp32 subnormals to zero)"""
    f = cast_expect(a)
    if defect == "truncate":                                 # round toward zero
        with np.errstate(all="ignore"):
            over = np.abs(f.astype(np.float64)) > np.abs(a)
            f = np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)
    if defect == "flush":
        f = np.where(np.abs(f) < np.finfo(np.float32).tiny, np.copysign(np.float32(0), f), f).astype(np.float32)
    return f


# ================================================================ 4. steps
STEP_M = (1, 8)
STEP_RESIDUES = (0, 1, 255)
STEP_ALPHAS = (0.0, -0.3, 1e-30, 1e30)
STEP_VARIANTS = 5
NPG_GDOTX = (3.7, -3.7, 0.0, 1e-300)
NPG_STEP_SIZE = 0.05
MIN_LOG_STD = -2.5


def num_params(n, h, m):
    return n * h + h + h * m + m + m


def step_policy(m, residue):
    """the one-hidden-layer policy (n, h) with the fewest parameters d > 256 (more than one workgroup) and d % 256 == residue"""
    best = None
    for h in range(2, 33):
        for n in range(1, 65):
            d = num_params(n, h, m)
            if d > 256 and d % 256 == residue and (best is None or d < best[0]):
                best = (d, n, h)
    return best[1], best[2], best[0]


def step_input(d, m, variant, seed):
    """-> theta, x (float32).  log_std block [d - m, d): variants 0..3 plant min_log_std - 0.5, the value just below min_log_std,
    min_log_std itself and the value just above it (rotated by the variant) in the first four entries, with x = 0 there, so the
    stepped value is the planted one for every step length; the other entries hover about min_log_std and move.  Variant 4: none
    planted.  The last weight, oS - 1, holds min_log_std - 1 with x = 0: it must not be clamped."""
    rng = np.random.RandomState(seed)
    theta, x = rng.randn(d).astype(np.float32), rng.randn(d).astype(np.float32)
    oS, mls = d - m, np.float32(MIN_LOG_STD)
    theta[oS:] = mls + rng.randn(m).astype(np.float32) * np.float32(0.05)
    plants = [mls - np.float32(0.5), np.nextafter(mls, np.float32(-10)), mls, np.nextafter(mls, np.float32(10))]
    if variant < 4:
        for j in range(min(m, 4)):
            theta[oS + j] = plants[(variant + j) % 4]
            x[oS + j] = 0.0
    theta[oS - 1], x[oS - 1] = mls - np.float32(1), 0.0
    return theta, x


def step_expect(theta, x, alpha, oS, mls=MIN_LOG_STD):
    """NumPy float32 arithmetic: the product rounded, then the sum; np.maximum from oS on"""
    with np.errstate(all="ignore"):
        v = theta + np.float32(alpha) * x
    assert v.dtype == np.float32
    v[oS:] = np.maximum(v[oS:], np.float32(mls))
    return v


def npg_alpha(gdotx, step_size=NPG_STEP_SIZE):
    return np.sqrt(np.abs(np.float64(step_size) / (np.float64(gdotx) + 1e-20)))


def emulate_step(buf, theta, x, alpha, oS, mls=MIN_LOG_STD, defect=None):
    """k_apply_step into the guarded fp32 buffer `buf`; defect: fma, clamp_early, clamp_late or last_unwritten"""
    d = len(theta)
    if defect == "fma":                                      # one rounding: the fp64 product of two floats is exact
        with np.errstate(all="ignore"):
            v = (theta.astype(np.float64) + np.float64(np.float32(alpha)) * x.astype(np.float64)).astype(np.float32)
        v[oS:] = np.maximum(v[oS:], np.float32(mls))
    else:
        c = oS - 1 if defect == "clamp_early" else oS + 1 if defect == "clamp_late" else oS
        v = step_expect(theta, x, alpha, c, mls)
    n = d - 1 if defect == "last_unwritten" else d
    buf[GUARD:GUARD + n] = v[:n].view(np.uint32)
    return buf
