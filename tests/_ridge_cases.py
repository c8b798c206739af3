"""The cases of tests/test_gpu_ridge_matrix.py, their inputs, the long-double references and the checks, shared by the GPU worker
(tests/_ridge_matrix_worker.py) and by tests/test_ridge_checks.py, which runs the same checks on NumPy emulations of the three Gram
arms (csrc/baseline.h: k_bl_gram_mfma, k_bl_gram_mfma_blk, k_bl_gram) with and without planted defects.  No GPU here.

Features (include/mjx.h, K6): o = clip(obs, -10, 10) / 10, tau = t / 1000; kind 0 [o, tau..tau^4], kind 1 [o, 1, tau..tau^4],
kind 2 [o, o_i o_j (i <= j, row-major), 1, tau..tau^4].  Every column is a product e[p] * e[q] of two entries of the sample's
extended vector e = [o_0 .. o_{n-1}, 1, tau, tau^2, tau^3, tau^4, y].

Inputs hold no NaN and no inf: the device clips with fmin / fmax, which return the other operand for a NaN, np.clip propagates it,
so the two differ there by design and no reference is defined."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MFMA, BLK, FMA = 0, 1, 2                                   # out6[0] of mjx_bl_gram_route
ARMS = ("k_bl_gram_mfma", "k_bl_gram_mfma_blk", "k_bl_gram")
TILE = (16, 128, 64)                                       # features a side of the tile the reduce kernel mirrors by (out6[4])
FMA_ENV = {"MJX_GRAM_FMA": "1"}
ERR_ARG, ERR_UNSUPPORTED = -1, -3
SMALL_N = (1, 31, 32, 33)
PLANTS = (10.0, -10.0, 10.000001, -10.000001, 0.0, -0.0)   # the clip's edges, just beyond them, both zeros
TPOS_HEAD = (2500, 0, 999, 1000)                           # tau 2.5 (> 1), 0, just below 1, exactly 1
# windows (first time index, rows) of ragged trajectories, repeated behind TPOS_HEAD
TPOS_WINDOWS = ((0, 3), (997, 4), (2499, 2), (0, 1), (0, 7), (990, 11), (0, 41), (2460, 41), (0, 1000), (0, 337))
LD_ROWS = 5000                                             # up to here the Gram reference is long double throughout
REF_BLOCK = 512                                            # beyond: fp64 products of 512 rows, summed in long double


def num_features(kind, n):
    return n + 4 if kind == 0 else n + 5 if kind == 1 else n + n * (n + 1) // 2 + 5


def feat_pairs(kind, n):
    """(p, q): column c = e[p[c]] * e[q[c]]; the constant 1 sits at e[n], tau^k at e[n + k], y at e[n + 5]"""
    one = n
    p, q = list(range(n)), [one] * n
    if kind == 2:
        for i in range(n):
            for j in range(i, n):
                p.append(i); q.append(j)
    if kind != 0:
        p.append(one); q.append(one)
    for k in range(1, 5):
        p.append(n + k); q.append(one)
    assert len(p) == num_features(kind, n)
    return np.array(p), np.array(q)


def route_expect(kind, n, N, fma=False):
    """(arm, Z) by the rule of csrc/fit_host.h gram_route, written out again: matrix cores up to 176 augmented features and n <= 24, feature blocks up to n = 64, FMA
    beyond and under MJX_GRAM_FMA=1; Z = clamp(ceil(N / per), 1, cap)"""
    FA = num_features(kind, n) + 1
    z = lambda per, cap: int(max(1, min(cap, -(-N // per))))
    if not fma and FA <= 176 and n <= 24:
        return MFMA, z(2048, 512)
    if not fma and n <= 64:
        nb = -(-FA // 128)
        return BLK, z(2048, -(-768 // (nb * (nb + 1) // 2)))
    nbt = -(-FA // 64)
    return FMA, z(4096, -(-2048 // (nbt * (nbt + 1) // 2)))


# ---------------------------------------------------------------- inputs
def make_tpos(N):
    one = np.concatenate([np.arange(a, a + l) for a, l in TPOS_WINDOWS])
    reps = max(0, N - len(TPOS_HEAD)) // len(one) + 1
    return np.concatenate([np.array(TPOS_HEAD), np.tile(one, reps)])[:N].astype(np.int32)


def make_inputs(n, N, seed, yscale=1.0):
    """-> obs (N x n fp64, randn * 4 with the PLANTS at up to 6 places), tpos (int32), y (randn * yscale)"""
    rng = np.random.RandomState(seed)
    obs = rng.randn(N, n) * 4.0
    k = min(len(PLANTS), (N * n + 1) // 2)
    stride = (N * n) // k
    pos = np.arange(k) * stride + rng.randint(0, stride, size=k)
    obs.flat[pos] = np.roll(np.array(PLANTS), seed % len(PLANTS))[:k]
    return obs, make_tpos(N), rng.randn(N) * yscale


def make_coef(kind, n, seed):
    """randn with per-column scales from 1e-3 to 1e3, in shuffled order"""
    rng = np.random.RandomState(seed)
    F = num_features(kind, n)
    return rng.randn(F) * rng.permutation(np.logspace(-3, 3, F))


# ---------------------------------------------------------------- references (long double)
def extended(obs, tpos, y=None, dtype=LD):
    """[o, 1, tau, tau^2, tau^3, tau^4, y] per row in dtype; the powers by dtype's pow"""
    N, n = obs.shape
    E = np.zeros((N, n + 6), dtype)
    E[:, :n] = np.clip(obs.astype(dtype), -10, 10) / dtype(10)
    E[:, n] = 1
    tau = tpos.astype(dtype) / dtype(1000)
    for k in range(1, 5):
        E[:, n + k] = tau ** k
    if y is not None:
        E[:, n + 5] = y.astype(dtype)
    return E


def features(kind, n, obs, tpos, y=None, dtype=LD):
    """N x F feature matrix, N x (F + 1) with the y column when y is given"""
    p, q = feat_pairs(kind, n)
    if y is not None:
        p, q = np.append(p, n + 5), np.append(q, n)
    E = np.ascontiguousarray(extended(obs, tpos, y, dtype).T)            # (gathering rows: the long-double gather is the cost)
    return (E[p] * E[q]).T


def gram_reference(kind, n, obs, tpos, y):
    """-> R = [A y]^T [A y] (long double), B = |A y|^T |A y| (fp64: it only scales the bound), b of the bound"""
    N = len(y)
    if N <= LD_ROWS:
        A = features(kind, n, obs, tpos, y)
        A64 = np.abs(A).astype(np.float64)
        FA, W = A.shape[1], 64                              # long-double products have no BLAS: the upper 64-column blocks, mirrored
        R = np.zeros((FA, FA), LD)
        for i in range(0, FA, W):
            for j in range(i, FA, W):
                R[i:i + W, j:j + W] = A[:, i:i + W].T @ A[:, j:j + W]
                if j > i:
                    R[j:j + W, i:i + W] = R[i:i + W, j:j + W].T
        return R, A64.T @ A64, 0
    FA = num_features(kind, n) + 1
    R, B = np.zeros((FA, FA), LD), np.zeros((FA, FA))
    slab = 32 * REF_BLOCK                                   # (features in long double a slab at a time, products a block at a time)
    for s0 in range(0, N, slab):
        S = features(kind, n, obs[s0:s0 + slab], tpos[s0:s0 + slab], y[s0:s0 + slab]).astype(np.float64)
        for s in range(0, S.shape[0], REF_BLOCK):
            A = S[s:s + REF_BLOCK]
            R += (A.T @ A).astype(LD)
        S = np.abs(S)
        B += S.T @ S
    return R, B, REF_BLOCK


def predict_reference(kind, n, obs, tpos, coef, rows=1 << 16):
    """-> ref (long double), S = sum_c |feat_c| |coef_c| per row (fp64)"""
    N = obs.shape[0]
    ref, S = np.zeros(N, LD), np.zeros(N)
    for s in range(0, N, rows):
        A = features(kind, n, obs[s:s + rows], tpos[s:s + rows])
        ref[s:s + rows] = A @ coef.astype(LD)
        S[s:s + rows] = np.abs(A).astype(np.float64) @ np.abs(coef)
    return ref, S


# ---------------------------------------------------------------- checks
def _ratio(err, bound):
    """err / bound, an exact zero allowed where the bound is zero; anything not finite is inf"""
    with np.errstate(all="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    r = np.asarray(r, np.float64)
    return np.where(np.isfinite(r), r, np.inf)


def gram_check(G, R, B, N, b, blk):
    """|G - R| <= (N + 32 + b) 2^-53 |A y|^T |A y| entry by entry: the forward bound of a dot product of N terms in any order, 32 for
    the at most 7 roundings of a device feature and the sum of the partials -> worst ratio, its index and tile, G == G.T, finite"""
    FA = R.shape[0]
    G = np.asarray(G, np.float64).reshape(FA, FA)
    ratio = _ratio(np.abs(G.astype(LD) - R), LD(N + 32 + b) * LD(U) * B.astype(LD))
    r, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return {"ratio": float(ratio[r, c]), "at": [int(r), int(c)], "tile": [int(r) // blk, int(c) // blk],
            "symmetric": bool(np.array_equal(G, G.T)), "finite": bool(np.all(np.isfinite(G)))}


def gram_ok(res):
    return res["ratio"] <= 1.0 and res["symmetric"] and res["finite"]


def predict_check(out, ref, S, F):
    """|out - ref| <= (F + 16) 2^-53 sum_c |feat_c| |coef_c| per row -> worst ratio and its row, finite"""
    out = np.asarray(out, np.float64)
    ratio = _ratio(np.abs(out.astype(LD) - ref), LD(F + 16) * LD(U) * S.astype(LD))
    i = int(np.argmax(ratio))
    return {"ratio": float(ratio[i]), "row": i, "finite": bool(np.all(np.isfinite(out)))}


def predict_ok(res):
    return res["ratio"] <= 1.0 and res["finite"]


def features_check(out, obs, tpos, n):
    """out: N x (n + 4) fp32.  Observation columns bit-equal to float32(clip(obs, -10, 10) / 10); time columns within 1 fp32 ulp of the
    long-double power rounded to fp32, and exact where tpos is 0 or 1000 -> counts of entries that miss"""
    N = obs.shape[0]
    out = np.ascontiguousarray(out, np.float32).reshape(N, n + 4)
    want = np.float32(np.clip(obs, -10, 10) / 10.0)
    obs_bad = int(np.sum(out[:, :n].view(np.int32) != want.view(np.int32)))
    tau = tpos.astype(LD) / LD(1000)
    ref = np.stack([(tau ** k).astype(np.float32) for k in range(1, 5)], axis=1)
    ulps = np.abs(out[:, n:].astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    ulps = np.where(np.isfinite(ulps), ulps, np.inf)
    sel = (tpos == 0) | (tpos == 1000)
    return {"obs_bad": obs_bad, "time_ulps": float(ulps.max()), "time_bad": int(np.sum(ulps > 1.0)),
            "exact_bad": int(np.sum(out[sel, n:] != ref[sel]))}


def features_ok(res):
    return res["obs_bad"] == 0 and res["time_bad"] == 0 and res["exact_bad"] == 0


# ---------------------------------------------------------------- the case lists of the GPU matrix
def _gram_cases():
    """(arm, kind, n, N, switches, Z or None where route_expect alone says it, y scale)"""
    out = []
    mf = [(2, 1), (2, 3), (2, 4), (2, 16), (2, 17), (1, 10), (1, 11), (1, 24), (0, 5)]
    out += [(MFMA, k, n, N, {}, None) for k, n in mf for N in SMALL_N]
    out += [(MFMA, k, n, N, {}, Z) for k, n in ((2, 17), (1, 24)) for N, Z in ((2048, 1), (2049, 2), (4097, 3))]
    out.append((MFMA, 1, 1, 2000000, {}, 512))             # chunk 3936: 509 ranges cover N, the last workgroups' ranges are empty
    bl = [(1, 25), (1, 64), (2, 18), (2, 21)]
    out += [(BLK, k, n, N, {}, None) for k, n in bl for N in SMALL_N + (2049, 4097)]
    out += [(BLK, 2, 64, N, {}, 1) for N in (1, 33)]
    out.append((BLK, 2, 18, 530000, {}, 256))              # chunk 2080: 255 ranges cover N, the last is empty
    big = (4096, 4097, 8193)
    out += [(FMA, k, n, N, FMA_ENV, None) for k, n in ((2, 3), (2, 10), (2, 17), (1, 58), (1, 59)) for N in SMALL_N + big]
    out += [(FMA, 1, n, N, {}, None) for n in (65, 126) for N in SMALL_N + big]
    out.append((FMA, 2, 65, 33, {}, 1))
    scales = (1.0, 1e-3, 37.0, 1e3, 0.25)
    return [c + (scales[i % len(scales)],) for i, c in enumerate(out)]


GRAM_CASES = _gram_cases()
PREDICT_N = (1, 32, 33, 64, 65, 128)


def predict_threads(n):
    """k_bl_predict's workgroup: one observation row per thread in 64 KiB of LDS"""
    return 256 if n <= 32 else 128 if n <= 64 else 64


PREDICT_CASES = [(k, n, N) for k in (1, 2) for n in PREDICT_N
                 for N in (1, predict_threads(n) - 1, predict_threads(n), predict_threads(n) + 1, 1000)]
PREDICT_CASES.append((1, 1, 8192 * 256 + 1))               # the grid is capped at 8192 workgroups: a second grid-stride pass
FEATURE_CASES = [(n, N) for n in (1, 17, 64) for N in (1, 255, 257)] + [(1, 419431)]     # 419 431 x 5 > 8192 x 256 elements


def case_name(arm, kind, n, N, env):
    return "%s kind %d n %d N %d%s" % (ARMS[arm], kind, n, N, " MJX_GRAM_FMA=1" if env else "")


def case_seed(kind, n, N):
    return 7000 + 1000 * kind + 13 * n + N % 997


# ---------------------------------------------------------------- NumPy emulations of the device's arithmetic (fp64)
DEFECTS = ("drop_last", "row32_twice", "tpos_off", "obs_fp32", "no_clip", "tau3", "mirror", "stale", "swap_y_const")


def device_features(kind, n, obs, tpos, y, defect=None):
    """[A y] as the kernels form it in fp64: clip, / 10, tau^k by repeated product, one multiply a column"""
    N = obs.shape[0]
    if defect == "obs_fp32":
        obs = obs.astype(np.float32).astype(np.float64)
    if defect == "tpos_off":
        tpos = tpos.copy(); tpos[-1] += 1
    E = np.zeros((N, n + 6))
    E[:, :n] = (obs if defect == "no_clip" else np.minimum(np.maximum(obs, -10.0), 10.0)) / 10.0
    E[:, n] = 1.0
    tau = tpos.astype(np.float64) / 1000.0
    t = tau.copy()
    for k in range(1, 5):
        E[:, n + k] = t
        t = t * tau
    if defect == "tau3":
        E[:, n + 4] = E[:, n + 3]
    E[:, n + 5] = y
    p, q = feat_pairs(kind, n)
    p, q = np.append(p, n + 5), np.append(q, n)
    A = E[:, p] * E[:, q]
    if defect == "swap_y_const":                            # (kinds 1 and 2: the constant column sits 5 before y)
        F = A.shape[1] - 1
        A[:, [F - 5, F]] = A[:, [F, F - 5]]
    return A


def emulate_gram(kind, n, obs, tpos, y, arm, Z, scratch, defect=None):
    """One mjx_bl_gram call: Z sample ranges (the matrix-core arms round a range up to 32 rows), chunks of 32 rows, products four
    rows at a time (one row at a time on the FMA arm), upper-triangle tiles into the partial-sum scratch, the reduce kernel's
    sum over z and mirror by tile.  `scratch` ((>= Z) x FA x FA) persists between calls as the device block does: the matrix-core
    block arm does not clear it, the other two do."""
    A = device_features(kind, n, obs, tpos, y, defect)
    N, FA = A.shape
    TS = TILE[arm]
    tiles = np.arange(FA) // TS
    upper = tiles[:, None] <= tiles[None, :]
    chunk = -(-obs.shape[0] // Z)
    if arm != FMA:
        chunk = (chunk + 31) & ~31
    part = scratch[:Z]
    if arm != BLK:
        part[:] = 0.0
    step = 1 if arm == FMA else 4
    for z in range(Z):
        idx = np.arange(min(N, z * chunk), min(N, (z + 1) * chunk))
        if defect == "drop_last":
            idx = idx[idx != N - 1]
        if defect == "row32_twice" and 32 in idx:
            idx = np.append(idx, 32)
        acc = np.zeros((FA, FA))
        for s0 in range(0, len(idx), 32):
            for k0 in range(s0, min(s0 + 32, len(idx)), step):
                rows = A[idx[k0:min(k0 + step, s0 + 32)]]
                acc = acc + rows.T @ rows
        if defect == "stale":
            part[z][upper] += acc[upper]
        else:
            part[z][upper] = acc[upper]
    S = np.zeros((FA, FA))
    for z in range(Z):
        S = S + part[z]
    if defect == "mirror":                                  # the lower tiles copied from their mirror tile without transposing
        r, c = np.meshgrid(np.arange(FA), np.arange(FA), indexing="ij")
        rr, cc = np.minimum((c // TS) * TS + r % TS, FA - 1), np.minimum((r // TS) * TS + c % TS, FA - 1)
        return np.where(upper, S, S[rr, cc])
    return np.where(upper, S, S.T)


def emulate_predict(kind, n, obs, tpos, coef, defect=None):
    """k_bl_predict: a += feature * coef, column by column in fp64"""
    A = device_features(kind, n, obs, tpos, np.zeros(obs.shape[0]))[:, :-1]
    if defect == "coef_shift":
        coef = np.roll(coef, 1)
    dt = np.float32 if defect == "fp32_acc" else np.float64
    a = np.zeros(obs.shape[0], dt)
    for c in range(A.shape[1]):
        a = (a + (A[:, c] * coef[c]).astype(dt)).astype(dt)
    return a.astype(np.float64)
