"""Cases, seeded recipe, conditions and a NumPy emulation for the path-reward matrix (csrc/path_reward.h, mjx_path_rewards), shared by
the GPU worker (tests/_path_reward_matrix_worker.py), the GPU tests (tests/test_gpu_path_reward_matrix.py), the CPU checks
(tests/test_path_reward_checks.py) and the yardstick generator (tests/golden/make_golden_path_reward_matrix.py).

The recipe is _mpc_learned_oracle.kernel_case's (nn.Linear-scaled weights, the same transform distributions) with three changes, all
seeded: the s' shift and scale of the reward transform are drawn on their own, dact and ract are separate, and wherever the mask flag
is on one dynamics out_scale entry is exactly 0 beside an out_shift of +-0.4, so that the mask moves the result.  The oracle is
_mpc_learned_oracle.ensemble_rewards (fp64, takes the flat transform vector as given).  Row sets are flat: obs (K, rows, n), shared
actions (rows, m), per-member actions (K, rows, m).

The emulation restates the kernel's data movement in fp32 with NumPy's own sums: both nets staged into ONE flat image with the
kernel's column maps and zero padding, the grid the host launches for a CU count, the tiles each wave walks with valid / vrow, the
lane's feature and action-slot selection, the store under valid && hi == 0.  It does not reproduce the MFMA summation order.  Memory
a wrong index would reach is emulated as what lies there: the rest of the image (then 0.5 beyond it), seeded foreign values behind a
shared action block, the next member's rows or the guard behind an output block."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _mpc_learned_oracle as L  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "path_reward_matrix.npz")
MARGIN = 3.0                 # tests/test_gpu_path_rewards.py's rule: the bar is 3 x the reference's own fp32 distance from fp64
GUARD = 64                   # NaN elements behind the last member's last row of every output block
CUS = 256                    # the MI355X's compute units: the count the CPU checks emulate
RELU, TANH = 0, 1
AFF, MASK, RES = 1, 2, 4
AXIS_ROWS = (165, 6)         # five tiles and a partial one; under one tile

# name -> n, m, dynamics hidden, dact, reward hidden, ract, dynamics flags, K, row sets, action modes, the instance <HB, NB, RB> and the
# image in KiB (both asserted from the arithmetic by the CPU checks), seed.  Why each is here: tests/test_gpu_path_reward_matrix.py.
def _c(n, m, dh, dact, rh, ract, flags, inst, kib, seed, K=2, rows=AXIS_ROWS, modes=("shared", "own")):
    return dict(n=n, m=m, dh=dh, dact=dact, rh=rh, ract=ract, flags=flags, K=K, rows=rows, modes=modes, inst=inst, kib=kib, seed=seed)


CASES = {
    # seeds: 7100 + the case's number, but a6 and a7 (a reward net that ends in ONE tanh unit): of twenty seeds each, many leave a member whose
    # rewards spread by under 5 % of the largest or hardly move with the residual; 7166 (spread 0.45, smallest move 1.4e-2 of max |r|) and
    # 7187 (0.69, 1.4e-2) have margin -- chosen from the fp64 oracle alone (tests/test_path_reward_checks.py asserts the conditions)
    "a1": _c(6, 2, (64, 64), RELU, (100, 100), RELU, 7, (2, 1, 4), 113.3, 7101),
    "a2": _c(11, 17, (64, 32), RELU, (128, 7), TANH, 5, (2, 1, 4), 85.5, 7102),
    "a3": _c(11, 25, (32, 64), TANH, (5, 128), RELU, 1, (2, 1, 4), 68.0, 7103),
    "a4": _c(39, 28, (96, 32), RELU, (64, 128), RELU, 7, (3, 2, 4), 158.5, 7104),
    "a5": _c(8, 8, (32, 32), TANH, (128, 128), TANH, 3, (1, 1, 4), 94.1, 7105),
    "a6": _c(1, 1, (32, 32), RELU, (1, 1), TANH, 7, (1, 1, 4), 21.0, 7166),
    "a7": _c(17, 6, (128, 128), RELU, (64, 1), TANH, 7, (4, 1, 2), 126.7, 7187),
    "a8": _c(32, 8, (96, 96), TANH, (33, 32), RELU, 0, (3, 1, 4), 96.6, 7108),
    "a9": _c(33, 1, (96, 96), RELU, (64, 65), RELU, 7, (3, 2, 4), 134.3, 7109),
    "a10": _c(64, 32, (64, 64), RELU, (64, 64), RELU, 7, (2, 2, 4), 121.3, 7110),
    "g1": _c(6, 2, (64, 64), RELU, (100, 100), RELU, 7, (2, 1, 4), 113.3, 7111, K=64, rows=(1200,)),
    "g2": _c(6, 2, (32, 32), RELU, (36, 72), TANH, 7, (1, 1, 4), 46.1, 7112, K=300, rows=(300,), modes=("own",)),
    "g3": _c(6, 2, (32, 32), RELU, (32, 32), RELU, 7, (1, 1, 4), 21.0, 7113, K=64, rows=(16400,), modes=("shared",)),
}
ORDER = sorted(CASES, key=lambda c: (c[0], int(c[1:])))
AXIS = [c for c in ORDER if c[0] == "a"]
GEOM = [c for c in ORDER if c[0] == "g"]
SUBSET_CASES = ("g3",)       # compared with fp64 on subset_rows only (rows are independent: the oracle runs on the subset alone)
# what the geometry table states for 256 CUs: (workgroups per member, most and fewest tiles of a wave that owns any, rows of the last tile)
WALK_AT_256 = {"g1": (4, 3, 2, 16), "g2": (1, 3, 2, 12), "g3": (4, 33, 32, 16)}


def sizes(name):
    c = CASES[name]
    return (c["n"] + c["m"],) + c["dh"] + (c["n"],), (2 * c["n"] + c["m"],) + c["rh"] + (1,)


def masked_column(name):
    c = CASES[name]
    return c["n"] // 2 if c["flags"] & MASK else None


def case(name):
    """seeded members and inputs -> (mem as ensemble_rewards takes it, {rows: (obs, shared actions or None, per-member or None)}), fp32"""
    c = CASES[name]
    n, m, K = c["n"], c["m"], c["K"]
    rng = np.random.RandomState(c["seed"])
    ds, rs = sizes(name)
    mem = dict(dyn_thetas=[], dyn_sizes=ds, dyn_trs=[], dact=c["dact"], dflags=c["flags"], rew_thetas=[], rew_sizes=rs, rew_trs=[], ract=c["ract"])
    col = masked_column(name)
    for _ in range(K):
        mem["dyn_thetas"].append(L._torch_like(rng, ds))
        mem["rew_thetas"].append(L._torch_like(rng, rs))
        dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
        sign = 1.0 if rng.rand() < 0.5 else -1.0
        if col is not None:
            dtr[2 * (n + m) + n + col] = 0.0
            dtr[2 * (n + m) + col] = 0.4 * sign
        s_sh, s_sc, a_sh, a_sc = rng.randn(n) * 0.2, rng.rand(n) + 0.6, rng.randn(m) * 0.2, rng.rand(m) + 0.6
        p_sh, p_sc = rng.randn(n) * 0.2, rng.rand(n) + 0.6                       # s' on its own
        rtr = np.concatenate([s_sh, a_sh, p_sh, s_sc, a_sc, p_sc, [rng.randn() * 0.5], [rng.rand() + 0.5]])
        mem["dyn_trs"].append(dtr.astype(np.float32))
        mem["rew_trs"].append(rtr.astype(np.float32))
    data = {}
    for rows in c["rows"]:
        obs = rng.standard_normal((K, rows, n)).astype(np.float32)
        shared = rng.standard_normal((rows, m)).astype(np.float32) if "shared" in c["modes"] else None
        own = rng.standard_normal((K, rows, m)).astype(np.float32) if "own" in c["modes"] else None
        data[rows] = (obs, shared, own)
    return mem, data


_CASE, _REF = {}, {}


def cached_case(name):
    if name not in _CASE:
        _CASE[name] = case(name)
    return _CASE[name]


def subset_rows(rows):
    """the rows of every member that meet fp64 in a subset case: the first tile, the last two tiles, every 64th row"""
    tiles = -(-rows // 32)
    return np.unique(np.concatenate([np.arange(32), np.arange(32 * (tiles - 2), rows), np.arange(0, rows, 64)]))


def compared_rows(name, rows):
    return subset_rows(rows) if name in SUBSET_CASES else np.arange(rows)


def oracle(name, mem, rows, mode):
    """fp64 rewards (K, compared rows) of a case under `mem` (the case's own, or a variant of it)"""
    obs, shared, own = cached_case(name)[1][rows]
    idx = compared_rows(name, rows)
    act = shared[idx] if mode == "shared" else own[:, idx]
    return L.ensemble_rewards(obs[:, idx], act, mem)


def reference(name):
    """{(rows, mode): fp64 rewards}, formed once and left unchanged"""
    if name not in _REF:
        mem = cached_case(name)[0]
        _REF[name] = {(rows, mode): oracle(name, mem, rows, mode) for rows in CASES[name]["rows"] for mode in CASES[name]["modes"]}
    return _REF[name]


def variant(mem, what):
    """the members a defective kernel would in effect compute: 'sp_as_s', 'ract_dact', or a flag bit to clear"""
    if what == "sp_as_s":
        n = mem["dyn_sizes"][-1]
        rin = mem["rew_sizes"][0]
        trs = []
        for t in mem["rew_trs"]:
            t = t.copy()
            t[rin - n:rin] = t[:n]
            t[2 * rin - n:2 * rin] = t[rin:rin + n]
            trs.append(t)
        return dict(mem, rew_trs=trs)
    if what == "ract_dact":
        return dict(mem, ract=mem["dact"])
    return dict(mem, dflags=mem["dflags"] & ~int(what))


def kref(name):
    return float(np.load(FIXTURE)["kref_" + name])


# ---- the host's launch arithmetic (path_rewards and path_rew_shape in model_host.h)
def instance(name):
    c = CASES[name]
    HB = max(c["dh"]) // 32
    return HB, (c["n"] + 31) // 32, 2 if HB == 4 else 4


def pad8(v):
    return (v + 7) & ~7


def layout(name):
    """offsets of the image's parts in floats, in the kernel's order, and its size"""
    c = CASES[name]
    HB, NB, RB = instance(name)
    n, m, (g1, g2) = c["n"], c["m"], c["rh"]
    HW, NS, n8, m8 = 32 * HB, 32 * NB, pad8(n), pad8(m)
    K1 = n8 + m8
    K1r, R1, R2 = K1 + n8, 32 * ((g1 + 31) // 32), 32 * ((g2 + 31) // 32)
    parts = [("W1s", HW * (K1 + 4)), ("W2s", HW * (HW + 4)), ("W3s", NS * (HW + 4)), ("b1s", HW), ("b2s", HW), ("b3s", NS), ("ish", K1), ("irs", K1),
             ("osc", NS), ("osh", NS), ("msk", NS), ("V1s", R1 * (K1r + 4)), ("V2s", R2 * (R1 + 4)), ("c1s", R1), ("c2s", R2), ("w3s", R2),
             ("rsh", K1r), ("rrs", K1r), ("hd", 4)]
    off, o = {}, 0
    for p, sz in parts:
        off[p] = o
        o += sz
    plan = HW * (K1 + 4) + HW * (HW + 4) + NS * (HW + 4) + 2 * HW + NS + 2 * K1 + 3 * NS             # plan_lds_floats
    rew = R1 * (K1r + 4) + R2 * (R1 + 4) + R1 + 2 * R2 + 2 * K1r + 4                                 # path_rew_lds_floats
    assert o == plan + rew
    return off, o, dict(HB=HB, NB=NB, RB=RB, HW=HW, NS=NS, n8=n8, m8=m8, K1=K1, K1r=K1r, R1=R1, R2=R2, g1b=R1 // 32, g2b=R2 // 32)


def image_kib(name):
    return 4 * layout(name)[1] / 1024.0


def walk(rows, K, cus, stride_groups=4, once=False):
    """the grid mjx_path_rewards launches and the tiles each of its waves owns: wave w of a member's 4 x grid waves starts at tile w
    and steps by 4 x grid -> dict(grid, cap, groups, tiles, most, fewest (over the waves that own any), last_rows, owned: per wave)"""
    groups, cap = (rows + 127) // 128, (cus + K - 1) // K
    grid = min(groups, cap)
    tiles = (rows + 31) // 32
    owned = []
    for w in range(4 * grid):
        t = list(range(w, tiles, stride_groups * grid))
        owned.append(t[:1] if once else t)
    counts = [len(t) for t in owned if t]
    return dict(grid=grid, cap=cap, groups=groups, tiles=tiles, most=max(counts), fewest=min(counts), last_rows=rows - 32 * (tiles - 1), owned=owned)


def walk_numbers(w):
    return [w["grid"], w["most"], w["fewest"], w["last_rows"]]


# ---- the emulation
DEFECTS = ("once", "stride1", "sp_under_s", "ract_from_dact", "drop_q2", "own_as_shared", "shared_as_own", "v2_stride", "guards_rb",
           "ignore_mask", "ignore_affine", "ignore_residual", "flags_on", "store_no_valid")
TAIL = 40000                 # floats a wrong stride or block guard can reach beyond the image
TAIL_VALUE = 0.5


def _act(x, code):
    return np.tanh(x) if code == TANH else np.maximum(x, np.float32(0))


def stage(name, mem, k):
    """member k's nets in the kernel's padded image (one flat fp32 array, TAIL floats of TAIL_VALUE behind it)"""
    c = CASES[name]
    off, total, d = layout(name)
    n, m, (h1, h2), (g1, g2) = c["n"], c["m"], c["dh"], c["rh"]
    din, rin = n + m, 2 * n + m
    HW, NS, n8, K1, K1r, R1, R2 = d["HW"], d["NS"], d["n8"], d["K1"], d["K1r"], d["R1"], d["R2"]
    img = np.zeros(total + TAIL, np.float32)
    img[total:] = TAIL_VALUE
    P, tr, Q, qtr = mem["dyn_thetas"][k], mem["dyn_trs"][k], mem["rew_thetas"][k], mem["rew_trs"][k]
    oB1 = h1 * din; oW2 = oB1 + h1; oB2 = oW2 + h2 * h1; oW3 = oB2 + h2; oB3 = oW3 + n * h2
    qB1 = g1 * rin; qW2 = qB1 + g1; qB2 = qW2 + g2 * g1; qW3 = qB2 + g2; qB3 = qW3 + g2
    cc = np.arange(K1r)
    # f = c < n8 ? (c < n ? c : -1) : c < K1 ? (c - n8 < m ? n + c - n8 : -1) : (c - K1 < n ? din + c - K1 : -1)
    f = np.where(cc < n8, np.where(cc < n, cc, -1), np.where(cc < K1, np.where(cc - n8 < m, n + cc - n8, -1), np.where(cc - K1 < n, din + cc - K1, -1)))
    fd, fr = f[:K1], f
    view = lambda p, r, s: img[off[p]:off[p] + r * s].reshape(r, s)
    W1s, W2s, W3s = view("W1s", HW, K1 + 4), view("W2s", HW, HW + 4), view("W3s", NS, HW + 4)
    W1s[:h1, np.nonzero(fd >= 0)[0]] = P[:oB1].reshape(h1, din)[:, fd[fd >= 0]]
    W2s[:h2, :h1] = P[oW2:oB2].reshape(h2, h1)
    W3s[:n, :h2] = P[oW3:oB3].reshape(n, h2)
    img[off["b1s"]:off["b1s"] + h1] = P[oB1:oW2]
    img[off["b2s"]:off["b2s"] + h2] = P[oB2:oW3]
    img[off["b3s"]:off["b3s"] + n] = P[oB3:oB3 + n]
    sc = tr[2 * din + n:2 * din + 2 * n]
    img[off["osc"]:off["osc"] + n] = sc + np.float32(1e-8)
    img[off["osh"]:off["osh"] + n] = tr[2 * din:2 * din + n]
    img[off["msk"]:off["msk"] + n] = (sc >= np.float32(1e-8)).astype(np.float32)
    img[off["ish"]:off["ish"] + K1] = np.where(fd >= 0, tr[np.maximum(fd, 0)], np.float32(0))
    img[off["irs"]:off["irs"] + K1] = np.where(fd >= 0, tr[din + np.maximum(fd, 0)] + np.float32(1e-8), np.float32(1))
    V1s, V2s = view("V1s", R1, K1r + 4), view("V2s", R2, R1 + 4)
    V1s[:g1, np.nonzero(fr >= 0)[0]] = Q[:qB1].reshape(g1, rin)[:, fr[fr >= 0]]
    V2s[:g2, :g1] = Q[qW2:qB2].reshape(g2, g1)
    img[off["c1s"]:off["c1s"] + g1] = Q[qB1:qW2]
    img[off["c2s"]:off["c2s"] + g2] = Q[qB2:qW3]
    img[off["w3s"]:off["w3s"] + g2] = Q[qW3:qB3]
    img[off["rsh"]:off["rsh"] + K1r] = np.where(fr >= 0, qtr[np.maximum(fr, 0)], np.float32(0))
    img[off["rrs"]:off["rrs"] + K1r] = np.where(fr >= 0, qtr[rin + np.maximum(fr, 0)] + np.float32(1e-8), np.float32(1))
    img[off["hd"]:off["hd"] + 4] = [Q[qB3], qtr[2 * rin + 1] + np.float32(1e-8), qtr[2 * rin], 0.0]
    return img


def _strided(img, start, nrows, ncols, stride):
    assert start + (nrows - 1) * stride + ncols <= img.size          # (a wrong stride stays inside the image and its tail)
    return np.lib.stride_tricks.as_strided(img[start:], shape=(nrows, ncols), strides=(4 * stride, 4), writeable=False)


def new_out(K, rows, dtype=np.float32):
    return np.full(K * rows + GUARD, np.nan, dtype)


def emulate(name, mem, obs, act, cus=CUS, defect=None):
    """route 1 as the kernel moves its data -> (r32 buffer, r64 buffer, the walk its waves really took).  act: (rows, m) shared
    (stride 0) or (K, rows, m)"""
    assert defect is None or defect in DEFECTS
    c = CASES[name]
    off, total, d = layout(name)
    n, m, K = c["n"], c["m"], c["K"]
    rows = obs.shape[1]
    HW, NS, n8, m8, K1, K1r, R1, RB = d["HW"], d["NS"], d["n8"], d["m8"], d["K1"], d["K1r"], d["R1"], d["RB"]
    flags = c["flags"]
    flags = 7 if defect == "flags_on" else flags & ~{"ignore_mask": MASK, "ignore_affine": AFF, "ignore_residual": RES}.get(defect, 0)
    dact, ract = mem["dact"], mem["dact"] if defect == "ract_from_dact" else mem["ract"]
    stride = 0 if act.ndim == 2 else rows * m
    if defect == "own_as_shared" and act.ndim == 3:
        stride = 0
    if defect == "shared_as_own" and act.ndim == 2:
        stride = rows * m
    act_flat = np.concatenate([act.ravel(), np.random.RandomState(5).standard_normal(K * rows * m).astype(np.float32)])   # (foreign memory behind the block)
    w = walk(rows, K, cus, stride_groups=1 if defect == "stride1" else 4, once=defect == "once")
    tiles = np.unique(np.concatenate([np.asarray(t, np.int64) for t in w["owned"]]))
    row = (tiles[:, None] * 32 + np.arange(32)[None, :]).ravel()
    valid = row < rows
    vrow = np.where(valid, row, 0)
    NQA = m8 // 8
    fa = np.arange(32)                                       # slot (q, hi, tt) is action f = 8 q + 4 hi + tt
    live = (fa // 8 < NQA) & (fa < m)
    nb1 = RB if defect == "guards_rb" else d["g1b"]
    nb2 = RB if defect == "guards_rb" else d["g2b"]
    T2 = (32 * RB if defect == "v2_stride" else R1) + 4
    out32, out64 = new_out(K, rows), new_out(K, rows, np.float64)
    store = np.ones_like(valid) if defect == "store_no_valid" else valid
    g = lambda img, p, cnt: img[off[p]:off[p] + cnt]
    for k in range(K):
        img = stage(name, mem, k)
        s = np.zeros((len(row), NS), np.float32)
        s[:, :n] = obs[k][vrow] * valid[:, None]
        an = np.where(valid[:, None] & live[None, :], act_flat[k * stride + vrow[:, None] * m + np.where(live, fa, 0)[None, :]], np.float32(0))
        W1 = _strided(img, off["W1s"], HW, K1, K1 + 4)
        x = np.concatenate([s[:, :n8], an[:, :m8]], 1)
        x = (x - g(img, "ish", K1)) / g(img, "irs", K1)
        if defect == "drop_q2":
            x[:, n8 + 16:] = 0                               # (the k-steps of slot groups q >= 2 never issued)
        h = _act(x @ W1.T + g(img, "b1s", HW), dact)
        h = _act(h @ _strided(img, off["W2s"], HW, HW, HW + 4).T + g(img, "b2s", HW), dact)
        z = h @ _strided(img, off["W3s"], NS, HW, HW + 4).T + g(img, "b3s", NS)
        if flags & AFF:
            z = z * g(img, "osc", NS) + g(img, "osh", NS)
        if flags & MASK:
            z = z * g(img, "msk", NS)
        if flags & RES:
            z = z + s
        sp = z.astype(np.float32)
        rsh, rrs = g(img, "rsh", K1r), g(img, "rrs", K1r)
        po = 0 if defect == "sp_under_s" else K1             # (part ? K1 : 0)
        xr = np.concatenate([(s[:, :n8] - rsh[:n8]) / rrs[:n8], (an[:, :m8] - rsh[n8:K1]) / rrs[n8:K1],
                             (sp[:, :n8] - rsh[po:po + n8]) / rrs[po:po + n8]], 1)
        if defect == "drop_q2":
            xr[:, n8 + 16:K1] = 0
        h = _act(xr @ _strided(img, off["V1s"], 32 * nb1, K1r, K1r + 4).T + g(img, "c1s", 32 * nb1), ract)
        h = _act(h @ _strided(img, off["V2s"], 32 * nb2, 32 * nb1, T2).T + g(img, "c2s", 32 * nb2), ract)
        hd = g(img, "hd", 4)
        r = ((h @ g(img, "w3s", 32 * nb2) + hd[0]) * hd[1] + hd[2]).astype(np.float32)
        out32[k * rows + row[store]] = r[store]
        out64[k * rows + row[store]] = r[store].astype(np.float64)
    return out32, out64, w


def plain_fp32(name, mem, obs, act):
    """a stand-in for route 0 in the CPU checks: the same operation as a plain fp32 chain with every layer's sum taken in the reverse
    order (another kernel, another summation order), every row -> (r32 buffer, r64 buffer)"""
    c = CASES[name]
    n, K = c["n"], c["K"]
    rows = obs.shape[1]
    ds, rs = sizes(name)
    out32 = new_out(K, rows)
    f32 = np.float32

    def net(theta, sz, tr, x, act_code, flags):
        din, dout = sz[0], sz[-1]
        h = (x - tr[:din]) / (tr[din:2 * din] + f32(1e-8))
        o = 0
        for i in range(len(sz) - 1):
            W = theta[o:o + sz[i + 1] * sz[i]].reshape(sz[i + 1], sz[i]); o += W.size
            b = theta[o:o + sz[i + 1]]; o += sz[i + 1]
            h = np.ascontiguousarray(h[:, ::-1]) @ np.ascontiguousarray(W[:, ::-1]).T + b
            if i < len(sz) - 2:
                h = _act(h, act_code)
        osh, osc = tr[2 * din:2 * din + dout], tr[2 * din + dout:]
        if flags & AFF:
            h = h * (osc + f32(1e-8)) + osh
        if flags & MASK:
            h = h * (osc >= f32(1e-8))
        if flags & RES:
            h = h + x[:, :dout]
        return h.astype(f32)

    for k in range(K):
        x = np.concatenate([obs[k], act if act.ndim == 2 else act[k]], 1)
        sp = net(mem["dyn_thetas"][k], ds, mem["dyn_trs"][k], x, mem["dact"], mem["dflags"])
        out32[k * rows:(k + 1) * rows] = net(mem["rew_thetas"][k], rs, mem["rew_trs"][k], np.concatenate([x, sp], 1), mem["ract"], AFF)[:, 0]
    return out32, out32.astype(np.float64)


# ---- the measurements and the checks, the same for the device and for the emulation
def _worse(a, b):
    """the larger error; NaN (an element that was never written) stays NaN"""
    return float("nan") if (a != a or b != b) else float(max(a, b))


def measure(name, runner, cus):
    """runner(route, name, mem, obs, act) -> (r32 buffer, r64 buffer, route taken or None), both K x rows + GUARD long and prefilled
    with NaN.  -> the record the tests read: errors against fp64 per route and between the routes (rel_max over all members' compared
    rows, the largest over row sets and action modes), unwritten and guard counts, row sets of 32 rows or more on which the routes
    agree to the bit, route_out, r64 against r32 widened, and the walk"""
    c = CASES[name]
    mem, data = cached_case(name)
    ref = reference(name)
    K = c["K"]
    rec = dict(err={"1": 0.0, "0": 0.0}, routes=0.0, unwritten=0, guard=0, same_bits=[], route_out_ok=True, widened=True, runs=[], walk={})
    for rows in c["rows"]:
        obs, shared, own = data[rows]
        idx = compared_rows(name, rows)
        rec["walk"][str(rows)] = walk_numbers(walk(rows, K, cus))
        for mode in c["modes"]:
            act = shared if mode == "shared" else own
            got = {}
            for route in (1, 0):
                b32, b64, taken = runner(route, name, mem, obs, act)
                assert b32.shape == (K * rows + GUARD,) and b64.shape == b32.shape
                rec["unwritten"] += int(np.isnan(b32[:K * rows]).sum() + np.isnan(b64[:K * rows]).sum())
                rec["guard"] += int((~np.isnan(b32[K * rows:])).sum() + (~np.isnan(b64[K * rows:])).sum())
                rec["widened"] = bool(rec["widened"] and np.array_equal(b64, b32.astype(np.float64), equal_nan=True))
                rec["route_out_ok"] = bool(rec["route_out_ok"] and taken in (None, route))
                got[route] = b32[:K * rows].reshape(K, rows)
                e = L.rel_max(got[route][:, idx], ref[(rows, mode)])
                rec["runs"].append("%s rows %d %s route %d: %.3e" % (name, rows, mode, route, e))
                rec["err"][str(route)] = _worse(rec["err"][str(route)], e)
            rec["routes"] = _worse(rec["routes"], L.rel_max(got[1], got[0]))
            if rows >= 32 and np.array_equal(got[1], got[0]):
                rec["same_bits"].append("%s %d %s" % (name, rows, mode))
    return rec


def checks(name, rec, yard, walked=None):
    """what tests/test_gpu_path_reward_matrix.py asserts of a record -> {check: passed}.  walked: the walk an emulation really took"""
    bar = MARGIN * yard
    out = dict(mfma=rec["err"]["1"] < bar, generic=rec["err"]["0"] < bar, routes=rec["routes"] < bar,
               written=rec["unwritten"] == 0 and rec["guard"] == 0, own_kernel=rec["same_bits"] == [], route_out=rec["route_out_ok"] is True,
               widened=rec["widened"] is True)
    if name in GEOM:
        out["walk"] = all(v[2] >= 2 for v in rec["walk"].values())
    if walked is not None:
        out["walk"] = out.get("walk", True) and all(walk_numbers(walked[r]) == rec["walk"][r] for r in rec["walk"])
    return out
