"""Cases, seeded recipes, measures, check functions and NumPy emulations for the plan matrix (csrc/plan.h: k_plan_rollout<HB, NB> behind
mjx_plan_rollout, and k_plan_disagree / k_plan_returns / k_plan_softmax / k_plan_sequence behind mjx_plan_score), shared by the GPU worker
(tests/_plan_matrix_worker.py), the GPU tests (tests/test_gpu_plan_matrix.py), the CPU checks (tests/test_plan_checks.py) and the
yardstick generator (tests/golden/make_golden_plan_matrix.py).  CPU only.

Rollout.  The recipe is _mpc_learned_oracle.kernel_case's and _refine_oracle.kernel_case's (nn.Linear-scaled weights, the same transform
distributions), with one out_scale entry exactly 0 beside an out_shift of +-0.4 in every case whatever its flags (column n // 2; 36 on
the n = 40 nets, in the second state block), so that both the presence and the absence of the mask flag show in the values.  The one
exception is n = 1 (r2, h2): the masked column would be the only one, every stored state would be s0 on both routes, and neither the
kernel's arithmetic nor the routes' different bits could show; those nets keep a plain out_scale.  The oracle is _dyn_oracle.rollout_next
per step (fp64 from the STORED state and action before it) and _mpc_oracle.rollout free-running.  The error of a block of states is
taken per state column of each member, relative to that column's largest |reference| over the compared rows, and reported as the
largest over the columns (col_err).  The column with the zero out_scale is left out of it wherever the mask flag is on: there it is
asserted exactly (0 of either sign under flags 3, s0's column under flags 7).

The rollout emulation restates the kernel's data movement in fp32 with NumPy's own sums: the staged image with feat()'s column map and
the zero padding to HW and NS, the tiles the launched waves own with valid / vrow, the lane's action slots and state registers, the
tail's read of the state before it is written, the store under valid.  It does not reproduce the MFMA summation order.

Scoring.  The reference is the reference's expressions (model_learning_mpc.py:70-74, 85-99) in np.longdouble (score_ld); the bounds are
forward bounds of the kernels' fixed summation orders (score_bounds; derived in tests/test_gpu_plan_matrix.py); the emulation restates
the four kernels in fp64 with exactly their orders (emu_score)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _dyn_oracle as O  # noqa: E402
import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "plan_matrix.npz")
MARGIN = 3.0                 # tests/test_gpu_path_rewards.py's rule: the bar is 3 x the reference's own fp32 distance from fp64
GUARD = 64                   # NaN elements behind the last element of every output block
RELU, TANH = 0, 1
AFF, MASK, RES = 1, 2, 4
AXIS_ROWS = (165, 6)         # one workgroup plus a second with one full tile and one of five rows; under one tile
BOTH = ("one", "rows")       # s0 as one state (s0_stride 0) and as (N, n)
FLOOR_TOP, CEIL_STATE = 1e-3, 1e3


# name -> n, m, hidden, activation, flags, the instance <HB, NB> (asserted from the host arithmetic by the CPU checks), seed, K, H, row
# counts, s0 modes.  Cases that share a seed and K share their nets (f3 with r3, f9 with r9, h2 with r2, g3 with r10).  Why each is here: tests/test_gpu_plan_matrix.py.
def _c(n, m, dh, act, flags, inst, seed, K=2, H=5, rows=AXIS_ROWS, s0=BOTH):
    return dict(n=n, m=m, dh=dh, act=act, flags=flags, inst=inst, seed=seed, K=K, H=H, rows=rows, s0=s0)


CASES = {
    "r1": _c(8, 8, (32, 32), TANH, 3, (1, 1), 7301),
    "r2": _c(1, 1, (32, 32), RELU, 7, (1, 1), 7302),
    "r3": _c(11, 17, (32, 64), RELU, 5, (2, 1), 7303),
    "r4": _c(11, 25, (64, 32), TANH, 1, (2, 1), 7304),
    "r5": _c(32, 8, (96, 96), TANH, 0, (3, 1), 7305),
    "r6": _c(17, 6, (32, 128), RELU, 7, (4, 1), 7306),
    "r7": _c(33, 1, (32, 32), RELU, 7, (1, 2), 7307),
    "r8": _c(39, 28, (64, 96), RELU, 7, (3, 2), 7308),
    "r9": _c(64, 32, (128, 128), RELU, 7, (4, 2), 7309),
    "r10": _c(40, 5, (64, 64), TANH, 3, (2, 2), 7310),
    "f3": _c(11, 17, (32, 64), RELU, 5, (2, 1), 7303, H=16, rows=(33,), s0=("rows",)),           # r3's nets, free-running over 16 steps
    "f9": _c(64, 32, (128, 128), RELU, 7, (4, 2), 7309, H=16, rows=(33,), s0=("rows",)),         # r9's nets
    "h2": _c(1, 1, (32, 32), RELU, 7, (1, 1), 7302, H=1),                                        # r2's nets at H = 1: only s0 is stored
    "g1": _c(11, 17, (32, 64), RELU, 5, (2, 1), 7311, K=5, H=3, rows=(417,), s0=("rows",)),      # r3's shape, five members
    "g2": _c(33, 1, (32, 32), RELU, 7, (1, 2), 7307, K=1, H=1, rows=(1,)),                       # r7's shape
    "g3": _c(40, 5, (64, 64), TANH, 3, (2, 2), 7310, H=3, rows=(31, 32, 33, 128, 129), s0=("one",)),   # r10's nets
}
ORDER = sorted(CASES, key=lambda c: (c[0], int(c[1:])))
STEPPED = [c for c in ORDER if CASES[c]["H"] > 1]            # the cases that store a computed state: they have yardsticks


def sizes(name):
    c = CASES[name]
    return (c["n"] + c["m"],) + c["dh"] + (c["n"],)


def zero_column(name):
    """the column whose out_scale is exactly 0 (None at n = 1)"""
    n = CASES[name]["n"]
    return None if n == 1 else (36 if n == 40 else n // 2)


def compared_columns(name):
    c = CASES[name]
    z = zero_column(name)
    return np.array([j for j in range(c["n"]) if not (c["flags"] & MASK and j == z)])


def case(name):
    """seeded members and inputs -> (mem: dict(thetas, trs, sizes, act, flags), {(rows, s0 mode): (s0, actions (rows, H, m))}), fp32"""
    c = CASES[name]
    n, m, K, H = c["n"], c["m"], c["K"], c["H"]
    rng = np.random.RandomState(c["seed"])
    ds = sizes(name)
    mem = dict(thetas=[], trs=[], sizes=ds, act=c["act"], flags=c["flags"])
    col = zero_column(name)
    for _ in range(K):
        mem["thetas"].append(L._torch_like(rng, ds))
        dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
        sign = 1.0 if rng.rand() < 0.5 else -1.0
        if col is not None:
            dtr[2 * (n + m) + n + col] = 0.0
            dtr[2 * (n + m) + col] = 0.4 * sign
        mem["trs"].append(dtr.astype(np.float32))
    data = {}
    for rows in c["rows"]:
        for mode in c["s0"]:
            drng = np.random.RandomState(c["seed"] * 31 + 1000 * H + 7 * rows + (mode == "rows"))
            s0 = (drng.randn(rows, n) if mode == "rows" else drng.randn(n)).astype(np.float32)
            data[(rows, mode)] = (s0, drng.randn(rows, H, m).astype(np.float32))
    return mem, data


_CASE, _FREE = {}, {}


def cached_case(name):
    if name not in _CASE:
        _CASE[name] = case(name)
    return _CASE[name]


def s0_rows(s0, N):
    return np.tile(s0, (N, 1)) if s0.ndim == 1 else s0


def free_reference(name, key):
    """the free-running fp64 rollout (K, N, H, n) of a run, formed once and left unchanged"""
    if (name, key) not in _FREE:
        mem, data = cached_case(name)
        s0, actions = data[key]
        _FREE[(name, key)] = M.rollout(s0, actions, mem["thetas"], mem["sizes"], mem["trs"], mem["act"], mem["flags"])
    return _FREE[(name, key)]


# ---- the measures
def col_err(got, ref, cols):
    """blocks (..., n) -> (the largest over `cols` of max |got - ref| / max |ref|, both over the rows; the smallest such max |ref|).
    NaN (an element never written) stays NaN"""
    g = np.asarray(got, np.float64)[..., cols].reshape(-1, len(cols))
    r = np.asarray(ref, np.float64)[..., cols].reshape(-1, len(cols))
    top = np.max(np.abs(r), 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.max(np.abs(g - r), 0) / top
    return float(np.max(q)), float(np.min(top))


def step_reference(obs_k, actions, mem, k):
    """one fp64 step from every stored state and action of member k but the last: (N, H - 1, n), the reference of obs_k[:, 1:]"""
    N, H, n = obs_k.shape
    ref = O.rollout_next(obs_k[:, :-1].reshape(N * (H - 1), n), actions[:, :-1].reshape(N * (H - 1), -1), np.float32(mem["thetas"][k]),
                         list(mem["sizes"]), np.float32(mem["trs"][k]), mem["act"], mem["flags"])
    return ref.reshape(N, H - 1, n)


def step_error(name, obs, actions, mem):
    """obs (K, N, H, n) -> (the per-column one-step error, the largest over members; the smallest column top)"""
    cols = compared_columns(name)
    out = [col_err(obs[k][:, 1:], step_reference(obs[k], actions, mem, k), cols) for k in range(obs.shape[0])]
    return _worst([e for e, _ in out]), min(t for _, t in out)


def free_error(name, obs, ref):
    cols = compared_columns(name)
    out = [col_err(obs[k][:, 1:], ref[k][:, 1:], cols) for k in range(obs.shape[0])]
    return _worst([e for e, _ in out]), min(t for _, t in out)


def _worst(v):
    v = [float(x) for x in v]
    return float("nan") if any(x != x for x in v) else max(v + [0.0])


def yard(name):
    G = np.load(FIXTURE)
    return float(G["pstep_" + name]), float(G["pfree_" + name])


# ---- the host's launch arithmetic (plan_shape in model_host.h, plan_lds_floats in mfma_chain.h)
def pad8(v):
    return (v + 7) & ~7


def instance(name):
    c = CASES[name]
    return max(c["dh"]) // 32, (c["n"] + 31) // 32


def layout(name):
    c = CASES[name]
    HB, NB = instance(name)
    n8, m8 = pad8(c["n"]), pad8(c["m"])
    return dict(HB=HB, NB=NB, HW=32 * HB, NS=32 * NB, n8=n8, m8=m8, K1=n8 + m8)


def plan_lds_floats(name):
    d = layout(name)
    HW, NS, K1 = d["HW"], d["NS"], d["K1"]
    return HW * (K1 + 4) + HW * (HW + 4) + NS * (HW + 4) + 2 * HW + NS + 2 * K1 + 3 * NS


def route(name):
    """plan_shape as arithmetic: 1 where k_plan_rollout serves the case"""
    c = CASES[name]
    h1, h2 = c["dh"]
    ok = h1 % 32 == 0 and h2 % 32 == 0 and h1 <= 128 and h2 <= 128 and c["n"] <= 64 and pad8(c["m"]) <= 32
    return int(ok and 4 * plan_lds_floats(name) <= 160 * 1024)


# ---- the rollout emulation
DEFECTS = ("w2_stride", "act_col_n", "drop_q3", "stale_actions", "residual_overwritten", "mask_skip_b1", "affine_forced", "s0_stride",
           "member0_tr", "store_no_valid", "tile_unowned")
TAIL, TAIL_VALUE = 20000, 0.5          # what a wrong stride reads behind a member's parameters


def _act(x, code):
    return np.tanh(x) if code == TANH else np.maximum(x, np.float32(0))


def stage(name, P, tr, defect=None):
    """DynImage::stage: one member's net in the kernel's padded blocks (without the + 4 of the row strides, which no read crosses)"""
    c = CASES[name]
    d = layout(name)
    n, m, (h1, h2) = c["n"], c["m"], c["dh"]
    din, HW, NS, n8, K1 = n + m, d["HW"], d["NS"], d["n8"], d["K1"]
    oB1 = h1 * din; oW2 = oB1 + h1; oB2 = oW2 + h2 * h1; oW3 = oB2 + h2; oB3 = oW3 + n * h2
    Pp = np.concatenate([P, np.full(TAIL, TAIL_VALUE, np.float32)])
    cc = np.arange(K1)
    nb = n if defect == "act_col_n" else n8              # feat(): c < n8 ? (c < n ? c : -1) : (c - n8 < m ? n + c - n8 : -1)
    f = np.where(cc < nb, np.where(cc < n, cc, -1), np.where(cc - nb < m, n + cc - nb, -1))
    im = dict(W1=np.zeros((HW, K1), np.float32), W2=np.zeros((HW, HW), np.float32), W3=np.zeros((NS, HW), np.float32))
    im["W1"][:h1, np.nonzero(f >= 0)[0]] = P[:oB1].reshape(h1, din)[:, f[f >= 0]]
    s2 = h2 if defect == "w2_stride" else h1
    im["W2"][:h2, :h1] = Pp[oW2 + np.arange(h2)[:, None] * s2 + np.arange(h1)[None, :]]
    im["W3"][:n, :h2] = P[oW3:oB3].reshape(n, h2)
    for key, src, w, full in (("b1", P[oB1:oW2], h1, HW), ("b2", P[oB2:oW3], h2, HW), ("b3", P[oB3:oB3 + n], n, NS)):
        im[key] = np.zeros(full, np.float32)
        im[key][:w] = src
    sc = tr[2 * din + n:2 * din + 2 * n]
    im["osc"], im["osh"], im["msk"] = np.zeros(NS, np.float32), np.zeros(NS, np.float32), np.zeros(NS, np.float32)
    im["osc"][:n] = sc + np.float32(1e-8)
    im["osh"][:n] = tr[2 * din:2 * din + n]
    im["msk"][:n] = (sc >= np.float32(1e-8)).astype(np.float32)
    im["ish"] = np.where(f >= 0, tr[np.maximum(f, 0)], np.float32(0)).astype(np.float32)
    im["irs"] = np.where(f >= 0, tr[din + np.maximum(f, 0)] + np.float32(1e-8), np.float32(1)).astype(np.float32)
    return im


def new_out(count, dtype=np.float32):
    return np.full(count + GUARD, np.nan, dtype)


def emulate(name, mem, s0, actions, defect=None):
    """route 1 as the kernel moves its data -> the obs buffer (K N H n + GUARD floats, NaN where nothing was stored)"""
    assert defect is None or defect in DEFECTS
    c = CASES[name]
    d = layout(name)
    n, m, K = c["n"], c["m"], len(mem["thetas"])
    N, H = actions.shape[:2]
    NS, n8, m8 = d["NS"], d["n8"], d["m8"]
    flags, act = mem["flags"], mem["act"]
    stride = 0 if (s0.ndim == 1 or defect == "s0_stride") else n
    s0f = s0.ravel()
    total = K * N * H * n
    buf = np.full(total + GUARD + 32 * H * n, np.nan, np.float32)      # (the slack takes what a store beyond the guard would hit)
    tiles = np.array([t for t in range(4 * ((N + 127) // 128)) if t * 32 < N])            # grid ceil(N / 128) x 4 waves, `return` past N
    if defect == "tile_unowned" and len(tiles) > 1:
        tiles = tiles[:-1]
    row = (tiles[:, None] * 32 + np.arange(32)[None, :]).ravel()
    valid = row < N
    vrow = np.where(valid, row, 0)
    fa = np.arange(32)                                       # slot (q, tt) of lane half hi is action f = 8 q + 4 hi + tt
    live = (fa // 8 < m8 // 8) & (fa < m)
    fcol = np.arange(n)
    store = np.ones_like(valid) if defect == "store_no_valid" else valid
    srow = row if defect == "store_no_valid" else vrow
    for k in range(K):
        im = stage(name, mem["thetas"][k], mem["trs"][0 if defect == "member0_tr" else k], defect)
        s = np.zeros((len(row), NS), np.float32)
        s[:, :n] = s0f[vrow[:, None] * stride + fcol[None, :]] * valid[:, None]
        for t in range(H):
            buf[(((k * N + srow[store]) * H + t) * n)[:, None] + fcol[None, :]] = s[store, :n]
            ta = 0 if defect == "stale_actions" else t
            an = np.where(valid[:, None] & live[None, :], actions[vrow, ta][:, np.where(live, fa, 0)], np.float32(0))
            x = (np.concatenate([s[:, :n8], an[:, :m8]], 1) - im["ish"]) / im["irs"]
            if defect == "drop_q3":
                x[:, n8 + 24:] = 0                           # (the k-steps of slot group 3 never issued)
            h = _act(x @ im["W1"].T + im["b1"], act)
            h = _act(h @ im["W2"].T + im["b2"], act)
            z = h @ im["W3"].T + im["b3"]
            if flags & AFF or defect == "affine_forced":
                z = z * im["osc"] + im["osh"]
            if flags & MASK:
                zm = z * im["msk"]
                if defect == "mask_skip_b1":
                    zm[:, 32:] = z[:, 32:]
                z = zm
            if flags & RES:
                if defect == "residual_overwritten":         # (block 1 adds block 0 of the state that was just written)
                    z[:, :32] = z[:, :32] + s[:, :32]
                    z[:, 32:] = z[:, 32:] + z[:, :NS - 32]
                else:
                    z = z + s                                # (block b reads s[b] before it writes it)
            s = z.astype(np.float32)
    return buf[:total + GUARD]


def plain_fp32(name, mem, s0, actions):
    """a stand-in for route 0 in the CPU checks: the same rollout as a plain fp32 chain with every layer's sum taken in the reverse
    order (another kernel, another summation order) -> the obs buffer"""
    c = CASES[name]
    n, K = c["n"], len(mem["thetas"])
    N, H = actions.shape[:2]
    sz = mem["sizes"]
    din = sz[0]
    f32 = np.float32
    obs = np.zeros((K, N, H, n), f32)
    for k in range(K):
        theta, tr = mem["thetas"][k], mem["trs"][k]
        s = s0_rows(s0, N).copy()
        for t in range(H):
            obs[k, :, t] = s
            xin = np.concatenate([s, actions[:, t]], 1)
            h = (xin - tr[:din]) / (tr[din:2 * din] + f32(1e-8))
            o = 0
            for i in range(3):
                W = theta[o:o + sz[i + 1] * sz[i]].reshape(sz[i + 1], sz[i]); o += W.size
                b = theta[o:o + sz[i + 1]]; o += sz[i + 1]
                h = np.ascontiguousarray(h[:, ::-1]) @ np.ascontiguousarray(W[:, ::-1]).T + b
                if i < 2:
                    h = _act(h, mem["act"])
            osh, osc = tr[2 * din:2 * din + n], tr[2 * din + n:]
            if mem["flags"] & AFF:
                h = h * (osc + f32(1e-8)) + osh
            if mem["flags"] & MASK:
                h = h * (osc >= f32(1e-8))
            if mem["flags"] & RES:
                h = h + s
            s = h.astype(f32)
    return np.concatenate([obs.ravel(), np.full(GUARD, np.nan, f32)])


# ---- the rollout record and its checks, the same for the device and for the emulation
def measure(name, runner):
    """runner(route, name, mem, s0, actions) -> the obs buffer, K N H n + GUARD floats prefilled with NaN.  -> the record the tests
    read: per route the per-column step error and the free-running error (the largest over the runs), the routes against each other,
    unwritten and guard counts, whether obs[:, :, 0] is s0 and the zero-scale column is exact, the runs of 32 rows or more on which the
    routes agree to the bit, the smallest column top and the largest |state| met, and the number of calls"""
    c = CASES[name]
    mem, data = cached_case(name)
    K, H, n, flags = c["K"], c["H"], c["n"], c["flags"]
    z = zero_column(name)
    rec = dict(step={"1": 0.0, "0": 0.0}, free={"1": 0.0, "0": 0.0}, routes=0.0, unwritten=0, guard=0, s0_exact=True, masked_exact=True,
               same_bits=[], runs=[], calls=0)
    for rows in c["rows"]:
        for mode in c["s0"]:
            s0, actions = data[(rows, mode)]
            total = K * rows * H * n
            start = s0_rows(s0, rows)
            got = {}
            for rt in (1, 0):
                buf = runner(rt, name, mem, s0, actions)
                assert buf.shape == (total + GUARD,)
                rec["calls"] += 1
                rec["unwritten"] += int(np.isnan(buf[:total]).sum())
                rec["guard"] += int((~np.isnan(buf[total:])).sum())
                obs = got[rt] = buf[:total].reshape(K, rows, H, n)
                rec["s0_exact"] = bool(rec["s0_exact"] and all(np.array_equal(obs[k][:, 0].view(np.int32), start.view(np.int32)) for k in range(K)))
                if z is not None and flags & MASK and H > 1:
                    want = np.broadcast_to(start[:, None, z], (rows, H - 1)) if flags & RES else np.zeros((rows, H - 1), np.float32)
                    rec["masked_exact"] = bool(rec["masked_exact"] and all(np.array_equal(obs[k][:, 1:, z], want) for k in range(K)))
                if H > 1:
                    e, _ = step_error(name, obs, actions, mem)
                    f, _ = free_error(name, obs, free_reference(name, (rows, mode)))
                    rec["runs"].append("%s rows %d s0 %s route %d: step %.3e free %.3e" % (name, rows, mode, rt, e, f))
                    rec["step"][str(rt)] = _worst([rec["step"][str(rt)], e])
                    rec["free"][str(rt)] = _worst([rec["free"][str(rt)], f])
            if H > 1:
                cols = compared_columns(name)
                rec["routes"] = _worst([rec["routes"]] + [col_err(got[1][k][:, 1:], got[0][k][:, 1:], cols)[0] for k in range(K)])
                if rows >= 32 and np.array_equal(got[1], got[0], equal_nan=True):
                    rec["same_bits"].append("%s %d %s" % (name, rows, mode))
    return rec


def checks(name, rec, pstep=None, pfree=None):
    """what tests/test_gpu_plan_matrix.py asserts of a record -> {check: passed}.  H = 1 cases store s0 alone: no error, no bar"""
    out = dict(written=rec["unwritten"] == 0 and rec["guard"] == 0, s0=rec["s0_exact"] is True, masked=rec["masked_exact"] is True)
    if CASES[name]["H"] > 1:
        bs, bf = MARGIN * pstep, MARGIN * pfree
        out.update(mfma=rec["step"]["1"] < bs and rec["free"]["1"] < bf, generic=rec["step"]["0"] < bs and rec["free"]["0"] < bf,
                   routes=rec["routes"] < 2 * bf, own_kernel=rec["same_bits"] == [])
    return out


# =========================================================================== scoring (mjx_plan_score)
U = 2.0 ** -53
U_EXP = U_POW = U_SQRT = 2.0           # ulps allowed to the device's fp64 exp, pow and sqrt: an assumption (tests/test_gpu_plan_matrix.py)
DENORM = 2.0 ** -1074
LD = np.longdouble
SCORE_MODES = ("reference", "trajectory", "none")
BASE = (4, 300, 6, 5, 3)


def _s(shape, kappa=3.0, gamma=0.95, omega=2.0, rscale=0.3, plant=None, equal=False):
    K, N, H, n, m = shape
    return dict(K=K, N=N, H=H, n=n, m=m, kappa=kappa, gamma=gamma, omega=omega, rscale=rscale, plant=plant, equal=equal)


SCORE_CASES = {
    "t1023": _s((3, 341, 4, 3, 2)), "t1024": _s((4, 256, 4, 3, 2)), "t1025": _s((5, 205, 4, 3, 2)),
    "n255": _s((2, 255, 4, 3, 2)), "n257": _s((2, 257, 4, 3, 2)),
    "hn63": _s((3, 40, 9, 7, 2)), "hn64": _s((3, 40, 8, 8, 2)), "hn65": _s((3, 40, 13, 5, 2)),
    "k1": _s((1, 40, 6, 5, 3)), "one": _s((1, 1, 1, 1, 1)), "h1": _s((3, 40, 1, 5, 3)), "wide": _s((2, 2, 3, 65, 33), kappa=0.5, gamma=0.99, omega=1.0),
    "gam0": _s(BASE, gamma=0.0), "gam1": _s(BASE, gamma=1.0), "gamh": _s(BASE, gamma=0.5), "om0": _s(BASE, omega=0.0),
    "kap0": _s(BASE, kappa=0.0), "kap800": _s(BASE, kappa=800.0, rscale=3.0), "equal": _s(BASE, equal=True),
    "max0": _s(BASE, plant=0), "maxT": _s(BASE, plant=4 * 300 - 1),
    # tid 1000 lies in wave 15, and element 1024 + 1000 is met on the second stride pass: that needs T > 2024, so N is 600 here
    "maxw15": _s((4, 600, 6, 5, 3), plant=1024 + 1000),
}
SCORE_ORDER = list(SCORE_CASES)
_SIN = {}


def score_modes(name):
    c = SCORE_CASES[name]
    return [mo for mo in SCORE_MODES if mo != "reference" or c["K"] <= c["N"]]


def score_inputs(name):
    """-> obs fp32 (K, N, H, n), rewards fp64 (K, N, H), actions fp64 (N, H, m); formed once"""
    if name not in _SIN:
        c = SCORE_CASES[name]
        K, N, H, n, m = c["K"], c["N"], c["H"], c["n"], c["m"]
        rng = np.random.RandomState(8800 + SCORE_ORDER.index(name))
        obs = rng.randn(K, N, H, n).astype(np.float32)
        rew = rng.randn(K, N, H) * c["rscale"]
        acts = rng.randn(N, H, m)
        if c["equal"]:
            rew[...] = rew[0, 0]                 # every trajectory of every member has the same rewards: with obs None every R is equal
        if c["plant"] is not None:
            rew.reshape(K * N, H)[c["plant"], 0] += 50.0          # the unique maximum, whatever omega dis adds
        _SIN[name] = (obs, rew, acts)
    return _SIN[name]


def gam(k):
    return k * U / (1.0 - k * U)


def score_ld(obs, rew, acts, c, mode):
    """the reference's lines in long double -> R (K N), S (K N), seq (H m), dis (N) -- all LD"""
    assert np.finfo(LD).nmant >= 63
    K, N, H = rew.shape
    r = rew.astype(LD).reshape(K * N, H)
    R = np.zeros(K * N, LD)
    dis = np.zeros(N, LD)
    if mode != "none":
        dis = np.sum(np.std(obs.astype(LD), axis=0), axis=(1, 2))
        idx = np.arange(K * N) // N if mode == "reference" else np.arange(K * N) % N
        R = R + LD(c["omega"]) * dis[idx]
    for t in range(H):
        R = R + (LD(c["gamma"]) ** t) * r[:, t]
    S = np.exp(LD(c["kappa"]) * (R - np.max(R)))
    a = acts.astype(LD).reshape(N, -1)
    seq = (S.reshape(K, N).sum(0)[:, None] * a).sum(0) / (np.sum(S) + LD(1e-6))
    return R, S, seq, dis


def score_bounds(obs, rew, acts, c, mode, ref):
    """forward bounds of the four kernels' fixed summation orders around the long-double values `ref` -> (B_R, B_S, B_seq) fp64.
    The derivation is in tests/test_gpu_plan_matrix.py's docstring; every step is restated beside its line here."""
    K, N, H = rew.shape
    R, S, seq, dis = ref
    T, HN = K * N, obs.shape[2] * obs.shape[3]
    B_dis = np.zeros(N, LD)
    if mode != "none":
        a = obs.astype(LD).reshape(K, N, HN)
        mabs = np.abs(a).sum(0) / K
        d = np.abs(a - a.sum(0) / K)
        e_mean = gam(K) * mabs                                           # K - 1 sums and one division
        e_d = U * d + e_mean                                             # d_k = a_k - mean: one rounding, and the mean's error
        vs = (d * d).sum(0)
        e_vs = ((2 * d + e_d) * e_d).sum(0) + gam(K + 1) * ((d + e_d) ** 2).sum(0)      # the squares' inputs; K products and K sums
        v = vs / K
        e_v = e_vs / K * (1 + U) + U * v                                 # the division by K
        sd = np.sqrt(v)
        with np.errstate(divide="ignore", invalid="ignore"):                 # |sqrt(v +- e) - sqrt(v)| <= min(e / sqrt(v), sqrt(e))
            e_sd = np.where(sd > 0, np.minimum(e_v / sd, np.sqrt(e_v)), np.sqrt(e_v))
        e_sd = e_sd + gam(U_SQRT) * (sd + e_sd)                          # the device's sqrt
        Ld = -(-HN // 64) + 6                                            # a thread's strided sum, then six xor levels
        B_dis = e_sd.sum(1) + gam(Ld) * (sd + e_sd).sum(1)
    idx = np.arange(T) // N if mode == "reference" else np.arange(T) % N
    om = abs(LD(c["omega"])) if mode != "none" else LD(0)
    g = np.abs(LD(c["gamma"])) ** np.arange(H)
    absR = om * (dis[idx] + B_dis[idx]) + (g * np.abs(rew.astype(LD).reshape(T, H))).sum(1)
    B_R = om * B_dis[idx] + gam(H + U_POW + 2) * absR                    # omega dis: one rounding; pow, the product, H sums
    top = np.max(R)
    near = R + B_R >= top - B_R[np.argmax(R)]                            # the scores the device may take for the maximum
    B_mx = np.max(B_R[near])
    kap = abs(LD(c["kappa"]))
    x = kap * np.abs(R - top)
    dx = kap * (B_R + B_mx) + gam(2) * (x + kap * (B_R + B_mx))          # the subtraction and the product round once each
    B_S = S * (np.expm1(dx) * (1 + gam(U_EXP)) + gam(U_EXP)) + (U_EXP + 1) * DENORM
    Ls = -(-T // 1024) + 6 + 16                                          # the strided sum, six xor levels, sixteen waves in order
    sumS = np.sum(S)
    e_sum = np.sum(B_S) + gam(Ls) * (sumS + np.sum(B_S))
    D = sumS + LD(1e-6)
    e_D = e_sum + U * (D + e_sum)
    A = np.abs(acts.astype(LD).reshape(N, -1))
    w, e_w = S.reshape(K, N).sum(0), B_S.reshape(K, N).sum(0)
    Lq = K + 1 + -(-N // 256) + 6 + 3                                    # the K members, the product, the strided sum, the tree, four waves
    e_num = (e_w[:, None] * A).sum(0) + gam(Lq) * ((w + e_w)[:, None] * A).sum(0)
    B_seq = (e_num + np.abs(seq) * e_D) / (D - e_D) + U * (np.abs(seq) + e_num / (D - e_D)) + DENORM
    return B_R.astype(np.float64), B_S.astype(np.float64), B_seq.astype(np.float64)


def share(got, ref, bound):
    """the largest |got - ref| / bound; a zero bound asks for a zero error.  NaN stays NaN"""
    err = np.abs(np.asarray(got, LD) - ref).astype(np.float64)
    if np.isnan(err).any():
        return float("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q))


SCORE_DEFECTS = ("sample_std", "gamma_t1", "idx_swapped", "max_1024", "one_pass", "no_1e6", "k0_only")


def _wave_sum(v):
    """plan_wave_sum over the last axis (64 lanes): lane 0's value"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _strided(vals, threads, one_pass=False):
    """a thread's partial sum of vals[..., tid], vals[..., tid + threads], ... in index order -> (..., threads)"""
    Lv = vals.shape[-1]
    P = -(-Lv // threads)
    x = np.zeros(vals.shape[:-1] + (P * threads,))
    x[..., :Lv] = vals
    x = x.reshape(vals.shape[:-1] + (P, threads))
    part = np.zeros(vals.shape[:-1] + (threads,))
    for p in range(1 if one_pass else P):
        part = part + x[..., p, :]
    return part


def emu_score(obs, rew, acts, c, mode, defect=None):
    """the four kernels in fp64 with their fixed summation orders -> (R, S, seq) buffers, each with GUARD NaN behind"""
    assert defect is None or defect in SCORE_DEFECTS
    K, N, H = rew.shape
    T = K * N
    one = defect == "one_pass"
    r = rew.reshape(T, H)
    sc = np.zeros(T)
    if mode != "none":
        traj = (mode == "trajectory") != (defect == "idx_swapped")
        need = N if traj else K
        a = obs[:, :need].astype(np.float64).reshape(K, need, -1)
        mean = np.zeros(a.shape[1:])
        for k in range(K):
            mean = mean + a[k]
        mean = mean / float(K)
        var = np.zeros_like(mean)
        for k in range(K):
            var = var + (a[k] - mean) * (a[k] - mean)
        with np.errstate(divide="ignore", invalid="ignore"):
            sd = np.sqrt(var / float(K - 1 if defect == "sample_std" else K))
        dis = _wave_sum(_strided(sd, 64, one))
        sc = c["omega"] * dis[np.arange(T) % N if traj else np.arange(T) // N]
    for t in range(H):
        sc = sc + np.power(c["gamma"], float(t + (defect == "gamma_t1"))) * r[:, t]
    R = sc
    mx = np.max(R[:1024]) if defect == "max_1024" else np.max(R)
    with np.errstate(over="ignore"):
        S = np.exp(c["kappa"] * (R - mx))
    red = _wave_sum(_strided(S, 1024, one).reshape(16, 64))
    sumS = 0.0
    for wv in range(16):
        sumS = sumS + red[wv]
    w = np.zeros(N)
    for k in range(1 if defect == "k0_only" else K):
        w = w + S[k * N:(k + 1) * N]
    terms = (w[:, None] * acts.reshape(N, -1)).T                         # (H m, N)
    red = _wave_sum(_strided(terms, 256, one).reshape(-1, 4, 64))
    seq = (((red[:, 0] + red[:, 1]) + red[:, 2]) + red[:, 3]) / (sumS + (0.0 if defect == "no_1e6" else 1e-6))
    nan = np.full(GUARD, np.nan)
    return np.concatenate([R, nan]), np.concatenate([S, nan]), np.concatenate([seq, nan])


def numpy_score(obs, rew, acts, c, mode):
    """NumPy's own fp64 evaluation of the reference's lines (_mpc_oracle) -> the same three buffers"""
    K = rew.shape[0]
    R = M.scores(obs, rew, c["omega"], c["gamma"], mode == "reference", mode != "none")
    S = M.weights(R, c["kappa"])
    nan = np.full(GUARD, np.nan)
    return np.concatenate([R, nan]), np.concatenate([S, nan]), np.concatenate([M.sequence(S, acts, K).ravel(), nan])


def score_measure(name, runner):
    """runner(name, mode, obs or None, rewards, actions, case) -> (R, S, seq) buffers with GUARD NaN behind each.  -> the record: the
    largest share of each bound over the modes, unwritten and guard counts, whether the device's maximum has weight exactly 1, and
    per case what it is here for (`special`)"""
    c = SCORE_CASES[name]
    obs, rew, acts = score_inputs(name)
    K, N, H, m = c["K"], c["N"], c["H"], c["m"]
    T = K * N
    rec = dict(R=0.0, S=0.0, seq=0.0, unwritten=0, guard=0, max_weight_one=True, special=True, calls=0, runs=[])
    outs = {}
    for mode in score_modes(name):
        ref = score_ld(obs, rew, acts, c, mode)
        B = score_bounds(obs, rew, acts, c, mode, ref)
        Rb, Sb, qb = runner(name, mode, None if mode == "none" else obs, rew, acts, c)
        assert Rb.shape == (T + GUARD,) and Sb.shape == (T + GUARD,) and qb.shape == (H * m + GUARD,)
        rec["calls"] += 1
        rec["unwritten"] += int(np.isnan(Rb[:T]).sum() + np.isnan(Sb[:T]).sum() + np.isnan(qb[:H * m]).sum())
        rec["guard"] += int((~np.isnan(Rb[T:])).sum() + (~np.isnan(Sb[T:])).sum() + (~np.isnan(qb[H * m:])).sum())
        sh = [share(Rb[:T], ref[0], B[0]), share(Sb[:T], ref[1], B[1]), share(qb[:H * m], ref[2], B[2])]
        rec["runs"].append("%s %s: R %.3f S %.3f seq %.3f of the bound" % (name, mode, sh[0], sh[1], sh[2]))
        for key, v in zip(("R", "S", "seq"), sh):
            rec[key] = _worst([rec[key], v])
        if not np.isnan(Rb[:T]).any():
            rec["max_weight_one"] = bool(rec["max_weight_one"] and Sb[int(np.argmax(Rb[:T]))] == 1.0)
        outs[mode] = (Rb[:T], Sb[:T], qb[:H * m])
    # what the case is here for, beyond the bounds
    sp = True
    if K == 1:                                           # every std is exactly 0: the disagreement term adds exactly nothing
        sp = all(np.array_equal(outs[mo][0], outs["none"][0]) for mo in outs)
    if c["kappa"] == 0.0:                                # all S = 1 and sum S = T: the sequence is the plain sum over T + 1e-6
        sp = all(np.all(o[1] == 1.0) for o in outs.values())
    if c["equal"]:
        o = outs["none"]
        sp = bool(np.all(o[0] == o[0][0]) and np.all(o[1] == 1.0))
    if c["kappa"] == 800.0:                              # most weights underflow to exactly 0
        sp = all(np.mean(o[1] == 0.0) > 0.5 for o in outs.values())
    if c["plant"] is not None:
        sp = all(int(np.argmax(o[1])) == c["plant"] and np.sum(o[1] == 1.0) == 1 for o in outs.values())
    rec["special"] = bool(sp)
    return rec


def score_checks(rec):
    return dict(R=rec["R"] <= 1.0, S=rec["S"] <= 1.0, seq=rec["seq"] <= 1.0, written=rec["unwritten"] == 0 and rec["guard"] == 0,
                max_weight_one=rec["max_weight_one"] is True, special=rec["special"] is True)
