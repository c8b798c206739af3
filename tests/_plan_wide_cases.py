"""Cases, seeded recipes, measures, check functions and the NumPy emulation for the wide plan rollout (csrc/plan_wide.h:
k_plan_rollout_wide behind mjx_plan_rollout_wide), shared by the GPU worker (tests/_plan_wide_worker.py), the GPU tests
(tests/test_gpu_plan_wide.py), the CPU checks (tests/test_plan_wide_cpu.py) and the yardstick generator
(tests/golden/make_golden_plan_wide.py).  CPU only.

The recipe and the measures are tests/_plan_cases.py's (col_err, step_reference, s0_rows, MARGIN, GUARD are imported from it):
nn.Linear-scaled weights, the same transform distributions, one out_scale entry exactly 0 beside an out_shift of +-0.4 in column
n // 2 of every case with n > 1; the error per state column of each member, relative to that column's largest |reference|, the
worst over columns; the zero-scale column left out of the error where the mask flag is on and asserted exactly there instead (0 of
either sign under flags 3, s0's column under flags 7).

The emulation restates the kernel's data movement in fp32 with NumPy's own sums: one workgroup per (tile of 32 sample columns,
member), the [unit][sample] tiles S, XD, H1, H2, Z3 with their zero padding rows, valid / vrow, the action rows of XD written one
step ahead (after the forward of the step before), the residual's read of S before it is overwritten, the store under valid.  It
does not reproduce the MFMA summation order.

The end-to-end case (MPC): two WorldModel(6, 2, hidden_size=(256, 256), learn_reward=True) carrying seeded parameters and
transforms (mpc_members loads them into either package's WorldModel), one MPCPolicy.get_action with N 40, H 8."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
from _plan_cases import GUARD, MARGIN, col_err, s0_rows, step_reference  # noqa: E402,F401

FIXTURE = os.path.join(HERE, "golden", "plan_wide.npz")
RELU, TANH = 0, 1
AFF, MASK, RES = 1, 2, 4
TILE = 32                    # sample columns of a workgroup's tile
LDS_MAX = 160 * 1024


# name -> n, m, hidden, activation, flags, seed, K, H, rows, s0 modes.  Each is the smallest shape that has its edge; cases that
# share a seed and K share their nets (f1 with q1).  Why each is here: tests/test_gpu_plan_wide.py.
def _c(n, m, dh, act, flags, seed, K, rows, s0, H=5):
    return dict(n=n, m=m, dh=dh, act=act, flags=flags, seed=seed, K=K, H=H, rows=rows, s0=s0)


CASES = {
    "q1": _c(11, 2, (256, 256), RELU, 7, 9101, 3, 33, ("one", "rows")),
    "q2": _c(6, 2, (256, 256), TANH, 3, 9102, 1, 65, ("rows",)),
    "q3": _c(17, 6, (160, 96), RELU, 5, 9103, 2, 31, ("rows",)),
    "q4": _c(1, 1, (129, 1), TANH, 1, 9104, 1, 1, ("one",)),
    "q5": _c(64, 64, (256, 256), RELU, 0, 9105, 1, 32, ("rows",)),
    "q6": _c(33, 9, (100, 200), RELU, 7, 9106, 2, 64, ("rows",)),
    "q7": _c(17, 6, (64, 64), TANH, 7, 9107, 1, 33, ("one",)),
    "q8": _c(6, 2, (256, 256), RELU, 7, 9108, 1, 32, ("rows",), H=1),
    "g1": _c(11, 2, (256, 256), RELU, 7, 9109, 5, 417, ("rows",), H=3),
    "f1": _c(11, 2, (256, 256), RELU, 7, 9101, 3, 33, ("rows",), H=16),
}
ORDER = sorted(CASES)
STEPPED = [c for c in ORDER if CASES[c]["H"] > 1 and c != "f1"]       # one-step yardsticks pstep_<case>
FREE = "f1"                                                           # the free-running yardstick pfree_f1
NARROW_ROUTE = {name: (1 if name == "q7" else 0) for name in CASES}   # mjx_plan_route's answer (plan_shape)
NAN_CASE, NAN_ROW = "q2", 40


def sizes(name):
    c = CASES[name]
    return (c["n"] + c["m"],) + c["dh"] + (c["n"],)


def zero_column(name):
    n = CASES[name]["n"]
    return None if n == 1 else n // 2


def compared_columns(name):
    c = CASES[name]
    z = zero_column(name)
    return np.array([j for j in range(c["n"]) if not (c["flags"] & MASK and j == z)])


def case(name):
    """seeded members and inputs -> (mem: dict(thetas, trs, sizes, act, flags), {s0 mode: (s0, actions (rows, H, m))}), fp32"""
    c = CASES[name]
    n, m, K, H, rows = c["n"], c["m"], c["K"], c["H"], c["rows"]
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
    for mode in c["s0"]:
        drng = np.random.RandomState(c["seed"] * 31 + 1000 * H + 7 * rows + (mode == "rows"))
        s0 = (drng.randn(rows, n) if mode == "rows" else drng.randn(n)).astype(np.float32)
        data[mode] = (s0, drng.randn(rows, H, m).astype(np.float32))
    return mem, data


_CASE, _FREE = {}, {}


def cached_case(name):
    if name not in _CASE:
        _CASE[name] = case(name)
    return _CASE[name]


def free_reference(name, mode):
    """the free-running fp64 rollout (K, N, H, n) of a run, formed once and left unchanged"""
    if (name, mode) not in _FREE:
        mem, data = cached_case(name)
        s0, actions = data[mode]
        _FREE[(name, mode)] = M.rollout(s0, actions, mem["thetas"], mem["sizes"], mem["trs"], mem["act"], mem["flags"])
    return _FREE[(name, mode)]


# ---- the measures (tests/_plan_cases.py's, on these cases)
def _worst(v):
    v = [float(x) for x in v]
    return float("nan") if any(x != x for x in v) else max(v + [0.0])


def step_error(name, obs, actions, mem):
    """obs (K, N, H, n) -> the per-column one-step error, the largest over the members"""
    cols = compared_columns(name)
    return _worst([col_err(obs[k][:, 1:], step_reference(obs[k], actions, mem, k), cols)[0] for k in range(obs.shape[0])])


def free_error(name, obs, ref):
    cols = compared_columns(name)
    return _worst([col_err(obs[k][:, 1:], ref[k][:, 1:], cols)[0] for k in range(obs.shape[0])])


def yard(name):
    G = np.load(FIXTURE)
    return float(G["pfree_f1"] if name == FREE else G["pstep_" + name])


# ---- the documented layout (include/mjx.h), restated
def pad(v, to):
    return (v + to - 1) // to * to


def lds_floats(n, m, h1, h2):
    """S, XD, H1, H2, Z3 rows of 36 floats, then the biases and transforms"""
    return 36 * (n + pad(n + m, 8) + pad(h1, 32) + pad(h2, 32) + pad(n, 32)) + h1 + h2 + 5 * n + 2 * m


def served(ds):
    """wide_plan_shape as arithmetic"""
    if len(ds) != 4:
        return 0
    n, m = ds[-1], ds[0] - ds[-1]
    ok = max(ds[1:3]) <= 256 and n <= 64 and m <= 64 and n + m <= 128
    return int(ok and 4 * lds_floats(n, m, ds[1], ds[2]) <= LDS_MAX)


# ---- the emulation
DEFECTS = ("actions_ahead", "member0_tr", "residual_overwritten", "store_no_valid")


def _act(x, code):
    return np.tanh(x) if code == TANH else np.maximum(x, np.float32(0))


def new_out(count):
    return np.full(count + GUARD, np.nan, np.float32)


def emulate(name, mem, s0, actions, defect=None):
    """route 2 as the kernel moves its data -> the obs buffer (K N H n + GUARD floats, NaN where nothing was stored)"""
    assert defect is None or defect in DEFECTS
    f32 = np.float32
    c = CASES[name]
    n, m, (h1, h2), K = c["n"], c["m"], c["dh"], len(mem["thetas"])
    N, H = actions.shape[:2]
    din, K0 = n + m, pad(n + m, 8)
    flags, act = mem["flags"], mem["act"]
    stride = 0 if s0.ndim == 1 else n
    s0f = s0.ravel()
    total = K * N * H * n
    buf = np.full(total + GUARD + TILE * H * n, np.nan, f32)             # (the slack takes what a store beyond the guard would hit)
    oB1 = h1 * din; oW2 = oB1 + h1; oB2 = oW2 + h2 * h1; oW3 = oB2 + h2; oB3 = oW3 + n * h2
    cols = np.arange(n)
    for k in range(K):
        P, tr = mem["thetas"][k], mem["trs"][0 if defect == "member0_tr" else k]
        # a layer's weights with the zero rows and columns the padded tiles see
        W1 = np.zeros((pad(h1, 32), K0), f32); W1[:h1, :din] = P[:oB1].reshape(h1, din)
        W2 = np.zeros((pad(h2, 32), pad(h1, 32)), f32); W2[:h2, :h1] = P[oW2:oB2].reshape(h2, h1)
        W3 = np.zeros((pad(n, 32), pad(h2, 32)), f32); W3[:n, :h2] = P[oW3:oB3].reshape(n, h2)
        b1, b2, b3 = P[oB1:oW2], P[oB2:oW3], P[oB3:oB3 + n]
        ish, isc, osh, osc = tr[:din], tr[din:2 * din], tr[2 * din:2 * din + n], tr[2 * din + n:]

        def norm_actions(a_raw):
            return (a_raw - ish[n:, None]) / (isc[n:, None] + f32(1e-8))

        for tile in range((N + TILE - 1) // TILE):                       # grid (ceil(N / 32), K)
            row = tile * TILE + np.arange(TILE)
            valid = row < N
            vrow = np.where(valid, row, 0)
            store = np.ones_like(valid) if defect == "store_no_valid" else valid
            srow = row if defect == "store_no_valid" else vrow

            def raw_actions(t):
                return np.where(valid[None, :], actions[vrow, t].T, f32(0)).astype(f32)          # (m, 32)

            S = (s0f[vrow[None, :] * stride + cols[:, None]] * valid[None, :]).astype(f32)       # (n, 32)
            XD = np.zeros((K0, TILE), f32)                               # rows din .. K0 - 1 stay zero
            XD[n:din] = norm_actions(raw_actions(0))
            for t in range(H):
                buf[(((k * N + srow[store]) * H + t) * n)[None, :] + cols[:, None]] = S[:, store]
                XD[:n] = (S - ish[:n, None]) / (isc[:n, None] + f32(1e-8))
                if t + 1 == H:
                    break
                an = raw_actions(t + 1)                                  # requested before the forward
                if defect == "actions_ahead":                            # (written before the forward read XD: step t runs on a[t + 1])
                    XD[n:din] = norm_actions(an)
                H1 = np.zeros((pad(h1, 32), TILE), f32); H1[:h1] = _act((W1 @ XD)[:h1] + b1[:, None], act)
                H2 = np.zeros((pad(h2, 32), TILE), f32); H2[:h2] = _act((W2 @ H1)[:h2] + b2[:, None], act)
                Z3 = np.zeros((pad(n, 32), TILE), f32); Z3[:n] = (W3 @ H2)[:n] + b3[:, None]
                z = Z3[:n]
                if flags & AFF:
                    z = z * (osc[:, None] + f32(1e-8)) + osh[:, None]
                if flags & MASK:
                    z = z * (osc[:, None] >= f32(1e-8)).astype(f32)
                if flags & RES:
                    z = z + (z if defect == "residual_overwritten" else S)                     # (S read before it is overwritten)
                S = z.astype(f32)
                XD[n:din] = norm_actions(an)                             # written after the forward's last read of XD
    return buf[:total + GUARD]


def plain_fp32(name, mem, s0, actions):
    """a stand-in for route 0 in the CPU checks: the same rollout as a plain fp32 chain with every layer's sum taken in the reverse
    order (another kernel, another summation order) -> the obs buffer"""
    f32 = np.float32
    n, K = CASES[name]["n"], len(mem["thetas"])
    N, H = actions.shape[:2]
    sz = mem["sizes"]
    din = sz[0]
    obs = np.zeros((K, N, H, n), f32)
    for k in range(K):
        theta, tr = mem["thetas"][k], mem["trs"][k]
        s = s0_rows(s0, N).copy()
        for t in range(H):
            obs[k, :, t] = s
            h = (np.concatenate([s, actions[:, t]], 1) - tr[:din]) / (tr[din:2 * din] + f32(1e-8))
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


# ---- the record and its checks, the same for the device and for the emulation
def measure(name, runner):
    """runner(route, name, mem, s0, actions) -> the obs buffer, K N H n + GUARD floats prefilled with NaN; route "2" is the wide
    kernel, "0" the same entry under MJX_PLAN_WIDE=0.  -> the record the tests read: per route the error against fp64 (per column and
    one step for the stepped cases, free-running for f1; the largest over the s0 modes), the routes against each other, unwritten
    and guard counts, whether obs[:, :, 0] is s0 and the zero-scale column is exact, and whether the routes agree to the bit"""
    c = CASES[name]
    mem, data = cached_case(name)
    K, H, n, rows, flags = c["K"], c["H"], c["n"], c["rows"], c["flags"]
    z = zero_column(name)
    rec = dict(err={"2": 0.0, "0": 0.0}, routes=0.0, unwritten=0, guard=0, s0_exact=True, masked_exact=True, same_bits=True, runs=[], calls=0)
    total = K * rows * H * n
    for mode in c["s0"]:
        s0, actions = data[mode]
        start = s0_rows(s0, rows)
        got = {}
        for rt in ("2", "0"):
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
                e = free_error(name, obs, free_reference(name, mode)) if name == FREE else step_error(name, obs, actions, mem)
                rec["runs"].append("%s s0 %s route %s: %.3e" % (name, mode, rt, e))
                rec["err"][rt] = _worst([rec["err"][rt], e])
        if H > 1:
            cols = compared_columns(name)
            rec["routes"] = _worst([rec["routes"]] + [col_err(got["2"][k][:, 1:], got["0"][k][:, 1:], cols)[0] for k in range(K)])
            rec["same_bits"] = bool(rec["same_bits"] and np.array_equal(got["2"], got["0"], equal_nan=True))
        else:
            rec["same_bits"] = False                                       # (s0 alone: equal bits say nothing)
    return rec


def checks(name, rec, yardstick=None):
    """what tests/test_gpu_plan_wide.py asserts of a record -> {check: passed}.  The H = 1 case stores s0 alone: no error, no bar"""
    out = dict(written=rec["unwritten"] == 0 and rec["guard"] == 0, s0=rec["s0_exact"] is True, masked=rec["masked_exact"] is True)
    if CASES[name]["H"] > 1:
        bar = MARGIN * yardstick
        out.update(wide=rec["err"]["2"] < bar, generic=rec["err"]["0"] < bar, routes=rec["routes"] < 2 * bar)
    return out


# ---- the end-to-end case
MPC = dict(n=6, m=2, hid=(256, 256), K=2, N=40, H=8, kappa=16.0, gamma=0.95, omega=1.0, fc=(0.5, 0.25, 0.8, 0.0), seed=9201, draw=9202)
MPC_DYN = (8, 256, 256, 6)
MPC_REW = (14, 100, 100, 1)
MPC_MIN_ESS = 5.0


def mpc_mem():
    """the seeded members as the oracles take them (_mpc_learned_oracle.ensemble_rewards' dict); dynamics ReLU, flags 7"""
    n, m, K = MPC["n"], MPC["m"], MPC["K"]
    rng = np.random.RandomState(MPC["seed"])
    mem = dict(dyn_thetas=[], dyn_sizes=MPC_DYN, dyn_trs=[], dact=0, dflags=7, rew_thetas=[], rew_sizes=MPC_REW, rew_trs=[], ract=0)
    for _ in range(K):
        mem["dyn_thetas"].append(L._torch_like(rng, MPC_DYN))
        mem["rew_thetas"].append(L._torch_like(rng, MPC_REW))
        dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
        s_sh, s_sc, a_sh, a_sc = dtr[:n], dtr[n + m:2 * n + m], dtr[n:n + m], dtr[2 * n + m:2 * (n + m)]
        rtr = np.concatenate([s_sh, a_sh, s_sh, s_sc, a_sc, s_sc, [rng.randn() * 0.5], [rng.rand() + 0.5]])
        mem["dyn_trs"].append(dtr.astype(np.float32))
        mem["rew_trs"].append(rtr.astype(np.float32))
    return mem


def mpc_members(WorldModel, torch):
    """WorldModel(6, 2, hidden_size=(256, 256), learn_reward=True) instances carrying mpc_mem()'s parameters and transforms (either
    package's WorldModel; a WorldModel's two nets share s_shift / s_scale / a_shift / a_scale, as fitted ones do)"""
    n, m = MPC["n"], MPC["m"]
    mem = mpc_mem()
    out = []
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32).copy())
    for k in range(MPC["K"]):
        wm = WorldModel(n, m, hidden_size=MPC["hid"], seed=70 + k, learn_reward=True)
        for net, th in ((wm.dynamics_net, mem["dyn_thetas"][k]), (wm.reward_net, mem["rew_thetas"][k])):
            o = 0
            for p in net.parameters():
                p.data = t(th[o:o + p.numel()].reshape(p.shape)); o += p.numel()
        dtr, rtr, din, rin = mem["dyn_trs"][k], mem["rew_trs"][k], n + m, 2 * n + m
        wm.dynamics_net.set_transformations(t(dtr[:n]), t(dtr[din:din + n]), t(dtr[n:din]), t(dtr[din + n:2 * din]), t(dtr[2 * din:2 * din + n]),
                                            t(dtr[2 * din + n:]))
        wm.reward_net.set_transformations(t(rtr[:n]), t(rtr[rin:rin + n]), t(rtr[n:din]), t(rtr[rin + n:rin + din]), float(rtr[2 * rin]),
                                          float(rtr[2 * rin + 1]))
        out.append(wm)
    return out


def mpc_obs():
    return np.random.RandomState(MPC["draw"] + 1).randn(MPC["n"]) * 0.5


def mpc_oracle(actions, reward):
    """the fp64 plan of the end-to-end call given its perturbed actions -> dict(R, S, seq): _mpc_learned_oracle.plan on
    reward='learned', _mpc_oracle.plan (the stand-in environment's reward) on reward='env'"""
    mem = mpc_mem()
    if reward == "learned":
        return L.plan(mpc_obs(), actions, mem, MPC["kappa"], MPC["gamma"], MPC["omega"])
    return M.plan(mpc_obs(), actions, mem["dyn_thetas"], MPC_DYN, mem["dyn_trs"], 0, 7, MPC["kappa"], MPC["gamma"], MPC["omega"])


def mpc_errors(R, seq, plan):
    """(scores max-relative, sequence relative L2) against the oracle's plan"""
    return float(np.max(np.abs(np.asarray(R, np.float64) - plan["R"])) / np.max(np.abs(plan["R"]))), M.rel_l2(seq, plan["seq"])


def mpc_key(what, reward):
    return "mpc_" + what + ("" if reward == "learned" else "_env")
