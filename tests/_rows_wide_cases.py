"""Cases, seeded recipes and measures for the wide passes over stored rollouts (csrc/rows_wide.h: mjx_path_rewards_wide,
mjx_rollout_disagreement_wide), shared by the CPU checks (tests/test_rows_wide_cpu.py), the GPU worker (tests/_rows_wide_worker.py)
and the yardstick generator (tests/golden/make_golden_rows_wide.py).  CPU only.

Nets by _mpc_learned_oracle._torch_like with the transform recipes of _path_reward_cases.case (rewards: the s' shift and scale drawn
on their own) and _rollout_batch_cases.members (dynamics); wherever the mask flag is on one dynamics out_scale entry is exactly 0
beside an out_shift of +-0.4.  The oracles are _mpc_learned_oracle.ensemble_rewards and _rollout_batch_cases.oracle_err (fp64); the
measure of both quantities is _rollout_batch_cases.row_err: per row relative to its oracle value, rows below FLOOR_TOP of the
case's largest value against that floor.  The bar is MARGIN x the yardstick (tests/golden/rows_wide.npz): the unmodified
reference's fp32 chain for the rewards, the plain fp32 torch-CPU restatement _rollout_batch_cases.torch_err32 for the disagreement,
each under the same measure, floored at (n + 8) 2^-24 where it is 0.

Each case is the smallest shape that has its edge; a tile is 64 stored rows.
Rewards (RCASES): rows 1, 63, 64, 65 (a second tile of one row) and 129 (a third, partial tile); dynamics 256 x 256 (two tiles a
wave), 160 x 96, 100 x 200, 129 x 1; reward nets 100 x 100, 256 x 256, 1 x 1, 33 x 130; (n, m) = (64, 32) (2 n + m = 160), (1, 1)
and (64, 64) (n + m = 128); ReLU and tanh, the two nets' activations different in r2 and r3; flags 7, 3, 5, 0, 1; K = 2, 3, 1;
shared and per-member actions.  The small row sets ride with a larger one of the same case, so that no yardstick rests on one row.
rg: 64 members of a 40 x 24 net over 330 rows: on a 256-CU card ceil(256 / 64) = 4 workgroups per member walk six tiles.
Disagreement (DCASES): the same five dynamics nets over shapes (P, H) whose P H and P (H - 1) both hit 63, 64, 65 and 129, with
H = 2, a path boundary inside a tile ((13, 5), (21, 3), (43, 3)) and a path's last row on a tile edge ((16, 4), (64, 2), (1, 64));
K rotates over 1, 2, 3; dg is rg's geometry ((66, 5): 330 rows).  The stored rollouts follow _rollout_batch_cases.dis_data:
member 0's fp64 prediction plus noise with a per-row sigma, so that fix_lim finds adjacent oracle errors 5 % apart; the cases
with at least 31 paths fix a limit (LIMITED)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _mpc_learned_oracle as L  # noqa: E402
import _rollout_batch_cases as B  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "rows_wide.npz")
MARGIN, FLOOR_TOP, GUARD, MIN_LEN = B.MARGIN, B.FLOOR_TOP, B.GUARD, B.MIN_LEN
RELU, TANH = 0, 1
AFF, MASK, RES = 1, 2, 4
TILE = 64
MOVES = 1e-3                 # a flag "moves the result": clearing it changes the oracle by more than this under row_err

# dynamics nets: name -> n, m, hidden, activation, flags, seed
NETS = {
    "n1": (11, 2, (256, 256), RELU, 7, 8101),
    "n2": (17, 6, (160, 96), TANH, 3, 8102),
    "n3": (64, 32, (100, 200), RELU, 5, 8103),
    "n4": (1, 1, (129, 1), TANH, 0, 8104),
    "n5": (64, 64, (256, 256), RELU, 1, 8105),
    "n6": (6, 2, (40, 24), RELU, 7, 8106),
}
# reward cases: name -> dynamics net, reward hidden, reward activation, K, row sets, action modes
RCASES = {
    "r1": ("n1", (100, 100), RELU, 2, (129, 1), ("shared", "own")),
    "r2": ("n2", (33, 130), RELU, 3, (65,), ("shared", "own")),
    "r3": ("n3", (256, 256), TANH, 1, (63,), ("shared", "own")),
    "r4": ("n4", (1, 1), TANH, 2, (64,), ("shared", "own")),
    "r5": ("n5", (100, 100), RELU, 2, (129,), ("shared", "own")),
    "rg": ("n6", (20, 12), TANH, 64, (330,), ("own",)),
}
RORDER = sorted(RCASES)
SHAPES = [(1, 64), (1, 65), (1, 130), (21, 3), (16, 4), (13, 5), (43, 3), (64, 2), (65, 2), (129, 2)]
assert {63, 64, 65, 129} <= {P * H for P, H in SHAPES} and {63, 64, 65, 129} <= {P * (H - 1) for P, H in SHAPES}
KS = (1, 2, 3)


def dis_cases():
    """(net, P, H, K): every shape under two of the five nets, K rotating; then the geometry case"""
    nets = ["n1", "n2", "n3", "n4", "n5"]
    out = []
    for j, (P, H) in enumerate(SHAPES):
        for d in (0, 2):
            out.append((nets[(j + d) % 5], P, H, KS[(j + d) % 3]))
    return out + [("n6", 66, 5, 64)]


def limited():
    return [c for c in dis_cases() if c[1] >= 31]


def dis_id(case):
    return "%s_P%d_H%d_K%d" % case


def dyn_sizes(net):
    n, m, dh = NETS[net][:3]
    return (n + m,) + dh + (n,)


def rew_sizes(name):
    n, m = NETS[RCASES[name][0]][:2]
    return (2 * n + m,) + RCASES[name][1] + (1,)


def masked_column(net):
    n, flags = NETS[net][0], NETS[net][4]
    return n // 2 if flags & MASK else None


def _dyn_tr(rng, net):
    n, m = NETS[net][:2]
    dtr = np.concatenate([rng.randn(n + m) * 0.3, rng.rand(n + m) + 0.5, rng.randn(n) * 0.1, rng.rand(n) * 0.3 + 0.1])
    sign = 1.0 if rng.rand() < 0.5 else -1.0
    col = masked_column(net)
    if col is not None:
        dtr[2 * (n + m) + n + col] = 0.0
        dtr[2 * (n + m) + col] = 0.4 * sign
    return dtr.astype(np.float32)


# ---- rewards
_RCASE, _RREF, _DDATA = {}, {}, {}


def rcase(name):
    """seeded members and inputs -> (mem as ensemble_rewards takes it, {rows: (obs (K, rows, n), shared actions (rows, m) or None,
    per-member actions (K, rows, m) or None)}), fp32; formed once and left unchanged"""
    if name not in _RCASE:
        net, rh, ract, K, rowsets, modes = RCASES[name]
        n, m, dh, dact, flags, seed = NETS[net]
        rng = np.random.RandomState(seed + 50 * RORDER.index(name))
        ds, rs = dyn_sizes(net), rew_sizes(name)
        mem = dict(dyn_thetas=[], dyn_sizes=ds, dyn_trs=[], dact=dact, dflags=flags, rew_thetas=[], rew_sizes=rs, rew_trs=[], ract=ract)
        for _ in range(K):
            mem["dyn_thetas"].append(L._torch_like(rng, ds))
            mem["rew_thetas"].append(L._torch_like(rng, rs))
            mem["dyn_trs"].append(_dyn_tr(rng, net))
            s_sh, s_sc, a_sh, a_sc = rng.randn(n) * 0.2, rng.rand(n) + 0.6, rng.randn(m) * 0.2, rng.rand(m) + 0.6
            p_sh, p_sc = rng.randn(n) * 0.2, rng.rand(n) + 0.6                       # s' on its own
            mem["rew_trs"].append(np.concatenate([s_sh, a_sh, p_sh, s_sc, a_sc, p_sc, [rng.randn() * 0.5], [rng.rand() + 0.5]]).astype(np.float32))
        data = {}
        for rows in rowsets:
            obs = rng.standard_normal((K, rows, n)).astype(np.float32)
            shared = rng.standard_normal((rows, m)).astype(np.float32) if "shared" in modes else None
            own = rng.standard_normal((K, rows, m)).astype(np.float32) if "own" in modes else None
            data[rows] = (obs, shared, own)
        _RCASE[name] = (mem, data)
    return _RCASE[name]


def roracle(name, mem, rows, mode):
    obs, shared, own = rcase(name)[1][rows]
    return L.ensemble_rewards(obs, shared if mode == "shared" else own, mem)


def rreference(name):
    """{(rows, mode): fp64 rewards (K, rows)}, formed once and left unchanged"""
    if name not in _RREF:
        mem = rcase(name)[0]
        _RREF[name] = {(rows, mode): roracle(name, mem, rows, mode) for rows in RCASES[name][4] for mode in RCASES[name][5]}
    return _RREF[name]


def without_flag(mem, bit):
    return dict(mem, dflags=mem["dflags"] & ~int(bit))


def _floored(y, n):
    return y if y > 0 else (n + 8) * 2.0 ** -24


def ryard(name):
    return _floored(float(np.load(FIXTURE)["r_" + name]), NETS[RCASES[name][0]][0])


# ---- the end-to-end step's yardstick (tests/_rows_wide_worker.py), checked on the CPU by tests/test_rows_wide_cpu.py
def torch_rewards32(mem, obs, act):
    """the yardstick's subject for the end-to-end rewards: RewardNet_k(s, a, DynamicsNet_k(s, a)) as plain fp32 torch on the CPU (the
    chain of _rollout_batch_cases.torch_err32, then the reward net with its output affine) -> (K, ...) fp32"""
    import torch

    def mlp(theta, sz, tr, x, act_code):
        din = sz[0]
        h = (x - tr[:din]) / (tr[din:2 * din] + 1e-8)
        o = 0
        for i in range(len(sz) - 1):
            Wm = theta[o:o + sz[i + 1] * sz[i]].reshape(sz[i + 1], sz[i]); o += Wm.numel()
            b = theta[o:o + sz[i + 1]]; o += sz[i + 1]
            h = torch.nn.functional.linear(h, Wm, b)
            if i < len(sz) - 2:
                h = torch.tanh(h) if act_code == TANH else torch.relu(h)
        return h

    out = []
    ds, rs = mem["dyn_sizes"], mem["rew_sizes"]
    n, din, rin = ds[-1], ds[0], rs[0]
    with torch.no_grad():
        for k in range(len(mem["dyn_thetas"])):
            t = lambda v: torch.from_numpy(np.array(v, np.float32))     # noqa: E731  (a copy: torch wants a writable array)
            s, a = t(obs[k]).reshape(-1, n), t(act[k]).reshape(-1, din - n)
            dtr, rtr = t(mem["dyn_trs"][k]), t(mem["rew_trs"][k])
            sp = mlp(t(mem["dyn_thetas"][k]), ds, dtr, torch.cat([s, a], -1), mem["dact"])
            osh, osc = dtr[2 * din:2 * din + n], dtr[2 * din + n:]
            if mem["dflags"] & AFF:
                sp = sp * (osc + 1e-8) + osh
            if mem["dflags"] & MASK:
                sp = sp * (osc >= 1e-8)
            if mem["dflags"] & RES:
                sp = sp + s
            r = mlp(t(mem["rew_thetas"][k]), rs, rtr, torch.cat([s, a, sp], -1), mem["ract"])
            out.append((r[:, 0] * (rtr[2 * rin + 1] + 1e-8) + rtr[2 * rin]).numpy().reshape(obs[k].shape[:-1]))
    return np.stack(out)


# ---- disagreement
def members(net, K):
    """K members of a dynamics net as _rollout_batch_cases.predict64 / oracle_err take them"""
    n, m, dh, act, flags, seed = NETS[net]
    rng = np.random.RandomState(seed + 7)
    ds = dyn_sizes(net)
    mem = dict(thetas=[], trs=[], sizes=ds, act=act, flags=flags)
    for _ in range(K):
        mem["thetas"].append(L._torch_like(rng, ds))
        mem["trs"].append(_dyn_tr(rng, net))
    return mem


def dis_data(case):
    """_rollout_batch_cases.dis_data's recipe -> (mem, obs (P, H, n) fp32, act (P, H, m) fp32), formed once and left unchanged"""
    if case not in _DDATA:
        net, P, H, K = case
        n, m, seed = NETS[net][0], NETS[net][1], NETS[net][5]
        mem = members(net, K)
        rng = np.random.RandomState(seed * 17 + 1000 * H + P + 31 * K)
        obs, act = np.zeros((P, H, n), np.float32), rng.randn(P, H, m).astype(np.float32)
        obs[:, 0] = rng.randn(P, n)
        sigma = np.exp(rng.uniform(np.log(0.1), np.log(30.0), (P, H)))
        for t in range(H - 1):
            obs[:, t + 1] = B.predict64(mem, 0, obs[:, t], act[:, t]) + sigma[:, t, None] * rng.randn(P, n)
        _DDATA[case] = (mem, obs, act)
    return _DDATA[case]


def dyard(case):
    return _floored(float(np.load(FIXTURE)["d_" + dis_id(case)]), NETS[case[0]][0])


def truncation_shares(err, lim, min_len=MIN_LEN):
    """of a limited case under its limit -> (paths that truncate, paths clamped to min_len, paths left whole, paths)"""
    v = B.first_violation(err, lim)
    return int(np.sum(v >= 0)), int(np.sum((v >= 0) & (v + 1 < min_len))), int(np.sum(v < 0)), len(v)


# ---- the host arithmetic (rows_wide_lds_floats in csrc/rows_wide.h, wide_rows_shape in csrc/model_host.h), restated
def pad(d, to):
    return (d + to - 1) // to * to


def lds_floats(n, m, h1, h2, g1=0, g2=0, ns=2):
    rows_a = max(pad(h1, 32), pad(n, 32), pad(g1, 32))
    rows_b = max(pad(n + m, 8), pad(h2, 32), max(pad(2 * n + m, 8), pad(g2, 32)) if g1 else 0)
    consts = h1 + h2 + n + 2 * (n + m) + 2 * n + ((g1 + 2 * g2 + 1 + 2 * (2 * n + m) + 2) if g1 else 0)
    return (rows_a + rows_b) * (32 * ns + 4) + consts


def wide_route(ds, rs=None):
    """mjx_rollout_disagreement_wide_route (rs None) / mjx_path_rewards_wide_route as arithmetic"""
    for sz in (ds,) + (() if rs is None else (rs,)):
        if len(sz) < 2 or any(s <= 0 for s in sz):
            return -1
    n, m = ds[-1], ds[0] - ds[-1]
    if m <= 0 or (rs is not None and (rs[-1] != 1 or rs[0] != 2 * n + m)):
        return -1
    if len(ds) != 4 or (rs is not None and len(rs) != 4):
        return 0
    if max(ds[1:3]) > 256 or (rs is not None and max(rs[1:3]) > 256) or n > 64 or m > 64 or n + m > 128:
        return 0
    return int(4 * lds_floats(n, m, ds[1], ds[2], *(rs[1:3] if rs is not None else (0, 0))) <= 160 * 1024)


def tiles_walked(rows, K, cus=256):
    """-> (workgroups per member, tiles, most tiles a workgroup walks)"""
    tiles = -(-rows // TILE)
    grid = min(tiles, -(-cus // K))
    return grid, tiles, -(-tiles // grid)
