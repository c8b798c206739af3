"""GPU worker for tests/test_gpu_dynamics_matrix.py: every learned-dynamics case of the matrix in ONE fresh process; prints one
RESULT JSON line of measured errors and counts (the test module compares them with its bars).
python tests/_dynamics_matrix_worker.py"""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _dyn_check as C  # noqa: E402
from tests import _dyn_oracle as O  # noqa: E402
from tests._dyn_check import rand_theta, rand_tr  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._worker_dev import KEEP, ints, stream, switch  # noqa: E402

FIT_STATIC_LDS = 128          # k_dyn_fit's __shared__ double red[16] (.group_segment_fixed_size of the gfx950 code object)
LDS = 160 * 1024
GRAD_FLOOR = 3e-7             # fit_params_over_lr counts the parameters whose first fp64 gradient reached this

dev = W.device()
lib = load()
ERR, CNT = {}, {}             # key -> [worst error, case];  key -> count of defects (0 when all is well)
t32 = functools.partial(W.up, keep=True)     # every uploaded block stays alive until the process ends (KEEP)


def put(key, val, case):
    if key not in ERR or val > ERR[key][0]:
        ERR[key] = [float(val), case]


def count(key, n):
    CNT[key] = CNT.get(key, 0) + int(n)


def nan_buf(*shape):
    t = torch.full(shape, float("nan"), device=dev)
    KEEP.append(t)
    return t


# ================================================================ 1. batched forward
def fwd_case(name, sizes, K, rows, act, flags, seed, per_member_x=False, zero_col=None):
    rng = np.random.RandomState(seed)
    din, dout = sizes[0], sizes[-1]
    th = rand_theta(rng, sizes, K)
    trs = np.stack([rand_tr(rng, din, dout, zero_col) for _ in range(K)])
    x = (rng.randn(K if per_member_x else 1, rows, din) * 1.5).astype(np.float32)
    out = nan_buf(K, rows, dout)
    check(lib.mjx_dyn_forward(ptr(t32(x)), rows * din if per_member_x else 0, rows, K, ints(sizes), len(sizes), ptr(t32(th)),
                              ptr(t32(trs)), act, flags, ptr(out), stream()))
    o = out.cpu().numpy()
    count("fwd_unwritten", C.unwritten(o))
    ref = np.stack([O.forward(th[k], sizes, trs[k], x[k if per_member_x else 0], act, flags) for k in range(K)])
    put("fwd", C.col_err(o, ref)[0], name)
    if zero_col is not None and flags & O.MASK:
        for k in range(K):
            count("fwd_mask_bad", C.masked_bad(o[k], x[k if per_member_x else 0], zero_col, flags & O.RES))


# widths: maxw from the input (d_in 40 > every hidden width), 48, 256 (96 KiB: the attribute), 426 (163 584 B, the largest)
fwd_case("input_maxw", [40, 24, 32, 6], 3, 77, 0, 7, 1)
for rows in (1, 31, 32, 33, 64, 12500):
    fwd_case("w48_r%d" % rows, [13, 48, 48, 11], 4, rows, 0, 7, 2 + rows, zero_col=3)
for rows in (33, 12500):
    fwd_case("w256_r%d" % rows, [13, 256, 256, 11], 4, rows, 0, 7, 3 + rows)
fwd_case("w426_K7", [13, 426, 426, 11], 7, 64, 1, 7, 4)
fwd_case("w426_K1", [13, 426, 426, 11], 1, 33, 0, 7, 5)
# members: K = 1, 7 with distinct parameters; each member its own rows (x_stride = rows * d_in)
fwd_case("K1", [13, 64, 64, 11], 1, 77, 0, 7, 6)
fwd_case("K7", [13, 64, 64, 11], 7, 77, 1, 3, 7)
fwd_case("stride_K4", [13, 64, 64, 11], 4, 45, 0, 7, 8, per_member_x=True, zero_col=0)
fwd_case("stride_w256", [13, 256, 256, 11], 3, 500, 0, 7, 9, per_member_x=True)
# depth: one Linear layer, and DYN_MAXL = 8 Linear layers
fwd_case("nl1", [13, 11], 3, 77, 0, 7, 10, zero_col=5)
fwd_case("nl8", [13, 32, 40, 32, 40, 32, 40, 32, 11], 3, 77, 1, 7, 11)
fwd_case("nl8_relu", [13, 32, 40, 32, 40, 32, 40, 32, 11], 2, 100, 0, 5, 12)
# every flag combination, ReLU and tanh, with a masked column (out_scale = 0)
for act in (0, 1):
    for flags in range(8):
        fwd_case("flags%d_act%d" % (flags, act), [13, 64, 64, 11], 3, 77, act, flags, 20 + 8 * act + flags, zero_col=2)

# width 427 (163 968 B): refused on the host, out untouched
rng = np.random.RandomState(40)
sz = [13, 427, 427, 11]
out = nan_buf(1, 33, 11)
rc = lib.mjx_dyn_forward(ptr(t32(rng.randn(33, 13))), 0, 33, 1, ints(sz), 4, ptr(t32(rand_theta(rng, sz, 1))),
                         ptr(t32(rand_tr(rng, 13, 11)[None])), 0, 7, ptr(out), stream())
torch.cuda.synchronize()
REFUSED = {"fwd_w427": [rc, C.unwritten(out.cpu().numpy()) == out.numel()]}

# ensemble_forward with members that differ in residual and activation: two launches or more, then out[ids] = o
from mjrl_amd.algos.model_accel import nn_dynamics as D  # noqa: E402

n_, m_ = 9, 3
rng = np.random.RandomState(41)
nets = []
for i, (res, tanh, mask) in enumerate([(True, False, True), (False, False, True), (True, True, True), (False, True, False),
                                       (True, False, True)]):
    net = D.DynamicsNet(n_, m_, hidden_size=(48, 40), residual=res, seed=50 + i, use_mask=mask)
    if tanh:
        net.nonlinearity = torch.tanh
    tr = rand_tr(rng, n_ + m_, n_, zero_col=4)
    net.set_transformations(tr[:n_], tr[n_ + m_:2 * n_ + m_], tr[n_:n_ + m_], tr[2 * n_ + m_:2 * (n_ + m_)],
                            tr[2 * (n_ + m_):2 * (n_ + m_) + n_], tr[2 * (n_ + m_) + n_:])
    nets.append((net, tr, res, tanh, mask))
x = (rng.randn(70, n_ + m_) * 1.5).astype(np.float32)
o = D.ensemble_forward([e[0] for e in nets], x, dev).cpu().numpy()
for k, (net, tr, res, tanh, mask) in enumerate(nets):
    th = np.concatenate([p.detach().cpu().numpy().ravel() for p in net.parameters()])
    flags = O.AFF | (O.MASK if mask else 0) | (O.RES if res else 0)
    ref = O.forward(th, list(net.layer_sizes), tr, x, 1 if tanh else 0, flags)
    put("fwd_ensemble_mixed", C.col_err(o[k:k + 1], ref[None])[0], "member%d" % k)
    if mask:
        count("fwd_mask_bad", C.masked_bad(o[k], x, 4, res))


# ================================================================ 2. rollout
def rollout_case(name, n, m, dsz, psz, K, N, H, act=0, flags=7, bounds="vec", noise=True, actions=False, seed=0):
    """one mjx_model_rollout against the fp64 oracle: teacher-forced at every H, free-running as well at H <= 6"""
    rng = np.random.RandomState(seed)
    dth = rand_theta(rng, dsz, K)
    dtr = np.stack([rand_tr(rng, n + m, n, zero_col=1 if flags & O.MASK else None) for _ in range(K)])
    pth = np.concatenate([rand_theta(rng, psz, gain=1.5), rng.randn(m) * 0.3 - 0.5]).astype(np.float32) if not actions else None
    ptr_ = np.concatenate([rng.randn(n) * 0.2, rng.rand(n) + 0.5, rng.randn(m) * 0.1, rng.rand(m) + 0.5]).astype(np.float32)
    s0 = rng.randn(N, n).astype(np.float32)
    nz = rng.randn(K, H, N, m).astype(np.float32) if noise and not actions else None
    acts = rng.randn(N, H, m).astype(np.float32) * 1.2 if actions else None
    if bounds == "scalar":
        bnd = [np.full(m, -0.8), np.full(m, 0.8), np.full(n, -3.0), np.full(n, 3.0)]
    elif bounds == "vec":
        bnd = [-0.4 - rng.rand(m), 0.4 + rng.rand(m), -2.0 - 2 * rng.rand(n), 2.0 + 2 * rng.rand(n)]
    else:
        bnd = None
    bnd = [np.float32(b) for b in bnd] if bnd is not None else None
    bd = [t32(b) for b in bnd] if bnd is not None else [None] * 4
    obs, ao = nan_buf(K, N, H, n), nan_buf(K, N, H, m)
    if actions:
        check(lib.mjx_model_rollout(ptr(t32(s0)), N, H, K, None, 0, None, None, None, ptr(t32(acts)), ints(dsz), len(dsz),
                                    ptr(t32(dth)), ptr(t32(dtr)), act, flags, ptr(bd[0]), ptr(bd[1]), ptr(bd[2]), ptr(bd[3]),
                                    ptr(obs), ptr(ao), stream()))
    else:
        check(lib.mjx_model_rollout(ptr(t32(s0)), N, H, K, ints(psz), len(psz), ptr(t32(pth)), ptr(t32(ptr_)),
                                    ptr(t32(nz)) if nz is not None else None, None, ints(dsz), len(dsz), ptr(t32(dth)),
                                    ptr(t32(dtr)), act, flags, ptr(bd[0]), ptr(bd[1]), ptr(bd[2]), ptr(bd[3]), ptr(obs), ptr(ao),
                                    stream()))
    ob, ac = obs.cpu().numpy(), ao.cpu().numpy()
    count("roll_unwritten", C.unwritten(ob) + C.unwritten(ac))
    count("roll_s0_bad", np.sum(ob[:, :, 0] != s0[None]))
    if actions:
        want = acts if bnd is None else np.maximum(np.minimum(acts, bnd[1]), bnd[0])
        count("roll_given_actions_bad", np.sum(ac != want[None]))
    tf = C.teacher_forced(ob, ac, (pth, psz, ptr_) if not actions else None, nz, (dth, dsz, dtr, act, flags), bnd,
                          actions=acts)
    put("roll_tf_act", tf["act"][0], "%s %s" % (name, tf["act"][1]))
    put("roll_tf_obs", tf["obs"][0], "%s %s" % (name, tf["obs"][1]))
    if H <= 6:
        ro, ra = O.rollout(s0, H, pth, psz, ptr_, nz, dth, dsz, dtr, act, flags, bnd, actions=acts)
        put("roll_free", max(C.col_err(C.by_step(ob).reshape(K * H, N, n), C.by_step(ro).reshape(K * H, N, n))[0],
                             C.col_err(C.by_step(ac).reshape(K * H, N, m), C.by_step(ra).reshape(K * H, N, m))[0]), name)


# production: dynamics [n + m, 256, 256, n], ReLU, flags 7; policy 32 x 32 / 64 x 64; K = 3 / 4; N = 250 (last tile 2 rows)
rollout_case("prod_p32_K3_H25_scalar", 11, 2, [13, 256, 256, 11], [11, 32, 32, 2], 3, 250, 25, bounds="scalar", seed=101)
rollout_case("prod_p64_K4_H50_vec", 11, 2, [13, 256, 256, 11], [11, 64, 64, 2], 4, 250, 50, bounds="vec", seed=102)
rollout_case("prod_p32_K4_H50_vec", 11, 2, [13, 256, 256, 11], [11, 32, 32, 2], 4, 250, 50, bounds="vec", seed=103)
rollout_case("prod_n24_m8_K3_H25", 24, 8, [32, 256, 256, 24], [24, 64, 64, 8], 3, 250, 25, bounds="vec", seed=104)
rollout_case("prod_actions_K4_H50", 11, 2, [13, 256, 256, 11], None, 4, 250, 50, bounds="vec", actions=True, seed=105)
# branches (H <= 6 also free-running)
rollout_case("tanh_dyn", 11, 2, [13, 64, 64, 11], [11, 32, 32, 2], 3, 13, 6, act=1, seed=110)
rollout_case("flags3", 11, 2, [13, 64, 64, 11], [11, 32, 32, 2], 3, 13, 6, flags=3, seed=111)
rollout_case("dyn_3hidden", 11, 2, [13, 48, 40, 48, 11], [11, 32, 32, 2], 2, 13, 6, seed=112)
rollout_case("pol_1hidden", 11, 2, [13, 64, 64, 11], [11, 32, 2], 2, 13, 6, seed=113)
rollout_case("pol_3hidden", 11, 2, [13, 64, 64, 11], [11, 32, 24, 32, 2], 2, 13, 6, seed=114)
rollout_case("pol_wider_than_dyn", 11, 2, [13, 48, 48, 11], [11, 128, 160, 2], 3, 13, 6, seed=115)
rollout_case("pol_n200_lds_over_64k", 200, 4, [204, 64, 64, 200], [200, 64, 64, 4], 2, 13, 4, seed=116)
rollout_case("eval_no_noise", 11, 2, [13, 64, 64, 11], [11, 32, 32, 2], 2, 13, 6, noise=False, bounds=None, seed=117)
for N in (1, 7, 8):
    rollout_case("N%d" % N, 11, 2, [13, 64, 64, 11], [11, 32, 32, 2], 3, N, 6, seed=120 + N)
    rollout_case("N%d_long" % N, 11, 2, [13, 256, 256, 11], [11, 64, 64, 2], 3, N, 30, seed=130 + N)


def rollout_untouched(name, n, m, psz, N, H, K=2):
    """a rollout that must launch nothing: H = 0, N = 0, or an LDS need over 160 KiB (refused on the host)"""
    rng = np.random.RandomState(140)
    dsz = [n + m, 32, n]
    obs, ao = nan_buf(K, 8, 2, n), nan_buf(K, 8, 2, m)      # larger than any write the call could make
    pth = np.concatenate([rand_theta(rng, psz), np.zeros(m)]).astype(np.float32)
    ptr_ = np.concatenate([np.zeros(n), np.ones(n), np.zeros(m), np.ones(m)]).astype(np.float32)
    s0 = rng.randn(max(N, 1), n).astype(np.float32)
    nz = rng.randn(K, max(H, 1), max(N, 1), m).astype(np.float32)
    rc = lib.mjx_model_rollout(ptr(t32(s0)), N, H, K, ints(psz), len(psz), ptr(t32(pth)), ptr(t32(ptr_)), ptr(t32(nz)), None,
                               ints(dsz), 3, ptr(t32(rand_theta(rng, dsz, K))), ptr(t32(np.stack([rand_tr(rng, n + m, n)] * K))),
                               0, 7, None, None, None, None, ptr(obs), ptr(ao), stream())
    torch.cuda.synchronize()
    REFUSED[name] = [rc, C.unwritten(obs.cpu().numpy()) == obs.numel() and C.unwritten(ao.cpu().numpy()) == ao.numel()]


rollout_untouched("roll_H0", 11, 2, [11, 32, 32, 2], 8, 0)
rollout_untouched("roll_N0", 11, 2, [11, 32, 32, 2], 0, 2)
rollout_untouched("roll_lds_over_160k", 600, 4, [600, 64, 64, 4], 8, 2)     # policy alone 171 552 B


# ================================================================ 3. fit
ROUTES = {"k_dyn_fit": 0, "k_dl_loss": 0}     # launches the kernel trace must show: persistent calls, launch-route steps


def persistent(sizes, batch, launches):
    fb = 4 * batch * (sum(sizes) + sizes[-1] + 2 * max(sizes[1:]))
    return not launches and all(h <= 128 for h in sizes[1:-1]) and batch <= 64 and fb + FIT_STATIC_LDS <= LDS


def gpu_fit(theta, sizes, tr, x, y, idx, steps, batch, act, tmode, lr, wd, launches, m=None, v=None, step0=0):
    din = sizes[0]
    P = t32(theta)
    mm = torch.zeros_like(P) if m is None else t32(m)
    vv = torch.zeros_like(P) if v is None else t32(v)
    loss = nan_buf(steps)
    ix = torch.as_tensor(np.ascontiguousarray(idx[:steps * batch], np.int32)).to(dev)
    KEEP.append(ix)
    with switch("MJX_DYN_FIT_LAUNCHES", "1" if launches else "0"):
        check(lib.mjx_dyn_fit_adam(ptr(t32(x)), ptr(t32(y)), x.shape[0], ints(sizes), len(sizes), ptr(t32(tr[:2 * din])),
                                   ptr(t32(tr[2 * din:])), tmode, act, ptr(P), ptr(mm), ptr(vv), step0, ptr(ix), steps, batch, lr, wd,
                                   ptr(loss), stream()))
    if persistent(sizes, batch, launches):
        ROUTES["k_dyn_fit"] += 1
    else:
        ROUTES["k_dl_loss"] += steps
    p, l, mo, vo = P.cpu().numpy(), loss.cpu().numpy(), mm.cpu().numpy(), vv.cpu().numpy()
    count("fit_unwritten", C.unwritten(l) + C.unwritten(p))
    return p, l, mo, vo


def fit_data(sizes, seed, Nf, batch, epochs=12):
    rng = np.random.RandomState(seed)
    din, dout = sizes[0], sizes[-1]
    th = rand_theta(rng, sizes)
    tr = rand_tr(rng, din, dout)
    xf = rng.randn(Nf, din).astype(np.float32)
    yf = (xf[:, :dout] * 0.8 + 0.3 * rng.randn(Nf, dout)).astype(np.float32) if dout <= din else rng.randn(Nf, dout).astype(np.float32)
    idx = np.concatenate([rng.permutation(Nf)[:(Nf // batch) * batch] for _ in range(epochs)])
    return th, tr, xf, yf, idx


def fit_case(name, sizes, batch, act=0, tmode=2, wd=1e-5, seed=0, Nf=400, lr=1e-3):
    """1 and 10 steps against fp64 on the route the shape takes; a shape the persistent route takes runs the launch route too"""
    th, tr, xf, yf, idx = fit_data(sizes, seed, Nf, batch)
    both = persistent(sizes, batch, False)
    for steps in (1, 10):
        g1 = np.zeros(th.size)
        ref, _, _, rl = O.adam_steps(th, sizes, tr, xf, yf, idx[:steps * batch], batch, act, tmode, lr, wd, g_first=g1)
        # Adam's step is g / (|g| + 1e-8) at t = 1: a parameter whose first gradient is near 1e-8 turns the fp32 rounding of
        # that gradient (~3e-10 absolute at these shapes) into percents of lr on any fp32 implementation, and keeps the error
        well = g1 >= GRAD_FLOOR
        count("fit_ill_conditioned", np.sum(~well))
        count("fit_params", th.size)
        outs = []
        for launches in ((False, True) if both else (False,)):
            p, l, _, _ = gpu_fit(th, sizes, tr, xf, yf, idx, steps, batch, act, tmode, lr, wd, launches)
            put("fit_params_over_lr", C.over_lr(p[well], ref[well], lr), "%s steps %d %s" % (name, steps, "launch" if launches else "default"))
            put("fit_ill_conditioned_over_lr", C.over_lr(p, ref, lr), "%s steps %d %s" % (name, steps, "launch" if launches else "default"))
            put("fit_loss", C.rel_max(l, rl), "%s steps %d" % (name, steps))
            outs.append(p)
        if both:
            put("fit_routes_over_lr", C.over_lr(outs[0], outs[1], lr), "%s steps %d" % (name, steps))


# production 256 x 256 (launch route), batch 16 and 64; tanh on the launch route
fit_case("w256_b16", [13, 256, 256, 11], 16, seed=201)
fit_case("w256_b64", [13, 256, 256, 11], 64, seed=202)
fit_case("w160_tanh", [13, 160, 160, 11], 32, act=1, tmode=1, seed=203)
# route edges: hidden 128 / 129, batch 64 / 65, dynamic LDS 163 584 B / 163 840 B (+ 128 B static) at batch 64
fit_case("h128", [10, 128, 128, 8], 32, seed=204)
fit_case("h129", [10, 129, 129, 8], 32, seed=205)
fit_case("b64", [10, 64, 64, 8], 64, seed=206)
fit_case("b65", [10, 64, 64, 8], 65, seed=207)
fit_case("lds_163584", [43, 128, 128, 42], 64, seed=208)
fit_case("lds_163840", [44, 128, 128, 42], 64, seed=209)
# shapes: one Linear layer, 3 and 7 hidden layers, RewardNet through the affine, B * d_out > 1024 (the loss head loops)
fit_case("nl1", [8, 6], 32, seed=210)
fit_case("hidden3", [10, 32, 48, 32, 8], 32, act=1, seed=211)
fit_case("hidden7", [10, 24, 32, 24, 32, 24, 32, 24, 8], 32, seed=212)
fit_case("reward", [24, 100, 100, 1], 32, tmode=0, wd=0.0, seed=213)
fit_case("reward_b64", [24, 100, 100, 1], 64, tmode=0, seed=214)
fit_case("loss_loop", [24, 64, 64, 20], 64, tmode=1, seed=215)
fit_case("loss_loop_w256", [24, 256, 256, 20], 64, seed=216)

# continuation: s1 steps, then s2 with the moments carried and step0 = s1, against one (s1 + s2)-step call bit for bit on each
# route, and the second call against the fp64 chain started from the device's own state after s1 steps (t0 = s1)
for name, sizes, batch, s1, s2 in [("narrow", [10, 64, 64, 8], 32, 3, 7), ("narrow", [10, 64, 64, 8], 32, 12, 5),
                                   ("w256", [13, 256, 256, 11], 32, 3, 7), ("w256", [13, 256, 256, 11], 32, 12, 5),
                                   ("reward", [24, 100, 100, 1], 16, 3, 4)]:
    tmode = 0 if name == "reward" else 2
    th, tr, xf, yf, idx = fit_data(sizes, 300 + s1 + len(sizes), 300, batch, epochs=30)
    lr, wd = 1e-3, 1e-5
    for launches in (False, True):
        p1, l1, m1, v1 = gpu_fit(th, sizes, tr, xf, yf, idx, s1, batch, 0, tmode, lr, wd, launches)
        p2, l2, _, _ = gpu_fit(p1, sizes, tr, xf, yf, idx[s1 * batch:], s2, batch, 0, tmode, lr, wd, launches, m1, v1, step0=s1)
        pa, la, _, _ = gpu_fit(th, sizes, tr, xf, yf, idx, s1 + s2, batch, 0, tmode, lr, wd, launches)
        count("fit_cont_not_bitwise", np.sum(p2 != pa) + np.sum(np.concatenate([l1, l2]) != la))
        ref, _, _, _ = O.adam_steps(p1, sizes, tr, xf, yf, idx[s1 * batch:(s1 + s2) * batch], batch, 0, tmode, lr, wd, m=m1, v=v1,
                                    t0=s1)
        put("fit_cont_over_lr", C.over_lr(p2, ref, lr), "%s t0 %d %s" % (name, s1, "launch" if launches else "default"))


# ================================================================ 4. truncation
def trunc_case(name, pred, sn, off, lim):
    K, rows, n = pred.shape
    err = torch.full((rows,), C.ERR_SENTINEL, device=dev)
    first = torch.full((len(off) - 1,), C.FIRST_SENTINEL, dtype=torch.int32, device=dev)
    offd = torch.as_tensor(np.asarray(off, np.int64)).to(dev)
    KEEP.extend([err, first, offd])
    check(lib.mjx_dyn_pred_error(ptr(t32(pred)), K, rows, n, ptr(t32(sn)), ptr(offd), len(off) - 1, lim, ptr(err), ptr(first),
                                 stream()))
    eref, fref = O.pred_error(pred, sn, off, lim)
    r = C.pred_err_errors(err.cpu().numpy(), first.cpu().numpy(), eref, fref)
    put("trunc_err", r["err"], name)
    for key in ("nan", "first", "unwritten"):
        count("trunc_" + key, r[key])
    count("trunc_cases_with_violations", int(np.any(fref >= 0)))


rng = np.random.RandomState(400)
# K = 4, 1000 segments of 49 rows (K * N paths, H - 1 rows each), a quarter of them with a violation somewhere
K, n = 4, 11
off = np.arange(0, 1001) * 49
sn = (rng.randn(49000, n) * 0.5).astype(np.float32)
pred = (sn[None] + rng.randn(K, 49000, n) * 0.05).astype(np.float32)
hot = rng.randint(0, 49000, 300)
pred[rng.randint(0, K, 300), hot] += 0.5
trunc_case("K4_1000x49", pred, sn, off, 0.03)
# K = 1, n = 1
sn = rng.randn(3000, 1).astype(np.float32)
pred = (sn[None] + rng.randn(1, 3000, 1) * 0.1).astype(np.float32)
trunc_case("K1_n1", pred, sn, np.array([0, 700, 1500, 1500, 3000]), 0.05)
# 700-row segments: violations on different loop trips of different threads, the earliest must win; violations at row 0 and at
# the last row; empty segments at the start, in the middle and at the end
K, n = 3, 5
off = np.array([0, 0, 700, 1400, 1400, 2100, 2800, 3500, 3500, 3500])
sn = (rng.randn(3500, n) * 0.3).astype(np.float32)
pred = (sn[None] + rng.randn(K, 3500, n) * 0.01).astype(np.float32)
for a0, rows_hit in [(0, [300, 520, 650, 301]), (700, [0, 699]), (1400, [699]), (2100, [257, 513, 2, 600]), (2800, [255, 256])]:
    for r in rows_hit:
        pred[r % K, a0 + r] += 1.0
trunc_case("seg700_trips_edges_empty", pred, sn, off, 0.05)
# errors exactly at the limit: d = 0.5 in every column -> 0.25 (exact in fp32 and fp64), not > 0.25; one row just above
sn = np.zeros((64, 4), np.float32)
pred = np.zeros((2, 64, 4), np.float32)
pred[0, 10:20] = 0.5
pred[1, 30:40] = -0.5
pred[1, 50] = 0.5
pred[1, 50, 0] = 0.5001                                     # 0.250025: above the limit however it is rounded
trunc_case("exactly_at_limit", pred, sn, np.array([0, 25, 45, 64]), 0.25)
trunc_case("exactly_at_limit_then_above", pred, sn, np.array([0, 64]), 0.25)
# inf and NaN in pred and in s_next, in one member and in all members; a NaN member next to another over the limit
K, n = 3, 6
sn = (rng.randn(400, n) * 0.3).astype(np.float32)
pred = (sn[None] + rng.randn(K, 400, n) * 0.01).astype(np.float32)
pred[1, 20, 2] = np.nan                                    # one member NaN, none over the limit
pred[0, 40, 1] = np.nan; pred[2, 40] += 1.0                # one member NaN, another over: the reference does not truncate here
pred[2, 41] += 1.0                                          # ... but at the next row
pred[:, 60, 3] = np.nan                                     # every member NaN
pred[2, 120, 0] = np.inf                                    # one member inf
pred[:, 140, 5] = -np.inf                                   # every member -inf
sn[160, 4] = np.nan                                         # s_next NaN (all members)
sn[180, 0] = np.inf                                         # s_next inf (all members)
sn[200, 1] = np.inf; pred[1, 200, 1] = np.inf              # inf - inf in one member, inf - finite in the others
pred[0, 399, 0] = np.nan                                    # NaN at a segment's last row
trunc_case("inf_nan", pred, sn, np.array([0, 30, 41, 50, 100, 130, 150, 170, 190, 210, 400]), 0.05)

W.emit({"err": ERR, "count": CNT, "refused": REFUSED, "routes": ROUTES})
