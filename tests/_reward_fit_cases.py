"""The case table of the reward-fit tests (tests/test_gpu_reward_fit.py, tests/test_reward_fit_cpu.py,
tests/test_reward_fit_checks.py), its data recipe and the comparison functions the GPU worker applies: NumPy only, so the CPU
tests read the same table and run the same comparisons the GPU worker runs."""
import numpy as np

from tests import _dyn_check as C
from tests._dyn_check import rand_theta, rand_tr

K, NF, LR, WD = 4, 400, 1e-3, 1e-5
GRAD_FLOOR = 3e-7             # parameters whose first fp64 gradient is below this are ill-conditioned for any fp32 Adam
BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3")

# name, sizes, batch, act (0 ReLU, 1 tanh): all target mode 0, all on route 1
CASES = [
    ("rw_ref_b64", [24, 100, 100, 1], 64, 0),       # the driver's shape
    ("rw_ref_b16", [24, 100, 100, 1], 16, 0),       # padded sample columns
    ("rw_tanh_b33", [14, 100, 100, 1], 33, 1),      # act'(0) = 1 in padded rows; batch just past a tile
    ("rw_w33_36", [9, 33, 36, 1], 32, 0),           # one unit past a tile; h % 8 != 0
    ("rw_w31_7", [5, 31, 7, 1], 8, 1),              # widths below a tile
    ("rw_w64_b32", [10, 64, 64, 1], 32, 0),         # aligned widths, the affine head alone
    ("rw_dout3", [10, 100, 72, 3], 32, 0),          # per-column c
]
# inputs in scratch, widths one short of the limit: kept out of the matrix (its own keys)
MAX_CASE = ("rw_max_b64", [128, 255, 250, 1], 64, 0)
# name, sizes, batch, act, MJX_REWARD_FIT_ENS: route 0, bit for bit K mjx_dyn_fit_adam calls in target mode 0
ROUTE0 = [
    ("rw_env0", [24, 100, 100, 1], 64, 0, "0"),
    ("rw_w300", [24, 300, 100, 1], 32, 0, None),
    ("rw_hidden3", [10, 64, 64, 64, 1], 32, 0, None),
    ("rw_b65", [24, 100, 100, 1], 65, 0, None),
]


def member_data(name, sizes, batch, k, epochs=12):
    """member k of a case -> (theta, transforms, x, y, row indices of `epochs` epochs), all float32 (indices int)"""
    rng = np.random.RandomState(700 + 17 * k + len(name))
    din, dout = sizes[0], sizes[-1]
    th = rand_theta(rng, sizes)
    tr = rand_tr(rng, din, dout)
    x = rng.randn(NF, din).astype(np.float32)
    y = (x[:, :dout] * 0.8 + 0.3 * rng.randn(NF, dout)).astype(np.float32)
    idx = np.concatenate([rng.permutation(NF)[:(NF // batch) * batch] for _ in range(epochs)])
    return th, tr, x, y, idx


def fixture_data(N, n, m, seed, zero_col=True):
    """the data function of tests/_model_accel_worker.py (the recipe tests/golden/model_accel.npz was recorded with)"""
    rng = np.random.RandomState(seed)
    s = rng.randn(N, n).astype(np.float32)
    a = rng.randn(N, m).astype(np.float32)
    W = rng.randn(n + m, n).astype(np.float32) * 0.3
    sp = (s + np.tanh(np.concatenate([s, a], 1) @ W) * 0.5).astype(np.float32)
    if zero_col:
        sp[:, 1] = s[:, 1]
    return s, a, sp


def block_slices(sizes):
    """flat-parameter slices of W1, b1, W2, b2, W3, b3 with their 2-D shapes (rows = units of the layer, columns = its inputs)"""
    out, k = [], 0
    for l in range(len(sizes) - 1):
        di, dj = sizes[l], sizes[l + 1]
        out.append(("W%d" % (l + 1), slice(k, k + di * dj), (dj, di))); k += di * dj
        out.append(("b%d" % (l + 1), slice(k, k + dj), (dj, 1))); k += dj
    return out


def edge_mask(sizes):
    """parameters in the rows (units) and columns (inputs) beyond the last full 32-tile of a hidden width: where a dropped or
    unmasked partial tile would show.  Empty (all False) for widths that are multiples of 32."""
    mask = np.zeros(sum(sizes[l] * sizes[l + 1] + sizes[l + 1] for l in range(len(sizes) - 1)), bool)
    for l, (name, sl, (dj, di)) in enumerate(block_slices(sizes)):
        layer = l // 2
        m2 = np.zeros((dj, di), bool)
        if layer + 1 < len(sizes) - 1 and dj % 32:             # this layer's units are a hidden width
            m2[(dj // 32) * 32:, :] = True
        if name[0] == "W" and layer > 0 and di % 32:           # this layer's inputs are a hidden width
            m2[:, (di // 32) * 32:] = True
        mask[sl] = m2.ravel()
    return mask


def compare_params(p, ref, well, sizes, lr=LR):
    """a device (or defective) chain against the fp64 chain over the well-conditioned parameters, in units of lr
    -> {"all": worst, "W1": ..., ..., "edge": worst over edge_mask (0.0 where it is empty)}"""
    p, ref = np.asarray(p, np.float64), np.asarray(ref, np.float64)
    out = {"all": C.over_lr(p[well], ref[well], lr) if well.any() else 0.0}
    for name, sl, _ in block_slices(sizes):
        w = well[sl]
        out[name] = C.over_lr(p[sl][w], ref[sl][w], lr) if w.any() else 0.0
    e = edge_mask(sizes) & well
    out["edge"] = C.over_lr(p[e], ref[e], lr) if e.any() else 0.0
    return out


def compare_losses(l, ref):
    return C.rel_max(l, ref)
