"""The comparisons of tests/test_gpu_reward_fit.py bite (no GPU): the comparison functions (tests/_reward_fit_cases.py) at
the GPU module's bars, run against NumPy chains that carry one defect each of those a wrong ragged / affine-head kernel would
leave.  The chains are tests/_dyn_oracle.adam_steps (target mode 0) step by step -- its forward, its gradient expressions,
its adam_update -- in fp32 with torch's once-rounded Adam constants, with a switch per defect; the clean fp32 chain must pass
every bar, and the fp64 chain is adam_steps itself.

Each defect is flagged at the smallest case where it can occur:
  units 96 .. 99 of a 100-wide layer never updated (the dropped partial delta tile)    1 step, [24, 100, 100, 1]: edge, blocks
  weight columns >= 96 of W2 / W3 never updated                                         1 step, the same: edge, W2 / W3
  delta3 without the factor c                                                           1 step, [10, 100, 72, 3] (per-column c;
      with ONE output column the factor scales the whole gradient, which Adam's m / sqrt(v) divides out again up to eps and the
      weight decay: there the defect cannot show in the parameters, and the loss does not depend on it)
  the loss taken on z instead of yhat                                                   1 step: the loss
  out_shift dropped                                                                     1 step: the loss
  a padded tanh row leaking a non-zero delta into b2's sum                              10 steps, [14, 100, 100, 1] tanh: b2,
      edge (one step of Adam moves b2 by lr * sign(g): the leak shows once it has turned a sign or entered the moments)"""
import numpy as np
import pytest

from tests import _dyn_oracle as O
from tests._reward_fit_cases import GRAD_FLOOR, LR, WD, block_slices, compare_losses, compare_params, edge_mask, member_data
from tests.test_gpu_reward_fit import BARS

PARAM_KEYS = ("all", "edge", "W1", "b1", "W2", "b2", "W3", "b3")
BAR_OF = {"all": "params_over_lr", "edge": "edge_over_lr"}


def chain(theta, sizes, tr, x, y, idx, batch, act, steps, defect=None, dtype=np.float32):
    """adam_steps(..., tmode 0) in `dtype`, step by step, with one defect switched on -> (theta, losses)"""
    f = dtype
    din, dout = sizes[0], sizes[-1]
    theta = np.array(theta, f)
    theta0 = theta.copy()
    tr = np.asarray(tr, f)
    x, y = np.asarray(x, f), np.asarray(y, f).reshape(len(x), -1)
    osh, c = tr[2 * din:2 * din + dout], tr[2 * din + dout:] + f(1e-8)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    coef = tuple(f(q) for q in O.ADAM_TORCH[:4]) + O.ADAM_TORCH[4:]
    frozen = np.zeros(theta.size, bool)
    for name, sl, (dj, di) in block_slices(sizes):
        m2 = np.zeros((dj, di), bool)
        if defect == "units_96_99" and name in ("W1", "b1", "W2", "b2"):
            m2[96:, :] = True
        if defect == "cols_96" and name in ("W2", "W3"):
            m2[:, 96:] = True
        frozen[sl] = m2.ravel()
    losses = []
    for s in range(steps):
        rows = idx[s * batch:(s + 1) * batch]
        hs = [((x[rows] - tr[:din]) / (tr[din:2 * din] + f(1e-8))).astype(f)]
        Ws, bs = O.unflatten(theta, sizes)
        for i, (W, b) in enumerate(zip(Ws, bs)):
            h = hs[-1] @ W.T + b
            hs.append(O.act_fn(h, act).astype(f) if i < len(Ws) - 1 else h.astype(f))
        z = hs[-1]
        yh = z * c + (f(0) if defect == "no_out_shift" else osh)
        err = (yh - y[rows]).astype(f)
        lerr = (z - y[rows]) if defect == "loss_on_z" else err
        losses.append(np.mean(np.asarray(lerr, np.float64) ** 2))
        dz = (f(2.0 / err.size) * err * (f(1) if defect == "delta3_no_c" else c)).astype(f)
        g = np.zeros_like(theta)
        gW, gb = O.unflatten(g, sizes)
        for l in range(len(Ws) - 1, -1, -1):
            gW[l][...] = dz.T @ hs[l]
            gb[l][...] = dz.sum(0)
            if defect == "tanh_pad_leak" and l == 1:
                gb[1][-1] += leak
            if l > 0:
                da = (dz @ Ws[l]).astype(f)
                if defect == "tanh_pad_leak" and l == 2:
                    # the padded row next to unit 99 of H2 holds h = 0, so act'(0) = 1 passes its unmasked product on (here: the
                    # product of a neighbouring column, as an unmasked read past W3's row end would form it) into b2's last sum
                    leak = da[:, 0].sum()
                dz = (da * ((f(1) - hs[l] ** 2) if act == 1 else (hs[l] > 0))).astype(f)
        g = (g + f(WD) * theta).astype(f)
        new, m, v = O.adam_update(theta, g, m, v, s + 1, LR, coef)
        new, m, v = new.astype(f), m.astype(f), v.astype(f)
        new[frozen] = theta0[frozen]
        theta = new
    return theta, np.array(losses)


def _flags(name, sizes, batch, act, steps, defect, k=0):
    """the keys of the GPU module's comparisons that are over their bars for a chain"""
    th, tr, x, y, idx = member_data(name, sizes, batch, k)
    g1 = np.zeros(th.size)
    ref, _, _, rl = O.adam_steps(th, sizes, tr, x, y, idx[:steps * batch], batch, act, 0, LR, WD, g_first=g1)
    well = g1 >= GRAD_FLOOR
    p, l = chain(th, sizes, tr, x, y, idx, batch, act, steps, defect)
    e = compare_params(p, ref, well, sizes)
    out = {k_ for k_ in PARAM_KEYS if not e[k_] < BARS[BAR_OF.get(k_, "block_" + k_)]}
    if not compare_losses(l, rl) < BARS["loss"]:
        out.add("loss")
    return out, e


REF = ("rw_ref_b16", [24, 100, 100, 1], 16, 0)
TANH = ("rw_tanh_b33", [14, 100, 100, 1], 33, 1)
DOUT3 = ("rw_dout3", [10, 100, 72, 3], 32, 0)


@pytest.mark.parametrize("case", [REF, TANH, DOUT3, ("rw_w33_36", [9, 33, 36, 1], 32, 0), ("rw_w31_7", [5, 31, 7, 1], 8, 1)])
@pytest.mark.parametrize("steps", [1, 10])
def test_clean_fp32_chain_passes_every_bar(case, steps):
    for k in range(2):
        flagged, e = _flags(*case, steps, None, k=k)
        assert not flagged, (flagged, e)


def test_edge_mask_is_the_rows_and_columns_beyond_the_last_full_tile():
    sizes = [24, 100, 100, 1]
    mk = edge_mask(sizes)
    want = {"W1": 4 * 24, "b1": 4, "W2": 4 * 100 + 96 * 4, "b2": 4, "W3": 4, "b3": 0}
    for name, sl, _ in block_slices(sizes):
        assert int(mk[sl].sum()) == want[name], name
    assert not edge_mask([10, 64, 64, 1]).any()
    assert edge_mask([5, 31, 7, 1]).sum() == 31 * 5 + 31 + 7 * 31 + 7 + 7     # widths below a tile: every hidden unit is edge


def test_dropped_partial_delta_tile_is_flagged():
    flagged, e = _flags(*REF, 1, "units_96_99")
    assert {"all", "edge", "W1", "b1", "W2", "b2"} <= flagged, (flagged, e)
    assert "loss" not in flagged and "W3" not in flagged


def test_unmasked_weight_columns_are_flagged():
    flagged, e = _flags(*REF, 1, "cols_96")
    assert {"all", "edge", "W2", "W3"} <= flagged, (flagged, e)
    assert not flagged & {"W1", "b1", "b2", "b3", "loss"}


def test_delta3_without_c_is_flagged_where_c_differs_by_column():
    flagged, e = _flags(*DOUT3, 1, "delta3_no_c")
    assert {"all", "W2", "W1"} <= flagged, (flagged, e)
    assert "loss" not in flagged


def test_loss_on_z_is_flagged():
    flagged, e = _flags(*REF, 1, "loss_on_z")
    assert flagged == {"loss"}, (flagged, e)


def test_dropped_out_shift_is_flagged():
    flagged, e = _flags(*REF, 1, "no_out_shift")
    assert "loss" in flagged, (flagged, e)


def test_padded_tanh_row_leaking_into_b2_is_flagged():
    flagged, e = _flags(*TANH, 10, "tanh_pad_leak")
    assert {"b2", "edge"} <= flagged, (flagged, e)
