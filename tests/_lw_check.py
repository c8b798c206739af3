"""Comparison helpers of the layer-wise fp64 tests (test_gpu_dispatch_matrix.py, test_gpu_gemm_chain.py): the blocks of the flat
parameter vector and the relative errors of a device result against the fp64 oracle, block by block and finer.

The finer checks exist because a whole-vector or whole-block norm absorbs an error that sits in one place: a wrong 128-column
remainder slab, a dropped partial row tile, a misplaced split, a bias sum that loses one row block.  tests/test_gemm_chain_checks.py
shows on CPU that each of those defects is flagged at the bars the GPU tests use."""
import numpy as np

from oracle import npg_oracle as O


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def out_layer_offsets(n, m, hid):
    """-> (offset of the output layer's weights, offset of its bias) in the flat parameter vector"""
    ls = O.layer_sizes(n, m, hid)
    k = sum(ls[i] * ls[i + 1] + ls[i + 1] for i in range(len(ls) - 2))
    return k, k + ls[-2] * m


def blocks(n, m, hid):
    """(label, index) of every block of the flat vector: W / b of each hidden layer, each output row with its bias, log_std"""
    ls = O.layer_sizes(n, m, hid)
    out, k = [], 0
    for i in range(len(ls) - 2):
        out.append(("W%d" % (i + 1), np.arange(k, k + ls[i] * ls[i + 1]))); k += ls[i] * ls[i + 1]
        out.append(("b%d" % (i + 1), np.arange(k, k + ls[i + 1]))); k += ls[i + 1]
    oW, ob = out_layer_offsets(n, m, hid)
    h = ls[-2]
    for a in range(m):
        out.append(("row%d" % a, np.r_[oW + a * h:oW + (a + 1) * h, ob + a]))
    out.append(("log_std", np.arange(ob + m, ob + 2 * m)))
    return out


def block_errors(dev, ref, n, m, hid):
    return {lab: rel(dev[ix], ref[ix]) for lab, ix in blocks(n, m, hid)}


def _floored(err, ref):
    """err / max(ref, rms(ref)) elementwise: the error of a row / column over its own size, but not over less than the block's
    typical size -- a row that is small through cancellation (at N = 1 a weight gradient is rank one, and delta_i or x_j may be
    a sum that nearly cancels) carries the absolute rounding of a typical row, not a larger relative one; a defect moves a row
    by about its typical size and stays O(1)"""
    return err / np.maximum(ref, np.sqrt(np.mean(ref * ref)))


def fine_errors(dev, ref, n, m, hid):
    """-> {"block": (worst error, where), "row": ..., "col": ..., "entry": ...} of a flat gradient-shaped result:
         block  relative L2 of every block of blocks(): hidden W_l, b_l, log_std, and each output row with its bias (over the
                larger of its norm and the rms of the output rows' norms)
         row    L2 error of every row (output unit) of every weight block, the output layer's included, over its norm (_floored)
         col    the same for every column (input unit) of every weight block
         entry  |dev - ref| of every bias entry (b_l, the output bias, log_std) over the rms of its vector"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    Wd, bd, sd = O.unflatten(dev, n, m, hid)
    Wr, br, sr = O.unflatten(ref, n, m, hid)
    worst = {}

    def put(key, errs, label):
        i = int(np.argmax(errs))
        if key not in worst or errs[i] > worst[key][0]:
            worst[key] = (float(errs[i]), label(i))

    bl = blocks(n, m, hid)
    rows = [(lab, ix) for lab, ix in bl if lab.startswith("row")]
    rn = np.array([np.linalg.norm(ref[ix]) for _, ix in rows])
    put("block", _floored(np.array([np.linalg.norm(dev[ix] - ref[ix]) for _, ix in rows]), rn), lambda i: rows[i][0])
    other = [(lab, ix) for lab, ix in bl if not lab.startswith("row")]
    put("block", np.array([rel(dev[ix], ref[ix]) for _, ix in other]), lambda i: other[i][0])
    for l, (a, b) in enumerate(zip(Wd, Wr)):
        put("row", _floored(np.linalg.norm(a - b, axis=1), np.linalg.norm(b, axis=1)), lambda i: "W%d row %d" % (l + 1, i))
        put("col", _floored(np.linalg.norm(a - b, axis=0), np.linalg.norm(b, axis=0)), lambda i: "W%d col %d" % (l + 1, i))
    for lab, a, b in [("b%d" % (l + 1), x, y) for l, (x, y) in enumerate(zip(bd, br))] + [("log_std", sd, sr)]:
        put("entry", np.abs(a - b) / np.sqrt(np.mean(b * b)), lambda i: "%s[%d]" % (lab, i))
    return worst


def row_errors(dev, ref):
    """worst L2 error over the rows of an (N, m) result (the policy's means), each over its norm (_floored) -> (error, row)"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    e = _floored(np.linalg.norm(dev - ref, axis=1), np.linalg.norm(ref, axis=1))
    return float(e.max()), int(e.argmax())


def over_bars(worst, bars):
    """the entries of fine_errors() at or above their bar: [] when the result passes"""
    return [(k, e, where, bars[k]) for k, (e, where) in sorted(worst.items()) if not e < bars[k]]
