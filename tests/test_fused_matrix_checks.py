"""The per-block / per-row / per-column / per-entry checks of tests/test_gpu_fused_matrix.py can fail: fp64 results with the defects
a wrong fused instance or row edge leaves behind are flagged at the bars that module uses, and the fp32 oracle's results on the
same inputs pass.  CPU only."""
import functools

import numpy as np
import pytest

from oracle import npg_oracle as O
from tests._fused_matrix_worker import fused_inputs, n_big
from tests._lw_check import fine_errors, out_layer_offsets, over_bars
from tests.test_gpu_fused_matrix import BAR_CAP, BARS

N_BIG = n_big(256)                     # 65 569 rows


@functools.lru_cache(maxsize=None)
def _inputs(n, m, hid, N):
    inp = fused_inputs(n, m, hid, N, n * 100 + m + N)
    f = {k: inp[k].astype(np.float64) for k in ("th", "th2", "obs", "act", "adv", "v")}
    f["tr"] = inp["tr"]
    return f


def _vpg(n, m, hid, N, drop=(), dtype=np.float64, old_is_new=True):
    """K1 with the samples in `drop` left out (their advantage zeroed: the same 1 / N, no contribution)"""
    f = _inputs(n, m, hid, N)
    adv = f["adv"].copy()
    adv[list(drop)] = 0.0
    tr = f["tr"] if dtype == np.float64 else O.Transforms(n, m, f["tr"].in_shift, f["tr"].in_scale, f["tr"].out_shift, f["tr"].out_scale,
                                                          dtype=dtype)
    c = lambda a: a.astype(dtype)
    return O.vpg(c(f["th"] if old_is_new else f["th2"]), c(f["th"]), c(f["obs"]), c(f["act"]), c(adv), n, m, hid, tr, tr).astype(np.float64)


def _fvp(n, m, hid, N, dtype=np.float64):
    f = _inputs(n, m, hid, N)
    tr = f["tr"] if dtype == np.float64 else O.Transforms(n, m, f["tr"].in_shift, f["tr"].in_scale, f["tr"].out_shift, f["tr"].out_scale,
                                                          dtype=dtype)
    return O.fvp(f["th"].astype(dtype), f["obs"].astype(dtype), f["v"].astype(dtype), n, m, hid, tr).astype(np.float64)


def _w1(g, n, m, hid):
    return O.unflatten(g, n, m, hid)[0][0]


def _b1(g, n, m, hid):
    return O.unflatten(g, n, m, hid)[1][0]


A = (17, 6, (64, 64))                  # the flagship instance (NPC 20)
B = (59, 32, (32, 32))                 # the 32-action variant at its widest


def _defects(case):
    if case == 0:                      # row 32 of 33 dropped from W1 only (a partial second tile lost in one accumulator)
        ref = _vpg(*A, 33)
        d = ref.copy()
        _w1(d, *A)[:] = _w1(_vpg(*A, 33, drop=[32]), *A)
        return "W1 without row 32 of 33", d, ref, A
    if case == 1:                      # the last 33 rows of N_big dropped (the partial last tile of a wave's second round)
        ref = _vpg(*A, N_BIG)
        return "last 33 rows of N_big dropped", _vpg(*A, N_BIG, drop=range(N_BIG - 33, N_BIG)), ref, A
    n, m, hid = B
    ref = _vpg(*B, 3000 + n)
    d = ref.copy()
    oW, ob = out_layer_offsets(n, m, hid)
    h = hid[-1]
    if case == 2:                      # output rows m - 2 and m - 1 swapped at m = 32
        W3, b3 = O.unflatten(d, n, m, hid)[0][2], O.unflatten(d, n, m, hid)[1][2]
        W3[[m - 2, m - 1]] = W3[[m - 1, m - 2]]
        b3[[m - 2, m - 1]] = b3[[m - 1, m - 2]]
        return "output rows 30 and 31 swapped", d, ref, B
    if case == 3:                      # one b3 entry zeroed
        d[ob + m - 1] = 0.0
        return "b3[31] zeroed", d, ref, B
    if case == 4:                      # one log_std entry taken from its neighbour
        d[ob + m + 17] = ref[ob + m + 16]
        return "log_std[17] from log_std[16]", d, ref, B
    # the bias column of W1 computed without one 32-row tile
    _b1(d, *B)[:] = _b1(_vpg(*B, 3000 + n, drop=range(64, 96)), *B)
    return "b1 without rows 64..95", d, ref, B


@pytest.mark.parametrize("case", range(6))
def test_each_defect_is_flagged(case):
    label, dev, ref, (n, m, hid) = _defects(case)
    worst = fine_errors(dev, ref, n, m, hid)
    for kind in BARS:                  # (the defect sits in a gradient-shaped vector: flagged at every result kind's bars)
        assert over_bars(worst, BARS[kind]), (label, kind, worst)


def test_unflatten_returns_views():
    """(the defects above are written through O.unflatten's blocks)"""
    g = np.zeros(O.num_params(*A))
    _w1(g, *A)[:] = 1.0
    assert g[:A[0] * 64].all() and not g[A[0] * 64:].any()


@pytest.mark.parametrize("shape,N", [(A, 1), (A, 33), (A, 3017), (B, 1), (B, 31), (B, 3059), ((1, 1, (64, 64)), 3001),
                                     ((23, 8, (64, 64)), 33), ((17, 16, (64, 64)), 3017), ((63, 8, (32, 32)), 3063)])
def test_fp32_oracle_passes(shape, N):
    n, m, hid = shape
    for kind, f64, f32 in (("g", _vpg(n, m, hid, N), _vpg(n, m, hid, N, dtype=np.float32)),
                           ("hv", _fvp(n, m, hid, N), _fvp(n, m, hid, N, dtype=np.float32)),
                           ("g2", _vpg(n, m, hid, N, old_is_new=False), _vpg(n, m, hid, N, dtype=np.float32, old_is_new=False))):
        worst = fine_errors(f32, f64, n, m, hid)
        print(shape, N, kind, worst)
        assert not over_bars(worst, BARS[kind]), (kind, worst)


def test_no_bar_above_the_cap():
    assert all(b <= BAR_CAP for kind in BARS.values() for b in kind.values())
