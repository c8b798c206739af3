"""The per-block / per-row / per-column / per-entry checks of tests/test_gpu_gemm_chain.py can fail: fp64 results with the defects a
wrong launch path leaves behind are flagged at the bars that module uses, and an fp64 result rounded to fp32 level passes.
CPU only."""
import numpy as np
import pytest

from oracle import npg_oracle as O
from oracle import synth
from tests._lw_check import fine_errors, over_bars
from tests.test_gpu_gemm_chain import BARS

n, m, hid = 11, 3, (320, 50)          # W2 is 50 x 320: a 256-column block plus a 128-column remainder launch on the device


def _inputs(N, seed):
    rng = np.random.RandomState(seed)
    th = synth.perturbed_params(synth.init_params(n, m, hid), scale=0.05).astype(np.float64)
    th2 = th + 0.004 * rng.randn(th.size)
    tr = O.Transforms(n, m, 0.1 * rng.randn(n), 1 + 0.1 * rng.rand(n), 0.05 * rng.randn(m), 1 + 0.2 * rng.rand(m))
    obs, act, adv = rng.randn(N, n), rng.randn(N, m), rng.randn(N)
    return th, th2, tr, obs, act, adv


def _vpg(N, seed, drop=()):
    """K1 with the samples in `drop` left out (their advantage zeroed: the same 1 / N, no contribution)"""
    th, th2, tr, obs, act, adv = _inputs(N, seed)
    adv = adv.copy()
    adv[list(drop)] = 0.0
    return O.vpg(th2, th, obs, act, adv, n, m, hid, tr, tr)


def _views(g):
    Ws, bs, s = O.unflatten(g, n, m, hid)
    return Ws, bs, s


def _defects():
    ref600, ref129 = _vpg(600, 1), _vpg(129, 2)
    out = []
    d = ref600.copy()                                         # one weight block without one 128-row tile of samples
    _views(d)[0][0][:] = _views(_vpg(600, 1, drop=range(128, 256)))[0][0]
    out.append(("W1 without rows 128..255", d, ref600))
    d = ref129.copy()                                         # the last sample of N = 129 dropped from one block
    _views(d)[0][1][:] = _views(_vpg(129, 2, drop=[128]))[0][1]
    out.append(("W2 without row 128 of 129", d, ref129))
    d = ref600.copy()                                         # one 128-column slab of the 320-column block zeroed
    _views(d)[0][1][:, 128:256] = 0.0
    out.append(("W2 columns 128..255 zeroed", d, ref600))
    d = ref600.copy()                                         # one output row (weights and bias) swapped with its neighbour
    W3, b3 = _views(d)[0][2], _views(d)[1][2]
    W3[[1, 2]] = W3[[2, 1]]
    b3[[1, 2]] = b3[[2, 1]]
    out.append(("output rows 1 and 2 swapped", d, ref600))
    d = ref600.copy()                                         # a bias sum that lost one row block
    _views(d)[1][0][:] = _views(_vpg(600, 1, drop=range(0, 128)))[1][0]
    out.append(("b1 without row block 0", d, ref600))
    return out


@pytest.mark.parametrize("case", range(5))
def test_each_defect_is_flagged(case):
    label, dev, ref = _defects()[case]
    bad = over_bars(fine_errors(dev, ref, n, m, hid), BARS["g2"])
    assert bad, label


def test_fp32_rounding_passes():
    ref = _vpg(600, 1)
    dev = ref.astype(np.float32).astype(np.float64) * (1 + 1e-7 * np.random.RandomState(3).randn(ref.size))
    worst = fine_errors(dev, ref, n, m, hid)
    assert not over_bars(worst, BARS["g2"]), worst
    for k in ("hv", "gh"):
        assert not over_bars(worst, BARS[k]), (k, worst)
