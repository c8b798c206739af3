"""The cached Fisher-vector product on bf16x3 MFMAs (csrc/fused_policy.h, k_fused<..., BF3 = true>): against the fp64 oracle, and
against the fp32 kernel (MJX_FVP_BF16X3=0).  The switch is read once per process, so both kernels run in child processes; every
comparison with the fp32 kernel also asserts that the bits differ, i.e. that the switch selected a different kernel for that
instance."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import npg_oracle as O
from oracle import synth
from tests._worker_run import run_child

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HID = (64, 64)
TOL_FVP = 3e-6
# every instance that takes the bf16x3 kernel: compile-time widths 8 (n 4, 7), 12 (n 9, 11), 20 (n 17, 19), runtime width (n 23)
INSTANCES = [(17, 6), (4, 1), (7, 8), (9, 6), (11, 1), (19, 8), (23, 6)]

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_fvp_bf16x3 import cached_products
out = {}
for k, spec in enumerate(json.loads(sys.argv[2])):
    for key, val in cached_products(**spec).items():
        out["%d_%s" % (k, key)] = val
np.savez(sys.argv[3], **out)
"""


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def case(n, m, N, seed=0, wscale=1.0, source="randn"):
    """(obs, act, adv, theta, v); source "bench": bench.py's 1M-timestep batch and initial parameters"""
    rng = np.random.RandomState(seed)
    if source == "bench":
        sys.path.insert(0, ROOT)
        import bench
        obs, act, adv = bench.synth_shard(0, 1)
        adv = ((adv - adv.mean()) / (adv.std() + 1e-6)).astype(np.float32)
        th = bench.initial_params().astype(np.float32)
        return obs, act, adv, th, rng.randn(th.size).astype(np.float32)
    obs = rng.randn(N, n).astype(np.float32)
    act = rng.randn(N, m).astype(np.float32)
    adv = rng.randn(N).astype(np.float32)
    th = synth.perturbed_params(synth.init_params(n, m, HID)).astype(np.float32)
    if wscale != 1.0:                          # large hidden weights: saturated tanh units
        fo = n * HID[0] + HID[0]
        th[:fo] *= np.float32(wscale)
        th[fo:fo + HID[1] * HID[0]] *= np.float32(wscale)
    v = rng.randn(th.size).astype(np.float32)
    return obs, act, adv, th, v


def cached_products(n, m, N, seed=0, wscale=1.0, scales=(1.0,), reps=1, source="randn"):
    """K1 (fills the caches), then the cached product of v * s for every s (and `reps` launches of the first one)."""
    import torch
    from mjrl_amd.engine import UpdateEngine
    obs, act, adv, th, v = case(n, m, N, seed, wscale, source)
    n, m = obs.shape[1], act.shape[1]
    tr = np.concatenate([np.zeros(n), np.ones(n), np.zeros(m), np.ones(m)]).astype(np.float32)
    eng = UpdateEngine(n, m, HID)
    assert eng.fused
    eng.set_policy(th, th, tr, tr)
    eng.set_batch(obs, act, adv)
    eng.surr_vpg()
    out = {}
    for i, s in enumerate(scales):
        vt = torch.from_numpy(v * np.float32(s)).to(eng.device)
        out["h%d" % i] = eng.fvp(vt).cpu().numpy().copy()
    vt = torch.from_numpy(v).to(eng.device)
    for r in range(reps):
        out["rep%d" % r] = eng.fvp(vt).cpu().numpy().copy()
    eng.close()
    return out


def in_children(tmp_path, specs):
    """-> (bf16x3 results, fp32 results): one child process per kernel, each running every spec"""
    res = []
    for on in (1, 0):
        path = os.path.join(str(tmp_path), "out_%d.npz" % on)
        run_child([sys.executable, "-c", _CHILD, ROOT, json.dumps(specs), path], 900, "MJX_FVP_BF16X3 = %d" % on,
                  env={"MJX_FVP_BF16X3": str(on)}, cwd=ROOT)
        res.append(dict(np.load(path)))
    return res


def oracle(n, m, N, seed=0, wscale=1.0):
    obs, act, adv, th, v = case(n, m, N, seed, wscale)
    return O.fvp(th.astype(np.float64), obs.astype(np.float64), v.astype(np.float64), n, m, HID)


def test_bf16x3_every_instance_vs_fp64_and_fp32(tmp_path):
    """every bf16x3 instance at 20 k rows against the fp64 oracle, and against the fp32 kernel (different bits: the bf16x3
    kernel ran; close: within 1e-6)"""
    specs = [dict(n=n, m=m, N=20000) for n, m in INSTANCES]
    a, b = in_children(tmp_path, specs)
    for k, (n, m) in enumerate(INSTANCES):
        h, h32 = a["%d_h0" % k], b["%d_h0" % k]
        assert not np.array_equal(h, h32), ("the switch selected the same kernel", n, m)
        assert rel(h, h32) < 1e-6, (n, m)
        assert rel(h, oracle(n, m, 20000)) < TOL_FVP, (n, m)


def test_bf16x3_200k_scale_and_zero():
    """200 k rows at v scaled by 1e-8, 1, 1e8 (the split is exact at any exponent); v = 0 gives exactly 0"""
    n, m, N = 17, 6, 200000
    out = cached_products(n, m, N, seed=1, scales=(1e-8, 1.0, 1e8, 0.0))
    ref = oracle(n, m, N, seed=1)
    for i, s in enumerate((1e-8, 1.0, 1e8)):
        assert rel(out["h%d" % i] / s, ref) < TOL_FVP, s
    assert not np.any(out["h3"])


def test_bf16x3_saturated_units():
    n, m, N = 17, 6, 20000
    h = cached_products(n, m, N, seed=2, wscale=8.0)["h0"]
    assert rel(h, oracle(n, m, N, seed=2, wscale=8.0)) < TOL_FVP


@pytest.mark.parametrize("N", [31, 32, 33])
def test_bf16x3_partial_tiles(N):
    h = cached_products(17, 6, N, seed=3)["h0"]
    assert rel(h, oracle(17, 6, N, seed=3)) < TOL_FVP


def test_bf16x3_vs_fp32_kernel_bench_batch(tmp_path):
    """bench.py's 1M-timestep batch (bench.synth_shard) and a batch of 1M - 7 rows (a partial last tile): the bf16x3 kernel
    against the fp32 one at 1e-6; launches of the same sweep direction are bitwise equal, the other direction within 1e-6"""
    specs = [dict(n=17, m=6, N=0, seed=4, reps=3, source="bench"), dict(n=17, m=6, N=1000000 - 7, seed=4, reps=3)]
    a, b = in_children(tmp_path, specs)
    for k in range(2):
        h, h32 = a["%d_h0" % k], b["%d_h0" % k]
        assert not np.array_equal(h, h32), "the switch selected the same kernel"
        assert rel(h, h32) < 1e-6
        assert np.array_equal(h, a["%d_rep1" % k]) and np.array_equal(a["%d_rep0" % k], a["%d_rep2" % k])
        assert rel(a["%d_rep0" % k], h) < 1e-6


def test_bf16x3_properties():
    """linearity, symmetry, PSD at 100 k rows"""
    import torch
    from mjrl_amd.engine import UpdateEngine
    n, m, N = 17, 6, 100000
    obs, act, adv, th, v = case(n, m, N, seed=5)
    tr = np.concatenate([np.zeros(n), np.ones(n), np.zeros(m), np.ones(m)]).astype(np.float32)
    eng = UpdateEngine(n, m, HID)
    eng.set_policy(th, th, tr, tr)
    eng.set_batch(obs, act, adv)
    eng.surr_vpg()
    rng = np.random.RandomState(6)
    v1 = torch.from_numpy(rng.randn(th.size).astype(np.float32)).to(eng.device)
    v2 = torch.from_numpy(rng.randn(th.size).astype(np.float32)).to(eng.device)
    h1, h2 = eng.fvp(v1).clone(), eng.fvp(v2).clone()
    h12 = eng.fvp(2.0 * v1 - 0.5 * v2).clone()
    assert rel(h12.cpu().numpy(), (2.0 * h1 - 0.5 * h2).cpu().numpy()) < 2e-6
    a, b = float(torch.dot(v1.double(), h2.double())), float(torch.dot(v2.double(), h1.double()))
    assert abs(a - b) < 1e-5 * max(abs(a), abs(b), 1e-12)
    assert float(torch.dot(v1.double(), h1.double())) > 0
    eng.close()
