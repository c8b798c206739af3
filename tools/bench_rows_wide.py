#!/usr/bin/env python
"""The two passes over stored rollouts at the reference's own configs, route 2 (csrc/rows_wide.h) against route 0 (the generic route,
which is what runs for these shapes without the _wide entries): mjx_rollout_disagreement_wide and mjx_path_rewards_wide, each alone
in HIP-event pairs with its MJX_..._WIDE switch alternating between 1 and 0 in one process, at
    (n, m) = (11, 2), dynamics 256 x 256, reward 100 x 100, K = 4, N = 250, H = 50     (reacher.txt, point_mass.txt)
    (n, m) = (17, 6), the same nets and counts
Disagreement reads P = K N paths of H rows (all members' rollouts back to back) under each of the K members; path rewards read
N H rows per member.  Per entry and shape: the median of --pairs (>= 50) event pairs per side after warm-up, the spread of route 0
against itself (the medians of its odd and its even samples, as a share), each side's algorithmic FLOPs (2 x the products of the
nets' layers per row-forward, counted from shapes) over its time and that rate's share of the fp32-MFMA peak (157.3 TFLOP/s,
v_mfma_f32_32x32x2_f32 dense).  Prints one JSON line.
    python tools/bench_rows_wide.py [--pairs 60]
MJX_LIB=<another libmjx.so> times another build (a -DMJX_RW_NS=1 build: the 32-row tile); "tile_rows" in the line is what the
library itself answers (mjx_rows_wide_tile_rows) and "lib" the file name of the library that ran."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import LIB_PATH, check, load, ptr  # noqa: E402

PAIRS = max(50, int(sys.argv[sys.argv.index("--pairs") + 1])) if "--pairs" in sys.argv else 60
FP32_MFMA_PEAK_TF = 157.3
K, N, H = 4, 250, 50
SHAPES = [(11, 2, (256, 256), (100, 100)), (17, 6, (256, 256), (100, 100))]


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def net_flops(sizes):
    return 2 * sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))


def blocks(sizes, rng, dev, tr_floats):
    P = sum(a * b + b for a, b in zip(sizes[:-1], sizes[1:]))
    th = np.concatenate([np.concatenate([rng.uniform(-1, 1, b * a) / np.sqrt(a), rng.uniform(-1, 1, b) / np.sqrt(a)])
                         for a, b in zip(sizes[:-1], sizes[1:])])
    assert th.size == P
    params = torch.from_numpy(np.stack([th * (1 + 0.01 * k) for k in range(K)]).astype(np.float32)).to(dev)
    return params, torch.from_numpy(np.tile(tr_floats.astype(np.float32), (K, 1))).to(dev)


def alternate(call, switch, pairs):
    """event pairs around call() with `switch` alternating 1, 0, 1, 0, ... -> {"1": sorted ms, "0": ms in the order taken}, routes"""
    routes = {}
    for v in ("1", "0", "1", "0", "1", "0"):            # warm-up: both sides' kernels loaded, LDS limits raised, scratch grown
        os.environ[switch] = v
        routes[v] = call()
    torch.cuda.synchronize()
    ev = {"1": [], "0": []}
    for _ in range(pairs):
        for v in ("1", "0"):
            os.environ[switch] = v
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            ev[v].append((a, b))
    torch.cuda.synchronize()
    os.environ.pop(switch)
    return {v: [a.elapsed_time(b) for a, b in ev[v]] for v in ev}, routes


def med(x):
    return float(np.median(x))


def report(ms, routes, flops):
    m1, m0 = med(ms["1"]), med(ms["0"])
    odd, even = med(ms["0"][1::2]), med(ms["0"][0::2])
    rate = lambda t: flops / (t * 1e-3) / 1e12      # noqa: E731
    return dict(route2_ms=m1, route0_ms=m0, speedup=m0 / m1, route0_self_spread=abs(odd - even) / m0, route2_min_ms=float(min(ms["1"])),
                route0_min_ms=float(min(ms["0"])), routes=[routes["1"], routes["0"]], gflop=flops / 1e9,
                route2_TFLOPs=rate(m1), route0_TFLOPs=rate(m0), route2_frac_of_fp32_mfma_peak=rate(m1) / FP32_MFMA_PEAK_TF,
                route0_frac_of_fp32_mfma_peak=rate(m0) / FP32_MFMA_PEAK_TF,
                faster_by_more_than_spread=bool(m1 < m0 * (1 - abs(odd - even) / m0)), pairs=len(ms["1"]))


def main():
    assert torch.cuda.is_available(), "bench_rows_wide.py needs a GPU"
    dev = torch.device("cuda", 0)
    lib = load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = dict(tool="bench_rows_wide", K=K, N=N, H=H, tile_rows=int(lib.mjx_rows_wide_tile_rows()), lib=os.path.basename(LIB_PATH), shapes={})
    for n, m, dh, rh in SHAPES:
        rng = np.random.RandomState(100 + n)
        ds, rs = (n + m,) + dh + (n,), (2 * n + m,) + rh + (1,)
        dtr = np.concatenate([np.zeros(n + m), np.ones(n + m), np.full(n, -0.02), np.full(n, 0.3)])
        rtr = np.concatenate([np.zeros(2 * n + m), np.ones(2 * n + m), [0.1], [1.5]])
        dP, dT = blocks(ds, rng, dev, dtr)
        rP, rT = blocks(rs, rng, dev, rtr)
        obs = torch.from_numpy(rng.randn(K, N, H, n).astype(np.float32)).to(dev)
        act = torch.from_numpy(rng.randn(K, N, H, m).astype(np.float32)).to(dev)
        err = torch.empty((K * N, H - 1), device=dev)
        r32 = torch.empty((K, N, H), device=dev)
        route = ctypes.c_int(-1)

        def dis():
            check(lib.mjx_rollout_disagreement_wide(ptr(obs), ptr(act), K * N, H, K, ints(ds), 4, ptr(dP), ptr(dT), 0, 7, ptr(err),
                                                    ctypes.byref(route), st))
            return route.value

        def rew():
            check(lib.mjx_path_rewards_wide(ptr(obs), ptr(act), N * H * m, N * H, K, ints(ds), 4, ptr(dP), ptr(dT), 0, 7, ints(rs), 4, ptr(rP),
                                            ptr(rT), 0, ptr(r32), None, ctypes.byref(route), st))
            return route.value

        # disagreement: K members x (K N H) rows, the rows of t = H - 1 included on route 2 (computed, never stored); counted as route 0
        # computes it: K x K N (H - 1) row-forwards.  Path rewards: K x N H rows through both nets.
        d_ms, d_routes = alternate(dis, "MJX_ROLLOUT_DISAGREE_WIDE", PAIRS)
        r_ms, r_routes = alternate(rew, "MJX_PATH_REWARDS_WIDE", PAIRS)
        out["shapes"]["%d_%d" % (n, m)] = dict(
            dyn=list(ds), rew=list(rs),
            disagreement=report(d_ms, d_routes, K * K * N * (H - 1) * net_flops(ds)),
            rewards=report(r_ms, r_routes, K * N * H * (net_flops(ds) + net_flops(rs))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
