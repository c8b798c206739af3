"""GPU worker for tests/test_gpu_fit_exchange.py: the wide and the team trainer of the MLP baseline share ONE uncached exchange block
and arrival counter per thread and device (csrc/fit_host.h fit_exchange).  One thread, one stream: wide fit A, team fit B, A again,
B again, every run from the same initial parameters and moments; prints one RESULT JSON line with the routes, whether the two runs
of each fit agree bit for bit (parameters, both moments, epoch losses) and whether every loss is finite.
python tests/_fit_exchange_worker.py"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mjrl_amd._lib import check, load, ptr  # noqa: E402
from tests import _worker_dev as W  # noqa: E402
from tests._dyn_check import rand_theta  # noqa: E402

HID, LR, WD = (128, 128), 1e-3, 1e-3
# name: (d_in, batch, N, seed) -- A: two workgroups on the wide route (56: the first width the one-workgroup layout no longer holds);
# B: two workgroups of a team; two steps, one epoch each
FITS = {"A": (56, 64, 192, 7101), "B": (9, 128, 384, 7102)}

lib = load()


def inputs(d_in, batch, N, seed):
    rng = np.random.RandomState(seed)
    th = rand_theta(rng, [d_in, 128, 128, 1])
    return dict(th=th, x=W.up(rng.randn(N, d_in), keep=True), y=W.up(1.0 + rng.randn(N), keep=True),
                perm=W.up(rng.permutation(N), np.int32, keep=True))


def route(d_in, batch, N):
    out = (ctypes.c_int32 * 6)()
    check(lib.mjx_mlp_fit_route(d_in, W.ints(HID), 2, batch, N, 1, out))
    return list(out)[:4]


def fit(d_in, batch, N, D):
    """-> [params, m, v, losses] on the host, after one epoch from D's initial parameters and zero moments"""
    bufs = [W.up(D["th"], keep=True), W.up(np.zeros(D["th"].size), keep=True), W.up(np.zeros(D["th"].size), keep=True),
            W.up([np.nan], np.float64, keep=True)]
    check(lib.mjx_mlp_fit_adam(ptr(D["x"]), ptr(D["y"]), N, d_in, W.ints(HID), 2, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), 0, ptr(D["perm"]), 1,
                               batch, LR, WD, ptr(bufs[3]), W.stream()))
    return bufs


data = {k: inputs(*FITS[k]) for k in FITS}
runs = {k: [] for k in FITS}
for k in ("A", "B", "A", "B"):                       # enqueued back to back on one stream: nothing waits in between
    runs[k].append(fit(*FITS[k][:3], data[k]))
torch.cuda.synchronize()
W.emit({"routes": {k: route(*FITS[k][:3]) for k in FITS},
        "bitwise": {k: [W.same_bits(a, b) for a, b in zip(*runs[k])] for k in FITS},
        "finite": {k: [bool(torch.isfinite(r[3]).all()) for r in runs[k]] for k in FITS},
        "moved": {k: not W.same_bits(runs[k][0][0], data[k]["th"]) for k in FITS}})
