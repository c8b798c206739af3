"""Every launch path of the layer-wise hidden-layer chain (LayerwiseWS, csrc/layerwise.h; routes csrc/lw_plan.h, launcher
csrc/lw_launch.h, kernels csrc/lw_gemm.h and csrc/lw_gemm_p.h) against the fp64 oracle, block by block, row by row and column by
column.

The device runs go through tests/_gemm_chain_worker.py in child processes, one per arm, with MJX_FORCE_LAYERWISE=1 and the
arm's switches in the child's environment (MJX_LW_WT and MJX_LW_OLD_OUTPUTS are read once per process, every other MJX_LW_*
switch at the start of each operation: the table in csrc/lw_plan.h).  Each case checks the policy's means
(mjx_policy_forward) row by row; K1 with an explicit old network, K2 at old == new and the general Hessian (old != new, the new
network with transforms of its own) against the fp64 oracle per block, per weight row, per weight column and per bias entry
(tests/_lw_check.fine_errors); K3's surrogate and KL at the bars of test_other_shapes_vs_oracle.

Routes at the default switches (n, m, hidden; N = 3000 + n unless noted).  "fwd" = forward / tangent products (M = N rows,
N = the layer's units), "delta" = the delta product towards the layer below, "wgrad" = weight gradients split over samples.
Which product shape reaches which kernel instance, grid and column slice -- at the defaults and under every switch below that
changes a route -- is asserted without a GPU by tests/test_lw_plan_cpu.py (table in tests/c/lw_plan.cpp); the table here says
which of those routes each case is there to reach.

    case       n, m, hidden            kernels reached (kernel trace of the default worker)
    odd        11, 3, (100, 50)        ldx 12: padded first layer (k_pad_rows, k_unpad_rows); k_gemm<128, 128, 512> forward /
                                       tangent / delta; thin k_gemm<128, 128, 256> for the 50 x 100 gradient, k_gemm<128, 64, 256>
                                       for the general Hessian's 3 x 50; narrow transposed output gradient k_gemm<128, 32, 256>
                                       (mode-2 operands: oW[2] = 6250); generic output chain; k_reduce_split and k_reduce_split4
    rem        39, 28, (320, 192)      320 = k_gemm<128, 256, 512> + a 128-column k_gemm<128, 128, 512> launch; 192 = one padded
                                       256 block; W_1^T (Wt) on the general kernel; thin k_gemm<128, 64, 256> first-layer
                                       gradient (39 -> 64 columns); generic output chain (192 is not a multiple of 128)
    h384       64, 8, (384, 384)       256 + 128 remainder launches everywhere, no persistent launch (384 % 256 != 0); k_lw_head<3>
    humanoid   376, 17, (256, 256)     k_gemm_p<0, BIAS_TANH / TANGENT / BACK> (the delta product reads Wt); 376 -> 384 padded
                                       first layer; 384-column first-layer gradient as 256 + 128 launches; k_lw_head8<1, 9>.
                                       N = 255: no persistent launch (M < 256); N = 256: persistent
    wide       12, 6, (1024, 1024)     k_gemm_p<0, *> over 4 column blocks; k_gemm<128, 256, 512> gradients; generic output chain
                                       (last hidden layer > 512)
    deep       24, 4, (256, 128, 64)   k_gemm_p<0, BACK> at layer 1 (Wt); thin k_gemm<128, 128, 256> / <128, 64, 256>;
                                       generic output chain (last hidden layer 64)
    small      17, 6, (32, 32)         k_gemm<128, 32, 256> for every product; k_colsum_narrow<32>
    m33, m64   20, 33 / 64, (128, 128) k_head with one sample per wave (m > 32); output bias through k_colsum; thin
                                       k_gemm<128, 128, 256> output gradient; generic output chain (m > 32)
    one        33, 2, (128,)           k_lw_head<1> (nL() = 2: the fused output pass runs), then backward(l_start = 0)
    mis128     12, 3, (50, 128)        last hidden 128 but oW[1] = 650 is not a multiple of 4: generic output chain, mode-2
                                       B operands; thin k_gemm<128, 64, 256> for the 128 x 50 gradient
    every case                         the general Hessian: EPI_RBACK, k_hvp_head, k_scale_dtanh, k_colsum + k_reduce_split

Edges (N): 1 and 127 / 128 / 129 (partial and whole 128-row tiles), 255 / 256 / 257 (persistent needs M >= 256), 1024 / 1025 (one
split writes the block, two go through the split reduction), 4096 / 4097 (bias sum of the top delta in one launch or 256 splits),
131072 / 131073 (1024 row blocks of column sums in the delta epilogue, or the two-stage sum).

Switch arms (test_arm_vs_oracle, same bars; MJX_LW_WT=0 and MJX_LW_FAST=0 are also compared bit for bit with the default):
    MJX_LW_TILES=0 / 2      128 x 128 tiles (512 / 256 threads); TILES=0 also reduces the splits with scalar k_reduce_split
    MJX_LW_THIN=0           the 33..128-column gradients on the wide tiles
    MJX_LW_THIN64=0         the 33..64-column gradients on k_gemm<128, 128, 256>
    MJX_LW_WT=0             the delta product reads W_l as it lies (k_gemm_p<1, BACK>, mode-1 B on the general kernel)
    MJX_LW_FAST=0           no interior fast k-loop
    MJX_LW_SPLITS=0         the split count without pick_splits' round balancing
    MJX_LW_CHAIN=256        many short sample splits;  MJX_LW_WG_CAP=64: few long ones
    MJX_LW_OVERLAP=1        weight gradients on a side stream (N >= 65536: the 131072 / 131073 cases)
"""
import functools
import json
import os
import sys

import numpy as np
import pytest

from oracle import npg_oracle as O
from oracle.torch_port import TorchPolicy
from tests._gemm_chain_worker import chain_inputs
from tests._lw_check import fine_errors, over_bars, rel, row_errors
from tests._worker_run import arm_runner, run_child

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

TOL_FVP = 3e-6

SHAPES = {
    "odd": (11, 3, (100, 50)), "rem": (39, 28, (320, 192)), "h384": (64, 8, (384, 384)), "humanoid": (376, 17, (256, 256)),
    "wide": (12, 6, (1024, 1024)), "deep": (24, 4, (256, 128, 64)), "small": (17, 6, (32, 32)), "m33": (20, 33, (128, 128)),
    "m64": (20, 64, (128, 128)), "one": (33, 2, (128,)), "mis128": (12, 3, (50, 128)),
}
EDGES = {
    "odd": (1, 127, 128, 129, 1024, 1025), "humanoid": (1, 129, 255, 256, 257, 1024, 1025), "wide": (255, 257),
    "rem": (129, 1025), "small": (1, 4096, 4097, 131072, 131073), "m33": (4096, 4097), "m64": (1, 129), "deep": (257,),
    "one": (129,),
}
# shapes whose routes the suite reached before (test_other_shapes_vs_oracle, whole-vector checks): the bars below are 3x the
# largest error measured on these
COVERED = ("humanoid", "one", "h384")


def _name(shape, N):
    return "%s_N%d" % (shape, N)


BASE = [_name(s, SHAPES[s][0] + 3000) for s in SHAPES]
DEFAULT_CASES = BASE + [_name(s, N) for s in EDGES for N in EDGES[s]]


def _base(*shapes):
    return [_name(s, SHAPES[s][0] + 3000) for s in shapes]


ARMS = {
    "default": ({}, DEFAULT_CASES),
    "tiles0": ({"MJX_LW_TILES": "0"}, _base("odd", "rem", "h384", "humanoid", "deep", "m33") + ["odd_N1025", "humanoid_N1025"]),
    "tiles2": ({"MJX_LW_TILES": "2"}, _base("odd", "rem", "h384", "humanoid", "deep", "m33") + ["odd_N1025", "humanoid_N1025"]),
    "thin0": ({"MJX_LW_THIN": "0"}, _base("odd", "rem", "deep", "m33", "m64", "mis128")),
    "thin64_0": ({"MJX_LW_THIN64": "0"}, _base("rem", "mis128")),
    "wt0": ({"MJX_LW_WT": "0"}, _base("humanoid", "rem", "deep", "h384", "wide") + ["humanoid_N257", "humanoid_N1025"]),
    "fast0": ({"MJX_LW_FAST": "0"}, DEFAULT_CASES),
    "splits0": ({"MJX_LW_SPLITS": "0"}, _base("humanoid", "odd", "rem", "wide") + ["small_N131073"]),
    "chain256": ({"MJX_LW_CHAIN": "256"}, _base("humanoid", "odd") + ["small_N131073"]),
    "wgcap64": ({"MJX_LW_WG_CAP": "64"}, _base("humanoid", "odd", "wide") + ["small_N131073"]),
    "overlap1": ({"MJX_LW_OVERLAP": "1"}, ["small_N131072", "small_N131073"]),
}
BITWISE_ARMS = ("wt0", "fast0")
ARM_CASES = [(arm, nm) for arm in ARMS if arm != "default" for nm in ARMS[arm][1]]

# stale workspace rows: a larger batch first, then a smaller one whose last 128-row tile is partial (77 rows)
STALE = {"humanoid": (2 * 128 * 3 + 77, 2 * 128 * 8 + 77), "odd": (2 * 128 * 3 + 77, 2 * 128 * 8 + 77)}

# Bars (fine_errors keys): 3x the largest error measured on MI355X over the COVERED shapes at the default switches, all their
# batch sizes included (N = 1 to 3376); in brackets the largest over every case and arm (the wide shape's K1 apart, below):
#   K1 (g2)   block 6.6e-6 (humanoid_N256 b2)       row 4.3e-6 (humanoid_N256)   col 6.8e-6 (humanoid_N1025)  entry 3.1e-5 (humanoid_N256)
#             [<= 0.39 of each bar]
#   K2 (hv)   block 9.6e-7 (humanoid_N1 row 8)      row 1.6e-6 (humanoid_N1)     col 1.6e-6 (humanoid_N1)     entry 2.3e-6 (humanoid_N1)
#             [small_N1: block 1.9e-6, row 1.9e-6, entry 2.8e-6]
#   Hessian   block 1.6e-6 (humanoid_N129 log_std)  row 2.1e-6 (humanoid_N1)     col 2.3e-6 (humanoid_N1024)  entry 6.4e-6 (humanoid_N129)
#   (gh)      [wide_N255: block 4.0e-6, entry 9.2e-6; odd_N1024: col 3.3e-6]
#   forward   1.07e-6 (h384_N3064)  [wide_N3012 2.7e-6]
BARS = {
    "g2": {"block": 2.0e-5, "row": 1.3e-5, "col": 2.1e-5, "entry": 9.4e-5},
    "hv": {"block": 2.9e-6, "row": 4.7e-6, "col": 5.0e-6, "entry": 7.0e-6},
    "gh": {"block": 4.9e-6, "row": 6.4e-6, "col": 6.9e-6, "entry": 1.93e-5},
}
BAR_FWD = 3.3e-6
# The wide shape (1024 x 1024) exceeds the K1 bars: block 2.0e-5, row 1.7e-5, col 2.3e-5, entry 8.2e-5 (wide_N255 / N257), and
# its whole K1 vector (5.8e-6 .. 9.0e-6) the 5e-6 of test_other_shapes_vs_oracle.  Its K2 and Hessian, which run the same GEMM
# chain under a different top delta, sit inside their bars (<= 0.82), so the excess enters through that delta: K1 at old != new
# weighs every sample with exp(LL_new - LL_old) of two forward passes, and the forward means of 1024-term fp32 dot products are
# 2.5x further from fp64 than the covered shapes' (2.7e-6 against 1.07e-6).  test_other_shapes_vs_oracle doubles its K1 bar
# from 256- to 512-wide layers for the same reason; here the K1 bars double above 512.
WIDE_K1 = 2.0


def spec(name):
    shape, N = name.rsplit("_N", 1)
    n, m, hid = SHAPES[shape]
    N = int(N)
    return dict(name=name, n=n, m=m, hid=list(hid), N=N, seed=n * 100 + m + N)


def stale_spec(shape):
    n, m, hid = SHAPES[shape]
    N, N_big = STALE[shape]
    return dict(name="stale_" + shape, n=n, m=m, hid=list(hid), N=N, N_big=N_big, seed=n * 100 + m + N)


# ---------------------------------------------------------------------------------------------------------------- oracle
@functools.lru_cache(maxsize=None)
def oracle(name):
    c = spec(name)
    n, m, hid = c["n"], c["m"], tuple(c["hid"])
    inp = chain_inputs(n, m, hid, c["N"], c["seed"])
    th, t2, tr, tr2 = inp["th"].astype(np.float64), inp["th2"].astype(np.float64), inp["tr"], inp["tr2"]
    obs, act, adv, v = (inp[k].astype(np.float64) for k in ("obs", "act", "adv", "v"))
    gen = TorchPolicy(inp["th2"], n, m, hid, theta_old=inp["th"], tr_new=tr2, tr_old=tr, dtype=np.float64)
    return dict(mu=O.forward(th, obs, n, m, hid, tr), g2=O.vpg(t2, th, obs, act, adv, n, m, hid, tr, tr),
                hv=O.fvp(th, obs, v, n, m, hid, tr), gh=gen.hvp(inp["obs"], inp["act"], inp["v"], 0.0),
                s=O.surrogate(t2, th, obs, act, adv, n, m, hid, tr, tr), kl=O.mean_kl(t2, th, obs, n, m, hid, tr, tr))


def errors(name, r):
    """-> {"fwd": (error, row), "g2" / "hv" / "gh": fine_errors(...)} of one case's device results"""
    c = spec(name)
    n, m, hid = c["n"], c["m"], tuple(c["hid"])
    ref = oracle(name)
    out = {"fwd": row_errors(r["mu"], ref["mu"])}
    for k in ("g2", "hv", "gh"):
        out[k] = fine_errors(r[k], ref[k], n, m, hid)
    return out


# ---------------------------------------------------------------------------------------------------------------- runs
def _run_worker(kind, arm, specs, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "spec.json")
    with open(path, "w") as f:
        json.dump({"kind": kind, "cases": specs}, f)
    run_child([sys.executable, os.path.join(HERE, "_gemm_chain_worker.py"), path, out_dir], 600, arm,
              env=dict(ARMS[arm][0], MJX_FORCE_LAYERWISE="1"))
    return {c["name"]: dict(np.load(os.path.join(out_dir, c["name"] + ".npz"))) for c in specs}


def _start(arm, out_dir):
    if arm == "stale":
        return _run_worker("stale", "default", [stale_spec(s) for s in STALE], out_dir)
    return _run_worker("cases", arm, [spec(nm) for nm in ARMS[arm][1]], out_dir)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """arm -> {case name: device results}; each arm's worker runs once, on first use ("stale": the stale-row runs), and none
    after one failed (arm_runner)"""
    return arm_runner(_start, lambda arm: str(tmp_path_factory.mktemp(arm)))


def check_case(name, r):
    c = spec(name)
    m, hid = c["m"], c["hid"]
    ref = oracle(name)
    e = errors(name, r)
    assert e["fwd"][0] < BAR_FWD, ("forward", e["fwd"])
    wide = WIDE_K1 if max(hid) > 512 else 1.0
    for k in ("g2", "hv", "gh"):
        bad = over_bars(e[k], {key: bar * (wide if k == "g2" else 1.0) for key, bar in BARS[k].items()})
        assert not bad, (k, bad)
    # whole-vector and K3 bars of test_other_shapes_vs_oracle
    assert rel(r["hv"], ref["hv"]) < TOL_FVP, "K2"
    assert rel(r["g2"], ref["g2"]) < wide * (5e-6 if m <= 16 else 1e-5 if max(hid) <= 256 else 2e-5), "K1 old != new"
    assert abs(float(r["s"]) - ref["s"]) < 5e-6
    assert abs(float(r["kl"]) - ref["kl"]) < 2e-5 * ref["kl"] + 1e-7


@pytest.mark.parametrize("name", DEFAULT_CASES)
def test_chain_vs_oracle(runs, name):
    check_case(name, runs("default")[name])


@pytest.mark.parametrize("arm,name", ARM_CASES)
def test_arm_vs_oracle(runs, arm, name):
    check_case(name, runs(arm)[name])


@pytest.mark.parametrize("arm,name", [(a, nm) for a, nm in ARM_CASES if a in BITWISE_ARMS])
def test_arm_is_bit_identical(runs, arm, name):
    """MJX_LW_WT=0: the delta product reads W_l as it lies instead of its transpose -- the same MFMAs in the same k-order;
    MJX_LW_FAST=0: the interior tiles through the edge-safe k-loop -- the same MFMA chain"""
    a, b = runs("default")[name], runs(arm)[name]
    for k in ("mu", "g2", "hv", "gh", "s", "kl"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shape", sorted(STALE))
def test_stale_workspace_rows_are_never_summed(runs, shape):
    """the padding rows of the workspace ("computed, never summed": reserve(), the persistent kernel, the delta epilogue) hold the
    rows of a larger batch bound before: K1, K3, K2 and the general Hessian are bit for bit those of a fresh engine"""
    r = runs("stale")["stale_" + shape]
    for k in ("g2", "s", "kl", "hv", "gh"):
        assert np.array_equal(r["fresh_" + k], r["used_" + k]), k
    assert np.abs(r["fresh_hv"]).max() > 0 and np.isfinite(r["fresh_gh"]).all()
