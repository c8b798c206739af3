"""k_path_rewards<HB, NB, RB> (csrc/path_reward.h) and mjx_path_rewards' launch and route-0 helper kernels per tile walk, transform
and width edge, against the fp64 chain per member (tests/_mpc_learned_oracle.ensemble_rewards).  tests/test_gpu_path_rewards.py
proves the seven shapes the feature needed; at those every wave owns at most one tile, the s' columns of the reward transform equal
the s columns, ract equals dact, at most two action slot groups are live, and only flags 7 and 3 run.  Here the inputs can tell those
apart.  Cases, seeded recipe and check functions: tests/_path_reward_cases.py; every check runs in ONE fresh worker process under a
time limit (tests/_path_reward_matrix_worker.py; it took 2.5 s on the MI355X, 0.9 s of it after the imports; the limit is 120 s); a worker that
failed is not started again -- the remaining tests fail with its output.  tests/test_path_reward_checks.py shows on the CPU that
these checks pass a NumPy emulation of the kernel's data movement and flag the defects a wrong kernel would leave.

Recipe: _mpc_learned_oracle.kernel_case's, with the s' shift and scale drawn on their own, dact and ract apart, and wherever the mask
flag is on one dynamics out_scale entry exactly 0 beside an out_shift of +-0.4.

Axis cases, K = 2, 165 rows (five tiles and a partial one) and 6 rows, shared actions (stride 0) and per-member actions, all on
route 1 by the image arithmetic (asserted on the CPU with mjx_path_rewards_route):
    a1  (6, 2)    64 x 64 ReLU    100 x 100 ReLU  flags 7  <2,1,4> 113.3 KiB  the planner's shape with distinct s' transforms
    a2  (11, 17)  64 x 32 ReLU    128 x 7 tanh    flags 5  <2,1,4>  85.5 KiB  three action slot groups; 4 reward blocks beside 1; mixed activations
    a3  (11, 25)  32 x 64 tanh    5 x 128 ReLU    flags 1  <2,1,4>  68.0 KiB  four slot groups; 1 reward block beside 4 (T2 = 36, not 132)
    a4  (39, 28)  96 x 32 ReLU    64 x 128 ReLU   flags 7  <3,2,4> 158.5 KiB  the largest served image found; m = 28; the Adroit dims
    a5  (8, 8)    32 x 32 tanh    128 x 128 tanh  flags 3  <1,1,4>  94.1 KiB  no padding anywhere: n8 = n, m8 = m, unpadded widths
    a6  (1, 1)    32 x 32 ReLU    1 x 1 tanh      flags 7  <1,1,4>  21.0 KiB  smallest everything
    a7  (17, 6)   128 x 128 ReLU  64 x 1 tanh     flags 7  <4,1,2> 126.7 KiB  the RB = 2 instance, g2 = 1
    a8  (32, 8)   96 x 96 tanh    33 x 32 ReLU    flags 0  <3,1,4>  96.6 KiB  n = 32 (one state block exactly full); no output affine
    a9  (33, 1)   96 x 96 ReLU    64 x 65 ReLU    flags 7  <3,2,4> 134.3 KiB  one feature in the second state block; m = 1; g2 = 65
    a10 (64, 32)  64 x 64 ReLU    64 x 64 ReLU    flags 7  <2,2,4> 121.3 KiB  n and m at the route's limits; residual over 64 states
Geometry cases.  The host launches min(ceil(rows / 128), ceil(CUs / K)) workgroups per member and wave w of a member's 4 x grid waves
owns tiles w, w + 4 grid, ...; the worker reads the CU count from the device, forms that arithmetic (_path_reward_cases.walk) and
reports the most and the fewest tiles of any wave that owns one.  The tests assert that every such wave owns at least 2 and, at 256
CUs, the numbers below, so a case cannot quietly stop covering the loop on another part:
    g1  a1's shape, K 64, 1 200 rows, both action modes      cap 4 workgroups; 38 tiles over 16 waves: 3 or 2 each; the last tile has 16 rows
    g2  (6, 2) 32 x 32 ReLU, 36 x 72 tanh, K 300, 300 rows   K > CUs, cap 1; 10 tiles over 4 waves (3, 3, 2, 2); the last tile has 12 rows; per-member actions
    g3  (6, 2) 32 x 32 ReLU, 32 x 32 ReLU, K 64, 16 400 rows K x rows = 1 049 600 > 2^20: k_pr_widen and both gathers take a second grid-stride
                                                             pass; 513 tiles over 16 waves: 33 or 32 each; shared actions
g3 meets fp64 on a fixed subset of rows of every member (the first tile, the last two tiles, every 64th row: rows are independent,
so the oracle runs on the subset alone, and so does the yardstick); the routes meet each other on all rows, route 0's fp32 output
equals two mjx_dyn_forward calls over [s, a] and [s, a, s'] rows assembled by torch bit for bit (the header's promise), and r64 is
r32 widened.

Every output block is prefilled with NaN and carries 64 NaN guard elements behind the last member's last row: every element inside
must be overwritten (a tile that no wave owns) and every guard element untouched (a store from a lane beyond `rows`).

Bars: the error is the largest absolute error over the compared rows of all members relative to the largest absolute reward
(_mpc_learned_oracle.rel_max), the largest over row sets and action modes; the yardstick is the unmodified reference's own fp32 result
on the same inputs against the same fp64 oracle, measured in the same way on the CPU (tests/golden/make_golden_path_reward_matrix.py
-> tests/golden/path_reward_matrix.npz, "kref_<case>"); the bar is 3 x that (tests/test_gpu_path_rewards.py's MARGIN: two fp32
chains of equal length in different summation orders differ by a small multiple), for each route against fp64 and for the routes
against each other.  Measured on the MI355X [in brackets: route 1 / route 0; the routes against each other]:
    a1   yardstick 1.216e-7  bar 3.647e-7  [1.394e-7 / 1.839e-7; 1.537e-7]
    a2   yardstick 3.251e-7  bar 9.754e-7  [2.541e-7 / 3.892e-7; 2.725e-7]
    a3   yardstick 1.614e-7  bar 4.842e-7  [1.614e-7 / 3.155e-7; 3.985e-7]
    a4   yardstick 7.458e-8  bar 2.238e-7  [7.455e-8 / 8.437e-8; 1.031e-7]
    a5   yardstick 1.365e-7  bar 4.094e-7  [1.241e-7 / 1.348e-7; 1.615e-7]
    a6   yardstick 7.582e-8  bar 2.275e-7  [8.287e-8 / 8.287e-8; 1.036e-7]
    a7   yardstick 1.431e-7  bar 4.292e-7  [1.541e-7 / 1.691e-7; 1.641e-7]
    a8   yardstick 1.542e-7  bar 4.627e-7  [1.429e-7 / 1.429e-7; 1.364e-7]
    a9   yardstick 1.946e-7  bar 5.839e-7  [1.789e-7 / 3.125e-7; 2.371e-7]
    a10  yardstick 2.113e-7  bar 6.339e-7  [2.350e-7 / 2.537e-7; 2.805e-7]
    g1   yardstick 1.285e-7  bar 3.856e-7  [1.349e-7 / 1.730e-7; 1.841e-7]
    g2   yardstick 9.882e-8  bar 2.965e-7  [1.035e-7 / 1.390e-7; 1.683e-7]
    g3   yardstick 1.019e-7  bar 3.057e-7  [9.126e-8 / 9.948e-8; 1.511e-7]
[no unwritten element and no touched guard element in 88 calls; at 256 CUs the walks are g1 (4, 3, 2, 16), g2 (1, 3, 2, 12),
g3 (4, 33, 32, 16): workgroups per member, most and fewest tiles of a wave that owns any, rows of the last tile.  No defect found.]"""
import os
import sys

import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _path_reward_cases as C  # noqa: E402

LIMIT = 120

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_path_reward_matrix_worker.py", LIMIT, "path-reward matrix")


def _checks(case):
    rec = _result()["cases"][case]
    print(case, "yardstick %.3e bar %.3e" % (C.kref(case), C.MARGIN * C.kref(case)), rec)
    return C.checks(case, rec, C.kref(case)), rec


@pytest.mark.parametrize("case", C.ORDER)
def test_route_1_against_fp64_per_member(case):
    assert _checks(case)[0]["mfma"]


@pytest.mark.parametrize("case", C.ORDER)
def test_route_0_against_fp64_per_member(case):
    """MJX_PATH_REWARDS_MFMA=0: the gathers, k_dyn_forward over [s, a], then over [s, a, s']"""
    assert _checks(case)[0]["generic"]


@pytest.mark.parametrize("case", C.ORDER)
def test_routes_agree(case):
    assert _checks(case)[0]["routes"]


@pytest.mark.parametrize("case", C.ORDER)
def test_every_row_is_written_and_no_guard_element(case):
    ok, rec = _checks(case)
    assert rec["unwritten"] == 0 and rec["guard"] == 0 and ok["written"]


@pytest.mark.parametrize("case", C.ORDER)
def test_route_1_really_runs_its_own_kernel(case):
    """equal bits between the routes on a row set of 32 rows or more would be a quiet fallback; route_out names the route that
    mjx_path_rewards_route promised (1) and the switch forced (0)"""
    ok, rec = _checks(case)
    assert _result()["served"][case] == 1
    assert rec["same_bits"] == [] and ok["own_kernel"] and ok["route_out"]


@pytest.mark.parametrize("case", C.ORDER)
def test_fp64_output_is_the_fp32_output_widened(case):
    assert _checks(case)[0]["widened"]


@pytest.mark.parametrize("case", C.GEOM)
def test_waves_walk_more_than_one_tile(case):
    """from the CU count of the device the worker ran on: every wave that owns a tile owns at least two, and the numbers are the
    host arithmetic's; at 256 CUs they are the table's"""
    r = _result()
    ok, rec = _checks(case)
    c = C.CASES[case]
    got = rec["walk"][str(c["rows"][0])]
    print(case, "CUs", r["cus"], "grid, most, fewest, rows of the last tile:", got)
    assert got == C.walk_numbers(C.walk(c["rows"][0], c["K"], r["cus"]))
    assert got[2] >= 2 and ok["walk"]
    if r["cus"] == 256:
        assert tuple(got) == C.WALK_AT_256[case]


def test_g3_route_0_is_two_dyn_forward_calls_bit_for_bit():
    assert _result()["g3_two_forwards_same_bits"] is True
