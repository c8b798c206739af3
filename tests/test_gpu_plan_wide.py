"""mjx_plan_rollout_wide (csrc/plan_wide.h) on the MI355X: every stored state of every case of tests/_plan_wide_cases.py against fp64
on route 2 and on route 0 (the same entry under MJX_PLAN_WIDE=0), the routes against each other, route reporting, bit-level
properties and MPCPolicy end to end on 256 x 256 members.  Every check runs in ONE fresh worker process under a time limit
(tests/_plan_wide_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.

The bars are 3 x the unmodified reference's own fp32 error on the same quantity (tests/golden/plan_wide.npz, written by
tests/golden/make_golden_plan_wide.py; the project's rule in tests/test_gpu_path_rewards.py), never a multiple of anything the kernel
produced.  No case and no column is left out of a bar but the zero-scale column under the mask flag, which is asserted exactly.
Measured on the MI355X: every case takes between 0.24 (q5) and 0.54 (q4) of its bar on route 2 and between 0.28 and 0.54 on route 0,
the routes against each other at most 0.51 of theirs (g1), the planner end to end at most 0.68 (the sequence on learned rewards).

Why each case is there (each the smallest shape that has its edge; H = 5 unless said):
  q1  (11, 2) 256 x 256 ReLU flags 7, K 3, 33 rows, s0 one and rows: the reference's config; one tile per wave per layer; a second
      workgroup with one row
  q2  (6, 2) 256 x 256 tanh flags 3, 65 rows: mask without residual; a third workgroup
  q3  (17, 6) 160 x 96 ReLU flags 5, K 2, 31 rows: ragged, unequal widths; under one tile
  q4  (1, 1) 129 x 1 tanh flags 1, one row: a one-unit layer, one row
  q5  (64, 64) 256 x 256 ReLU flags 0, 32 rows: n, m and n + m at their limits; the largest LDS layout
  q6  (33, 9) 100 x 200 ReLU flags 7, K 2, 64 rows: n in a second 32-block; h1 < h2; zero column 16
  q7  (17, 6) 64 x 64 tanh flags 7, 33 rows: a shape route 1 serves: the wide entry reports 2, and 1 under MJX_PLAN_WIDE=0
  q8  (6, 2) 256 x 256 ReLU flags 7, 32 rows, H = 1: only s0 stored, compared exactly
  g1  q1's shape, K 5, 417 rows, H = 3: five members, 14 tiles each
  f1  q1's nets, 33 rows, H = 16, free-running"""
import os
import sys

import numpy as np
import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _plan_wide_cases as C  # noqa: E402

G = np.load(C.FIXTURE)
BARRED = [c for c in C.ORDER if C.CASES[c]["H"] > 1]


def _result():
    return worker_result("_plan_wide_worker.py", 300, "wide plan rollout")


def _checks(case):
    rec = _result()["rec"][case]
    for line in rec["runs"]:
        print(line)
    return rec, C.checks(case, rec, C.yard(case) if C.CASES[case]["H"] > 1 else None)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["wide", "generic"])
@pytest.mark.parametrize("case", BARRED)
def test_every_stored_state_against_fp64(case, route):
    """one fp64 step from the stored state before it, per column (f1: the free-running fp64 rollout), within 3 x the reference's own
    fp32 distance"""
    rec, ok = _checks(case)
    print("%s %s: %.3e (bar %.3e)" % (case, route, rec["err"]["2" if route == "wide" else "0"], C.MARGIN * C.yard(case)))
    assert ok[route]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BARRED)
def test_routes_agree_with_each_other(case):
    """route 2 against route 0 over every stored state, within the sum of their bars"""
    rec, ok = _checks(case)
    print("%s: %.3e (bar %.3e)" % (case, rec["routes"], 2 * C.MARGIN * C.yard(case)))
    assert ok["routes"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", C.ORDER)
def test_blocks_written_s0_first_and_masked_column_exact(case):
    """no element unwritten and no guard touched in any block; every member's obs[:, :, 0] is s0; the zero-scale column is exact under
    the mask flag (0 of either sign under flags 3, s0's column under flags 7)"""
    rec, ok = _checks(case)
    assert rec["calls"] == 2 * len(C.CASES[case]["s0"])
    assert ok["written"] and ok["s0"] and ok["masked"]


@pytest.mark.gpu
def test_h1_returns_s0_exactly():
    assert _result()["h1_s0_exact"] is True


@pytest.mark.gpu
def test_route_reporting():
    """route_out is 2 on every case and agrees with the route function; under MJX_PLAN_WIDE=0 the outputs are mjx_plan_rollout's bit
    for bit with route 0 (1 on q7); under MJX_PLAN_MFMA=0 the route is 0; routes 2 and 0 differ in their bits on at least one case"""
    r = _result()
    for case in C.ORDER:
        narrow = C.NARROW_ROUTE[case]
        assert r["route_fn"][case] == 1 and r["narrow_fn"][case] == narrow, case
        assert r["route_out"][case] == [[2], [narrow], narrow, 0], case
        assert r["switch_bits"][case] is True, case
    assert any(not r["rec"][case]["same_bits"] for case in BARRED)


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    assert _result()["repeat"] is True


@pytest.mark.gpu
def test_one_start_state_equals_the_same_state_tiled():
    assert _result()["s0_tiled"] is True


@pytest.mark.gpu
def test_a_nan_trajectory_stays_alone():
    """a NaN in row 40 of q2's s0: every other row's bits are the clean run's, row 40's stored s0 is NaN and the guards are intact
    (asserted by the worker)"""
    assert _result()["nan"] == dict(others=True, s0_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("reward", ["learned", "env"])
def test_mpc_policy_end_to_end_on_wide_members(reward):
    """two WorldModel(6, 2, hidden_size=(256, 256), learn_reward=True) with seeded parameters, MPCPolicy(wide=True) with N 40, H 8: route(),
    reward_route() and last_routes() report 2, and 0 under MJX_PLAN_WIDE=0 plus MJX_PATH_REWARDS_WIDE=0; on both settings the scores
    and the planned sequence are within 3 x the reference's own fp32 planner's distance from the fp64 oracle"""
    py = _result()["python"]
    bar_R, bar_seq = C.MARGIN * float(G[C.mpc_key("R", reward)]), C.MARGIN * float(G[C.mpc_key("seq", reward)])
    for setting, route in (("wide", 2), ("narrow", 0)):
        p = py["%s_%s" % (reward, setting)]
        print("%s %s: R %.3e (bar %.3e)  seq %.3e (bar %.3e)  ESS %.1f" % (reward, setting, p["R"], bar_R, p["seq"], bar_seq, p["ess"]))
        assert p["route"] == route and p["last"]["rollout"] == route
        if reward == "learned":
            assert p["reward_route"] == route and p["last"]["rewards"] == route
        else:
            assert p["reward_route"] is None and p["last"]["rewards"] is None
        assert p["R"] <= bar_R and p["seq"] <= bar_seq
