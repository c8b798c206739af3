"""Learned path rewards on the MI355X (csrc/path_reward.h, mjx_path_rewards) and MPCPolicy(reward='learned'): the kernel on both
routes against the fp64 oracle per member (tests/_mpc_learned_oracle.py), the routes against each other and against
ensemble_path_rewards, and the planner on an environment with NO compute_path_rewards against the unmodified reference's fixture
(tests/golden/mpc_learned.npz, tests/golden/make_golden_mpc_learned.py).  Every check runs in ONE fresh worker process under a time
limit (tests/_path_reward_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.

Kernel bars: the error is the largest absolute error over the rows relative to the largest absolute reward; the yardstick is the
unmodified reference's own fp32 result on the same inputs against the same fp64 oracle, computed on the CPU by the generator and
kept in the fixture ("kref_<case>"), measured there exactly as the worker measures the kernel (per row set and action mode over all
members' rows, the largest of those): k1 1.41e-7, k2 3.54e-7, k3 1.08e-7.  The bar is 3 x that, because two fp32 chains of equal
length in different summation orders differ by a small multiple.  Measured on the MI355X [in brackets, MFMA route / generic route]:
    k1  bar 4.22e-7  [1.55e-7 / 1.61e-7; the routes against each other 2.0e-7]
    k2  bar 1.06e-6  [3.08e-7 / 4.04e-7; 3.9e-7]
    k3  bar 3.23e-7  [9.4e-8 / 1.35e-7; 9.8e-8]
k4 .. k7 run the four instances that k1 .. k3 do not reach, one member each, under the same rule (yardsticks 4.80e-7, 1.62e-7,
7.6e-8, 2.18e-7):
    k4  bar 1.44e-6  [3.2e-7 / 4.0e-7; 4.9e-7]
    k5  bar 4.85e-7  [1.67e-7 / 1.34e-7; 2.1e-7]
    k6  bar 2.28e-7  [7.4e-8 / 1.03e-7; 9.9e-8]
    k7  bar 6.53e-7  [1.92e-7 / 1.65e-7; 2.3e-7]
Planner bars: the planned sequence within 1e-5 relative L2 of the reference's (TOL_STEP); R within tests/test_gpu_mpc.py's scoring
bar BAR_R = 5.9e-7, here relative to R's SPREAD (max R - min R), which is what moves the softmax weights.  Under NumPy 2 the
reference rounds every gamma ** t * r to fp32 (r is np.float32 and a Python float times it stays fp32) before it adds it to the fp64
score, while mjx_plan_score forms the product in fp64: that rounding, at most 2^-25 of each term, is part of the observed distance
[R / spread: la 2.9e-7 on the MFMA reward route, 3.2e-7 on the generic one; lb 4.5e-7 / 4.7e-7;
the planned sequence at most 3.6e-7 call by call and 4.3e-7 over three chained calls; the member rewards against the reference's
4.6e-7 .. 1.2e-6 of the largest reward: two fp32 chains on two fp32 rollouts]."""
import os
import sys

import numpy as np
import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mpc_learned_oracle as L  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "mpc_learned.npz"))
TOL_STEP = 1e-5
BAR_R = 5.9e-7                # tests/test_gpu_mpc.py's BAR_R
MARGIN = 3.0


def _bar(case):
    return MARGIN * float(G["kref_" + case])


def _result():
    return worker_result("_path_reward_worker.py", 600, "path-reward")


PLAN_NAMES = set(L.PLAN_CASES) | {c + "_generic" for c in L.PLAN_CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(L.KCASES))
def test_mfma_kernel_against_fp64_per_member(case):
    """k_path_rewards: 165 rows (N = 33, H = 5: five tiles and a partial one) and 6 rows (under one tile), shared actions (stride 0)
    and per-member actions, every member against its own fp64 chain.  k1: the planner's shape; k2: padding in n8, m8, HB and both
    ragged reward widths, tanh, a masked dynamics output column; k3: two state blocks, m8 = 16; k4 .. k7: the instances <2, 2, 4>,
    <3, 2, 4>, <4, 1, 2> and <4, 2, 2>"""
    r = _result()
    print(case, r["kernel_mfma"][case], "yardstick", r["kref"][case])
    assert r["kref"][case] == float(G["kref_" + case])
    assert r["kernel_mfma"][case] < _bar(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(L.KCASES))
def test_generic_route_against_fp64_per_member(case):
    """the same cases with MJX_PATH_REWARDS_MFMA=0: k_dyn_forward over [s, a], then over [s, a, s']"""
    r = _result()
    print(case, r["kernel_generic"][case])
    assert r["kernel_generic"][case] < _bar(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(L.KCASES))
def test_routes_agree(case):
    r = _result()
    print(case, r["routes"][case])
    assert r["routes"][case] < _bar(case)


@pytest.mark.gpu
def test_the_mfma_route_really_runs_its_own_kernel():
    """mjx_path_rewards falls back to the generic route when the LDS limit cannot be raised: equal bits over hundreds of values
    would mean that both sides ran the same kernel.  route_out must name the route mjx_path_rewards_route promised"""
    r = _result()
    assert r["routes_same_bits"] == []
    assert r["route_out_ok"] is True


@pytest.mark.gpu
def test_outputs_fp64_is_fp32_widened_and_either_may_be_left_out():
    r = _result()
    assert r["widened_exact"] is True           # (... and every row was written: the blocks start as NaN)
    assert r["single_output_ok"] is True
    assert r["empty_ok"] == [0, 1]


@pytest.mark.gpu
def test_route_0_is_ensemble_path_rewards_bit_for_bit():
    """forced by the switch on a served shape, and by the shape (dynamics 256 x 256), with per-member and with shared actions;
    ensemble_path_rewards_device's fp64 copy is its fp32 result widened, and members packed once give the same bits"""
    b = _result()["route0_bits"]
    assert b == dict(forced=True, mfma_differs=True, want64=True, packed=True, unserved=True, unserved_shared=True)


@pytest.mark.gpu
def test_planner_on_learned_rewards_without_compute_path_rewards():
    """MPCPolicy(reward='learned') on an environment object that has no compute_path_rewards, each of the three calls of each case
    from the fixture's input act_sequence, on both reward routes: the planned sequence and R against the reference's"""
    r = _result()
    print(r["policy_seq"], r["policy_R"], r["policy_rewards"])
    assert set(r["policy_seq"]) == PLAN_NAMES
    assert r["last_rewards_ok"] is True
    assert max(r["policy_seq"].values()) < TOL_STEP
    assert max(r["policy_R"].values()) < BAR_R


@pytest.mark.gpu
def test_numpy_stream_after_a_learned_reward_call_is_the_references():
    assert _result()["streams_equal"] is True


@pytest.mark.gpu
def test_three_chained_calls_on_learned_rewards():
    r = _result()["chained_seq"]
    print(r)
    assert set(r) == PLAN_NAMES
    assert max(r.values()) < TOL_STEP


@pytest.mark.gpu
def test_bare_world_model_on_learned_rewards_against_the_oracle():
    """K = 1 and no disagreement term (the reference raises TypeError on a bare model): the action (relative L2) and R (relative
    to max |R|, tests/test_gpu_mpc.py's BAR_BARE_R) against the fp64 restatement"""
    r = _result()["bare"]
    print(r)
    assert r["ess"] >= 5.0
    assert r["action"] < TOL_STEP
    assert r["R"] < BAR_R


@pytest.mark.gpu
def test_a_refit_reward_net_is_planned_on_with_its_new_weights():
    """WorldModel.fit_reward(..., set_transformations=False) on one member between two get_action calls: the device copy is made
    again (and only then), the other members' rewards keep their bits, and the planner's rewards agree with the fp64
    chain on the NEW weights and not with the one on the old.  Both chains run on the observations of the planner's own rollout,
    so the distance is the kernel's alone.  Its yardstick is the reference's own fp32 distance from fp64 on the same rows of
    this very call (case lb, call 0, the fixture's members: "lb_0_pref" = 4.63e-7, measured by the generator on the reference's
    own observations as the kernel cases' yardsticks are; the largest reward there is 0.31, so an absolute error like k1's is a
    larger share of it than in k1, whose random nets do not stand for these inputs); the bar is 3 x that, before the refit, and
    after it, where one member's reward weights have moved by fit steps on data of the same kind.
    [before 4.73e-7, after 4.47e-7; against the old weights 0.27]"""
    r = _result()["refit"]
    print(r)
    assert r["same_before"] is True and r["repacked"] is True and r["moved"] > 1e-3 and r["others_unchanged"] is True
    assert r["pref"] == float(G["lb_0_pref"])
    assert r["rewards_before"] < MARGIN * float(G["lb_0_pref"])
    assert r["rewards_vs_new"] < MARGIN * float(G["lb_0_pref"])
    assert r["rewards_vs_old"] > 10 * MARGIN * float(G["lb_0_pref"])
    assert r["action_vs_new"] < TOL_STEP


@pytest.mark.gpu
def test_reward_env_is_still_todays_planner():
    """reward='env' (the default) on case a of tests/golden/mpc.npz within tests/test_gpu_mpc.py's bars"""
    r = _result()["env_mode"]
    print(r)
    assert r["streams"] is True and r["no_rewards"] is True
    assert r["seq"] < TOL_STEP
    assert r["R"] < BAR_R
