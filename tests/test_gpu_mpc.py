"""MPC planning on the MI355X (csrc/plan.h, mjrl_amd/algos/model_accel/model_learning_mpc.py): mjx_plan_rollout on both routes
against the fp64 oracle step by step, the routes against each other, mjx_plan_score against NumPy fp64, and
MPCPolicy.get_action against the unmodified reference's fixtures (tests/golden/mpc.npz, tests/golden/make_golden_mpc.py) call
by call and chained under warm start.  Every check runs in ONE fresh worker process under a time limit (tests/_mpc_worker.py);
a worker that failed is not started again -- the remaining tests fail with its output.

The planned sequence and the returned action must lie within 1e-5 relative L2 of the reference's (the project's TOL_STEP for an
update direction; the reference itself is at most 3.1e-6 from the fp64 restatement on these inputs, tests/test_mpc_cpu.py).
Every other bar is 3x the error measured on the MI355X against the oracle or the fixture (in brackets); BAR_BARE_R and BAR_REFIT_R
take BAR_R: the same quantity (measured since: in their brackets)."""
import os
import sys

import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mpc_oracle as M  # noqa: E402

TOL_STEP = 1e-5
BAR_STEP_MFMA = 7.8e-7        # [2.6e-7: case b; the edge shapes 2.4e-7]
BAR_STEP_GENERIC = 6.9e-7     # [2.3e-7: case b]
BAR_FREE_MFMA = 9.2e-7        # [3.1e-7: case d (the generic kernel on both sides); the MFMA kernel's largest 2.8e-7, case c at H = 32]
BAR_FREE_GENERIC = 9.2e-7     # [3.1e-7: case d]
BAR_ROUTES = 7.2e-7           # [2.4e-7 between the routes: case c]
BAR_SCORE = 8.7e-15           # [2.9e-15]
BAR_R = 5.9e-7                # [1.95e-7: case f on the generic route; 1.5e-7 on the MFMA route]
# three chained calls: 3x the measured 3.7e-6 (case c, generic route; 2.6e-6 on the MFMA route) would exceed TOL_STEP, so TOL_STEP it is.
# The reference's own third call is 3.1e-6 from fp64 here (tests/test_mpc_cpu.py): the distance is the two fp32 rollouts', not drift.
BAR_CHAINED = TOL_STEP
BAR_BARE_R = 5.9e-7           # the same quantity as BAR_R (R of an fp32 rollout against fp64, relative to max |R|): its bar; [1.1e-7]
BAR_REFIT_R = 5.9e-7          # as BAR_BARE_R; [3.5e-8]


def _result():
    return worker_result("_mpc_worker.py", 600, "mpc")


MFMA_CASES = sorted(c for c in M.CASES if M.ROUTES[c])


@pytest.mark.gpu
def test_mfma_rollout_step_by_step_against_fp64():
    """every fixture case (the generic case d included: MJX_PLAN_MFMA=1 leaves it on the generic route), N = 1, 31, 32, 33, 129,
    H = 1 and 7, s0 as one state and as (N, n), ReLU / tanh, flags 7 / 3 / 1 / 5 ("edge"), and the instances no case reaches
    ("wide": <4, 2> at [96, 128, 128, 64], <1, 2> at [45, 32, 32, 40], <3, 2> at [42, 96, 64, 33]): every stored state against one
    fp64 step from the stored state before it"""
    r = _result()["rollout_step_mfma"]
    print(r)
    assert set(r) == set(M.CASES) | {"edge", "wide"}
    assert max(r.values()) < BAR_STEP_MFMA


@pytest.mark.gpu
def test_generic_rollout_step_by_step_against_fp64():
    """the same cases and shapes with MJX_PLAN_MFMA=0: k_model_rollout with the actions given"""
    r = _result()["rollout_step_generic"]
    print(r)
    assert set(r) == set(M.CASES) | {"edge", "wide"}
    assert max(r.values()) < BAR_STEP_GENERIC


@pytest.mark.gpu
def test_free_running_rollouts_against_fp64():
    """the whole H-step rollout against the free-running fp64 rollout, per route"""
    r = _result()
    print(r["rollout_free_mfma"], r["rollout_free_generic"])
    assert max(r["rollout_free_mfma"].values()) < BAR_FREE_MFMA
    assert max(r["rollout_free_generic"].values()) < BAR_FREE_GENERIC


@pytest.mark.gpu
def test_masked_output_column_is_exact_and_empty_calls_return():
    r = _result()
    assert r["masked_exact"] is True
    assert r["empty_ok"] == [0, 0]


@pytest.mark.gpu
def test_routes_agree_on_the_mfma_eligible_cases():
    r = _result()["routes"]
    print(r)
    assert set(r) == set(MFMA_CASES) | {"edge", "wide"}
    assert max(r.values()) < BAR_ROUTES


@pytest.mark.gpu
def test_the_mfma_route_really_runs_its_own_kernel():
    """mjx_plan_rollout falls back to the generic kernel when the LDS limit cannot be raised.  Two kernels with different
    summation orders never agree to the bit over thousands of values, so equal bits on an eligible shape mean that both sides
    ran k_model_rollout and the tests above compared it with itself."""
    assert _result()["routes_same_bits"] == []


@pytest.mark.gpu
def test_plan_score_against_numpy_fp64():
    """R relative to max |R|, S absolute (S <= 1), the sequence relative L2: the reference's index and the per-trajectory one,
    K = 1, no disagreement term, N below the workgroup size and above it"""
    assert _result()["score"] < BAR_SCORE


@pytest.mark.gpu
def test_get_action_agrees_with_the_reference_call_by_call():
    """each of the three calls of each case from the fixture's input act_sequence: the planned sequence (returned action + the
    shifted act_sequence) and the action within TOL_STEP, R relative to max |R|; on the generic route too where the MFMA route
    serves the case"""
    r = _result()
    print(r["policy_seq"], r["policy_action"], r["policy_R"])
    assert set(r["policy_seq"]) == set(M.CASES) | {c + "_generic" for c in MFMA_CASES}
    assert max(r["policy_seq"].values()) < TOL_STEP         # [MFMA route 4.0e-6, generic route 6.2e-6: both case c]
    assert max(r["policy_action"].values()) < TOL_STEP      # [MFMA route 5.0e-6, generic route 7.8e-6: both case c]
    assert max(r["policy_R"].values()) < BAR_R


@pytest.mark.gpu
def test_numpy_stream_after_get_action_is_the_references():
    assert _result()["streams_equal"] is True


@pytest.mark.gpu
def test_three_chained_calls_under_warm_start():
    r = _result()["chained_seq"]
    print(r)
    assert set(r) == set(M.CASES) | {c + "_generic" for c in MFMA_CASES}
    assert max(r.values()) < BAR_CHAINED


@pytest.mark.gpu
def test_members_are_packed_once_and_again_when_a_parameter_changes():
    assert _result()["repack"] == [True, True, True]


@pytest.mark.gpu
def test_a_refit_member_is_planned_on_with_its_new_weights():
    """WorldModel.fit_dynamics(..., set_transformations=False) on one member between two get_action calls: the device copy is
    made again and the second call agrees with the fp64 restatement on the NEW weights and not with the one on the old"""
    r = _result()["refit"]
    print(r)
    assert r["repacked"] is True and r["moved"] > 1e-3 and r["ess"] >= 5.0
    assert r["action_vs_new"] < TOL_STEP                    # [2.7e-7]
    assert r["R_vs_new"] < BAR_REFIT_R
    assert r["action_vs_old"] > 10 * TOL_STEP               # the check can tell the two apart [0.29]


@pytest.mark.gpu
def test_bare_world_model_and_per_trajectory_index_against_the_oracle():
    """a bare WorldModel (ReLU 96 x 32 and tanh 32 x 32; the reference raises TypeError there) and reference_indexing=False on the
    fitted ensemble: the returned action (relative L2) and R (relative to max |R|) against the fp64 restatement"""
    r = _result()
    assert r["bare_min_ess"] >= 5.0
    assert r["bare_action"] < TOL_STEP                      # [2.0e-6 was the larger of this and the R error below]
    assert r["bare_R"] < BAR_BARE_R
