"""ModelAccelNPG.get_refined_action on the MI355X against the unmodified reference's pieces (tests/golden/refine.npz,
tests/golden/make_golden_refine.py) call by call on both rollout routes, the host reward callable against the fp64 restatement,
the members' pack key, and the neighbours that must not change.  Every check runs in ONE fresh worker process under a time limit
(tests/_refine_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.

The action must lie within 1e-5 relative L2 of the reference's (the project's TOL_STEP; the reference itself is at most 1.3e-6
from the fp64 restatement on these inputs, tests/test_refine_cpu.py) and R within tests/test_gpu_mpc.py's BAR_R.  Measured on the
MI355X: action at most 9.3e-7 (case ra, route 1), R at most 2.8e-7 (case ra, route 0); the host-callable action 3.4e-8 from fp64."""
import os
import sys

import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refine_oracle as F  # noqa: E402

TOL_STEP = 1e-5
BAR_R = 5.9e-7                # tests/test_gpu_mpc.py's bar on the same quantity


def _result():
    return worker_result("_refine_worker.py", 300, "refine")


KEYS = ["%s%s_%d" % (case, route, c) for case in sorted(F.RCASES) for route in "10" for c in range(F.RCALLS)]


@pytest.mark.gpu
def test_refined_action_agrees_with_the_reference_call_by_call():
    """cases ra and rb (rb: omega 5, the per-trajectory disagreement term), two calls each after torch.manual_seed(s), on the MFMA
    route and under MJX_POLICY_ROLLOUT_MFMA=0"""
    r = _result()
    assert set(r["fixture"]) == set(KEYS)
    for k in KEYS:
        e_a, e_R = r["fixture"][k]
        print("%s: action %.2e  R %.2e  route %d" % (k, e_a, e_R, r["routes"][k]))
        assert e_a < TOL_STEP and e_R < BAR_R, k
        assert r["routes"][k] == int(k[2]), k


@pytest.mark.gpu
def test_torch_stream_after_a_refined_call_is_the_references():
    r = _result()["after"]
    assert set(r) == set(KEYS) and all(r.values())


@pytest.mark.gpu
def test_host_reward_function_gives_the_same_action():
    """members that do not learn rewards: the callable is asked once per member, as train_step asks it, and with the members' own
    reward chain inside it the action is the fp64 restatement's; with neither source the call raises ValueError"""
    r = _result()
    print(r["callable"])
    assert r["callable"][0] < TOL_STEP and r["callable"][1] == 3
    assert r["neither"] == "ValueError"


@pytest.mark.gpu
def test_members_are_packed_once_and_again_after_a_fit():
    """once over two calls; again after a member's fit_dynamics and after a fit_reward (the action moves with them); not for a
    policy.set_param_values, which every call reads afresh and which changes the action"""
    r = _result()
    assert r["packs_two_calls"] == 1
    assert r["packs"] == [1, 2, 3, 3]
    assert r["same_call_same_action"]
    assert all(v > 0.0 for v in r["moved"]), r["moved"]


@pytest.mark.gpu
def test_neighbours_are_unchanged():
    """refine=False hands policy.get_action's value on; train_step runs on the same object after refined calls; the agent pickles
    without its device blocks and the copy acts"""
    r = _result()
    assert r["unrefined"] and r["train_step"] and r["pickle"] and r["pickle_acts"]
