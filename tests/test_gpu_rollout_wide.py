"""mjx_policy_rollout_wide (csrc/policy_rollout_wide.h) on the MI355X: every stored action and state of every case of
tests/_rollout_wide_cases.py against fp64 on route 2 and on route 0 (the same entry under MJX_POLICY_ROLLOUT_WIDE=0), the routes
against each other, route reporting, bit-level properties and the Python layer that reaches the entry.  Every check runs in ONE fresh
worker process under a time limit (tests/_rollout_wide_worker.py); a worker that failed is not started again -- the remaining tests
fail with its output.

The bars are 3 x the unmodified reference's own fp32 error on the same quantity (tests/golden/rollout_wide.npz, written by
tests/golden/make_golden_rollout_wide.py), never a multiple of anything the kernel produced.  Measured on the MI355X: every case
takes between 0.22 and 0.44 of its bar on either route (w3's actions on route 0 the most), the routes against each other at most
0.40 of theirs (w1's states), free-running w1 at most 0.26 (route 2) and 0.34 (route 0)."""
import os
import sys

import numpy as np
import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rollout_wide_cases as W  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "rollout_wide.npz"))
GR = np.load(os.path.join(ROOT, "tests", "golden", "refine.npz"))
CASES = sorted(W.WCASES)


def _result():
    return worker_result("_rollout_wide_worker.py", 300, "wide rollout")


def _bars(name, g=G):
    return 3.0 * float(g["kya_" + name]), 3.0 * float(g["kys_" + name])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["2", "0"])
@pytest.mark.parametrize("case", CASES)
def test_every_stored_step_against_fp64(case, route):
    """step by step (_refine_oracle.step_errors): within 3 x the reference's own fp32 step error; for the H = 1 case the state
    yardstick is 0 and s0 comes back exact"""
    r = _result()
    e_a, e_s = r["step"][route][case]
    bar_a, bar_s = _bars(case)
    print("%s route %s: action %.2e (bar %.2e)  state %.2e (bar %.2e)" % (case, route, e_a, bar_a, e_s, bar_s))
    assert e_a <= bar_a and e_s <= bar_s
    if W.WCASES[case][8] == 1:
        assert bar_s == 0.0 and e_s == 0.0 and r["h1_s0_exact"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["2", "0"])
def test_free_running_rollout_against_fp64(route):
    """w1 at H = 16 against the fp64 free-running rollout, within 3 x the reference's own distance"""
    e_a, e_o = _result()["free"][route]
    print("route %s: actions %.2e (bar %.2e)  states %.2e (bar %.2e)" % (route, e_a, 3 * float(G["kfree_act"]), e_o, 3 * float(G["kfree_obs"])))
    assert e_a <= 3.0 * float(G["kfree_act"]) and e_o <= 3.0 * float(G["kfree_obs"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_routes_agree_with_each_other(case):
    """route 2 against route 0 over the whole stored rollout, within the sum of the two bars"""
    e_a, e_o = _result()["routes"][case]
    bar_a, bar_s = _bars(case)
    print("%s: actions %.2e  states %.2e" % (case, e_a, e_o))
    assert e_a <= 2.0 * bar_a and e_o <= 2.0 * bar_s


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["p1", "p7"])
def test_wide_kernel_on_shapes_the_chained_route_serves(case):
    """called directly the wide route serves _refine_oracle's p1 and p7 and stays within tests/golden/refine.npz's bars"""
    e_a, e_s, route = _result()["chained"][case]
    bar_a, bar_s = _bars(case, GR)
    print("%s: action %.2e (bar %.2e)  state %.2e (bar %.2e)" % (case, e_a, bar_a, e_s, bar_s))
    assert route == 2 and e_a <= bar_a and e_s <= bar_s


@pytest.mark.gpu
def test_masked_column_is_exactly_zero():
    assert _result()["masked_zero"] is True


@pytest.mark.gpu
def test_route_reporting():
    """route_out is 2 and agrees with the route function on every case; 0 under either switch (no case has a chained route);
    under MJX_POLICY_ROLLOUT_WIDE=0 the outputs are mjx_policy_rollout's bit for bit; routes 2 and 0 are different kernels"""
    r = _result()
    for case in CASES:
        assert r["route_fn"][case] == 1 and r["route_out"][case] == [2, 0, 0, 0], case
        assert r["switch_bits"][case] is True, case
    assert any(r["differ"].values())


@pytest.mark.gpu
def test_shared_noise_and_start_state_give_every_member_the_same_first_action():
    assert _result()["shared"] is True


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    assert _result()["repeat"] is True


@pytest.mark.gpu
def test_a_nan_trajectory_stays_alone():
    """a NaN in row 40 of w2's s0: every other row's outputs are the clean run's bit for bit, row 40's stored s0 is NaN and the
    guards are intact (asserted by the worker)"""
    assert _result()["nan"] == dict(others=True, s0_nan=True)


@pytest.mark.gpu
def test_python_layer_reaches_the_wide_route():
    """two WorldModel(6, 2, hidden_size=(256, 256)) and an MLP 32 x 32: rollout_models_device reports route 2 and is a direct entry
    call's bits; refine_route() is 2 before and after get_refined_action; a resident train_step without truncation reports
    rollout route 2, keeps every path at length H and hands the rollout's rows on bit for bit"""
    py = _result()["python"]
    assert py["device"] == [2, 2, True]
    assert py["refine"] == [2, 2, True]
    assert py["train"] == [True, 2, 80, [8], True]
