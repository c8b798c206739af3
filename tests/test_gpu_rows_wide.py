"""mjx_path_rewards_wide and mjx_rollout_disagreement_wide (csrc/rows_wide.h) on the MI355X: every row of every case of
tests/_rows_wide_cases.py against fp64 on route 2 and on route 0 (the same _wide entry under its MJX_..._WIDE=0 switch), the routes
against each other, the truncation decision, route reporting, bit-level properties, guards and the Python layer that reaches the
entries.  Every check runs in ONE fresh worker process under a time limit (tests/_rows_wide_worker.py); a worker that failed is not
started again -- the remaining tests fail with its output.

The bars are 3 x a yardstick measured without the kernels (tests/golden/rows_wide.npz, written by
tests/golden/make_golden_rows_wide.py): the unmodified reference's own fp32 chain for the rewards, the existing plain fp32 torch-CPU
restatement for the disagreement, each against the fp64 oracle under the measure used here (_rollout_batch_cases.row_err: per row,
relative to the row's oracle value, rows below 1e-3 of the case's largest value against that floor).  Never a multiple of anything
the kernels produced.  Measured on the MI355X (profiles/r17_rows_wide/rows_wide_worker.json): the rewards take between 0.23 and 0.72
of their bar on route 2 (r1 the most) and up to 0.90 on route 0 (r3: the generic kernel on a 256 x 256 tanh reward net); the
disagreement takes between 0.15 and 0.55 on route 2 (n5_P1_H130_K2 the most) and up to 0.43 on route 0; the routes against each
other at most 0.54 (rewards, r3) and 0.30 (disagreement) of the sum of their bars.  With the disagreement mean summed in fp32, as
first built, n5_P129_H2_K1 (n = 64) was 4.81e-7 against its bar of 3.52e-7; summed in fp64 it is 7.2e-8 (csrc/rows_wide.h;
tests/test_rows_wide_cpu.py reproduces both figures' cause on the CPU).  The end-to-end step's rewards are 5.1e-6 from the same step's
under both _WIDE=0 switches, against a bar of 3.5e-5."""
import os
import sys

import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rows_wide_cases as W  # noqa: E402

RCASES = W.RORDER
DCASES = W.dis_cases()
DIDS = [W.dis_id(c) for c in DCASES]
LIMITED = [W.dis_id(c) for c in W.limited()]


def _result():
    return worker_result("_rows_wide_worker.py", 300, "wide rows")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["2", "0"])
@pytest.mark.parametrize("case", RCASES)
def test_rewards_against_fp64(case, route):
    """every row of every member, row set and action mode within 3 x the reference's own fp32 distance"""
    e = _result()["rew"]["err"][route][case]
    bar = W.MARGIN * W.ryard(case)
    print("%s route %s: %.3e (bar %.3e)" % (case, route, e, bar))
    assert e <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("case", RCASES)
def test_reward_routes_agree_with_each_other(case):
    e = _result()["rew"]["routes"][case]
    print("%s: %.3e (bar %.3e)" % (case, e, 2 * W.MARGIN * W.ryard(case)))
    assert e <= 2 * W.MARGIN * W.ryard(case)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["2", "0"])
@pytest.mark.parametrize("case", DCASES, ids=DIDS)
def test_disagreement_against_fp64(case, route):
    """every stored row with a next state within 3 x the fp32 torch restatement's distance"""
    e = _result()["dis"]["err"][route][W.dis_id(case)]
    bar = W.MARGIN * W.dyard(case)
    print("%s route %s: %.3e (bar %.3e)" % (W.dis_id(case), route, e, bar))
    assert e <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("case", DCASES, ids=DIDS)
def test_disagreement_routes_agree_with_each_other(case):
    e = _result()["dis"]["routes"][W.dis_id(case)]
    print("%s: %.3e (bar %.3e)" % (W.dis_id(case), e, 2 * W.MARGIN * W.dyard(case)))
    assert e <= 2 * W.MARGIN * W.dyard(case)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", LIMITED)
def test_truncation_decision_is_the_oracles(cid):
    """under _rollout_batch_cases.fix_lim's limit the first violation per path equals the fp64 oracle's, exactly, on both routes"""
    assert _result()["dis"]["first"][cid] == [True, True]


@pytest.mark.gpu
def test_route_reporting():
    """route_out is 2 and agrees with the route functions on every case; under MJX_..._WIDE=0 and under MJX_..._MFMA=0 it is the
    narrow entry's (0: no case has a narrow MFMA route, the narrow route functions say so) and the outputs are the narrow entry's bit
    for bit; routes 2 and 0 are different kernels; on a shape the register-resident kernel serves too the wide entry reports 2,
    and 1 with the narrow entry's bits under the switch"""
    r = _result()
    for name in RCASES:
        assert r["rew"]["route_fn"][name] == [1, 0] and r["rew"]["route_out"][name] == [[2, 0, 0, 0]], name
        assert r["rew"]["switch_bits"][name] is True, name
    for cid in DIDS:
        assert r["dis"]["route_fn"][cid] == [1, 0] and r["dis"]["route_out"][cid] == [2, 0, 0, 0], cid
        assert r["dis"]["switch_bits"][cid] is True, cid
    assert any(r["rew"]["differ"].values()) and any(r["dis"]["differ"].values())
    ch = r["rew"]["chained"]
    assert ch["routes"] == [2, 1, 1] and ch["bits"] is True


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    r = _result()
    assert r["rew"]["repeat"] is True and r["dis"]["repeat"] is True


@pytest.mark.gpu
def test_each_output_pointer_alone_gives_the_same_bits():
    """r32_out alone and r64_out alone against the call with both (r64 is r32 widened: asserted by the worker on every call)"""
    assert _result()["rew"]["alone"] is True


@pytest.mark.gpu
def test_masked_column_contributes_as_the_oracle_says():
    """the masked column's out_shift moved from +-0.4 to -0.7: the fp64 oracle's bits do not change, and neither do the kernels'"""
    r = _result()
    assert r["rew"]["masked"] == dict(kernel=True, oracle=True) and r["dis"]["masked"] == dict(kernel=True, oracle=True)


@pytest.mark.gpu
def test_a_nan_row_stays_alone():
    """a NaN in one stored row: every other row's bits are the clean run's, that row alone is NaN, the guards are intact (asserted
    by the worker)"""
    r = _result()
    assert r["rew"]["nan"] == dict(others=True, row_nan=True) and r["dis"]["nan"] == dict(others=True, row_nan=True)


@pytest.mark.gpu
def test_python_layer_reaches_the_wide_routes():
    """two WorldModel(6, 2, hidden_size=(256, 256), learn_reward=True) (reward nets 100 x 100) and an MLP 32 x 32: a resident train_step
    under a limit fixed by fix_lim on route 0's errors reports routes 2, 2, 2, gives the path lengths and terminated flags of the same
    step under both _WIDE=0 switches (which reports 2, 0, 0) with some paths truncated and some not, and rewards within the bar of
    that step's; ensemble_path_rewards_device without wide=True is still the generic route's bits"""
    py = _result()["python"]
    assert py["lim_route"] == 0
    assert py["routes"] == [dict(rollout=2, rewards=2, disagreement=2), dict(rollout=2, rewards=0, disagreement=0), True, True]
    assert py["lens"][:2] == [True, True] and 0 < py["lens"][2] < py["lens"][3] == 80
    assert py["plain_is_generic"] is True
    rw = py["rewards"]
    bar = W.MARGIN * rw["yard"]
    print("rewards: wide %.3e narrow %.3e between %.3e step %.3e (bar %.3e)" % (rw["wide"], rw["narrow"], rw["between"], py["step_rewards"], bar))
    assert rw["yard"] > 0 and rw["wide"] <= bar and rw["narrow"] <= bar and rw["between"] <= 2 * bar and py["step_rewards"] <= bar
