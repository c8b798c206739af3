"""k_rollout_disagree<HB, NB> and the pack kernels (csrc/rollout_batch.h) behind mjx_rollout_disagreement and mjx_rollout_pack on the
MI355X, per instance, member count, row edge and truncation pattern (cases, recipes and measures: tests/_rollout_batch_cases.py).
Every check runs in ONE fresh worker process under a time limit (tests/_rollout_batch_worker.py); a worker that failed is not started
again -- the remaining tests fail with its output.

Disagreement: _plan_cases' nets r1 .. r10 (all eight instances, ReLU and tanh, flags 0, 1, 3, 5, 7, the zero-scale column, n = 1) at
K = 1, 2, 3, 5 and fourteen (P, H) whose P H and P (H - 1) hit 31, 32, 33, 128, 129 and 165 rows, H = 2 and H = 6 among them.  Per row
against the fp64 oracle, relative to the row's oracle value (rows below 1e-3 of the case's largest against that floor); the bar is
3 x the yardstick, a plain fp32 torch restatement's distance from the same oracle (tests/golden/rollout_batch.npz), on both routes.
Pack: every output bit for bit against the NumPy emulation, and nothing written at or behind row off[P]."""
import os
import sys

import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rollout_batch_cases as B  # noqa: E402



def _result():
    return worker_result("_rollout_batch_worker.py", 300, "rollout batch")


@pytest.mark.gpu
@pytest.mark.parametrize("case", B.dis_cases(), ids=B.dis_id)
def test_disagreement_against_fp64_on_both_routes(case):
    r = _result()["dis"][B.dis_id(case)]
    bar = B.MARGIN * B.yard(case)
    print("%s: route 1 %.3e, route 0 %.3e, bar %.3e" % (B.dis_id(case), r["err1"], r["err0"], bar))
    assert r["err1"] <= bar
    assert r["err0"] <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("case", B.dis_cases(), ids=B.dis_id)
def test_disagreement_routes_guards_and_bits(case):
    """route_out is what the route function promises (1) and 0 under the switch; route 0 carries the bits of mjx_dyn_forward +
    mjx_dyn_pred_error on host-gathered rows; the 64 NaN guard elements stay NaN; and the two routes' bits differ (equal bits over
    31 rows or more would mean that both calls ran the same kernel).  At n = 1 (r2) the mean is one square, which both routes form
    alike, and the residual absorbs most of the nets' last-bit differences: those cases are counted together below"""
    r = _result()["dis"][B.dis_id(case)]
    assert r["routes"] == [1, 0, 1]
    assert r["host_equal"] and r["guards"]
    print("%s: %d of %d rows differ in their bits" % (B.dis_id(case), r["differ"], r["rows"]))
    assert r["differ"] > 0 or case[0] == "r2"


@pytest.mark.gpu
@pytest.mark.parametrize("net", B.NETS)
def test_the_routes_differ_in_their_bits_on_every_net(net):
    got = [_result()["dis"][B.dis_id(c)] for c in B.dis_cases() if c[0] == net]
    differ, rows = sum(r["differ"] for r in got), sum(r["rows"] for r in got)
    print("%s: %d of %d rows differ in their bits" % (net, differ, rows))
    assert differ > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", B.limited(), ids=B.dis_id)
def test_truncation_decisions_at_the_fixed_limit_are_the_oracles(case):
    """the limit lies in a 5 % gap of the fp64 errors (fix_lim), five orders above the kernels' error: the first violation of every
    path, taken from either route's errors, is the oracle's"""
    assert _result()["dis"][B.dis_id(case)]["first"] == [True, True]


@pytest.mark.gpu
def test_a_nan_member_makes_the_row_nan_on_both_routes():
    r = _result()
    assert r["nan"] == [True, True] and r["nan_clean"]


@pytest.mark.gpu
def test_h1_and_p0_return_without_touching_the_output():
    r = _result()
    assert r["h1"] == [True, 1] and r["p0"] == [True, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(B.PACK_CASES))
def test_pack_equals_the_emulation_exactly(name):
    r = _result()["pack"][name]
    for key in ("off", "first", "term", "obs", "act", "rew", "obs64", "tpos"):
        assert r[key] == [True, True], key
    P, H = B.PACK_CASES[name][:2]
    assert 0 < r["rows"][0] <= P * H
