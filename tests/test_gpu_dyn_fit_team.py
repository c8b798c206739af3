"""The team ensemble fit (mjx_dyn_fit_ensemble_team, csrc/dyn_fit_ens_team.h; fit_ensemble(team=True) of nn_dynamics.py) against the
fp64 oracle (tests/_dyn_oracle.adam_steps) and against itself bit for bit, in ONE fresh worker process under a time limit
(tests/_dyn_fit_team_worker.py; never started again after a failure).  Cases and data recipe: tests/_dyn_fit_team_cases.py (K = 3
members a case, N = 5 batch + 7 rows, lr 1e-3, weight decay 1e-3, 1 and 10 steps).

Against fp64, per member: parameters in units of lr per block (W1 .. b3) over those whose first fp64 gradient reached 3e-7 (the
share left out: tests/test_dyn_fit_team_cpu.py), m and v over the block's largest entry, every step's loss.  Bit for bit: member 1
of K = 3 = that member alone; 4 + 6 steps with carried moments and per-member step0 = 10 steps; an unserved shape,
MJX_DYN_FIT_TEAM=0 and batch 65 = mjx_dyn_fit_ensemble with its route; fit_ensemble(team=True) on 128 x 128 WorldModels = the direct call.
Bars are 3x the errors measured on the MI355X (in brackets, with the case that gave them)."""
import pytest

from tests._dyn_fit_team_cases import CASES, FALL_THROUGH, ILL_SHARE
from tests._worker_run import worker_result

BARS = {
    "params_over_lr": 3.2e-3,         # [1.06e-3: w128_b33, 10 steps, member 0, W2]
    "m": 5.5e-5,                      # [1.85e-5: w128_b33, 10 steps, member 0, b1]
    "v": 2.8e-5,                      # [9.2e-6: w128_b33, 10 steps, member 0, W2]
    "loss": 6.2e-7,                   # [2.05e-7: w128_b33, 10 steps, member 0]
}

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_dyn_fit_team_worker.py", 300, "team-ensemble-fit")


@pytest.mark.parametrize("key", sorted(BARS))
def test_every_member_against_fp64(key):
    r = _result()
    e, case = r["err"][key]
    print("%s = %.3e (%s), bar %.1e" % (key, e, case, BARS[key]))
    assert r["count"].get("unwritten", 0) == 0 and r["count"].get("ill_not_finite", 0) == 0
    assert e < BARS[key], (key, e, case)
    assert r["err"]["ill_share"][0] <= ILL_SHARE, r["err"]["ill_share"]


@pytest.mark.parametrize("name, G", [(c[0], c[6]) for c in CASES])
def test_the_team_kernel_ran(name, G):
    r = _result()
    assert (r["info"]["G"][name], r["info"]["route"][name]) == (G, 2)      # (DfeTeamLayout takes every case, max_b64 at 139 KiB)


@pytest.mark.parametrize("key", ["alone_not_bitwise", "cont_not_bitwise", "fall_not_bitwise", "public_not_bitwise", "public_state_differs"])
def test_bit_for_bit(key):
    r = _result()
    assert all(r["info"]["fall"][c[0]][0] in (0, 1) for c in FALL_THROUGH), r["info"]["fall"]
    assert r["count"].get(key, 0) == 0, (key, r["count"][key])
