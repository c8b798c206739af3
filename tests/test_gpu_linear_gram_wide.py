"""The wide Gram route of LinearPolicy's NPG / TRPO update, 64 <= n <= 127 (csrc/linear_policy_wide.h), against
oracle/npg_oracle.py in fp64.  The cases run once, in tests/_linear_gram_wide_worker.py; the bars are those of
tests/test_gpu_linear_gram.py."""
import pytest

from tests._worker_run import worker_result
from tests.test_gpu_linear_gram import TOL_KL
from tests.test_gpu_operators import TOL_FVP, TOL_STEP, TOL_VPG

pytestmark = pytest.mark.gpu

# A workgroup chain is ceil(rounds / CUs) rounds of 128 rows, 8 at the most, so on a device of 256 CUs:
# (n, m, N): the first wide n, one action, one row into a second round | NP = 96 at its last n, one partial tile | NP = 128 at its
# first n, a ninth round of one row | the largest shape, a partial last round | Ant's shape, 33 chains of one round, a tail of 3
# rows in which three waves stage nothing | chains of 3 rounds (547 rounds): the barriers between rounds, the tile loaded ahead,
# fp32 sums across rounds, a last chain of one round
CASES = ["64_1_129", "95_6_33", "96_17_1025", "127_32_1500", "111_8_4099", "111_8_70001"]
# 2049 rounds: the clamp to chains of 8 rounds (1024 rows of fp32), a 257th chain of one round with 3 rows; pass 1 alone
MOMENTS_ONLY = ["96_1_262147"]


def results():
    return worker_result("_linear_gram_wide_worker.py", 240, "wide linear Gram")


@pytest.mark.parametrize("case", CASES + MOMENTS_ONLY)
def test_moments_vs_oracle(case):
    r = results()[case]
    print(case, r)
    assert r["fvp"] < TOL_FVP and r["vpg"] < TOL_VPG and r["surr"] < 1e-6, r
    assert r["rows"] == int(case.split("_")[2]) and r["tail"] == [0.0, 0.0] and r["pad"] == 0.0 and r["same_bits"], r


@pytest.mark.parametrize("case", CASES)
def test_npg_update_vs_oracle(case):
    r = results()[case]
    g = r["npg"]
    print(case, g)
    assert r["route"] == 2
    assert g["x"] < TOL_STEP and g["step"] < TOL_STEP and g["grad"] < TOL_VPG, g
    assert g["kl"] < TOL_KL and g["surr_after"] < 2e-5 and g["alpha"] < 1e-5, g


@pytest.mark.parametrize("case", CASES)
def test_trpo_update_vs_oracle(case):
    """the oracle's trial count; every trial's closed-form KL and the closing batch KL against the oracle's"""
    r = results()[case]["trpo"]
    print(case, r)
    assert r["route"] == 2 and r["accepted"] == 1.0 and r["trials"] == r["want_trials"], r
    assert r["alpha"] < 1e-5 and r["x"] < TOL_STEP and r["step"] < TOL_STEP and r["ring"] < TOL_KL and r["kl"] < TOL_KL, r


def test_switch_and_host_classes():
    r = results()["once"]
    assert r["switch"] == dict(route=0, same=True), r
    assert r["classes"] == dict(wide=2, narrow=0, dapg="ValueError"), r
