"""k_policy_fit_wide (csrc/policy_fit_wide.h), route 2 of mjx_policy_minibatch_adam_wide, against the fp64 oracle of
tests/_fit_oracle.py, in ONE fresh worker process under a time limit (tests/_policy_fit_wide_worker.py; inputs from
tests/_fit_cases.pol_data).  Cases (n, m, H, B), each for MSE, MLE, the clipped surrogate with the old network on the current weights
and with a fixed old policy, with 1 and 10 steps:
    (33, 17, 32, 8)    n just above H, one action in the second 16-lane half, the smallest B
    (46, 30, 32, 64)   the hand-manipulation shape at a full batch
    (64, 32, 32, 12)   full input blocks and the full action width, a partial 16-row tile
    (39, 28, 32, 32)   the hand_dapg behaviour-cloning minibatch
    (17, 17, 64, 20)   H = 64, a narrow input, a partial tile
    (48, 32, 64, 32)   the largest must-serve H = 64 shape
    (45, 24, 64, 32)   H = 64 at the last B the route serves with a fixed old policy (tests/test_policy_fit_wide_route_cpu.py)
Per case: route 2 from the route function and from the call; parameters in units of lr and m, v element-wise per block (W1, b1, W2,
b2, W3, b3, log_std); every loss entry; NaN tails intact; under MSE log_std and its non-zero moments bit-identical; step0 = 3 with
carried moments equals the longer call bit for bit.  Parameters whose first fp64 gradient is below 3e-7 are counted, not compared.

Bars: 3x the larger of two errors measured on the MI355X against the fp64 oracle on these cases (r24) -- route 2, and the existing
entry (the per-step launches here) -- never one route against the other:
    [route 2 | launches, with the case of the larger]"""
import pytest

from tests._fit_cases import MODES
from tests._worker_run import worker_result

BARS = {
    "params_over_lr": 2.1e-3,     # [5.1e-4 | 7.1e-4: (48, 32, 64, 32) clipped surrogate, fixed old policy]
    "m": 2.4e-5,                  # [7.9e-6: (48, 32, 64, 32) clipped surrogate, fixed old policy | 7.0e-6]
    "v": 4.8e-5,                  # [1.6e-5: (45, 24, 64, 32) clipped surrogate, old network on the current weights | 1.3e-5]
    "loss": 1.9e-5,               # [3.8e-6 | 6.2e-6: (45, 24, 64, 32) clipped surrogate, old network on the current weights]
}
FIT_ILL_CONDITIONED = 2.8e-2      # tests/test_gpu_fit_matrix.py's bar [0.03 % here, from the oracle alone]
CASES = [(33, 17, 32, 8), (46, 30, 32, 64), (64, 32, 32, 12), (39, 28, 32, 32), (17, 17, 64, 20), (48, 32, 64, 32), (45, 24, 64, 32)]

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_policy_fit_wide_worker.py", 300, "policy fit wide")


@pytest.mark.parametrize("loss, track", MODES)
@pytest.mark.parametrize("n, m, H, B", CASES)
def test_wide_fit_against_fp64(n, m, H, B, loss, track):
    r = _result()["cases"]["(%d, %d, %d, %d) loss %d track %d" % (n, m, H, B, loss, track)]
    assert r["route"] == 2 and r["ran"] == [2, 2], (r["route"], r["ran"])
    for k in BARS:
        print("[policy fit wide] %-15s route 2 %.2e  launches %.2e" % (k, r["wide"][k], r["base"][k]))
    for k, bar in BARS.items():
        assert r["wide"][k] < bar, (k, r["wide"][k])
    assert r["ill"] < FIT_ILL_CONDITIONED, r["ill"]
    assert r["guards_ok"] and r["log_std_touched"] == 0 and r["cont_not_bitwise"] == 0, r


def test_bc_and_ppo_with_wide_fit():
    """BC(wide_fit=True).fit on (39, 28, 32 x 32) at mb 32 runs route 2 and lands on the oracle within the bar, as wide_fit=False
    does; a PPO(wide_fit=True) step runs route 2"""
    h = _result()["host"]
    print("[policy fit wide] BC params / lr vs fp64: wide_fit %.2e, default %.2e" % (h["bc_wide"], h["bc_base"]))
    assert h["bc_route_wide"] == 2 and h["bc_route_base"] is None
    assert h["bc_wide"] < BARS["params_over_lr"] and h["bc_base"] < BARS["params_over_lr"]
    assert h["ppo_route_wide"] == 2 and h["ppo_finite"]
