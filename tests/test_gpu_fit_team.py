"""The team trainer of the MLP baseline (csrc/mlp_fit_team.h: minibatches of 128 .. 512 rows, B / 64 workgroups a step) against the
fp64 oracle (tests/_fit_oracle.py), in ONE fresh worker process under a time limit (tests/_fit_team_worker.py), not restarted
after a failure.

Cases (d_in, B), each the smallest that reaches an edge: (9, 128) G 2, NF1 1; (31, 192) G 3, the last NF1 = 1 width; (32, 320) G 5
(a part-filled group of four slots in the reader), the first NF1 = 2 width; (55, 512) G 8, the last width that fits LDS; (24, 256) the
model-based driver's batch, also without weight decay.  N = 6 B + 37 (five steps an epoch, e N no multiple of B, a tail never
visited), two epochs, and a single-step fit at N = 2 B; lr 1e-3, weight decay 1e-3; x ~ N(0, 1), y = 1 + N(0, 1).  Continuation at
(24, 256), step0 0 and 12: epochs = 1 twice with the moments carried equals one epochs = 2 call bit for bit, and that call
repeated gives the same bits.  MLPBaseline(batch_size=256) on four 200-row paths against the oracle chain on its own features.
Bars are 3x the errors of the unchanged launch route (MJX_FIT_TEAM=0) on the same cases against the same fp64 oracle, measured on
the MI355X; in brackets [launch route, team route, the team route's worst case]."""
import pytest

from tests._worker_run import worker_result

BARS = {
    "params_over_lr": 4.9e-4,         # [1.65e-4, 1.65e-4: (9, 128) 2 epochs, W1 -- and the MLPBaseline fit, held to the same bar]
    "m": 2.2e-5,                      # [7.2e-6, 6.8e-6: (9, 128) 2 epochs, the one-entry b3]
    "v": 4.1e-5,                      # [1.36e-5, 1.35e-5: (55, 512) 2 epochs, W3 -- 1 - beta2 formed as 1.0f - 0.999f on every route]
    "v_bias": 3.9e-5,                 # [1.31e-5, 1.30e-5: (31, 192) 1 step, W1 -- that coefficient]
    "loss": 5.5e-7,                   # [1.83e-7, 1.86e-7: (55, 512) 2 epochs]
    "ill_share": 2.8e-2,              # the project's fit_ill_conditioned [0.71 %: (24, 256) without weight decay, from the oracle alone]
}

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_fit_team_worker.py", 300, "fit team")


def test_every_case_ran_on_the_team_route():
    r = _result()
    assert r["count"]["route_mismatch"] == 0, r["routes"]
    assert r["routes"]["MLPBaseline"] == [4, 1, 1, 4] and r["count"]["baseline_steps"] == 2


@pytest.mark.parametrize("key", sorted(BARS))
def test_team_fit_against_fp64(key):
    e, case = _result()["err"][key]
    print("[fit team] %-16s %.2e  %s" % (key, e, case))
    assert e < BARS[key], (key, e, case)


def test_guards_and_bitwise_continuation():
    r = _result()
    assert r["count"]["guard_bad"] == 0 and r["count"]["not_bitwise"] == 0, r["count"]
