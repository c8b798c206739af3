"""The learned-dynamics kernels (csrc/dynamics.h) at production shapes, at every route edge and at the edges where kernels go
wrong, against the fp64 oracle (tests/_dyn_oracle.py).  Every check runs in ONE fresh worker process under a time limit
(tests/_dynamics_matrix_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.
Every output buffer is prefilled with a sentinel (NaN; -1 / -7 for the truncation's err / first) and every element must be
overwritten.  Comparison helpers: tests/_dyn_check.py; tests/test_dynamics_checks.py shows on CPU that they flag the defects.

Batched forward (mjx_dyn_forward, ensemble_forward); each output column of each member over its own scale:
    maxw from the input (d_in 40 > hidden 24 / 32); maxw 48; 256 (96 KiB: the attribute); 426 (163 584 B: the largest)
    rows 1, 31, 32, 33, 64 and 12 500 (N * H at N = 250, H = 50); K = 1, 3, 4, 7 with distinct parameters
    x_stride = rows * d_in (every member its own rows); 1 Linear layer; 8 (DYN_MAXL); all 8 flag values with ReLU and tanh,
    the masked column exactly 0 (exactly x[:, j] with the residual); width 427 refused (MJX_ERR_UNSUPPORTED), out untouched
    ensemble_forward with members that differ in residual, activation and mask (four launches, then out[ids] = o)

Rollout (mjx_model_rollout):
    production  dynamics [13, 256, 256, 11] ReLU, flags 7; policy 32 x 32 and 64 x 64; K = 3 and 4; N = 250 (last tile 2 rows);
                H = 25 and 50; noise on, scalar and vector bounds; n, m = 24, 8 with 64 x 64; given actions at K = 4, H = 50
    branches    tanh dynamics; flags 3; 3 hidden dynamics layers; policies with 1 and 3 hidden layers; a policy wider than
                the dynamics net; n = 200 (the policy alone 69 152 B: LDS over 64 KiB); eval mode without bounds;
                N = 1, 7, 8 at H = 6 and at H = 30 with the 256-wide net
    refused     H = 0 and N = 0 launch nothing; n = 600 (171 552 B of policy) returns MJX_ERR_UNSUPPORTED, outputs untouched
  Every case is checked teacher-forced: the fp64 oracle takes the kernel's own obs[k, i, t] and act[k, i, t] and reproduces
  act[k, i, t] = clamp(policy_mean(obs) + noise[k, t, i] * exp(log_std)) and obs[k, i, t + 1] = clamp(f_k(obs, act)), per
  member, per step and per column (over 50 steps, fp32 and fp64 free-running trajectories part for reasons that are not bugs).
  At H <= 6 the free-running comparison runs as well; obs[:, :, 0] must be s0 exactly, given actions clamp(actions) exactly.

Fit (mjx_dyn_fit_adam), 1 and 10 Adam steps against fp64 (parameters in units of lr, losses), routes as the kernel trace of the
worker shows them (k_dyn_fit: one launch per persistent call; k_dl_*: one k_dl_loss per step of a launch-route call):
    persistent  [10, 128, 128, 8] B 32; [10, 64, 64, 8] B 64; [43, 128, 128, 42] B 64 (163 584 + 128 static B of LDS);
                [8, 6] (one Linear layer); 3 and 7 hidden layers; RewardNet [24, 100, 100, 1] through the affine, B 32 and 64;
                [24, 64, 64, 20] B 64 (B * d_out = 1280 > 1024: the loss head loops).  Each also on the launch route
                (MJX_DYN_FIT_LAUNCHES=1), and the two routes agree
    launch      [13, 256, 256, 11] B 16 / 32 / 64; [10, 129, 129, 8]; [10, 64, 64, 8] B 65; [44, 128, 128, 42] B 64 (163 840
                + 128 B: over the limit by the static bytes); [13, 160, 160, 11] tanh; [24, 256, 256, 20] B 64
  Continuation: s1 steps, then s2 with the moments carried and step0 = s1, equals one (s1 + s2)-step call bit for bit on each
  route, and matches the fp64 chain started from the device's state after s1 steps (t0 = 3 and 12; a bias correction off by
  one moves a step by far more than the bar at these t0).

Truncation (mjx_dyn_pred_error) against the reference's expression itself (model_accel_npg.py:139-150: np.maximum from zeros
in model order): K = 4 with 1000 segments of 49 rows; K = 1, n = 1; 700-row segments with violations on different loop trips
(the earliest wins), at row 0 and at the last row; empty segments at the start, middle and end; errors exactly at the limit
(not a violation); inf and NaN in pred and s_next, in one member and in all.  err with equal_nan, first exactly.

Bars are 3x the errors measured on the MI355X (in brackets)."""
import pytest

from tests._worker_run import worker_result

BARS = {
    "fwd": 1.4e-6,                    # [4.8e-7]
    "fwd_ensemble_mixed": 1.1e-6,     # [3.7e-7]
    "roll_tf_act": 5.4e-6,            # [1.8e-6: n, m = 24, 8 with the 64 x 64 policy]
    "roll_tf_obs": 2.6e-6,            # [8.7e-7]
    "roll_free": 4.9e-6,              # [1.6e-6]
    "fit_params_over_lr": 6.6e-3,     # [2.2e-3: 256 x 256, batch 64, 10 steps -- a first gradient just above the floor
                                      #  leaves sqrt(v) small, and later gradient rounding moves the step by ~rounding / g1]
    "fit_ill_conditioned": 2.8e-2,    # share of parameters whose first fp64 gradient is below 3e-7 [0.93 %]
    "fit_loss": 6.4e-6,               # [2.1e-6]
    "fit_routes_over_lr": 1e-6,       # the bar of tests/test_gpu_model_accel.py [0: the same per-element arithmetic]
    "fit_cont_over_lr": 3e-4,         # [9.8e-5]
    "trunc_err": 4.7e-7,              # [1.6e-7]
}

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_dynamics_matrix_worker.py", 600, "dynamics matrix")


def _under(r, *keys):
    for k in keys:
        e, case = r["err"][k]
        assert e < BARS[k], (k, e, case)


def _zero(r, *keys):
    for k in keys:
        assert r["count"][k] == 0, (k, r["count"][k])


def test_forward_every_column_against_fp64():
    r = _result()
    _under(r, "fwd", "fwd_ensemble_mixed")
    _zero(r, "fwd_unwritten", "fwd_mask_bad")


def test_forward_over_the_lds_limit_is_refused():
    assert _result()["refused"]["fwd_w427"] == [-3, True]


def test_rollout_teacher_forced_against_fp64():
    r = _result()
    _under(r, "roll_tf_act", "roll_tf_obs")
    _zero(r, "roll_unwritten", "roll_s0_bad", "roll_given_actions_bad")


def test_rollout_free_running_at_short_horizons():
    _under(_result(), "roll_free")


def test_rollouts_that_launch_nothing_leave_the_outputs_untouched():
    r = _result()["refused"]
    assert r["roll_H0"] == [0, True]
    assert r["roll_N0"] == [0, True]
    assert r["roll_lds_over_160k"] == [-3, True]


def test_fit_against_fp64_on_every_route():
    """parameters whose first fp64 gradient reached 3e-7, in units of lr; the others are ill-conditioned for any fp32 Adam
    (at t = 1 the step is g / (|g| + 1e-8): 3e-10 of gradient rounding moves it by 3 % of lr near |g| = 1e-8), only counted"""
    r = _result()
    _under(r, "fit_params_over_lr", "fit_loss")
    _zero(r, "fit_unwritten")
    assert r["count"]["fit_ill_conditioned"] < BARS["fit_ill_conditioned"] * r["count"]["fit_params"]


def test_fit_routes_agree():
    _under(_result(), "fit_routes_over_lr")


def test_fit_continuation_with_carried_moments():
    r = _result()
    _zero(r, "fit_cont_not_bitwise")
    _under(r, "fit_cont_over_lr")


def test_truncation_against_the_reference_expression():
    r = _result()
    _under(r, "trunc_err")
    _zero(r, "trunc_nan", "trunc_first", "trunc_unwritten")
    assert r["count"]["trunc_cases_with_violations"] == 6
