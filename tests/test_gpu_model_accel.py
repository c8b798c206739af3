"""Model-based NPG on the MI355X (csrc/dynamics.h, mjrl_amd/algos/model_accel/): the batched forward, the fused learned-model
rollout, both fit routes and the truncation reduction against the fp64 oracle (tests/_dyn_oracle.py), and fit_dynamics /
fit_reward / policy_rollout / ModelAccelNPG.train_step against the unmodified reference's fixtures (tests/golden/model_accel.npz,
tests/golden/make_golden_model_accel.py).  Every check runs in ONE fresh worker process under a time limit
(tests/_model_accel_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.

Bars are 3x the errors measured on the MI355X (in brackets)."""
import pytest

from tests._worker_run import worker_result


def _result():
    return worker_result("_model_accel_worker.py", 600, "model_accel")


@pytest.mark.gpu
def test_forward_every_column_against_fp64():
    """K = 3 members, ReLU and tanh, flags none / affine / affine + mask / all / affine + residual; the masked column exact"""
    assert _result()["forward"] < 1.3e-6            # [4.2e-7]


@pytest.mark.gpu
def test_rollout_step_by_step_against_fp64():
    """H = 1 and 6, N = 13 (not a multiple of the 8-trajectory tile) and 8, eval / scalar bounds / vector bounds, given actions"""
    assert _result()["rollout"] < 1.5e-6            # [4.8e-7]


@pytest.mark.gpu
def test_truncation_reduction_against_numpy():
    r = _result()
    assert r["pred_error"] < 3e-8                     # [7.5e-9]
    assert r["pred_error_first"][0] == r["pred_error_first"][1]


@pytest.mark.gpu
def test_fit_adam_steps_against_fp64_on_both_routes():
    """1 and 10 Adam steps (residual / plain / through-the-affine targets, ReLU and tanh, wd 0 and 1e-5, batch 16-64): the
    parameters within a small fraction of one step (lr) of the fp64 chain, on the persistent and on the launch route"""
    r = _result()
    assert r["fit_params_over_lr"] < 7e-4             # [2.3e-4]
    assert r["fit_loss"] < 3.3e-6                      # [1.1e-6]


@pytest.mark.gpu
def test_fit_routes_agree():
    assert _result()["fit_routes_over_lr"] < 1e-6     # [0: the same per-element arithmetic]


@pytest.mark.gpu
def test_fits_agree_with_the_reference_fixtures():
    """five fit_dynamics runs (64 x 64, 256 x 256, 100 x 100; batch 16 / 32 / 64; wd 0 / 1e-5; residual on / off; a masked
    state column) and one fit_reward: epoch losses, compute_loss and predictions; parameter difference relative to the
    distance the fit moved them"""
    r = _result()
    assert r["fixture_fit_losses"] < 2.5e-5           # [8.2e-6]
    assert r["fixture_fit_params_rel_step"] < 2e-5    # [6.7e-6]
    assert r["fixture_reward"] < 2.6e-5               # [8.5e-6]


@pytest.mark.gpu
def test_fit_max_steps_stops_after_the_crossing_epoch():
    """fit 3: 10 epochs of 12 steps with max_steps 30 -> 3 epochs, as the reference; every fixture fit's epoch count equal"""
    r = _result()
    for ours, ref in r["fixture_fit_epoch_counts"]:
        assert ours == ref
    assert r["fixture_fit_epoch_counts"][3] == [3, 3]


@pytest.mark.gpu
def test_policy_rollout_agrees_with_the_reference_fixture():
    r = _result()
    assert r["fixture_rollout_shapes"][0] == r["fixture_rollout_shapes"][1]
    assert r["fixture_rollout_eval"] < 2.7e-7         # [8.9e-8]
    assert r["fixture_rollout_noisy"] < 1.4e-7        # [4.5e-8]
    a, b, c, d = r["streams_after_rollout"]
    assert (a, b) == (c, d)


@pytest.mark.gpu
def test_model_accel_train_step_agrees_with_the_reference_fixture():
    r = _result()
    assert r["train_step_pol0"] == 0.0
    assert r["train_step_lens_equal"]
    assert r["train_step_keys"][0] == r["train_step_keys"][1]
    assert r["train_step_seed"][0] == r["train_step_seed"][1]
    assert r["train_step_stats"] < 3e-6                 # [3.6e-8 at 15 paths: the returns of the learned-model rollouts]
    # the NPG step itself (10 CG iterations, damping 1e-4, ~1 300 samples for 162 parameters) is an ill-conditioned solve in
    # which two fp32 implementations part by percents; the update path has its own parity tests (test_gpu_parity.py)
    assert r["train_step_policy_rel_l2"] < 6.5e-2      # [2.1e-2]
