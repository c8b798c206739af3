"""The reward-net ensemble fit (mjx_reward_fit_ensemble, the ragged / affine-head instance of csrc/dyn_fit_ens.h;
fit_reward_ensemble, fit_world_models and ensemble_path_rewards of nn_dynamics.py) against the fp64 oracle
(tests/_dyn_oracle.adam_steps, target mode 0), against the member-by-member path, and against itself bit for bit.  Conventions
of tests/test_gpu_dynamics_ensemble.py: every check runs in ONE fresh worker process under a time limit
(tests/_reward_fit_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.  Every
loss block is prefilled with NaN and every element must be overwritten.  Cases, data recipe and comparison functions:
tests/_reward_fit_cases.py (K = 4 members a case, each with its own theta, transforms, rows and index stream; N = 400,
lr 1e-3, wd 1e-5); tests/test_reward_fit_checks.py shows on the CPU that these comparisons at these bars flag the defects a
wrong kernel would leave.

Against fp64, 1 and 10 steps, per member: parameters in units of lr over those whose first fp64 gradient reached 3e-7 -- over
all of them, per block (W1, b1, W2, b2, W3, b3), and over the rows and columns beyond the last full 32-tile of a ragged width
(`edge`) -- and every step loss.  The share of parameters left out is a condition: at most 2.8 % over the matrix and 3 % in any
member (the fp64 oracle alone gives 0.53 % and 1.34 %, rw_dout3 member 3); for rw_max_b64 (the gathered inputs live in scratch;
its own keys) at most 3 % in any member (the oracle gives 0.32 %).  The left-out ones must be finite.
Route: 1 for every case; 0, with results equal bit for bit to K mjx_dyn_fit_adam calls in target mode 0, for
MJX_REWARD_FIT_ENS=0, a 300-wide layer, three hidden layers and batch 65.
Bit for bit on route 1: member k of the K = 4 call = the K = 1 call of that member; shared y (stride 0) = y replicated; 3 steps
then 9 with the moments carried = one 12-step call, with step0 all 0 and (0, 3, 12, 40), and that run matches the fp64 chain
started from the device's state after 3 steps.
fit_reward_ensemble on three WorldModel(11, 2, learn_reward=True, hidden (64, 64)) (reward nets [24, 100, 100, 1]), 400 rows,
batch 64, 2 epochs, dynamics fitted first, against a deep copy fitted by the fit_reward loop from the same NumPy seed, twice
(the second call carries the moments) -- with set_transformations=False after the transforms were set by hand, as the
reference's fit_reward fixture runs: fit_reward's own transform line reads r_shift before it is bound, here as in the reference
(nn_dynamics.py:138), and fit_reward_ensemble forms the same expressions; fit_world_models against the driver's interleaved loop; the reference's
fit_reward fixture (tests/golden/model_accel.npz) through fit_reward_ensemble([wm]); ensemble_path_rewards (K = 3, one member
tanh, N = 5, H = 7) against each member's compute_path_rewards bit for bit.

Bars are 3x the errors measured on the MI355X (in brackets), and none exceeds what tests/test_gpu_dynamics_ensemble.py holds
the dynamics kernel to for the same quantity (6.6e-3 lr, 6.4e-6, 3e-4); where 3x the measurement is more, the bar is that
cap.  rw_max_b64's 5.05e-3 lr is one entry of W2 (member 1) whose first fp64 gradient is 6.7e-7, just above the floor; an fp32
NumPy chain of that member (tests/test_reward_fit_checks.chain) is 6.9e-3 lr off at the same entry, and every other block of
the case is within 1.9e-4."""
import pytest

from tests._reward_fit_cases import BLOCKS, CASES, MAX_CASE, ROUTE0
from tests._worker_run import worker_result

CAP_PARAMS, CAP_LOSS, CAP_CONT, CAP_FIXTURE = 6.6e-3, 6.4e-6, 3e-4, 2.6e-5
BARS = {
    "params_over_lr": 7.3e-4,            # [2.43e-4: rw_dout3, 10 steps, member 3; the other cases 9.1e-5 .. 1.8e-4]
    "edge_over_lr": 7.3e-4,              # [2.43e-4: rw_dout3, 10 steps, member 3]
    "block_W1": 5.4e-4,                  # [1.80e-4: rw_w64_b32]
    "block_b1": 2.4e-4,                  # [8.13e-5: rw_w33_36]
    "block_W2": 7.3e-4,                  # [2.43e-4: rw_dout3]
    "block_b2": 1.2e-4,                  # [3.92e-5: rw_w33_36]
    "block_W3": 3.2e-4,                  # [1.08e-4: rw_w31_7]
    "block_b3": 3.9e-5,                  # [1.29e-5: rw_w31_7, 1 step]
    "loss": 5.3e-7,                      # [1.78e-7: rw_tanh_b33, 10 steps]
    "cont_over_lr": CAP_CONT,            # the cap [1.65e-4: rw_w33_36]
    "max_params_over_lr": CAP_PARAMS,    # the cap [5.05e-3: one entry of W2, member 1, 10 steps; the other blocks <= 1.9e-4]
    "max_edge_over_lr": 1.6e-4,          # [5.18e-5]
    "max_loss": 5.8e-7,                  # [1.92e-7]
    "wm_params_over_lr": 4.6e-3,         # [1.53e-3: two fp32 chains, ill-conditioned parameters included]
    "wm_loss": 5.4e-7,                   # [1.79e-7]
    "fwm_dyn_params_over_lr": 6.5e-4,    # [2.16e-4]
    "fwm_rew_params_over_lr": 1.2e-3,    # [4.04e-4]
    "fwm_dyn_loss": 1.3e-6,              # [4.23e-7]
    "fwm_rew_loss": 2.7e-7,              # [8.94e-8]
    "fixture_reward": 6.2e-7,            # [2.06e-7; the existing route is held to 2.6e-5]
}
ILL_AGGREGATE, ILL_MEMBER = 2.8e-2, 3e-2

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_reward_fit_worker.py", 300, "reward-fit")


def _under(r, *keys):
    for k in keys:
        e, case = r["err"][k]
        print("%s = %.3e (%s), bar %.1e" % (k, e, case, BARS[k]))
        assert e < BARS[k], (k, e, case)


def _zero(r, *keys):
    for k in keys:
        assert r["count"].get(k, 0) == 0, (k, r["count"][k])


def test_every_member_parameters_against_fp64():
    r = _result()
    print("per case:", r["info"]["params_over_lr_by_case"])
    _zero(r, "unwritten", "ill_not_finite")
    _under(r, "params_over_lr")


def test_every_block_and_the_ragged_edges_against_fp64():
    """per block, and over the unit rows and weight columns beyond the last full 32-tile: a dropped partial tile must not hide
    in a maximum over 12 000 entries"""
    r = _result()
    _under(r, "edge_over_lr", *["block_" + b for b in BLOCKS])
    assert r["err"]["edge_over_lr"][0] > 0.0          # (the ragged cases have such parameters, and they moved)


def test_every_member_losses_against_fp64():
    r = _result()
    _zero(r, "unwritten")
    _under(r, "loss")


def test_share_of_ill_conditioned_parameters():
    """a condition on the recipe, not a measurement: the comparison above must not be emptied by the floor"""
    r = _result()
    share = r["count"]["ill_conditioned"] / r["count"]["params"]
    print("ill-conditioned share: aggregate %.4f, worst member %.4f (%s)" % ((share,) + tuple(r["err"]["ill_share_member"])))
    assert share <= ILL_AGGREGATE
    assert r["err"]["ill_share_member"][0] <= ILL_MEMBER


def test_widths_one_short_of_the_limit_with_inputs_in_scratch():
    r = _result()
    _under(r, "max_params_over_lr", "max_edge_over_lr", "max_loss")
    print("ill-conditioned share, worst member: %.4f" % r["err"]["max_ill_share_member"][0])
    assert r["err"]["max_ill_share_member"][0] <= ILL_MEMBER
    assert r["info"]["route"][MAX_CASE[0]] == 1


def test_route_1_for_every_case():
    r = _result()
    for name, _, _, _ in CASES:
        assert r["info"]["route"][name] == 1, name


def test_route_0_is_the_member_by_member_path_bit_for_bit():
    r = _result()
    for name, _, _, _, _ in ROUTE0:
        assert r["info"]["route0"][name] == 0, name
    _zero(r, "route0_not_bitwise")


def test_a_member_does_not_depend_on_its_neighbours():
    r = _result()
    _zero(r, "k4_vs_k1_not_bitwise", "k4_members_equal", "shared_y_not_bitwise")


def test_continuation_with_carried_moments_and_per_member_step_counts():
    r = _result()
    _zero(r, "cont_not_bitwise")
    _under(r, "cont_over_lr")


def test_fit_reward_ensemble_stands_for_the_fit_reward_loop():
    r = _result()
    _zero(r, "wm_rng_state_differs", "wm_state_differs", "wm_epochs_bad", "wm_unchanged", "wm_not_finite", "wm_mixed_differs")
    print("moments: %.3e" % r["err"]["wm_moments"][0])
    _under(r, "wm_params_over_lr", "wm_loss")


def test_fit_world_models_stands_for_the_drivers_interleaved_loop():
    r = _result()
    _zero(r, "fwm_rng_state_differs", "fwm_epochs_bad", "fwm_state_differs", "fwm_nolearn_differs")
    _under(r, "fwm_dyn_params_over_lr", "fwm_rew_params_over_lr", "fwm_dyn_loss", "fwm_rew_loss")


def test_reference_fit_reward_fixture_through_the_ensemble_entry():
    r = _result()
    assert r["info"]["fixture_route"] == 1
    _under(r, "fixture_reward")


def test_ensemble_path_rewards_is_each_members_compute_path_rewards_bit_for_bit():
    r = _result()
    _zero(r, "path_rewards_not_bitwise", "path_rewards_members_equal")
