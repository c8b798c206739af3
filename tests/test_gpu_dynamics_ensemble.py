"""The ensemble fit (mjx_dyn_fit_ensemble, csrc/dyn_fit_ens.h; fit_ensemble of nn_dynamics.py) against the fp64 oracle
(tests/_dyn_oracle.adam_steps), against the member-by-member path, and against itself bit for bit.  Conventions of
tests/test_gpu_dynamics_matrix.py: every check runs in ONE fresh worker process under a time limit
(tests/_dyn_ensemble_worker.py); a worker that failed is not started again -- the remaining tests fail with its output.  Every
loss block is prefilled with NaN and every element must be overwritten.  Cases and data recipe: tests/_dyn_ensemble_cases.py
(K = 4 members a case, each with its own theta, transforms, rows and index stream; N = 400, lr 1e-3, wd 1e-5).

Against fp64, 1 and 10 steps, per member: parameters in units of lr over those whose first fp64 gradient reached 3e-7, and the
step losses.  The share of parameters left out is a condition: at most 2.8 % over the matrix (the project's
fit_ill_conditioned cap) and 8 % in any one member (the oracle alone gives 1.67 % and 4.96 %, pm_b16 member 1); the left-out
ones must be finite.  The case with every served limit at once (max_b64: the gathered inputs live in scratch) is held to the
same bars under its own keys.
Route: 1 for every case of the matrix; 0, with results equal bit for bit to K mjx_dyn_fit_adam calls, for 288-wide layers,
three hidden layers, the RewardNet shape with target mode 0, batch 65 and MJX_DYN_FIT_ENS=0.
Bit for bit on route 1: member k of the K = 4 call = the K = 1 call of that member (parameters, moments, losses); K = 7 with
members 0 and 5 given identical inputs; 3 steps then 9 with the moments carried = one 12-step call, with step0 all 0 and
(0, 3, 12, 40), and that run matches the fp64 chain started from the device's state after 3 steps; shared rows (strides 0) =
the rows replicated per member.
fit_ensemble on three WorldModel(13, 4, hidden (256, 256)), 400 rows, batch 64, 2 epochs, against a deep copy fitted by the
fit_dynamics loop from the same NumPy seed: the stream state afterwards, epoch losses, all parameters, step_count, _generation,
MPCPolicy._pack_key.

Bars are 3x the errors measured on the MI355X (in brackets), and none exceeds the bar tests/test_gpu_dynamics_matrix.py holds
the existing fp32 routes to for the same quantity against the same oracle (6.6e-3, 6.4e-6, 3e-4); where 3x the measurement is
more, the bar is that cap.

The member-by-member path is run on the same members for the record (seq_params_over_lr, printed, not asserted): it measures
2.2e-2 lr on w256_b16, because dyn_adam forms 1 - beta2 as `1.0f - 0.999f` (1.3e-5 low); the ensemble kernel uses torch's
once-rounded 0.001f."""
import pytest

from tests._dyn_ensemble_cases import CASES, ROUTE0
from tests._worker_run import worker_result

BARS = {
    "params_over_lr": 3.1e-3,         # [1.03e-3: w256_b16, 10 steps, member 0]
    "loss": 4.3e-7,                   # [1.43e-7: pm_b16, 10 steps]
    "cont_over_lr": 3e-4,             # the cap [1.74e-4: h64_96_tanh]
    "xscr_params_over_lr": 9.6e-4,    # [3.2e-4]
    "xscr_loss": 1.6e-7,              # [5.1e-8]
    "wm_params_over_lr": 6.6e-3,      # the cap [3.0e-3: two fp32 chains, ill-conditioned parameters included]
    "wm_loss": 6.4e-6,                # the cap [2.3e-6]
}
ILL_AGGREGATE, ILL_MEMBER = 2.8e-2, 8e-2

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_dyn_ensemble_worker.py", 480, "ensemble-fit")


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
    print("per case:", r["info"]["params_over_lr_by_case"], "; the member-by-member path on the same members:", r["err"]["seq_params_over_lr"])
    _zero(r, "unwritten", "ill_not_finite")
    _under(r, "params_over_lr")


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


def test_every_served_limit_at_once_against_fp64():
    r = _result()
    _under(r, "xscr_params_over_lr", "xscr_loss")
    assert r["err"]["xscr_ill_share_member"][0] <= ILL_MEMBER
    assert r["info"]["route"]["max_b64"] == 1


def test_route_1_for_every_case_of_the_matrix():
    r = _result()
    for name, _, _, _, _ in CASES:
        assert r["info"]["route"][name] == 1, name


def test_route_0_is_the_member_by_member_path_bit_for_bit():
    r = _result()
    for name, _, _, _, _, _ in ROUTE0:
        assert r["info"]["route0"][name] == 0, name
    _zero(r, "route0_not_bitwise")


def test_a_member_does_not_depend_on_its_neighbours():
    r = _result()
    _zero(r, "k4_vs_k1_not_bitwise", "k7_twins_differ", "k7_members_equal", "shared_rows_not_bitwise")


def test_continuation_with_carried_moments_and_per_member_step_counts():
    r = _result()
    _zero(r, "cont_not_bitwise")
    _under(r, "cont_over_lr")


def test_fit_ensemble_stands_for_the_fit_dynamics_loop():
    r = _result()
    _zero(r, "wm_rng_state_differs", "wm_state_differs", "wm_epochs_bad", "wm_unchanged", "wm_not_finite", "wm_pack_key_unchanged")
    print("moments: %.3e" % r["err"]["wm_moments"][0])
    _under(r, "wm_params_over_lr", "wm_loss")
