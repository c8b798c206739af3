"""The kernels that turn rollouts into what the update consumes (csrc/vecops.h) against long-double references and the NumPy
expressions include/mjx.h names, mode by mode and edge by edge: k_traj_scan<0/1/2> behind mjx_discount_scan and mjx_gae,
k_sum_stats_partial / k_sum_stats_final behind mjx_sum_stats, k_whiten_cast, k_cast_f64_f32, k_apply_step and k_apply_npg_step.
Every check runs in ONE fresh worker process under a time limit (tests/_samplepath_worker.py, through the C entries; cases,
inputs, references and check functions in tests/_samplepath_cases.py); a worker that failed is not started again -- the remaining
tests fail with its output.  tests/test_samplepath_checks.py shows on CPU that the checks pass NumPy emulations of the kernels and
flag the defects a wrong kernel would leave.

Every output buffer has 64 guard elements of a fixed bit pattern before and behind the written range, compared as integers, and is
prefilled with a NaN of another pattern, so an element that was not written, or one written where none is due, is counted.

Scans (one workgroup of 256 threads per trajectory, segments of ceil(T / 256) steps, thread 0 chains the carries).  Lengths 0, 1, 2,
3, 255, 256, 257, 511, 512, 513, 1000, 4099, 65 537 (segments of 257), each as a call of its own and all in one ragged batch with
empty trajectories at the start, in the middle and at the end; 70 000 trajectories of 0 to 3 steps in one call; a call whose
offsets[0] is 1000, with 1e30 before it.  Inputs standard normal, all positive, and standard normal times 10**randint(-8, 9) per
element.
    mjx_discount_scan   g 0, 0.5, 0.9, 0.995, 1:  |y - ref| <= (2 rem + 4) 2^-53 A[t],  rem = T - t, A the recurrence over |x|
    mjx_gae             (gamma, lambda) (0.995, 0.97), (1, 1), (0.9, 0), (0, 0.5), (0.99, 1); terminated flags in a pattern that is not
                        periodic in 2, all 0, all 1, NULL; baselines at scale 1 and 1e6:
                        |adv - ref| <= (2 rem + 6) 2^-53 A_V[t],  A_V the recurrence over |r| + gamma |b_next| + |b|
    lambda -1, 1.5, NaN bit-equal to NumPy's x - b
A term x_s reaches y_t through s - t products and at most s - t + 2 sums (one more for the carry chain; the carry weights hold
exactly the products the sequential form makes; a fused multiply-add only removes roundings); the GAE residual adds three
roundings.  A zero bound asks for a zero error.  The references are the sequential recurrences in long double (the worker
asserts nmant >= 63), the scan's factor the fp64 product gamma * lambda as the header defines it.  The bar is 1.  Measured on
the MI355X, worst ratio error / bound:
    [k_traj_scan<0>  0.184: 70 000 trajectories, trajectory 30030, step 0; on the edge lengths 0.139: g 1, mixed scales, the batch,
                     T 513, step 508]
    [k_traj_scan<1>  0.250: 70 000 trajectories, trajectory 45181, step 0; on the edge lengths 0.207: (1, 1), baseline x 1e6, the
                     batch, T 65 537, step 65 535]
(the fp64 NumPy emulation of the segmented order rounds every product and sum on its own, where the device may fuse them: 0.33
and 0.37 on the 70 000 short trajectories, at most 0.17 on the edge lengths, tests/test_samplepath_checks.py).  n_traj = 0 returns
MJX_OK with null pointers; n_traj < 0 and a null x are refused with MJX_ERR_ARG and write nothing.

Statistics (512 x 256 threads with a grid stride, then one workgroup).  N 0, 1, 255, 256, 257, 131 071, 131 072, 131 073, 300 001 of
randn + mu, mu 0 and 1e8, each about 0 and then about the first pass's mean, as engine.whitened_advantages calls it:
    |s - ref| <= (N + 2) 2^-53 sum |v|,   |q - ref| <= (N + 4) 2^-53 sum v^2,   v = x - shift in long double,   out[2] == N
-- forward bounds of an N-term sum in any order plus the roundings of v and v^2; N = 0 gives [0, 0, 0].  Measured:
    [sum 0.0021: N 257, mu 1e8, shift 0; sum of squares 0.096: N 1, mu 1e8, shift 0 -- the one rounding of x^2]
and the two-pass standard deviation at mu = 1e8 within 1e-12 relative of the long-double value [measured 1.2e-16 at N 300 001;
8.6e-17 at mu = 0].

Casts, bit for bit as uint32 (NaN against NaN by NaN-ness): mjx_whiten_cast against ((a - mean) / (std + eps)).astype(float32) at
N 1, 255, 256, 257, 1 048 576, 1 048 577 (the grid's cap of 4096 workgroups and one more), with the data's own mean and std, with
std = 0, and with mean 1e8 on data of std 1; mjx_cast_f64_f32 against a.astype(float32) at N 1, 255, 256, 257, 2 097 152, 2 097 153
(cap 8192) on randn * 10**uniform(-50, 42) with +-0, +-inf, NaN, +-FLT_MAX, +-3.4028235677973366e38 (the first value that rounds
to inf), +-1e39, the ties 1 + 2^-24 and 1 + 3 2^-24, 1 + 2^-24 + 2^-52 (the first fp64 value above a tie), 1e-40, 2^-149, 2^-150,
2^-150 (1 + 2^-52), 1e-46 and their negatives planted at the front and on the last elements.  count = 0 returns MJX_OK.
    [measured: no mismatch in 18 + 6 calls; fp32 subnormals are kept, ties go to even, the first inf is where NumPy has it]

Steps, bit for bit against np.maximum-clamped theta + float32(alpha) * x in NumPy float32, the clamp from oS = d - m on:
one-hidden-layer policies with d = 512, 257, 767 (m = 1) and 512, 513, 511 (m = 8), d asserted with mjx_num_params; log_std
entries planted below, just below, exactly at and just above min_log_std, the last weight oS - 1 below it; alpha 0, -0.3, 1e-30,
1e30; mjx_apply_npg_step with g.x 3.7, -3.7, 0, 1e-300 at step_size 0.05, alpha_out bit-equal to
np.sqrt(np.abs(step_size / (gdotx + 1e-20))) and accepted as NULL.
    [measured: no mismatch in 120 + 120 calls, alpha_out equal in all 96 that ask for it]"""
import pytest

from tests._worker_run import worker_result

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_samplepath_worker.py", 600, "sample-path")


def _within(r, key, bar=1.0):
    if key + "_edge" in r["err"]:
        print("[samplepath matrix] %-18s %.3g  %s" % ((key + "_edge",) + tuple(r["err"][key + "_edge"])))
    e, case = r["err"][key]
    print("[samplepath matrix] %-18s %.3g  %s" % (key, e, case))
    assert e <= bar, (key, e, case)


def _zero(r, *keys):
    for k in keys:
        assert r["count"][k] == 0, (k, r["count"][k], r["first"].get(k))


def test_worker_ran_every_case_and_its_device_part_is_short():
    r = _result()
    from tests import _samplepath_cases as K
    per = 1 + len(K.SCAN_LENGTHS)                            # the batch and one call per length
    assert r["cases"]["scan0"] == len(K.SCAN0_CONFIGS) * per + 2 and r["cases"]["scan1"] == len(K.SCAN1_CONFIGS) * per + 2
    assert r["cases"]["scan2_bits_bad"] == len(K.SCAN2_LAMBDAS) * per + 2
    assert r["cases"]["stats_s"] == 2 * 2 * len(K.STATS_N) and r["cases"]["std_rel_mu_1e+08"] == len(K.STATS_N) - 1
    assert r["cases"]["whiten_bad"] == len(K.WHITEN_SIZES) * len(K.WHITEN_VARIANTS) and r["cases"]["cast_bad"] == len(K.CAST_SIZES)
    calls = len(K.STEP_M) * len(K.STEP_RESIDUES) * K.STEP_VARIANTS
    assert r["cases"]["step_bad"] == calls * len(K.STEP_ALPHAS) and r["cases"]["npg_bad"] == calls * len(K.NPG_GDOTX)
    print("[samplepath matrix] seconds", r["seconds"], r["policies"])
    assert r["seconds"]["all"] < 60


def test_discount_scan_against_long_double_on_every_length_and_factor():
    _within(_result(), "scan0")


def test_gae_against_long_double_on_every_length_factor_and_flag_pattern():
    _within(_result(), "scan1")


def test_lambda_outside_the_unit_interval_gives_numpys_difference_bit_for_bit():
    _zero(_result(), "scan2_bits_bad")


def test_scans_write_every_step_of_every_trajectory_and_nothing_else():
    _zero(_result(), "scan_unwritten", "scan_outside_touched", "scan_guard_touched")


def test_scans_refuse_bad_arguments_on_the_host_and_accept_an_empty_batch():
    _zero(_result(), "scan_rc_bad")


def test_sum_stats_against_long_double_below_at_and_beyond_one_grid_pass():
    r = _result()
    _within(r, "stats_s")
    _within(r, "stats_q")
    _zero(r, "stats_n_bad", "stats_guard_touched")


def test_two_pass_standard_deviation_on_a_large_mean():
    """(N + 4) 2^-53 bounds q's relative error by 3.3e-11 at N = 300 001 in the worst case; a pairwise order stays orders below"""
    r = _result()
    print("[samplepath matrix] mu 0: %.3g  %s" % tuple(r["err"]["std_rel_mu_0"]))
    _within(r, "std_rel_mu_1e+08", 1e-12)


def test_whiten_cast_is_the_correctly_rounded_numpy_expression():
    _zero(_result(), "whiten_bad", "whiten_guard_touched")


def test_cast_is_numpys_astype_float32_at_overflow_ties_and_subnormals():
    _zero(_result(), "cast_bad", "cast_guard_touched", "cast_rc_bad")


def test_apply_step_is_the_numpy_float32_step_with_the_clamp_from_oS():
    _zero(_result(), "step_d_bad", "step_bad", "step_guard_touched")


def test_apply_npg_step_forms_numpys_step_length_and_the_same_step():
    _zero(_result(), "npg_alpha_bad", "npg_bad", "npg_guard_touched")
