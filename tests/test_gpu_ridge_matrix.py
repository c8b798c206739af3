"""The device half of the ridge value baselines (csrc/baseline.h, K6) against long-double references, arm by arm and edge by edge:
the three Gram kernels behind mjx_bl_gram (k_bl_gram_mfma, k_bl_gram_mfma_blk, k_bl_gram) with the reduce / mirror kernel,
mjx_bl_predict and mjx_bl_features_f32.  Every check runs in ONE fresh worker process under a time limit
(tests/_ridge_matrix_worker.py; cases, inputs, references and check functions in tests/_ridge_cases.py); a worker that failed is
not started again -- the remaining tests fail with its output.  tests/test_ridge_checks.py shows on CPU that the checks pass
NumPy emulations of the three arms and flag the defects a wrong kernel would leave.

Inputs: observations randn * 4 (about 1.2 % beyond the +-10 clip) with +10, -10, +-10.000001, 0.0 and -0.0 planted; tpos from
ragged trajectory windows, beginning 2500, 0, 999, 1000 (tau 2.5, 0, just below 1, exactly 1); y randn times a scale that differs
per case (1e-3 .. 1e3).  No NaN and no inf: the device clips with fmin / fmax, which drop a NaN, np.clip propagates it -- the two
differ there by design.

Gram.  Every case first asserts arm and Z with mjx_bl_gram_route under the same switch.
    k_bl_gram_mfma      quadratic n 1 (8 columns), 3 (15), 4 (20), 16 (158: partial last tile), 17 (176: all 66 tiles); linear n 10
                        (16 columns), 11 (17), 24 (32 n fills the 3 x 256 staging slots); MLP features n 5 (no constant column);
                        each at N 1, 31, 32, 33; quadratic 17 and linear 24 also at N 2048, 2049, 4097 (Z 1, 2, 3; the last range
                        ragged); linear n 1 at N 2 000 000 (Z 512, the last workgroups' ranges empty)
    k_bl_gram_mfma_blk  linear n 25 (one diagonal block), 64 (fills the 8 x 256 slots); quadratic n 18 (195 columns: second block 67
                        wide), 21 (258: third block 2 wide) at N 1, 31, 32, 33, 2049, 4097; quadratic n 64 (2150 columns, 153 block
                        pairs, the reduce kernel grid-strides) at N 1, 33; quadratic 18 at N 530 000 (Z 256, the last range empty).
                        Each preceded by a call of the same shape -- as many partials, as large -- with y scaled by 1e6: this arm's
                        scratch block is not cleared between calls, and a partial it did not rewrite would show
    k_bl_gram           MJX_GRAM_FMA=1: quadratic n 3, 10 (71 columns: second tile 7 wide), 17 (176: last tile 48 wide), linear 58 (64
                        columns), 59 (65); without it: linear 65 (first shape only this arm serves), 126 (64 KiB of dynamic LDS);
                        at N 1, 31, 32, 33, 4096, 4097, 8193; quadratic n 65 (2216 columns) at N 33
    refused             linear n 127: MJX_ERR_UNSUPPORTED, a sentinel-filled G untouched; N 0: MJX_ERR_ARG
Check: R = [A y]^T [A y] with the features formed from the fp64 inputs in long double (the worker asserts nmant >= 63) and summed in
long double; beyond 5000 rows each 512-row block's product in fp64 and the blocks summed in long double.  For every entry
    |G - R| <= (N + 32 + b) 2^-53 (|A y|^T |A y|),   b = 512 for the blocked reference, 0 otherwise
-- the forward bound of a dot product of N terms in any order, so it holds for all three arms; 32 covers the at most 7 roundings of
a device feature and the sum of the partials.  Reported: the worst ratio error / bound per arm with its case, tile and index;
G == G.T bit for bit; every entry finite; NaNs behind G intact.  The bar is 1.  Measured on the MI355X:
    [k_bl_gram_mfma      0.123: quadratic n 17, N 1, tile (10, 10), entry (164, 164)]
    [k_bl_gram_mfma_blk  0.161: quadratic n 21, N 1, block (1, 1), entry (197, 197)]
    [k_bl_gram           0.128: quadratic n 65, N 33, tile (14, 34), entry (935, 2200)]
(NumPy emulations of the arms' summation orders: at most 0.06, tests/test_ridge_checks.py.)

Predict (k_bl_predict: 256 threads up to n 32, 128 up to 64, 64 up to 128).  Kinds 1 and 2 at n 1, 32, 33, 64, 65, 128, each at
N 1, nth - 1, nth, nth + 1, 1000; linear n 1 at N 8192 * 256 + 1 (the grid is capped: a second grid-stride pass); n 129 is
refused and leaves the output alone.  Coefficients randn with per-column scales 1e-3 .. 1e3.  Per row
    |out - ref| <= (F + 16) 2^-53 sum_c |feat_c| |coef_c|
against the long-double reference.  Measured on the MI355X:
    [k_bl_predict        0.215: quadratic n 1, N 1000, row 457; 0.199 in the second grid-stride pass]

Features (k_bl_features_f32): n 1, 17, 64 at N 1, 255, 257, and n 1 at N 419 431 (the first element count beyond 8192 x 256).
Observation columns bit-equal to float32(clip(obs, -10, 10) / 10); time columns within 1 fp32 ulp of the long-double power
rounded to fp32 [measured: 0 ulp in all ten cases] and exact at tpos 0 and 1000; a NaN tail behind the output stays NaN."""
import pytest

from tests._worker_run import worker_result

pytestmark = pytest.mark.gpu


def _result():
    return worker_result("_ridge_matrix_worker.py", 600, "ridge matrix")


def _within_bound(r, key):
    e, case = r["err"][key]
    print("[ridge matrix] %-14s %.3f  %s" % (key, e, case))
    assert e <= 1.0, (key, e, case)


def _zero(r, *keys):
    for k in keys:
        assert r["count"][k] == 0, (k, r["count"][k])


def test_every_gram_case_ran_on_the_arm_and_ranges_it_is_named_for():
    r = _result()
    assert r["count"]["route_mismatch"] == 0, {k: v for k, v in r["routes"].items() if "expected" in v}
    from tests import _ridge_cases as K
    named = [k for k in r["routes"] if not k.startswith("refused")]
    assert len(named) == len(K.GRAM_CASES)
    for arm in K.ARMS:
        assert any(v.startswith(arm + " ") for v in r["routes"].values()), arm
    zs = {(k, v.split(" Z ")[1]) for k, v in r["routes"].items() if " Z " in v}
    assert ("k_bl_gram_mfma kind 1 n 1 N 2000000", "512") in zs and ("k_bl_gram_mfma_blk kind 2 n 18 N 530000", "256") in zs


def test_gram_on_one_workgroup_of_matrix_cores_against_long_double():
    _within_bound(_result(), "gram_mfma")


def test_gram_by_feature_blocks_against_long_double_after_a_poisoned_call():
    _within_bound(_result(), "gram_blk")


def test_gram_fma_arm_against_long_double():
    _within_bound(_result(), "gram_fma")


def test_gram_is_symmetric_finite_and_stays_inside_its_output():
    _zero(_result(), "gram_not_symmetric", "gram_not_finite", "gram_tail_touched")


def test_gram_refuses_what_no_arm_serves_and_leaves_the_output_alone():
    r = _result()
    _zero(r, "gram_refusal_bad")
    assert r["routes"]["refused kind 1 n 127 N 33"] == "rc -3" and r["routes"]["refused kind 1 n 5 N 0"] == "rc -1"


def test_predict_against_long_double_at_every_workgroup_size():
    r = _result()
    _within_bound(r, "predict")
    _zero(r, "predict_not_finite", "predict_tail_touched", "predict_refusal_bad")
    assert len(r["cases"]["predict"]) == 61


def test_mlp_features_bitwise_observations_and_time_powers_within_one_ulp():
    r = _result()
    print("[ridge matrix] time columns: %.3f ulp  %s" % tuple(r["err"]["feat_time_ulps"]))
    _zero(r, "feat_obs_bad", "feat_time_bad", "feat_exact_bad", "feat_tail_touched")
    assert len(r["cases"]["feat_time_ulps"]) == 10
