"""The checks of tests/test_gpu_ridge_matrix.py can fail, and pass what they should (CPU only).  tests/_ridge_cases.py emulates
the three Gram arms of csrc/baseline.h in NumPy fp64 -- Z sample ranges, chunks of 32 rows, products four rows at a time on the
matrix-core arms and one on the FMA arm, partial sums in a scratch block that persists between calls, the reduce kernel's mirror
by tile -- and k_bl_predict's column-by-column sum.  The honest emulations pass gram_check / predict_check with room (the
largest ratio error / bound over the shapes below is 0.06); each planted defect is flagged at the smallest N at which it can
occur, and at a larger one."""
import numpy as np
import pytest

from tests import _ridge_cases as K
from tests._ridge_cases import BLK, FMA, MFMA


def _scratch(kind, n, Z):
    FA = K.num_features(kind, n) + 1
    return np.zeros((Z, FA, FA))


def _run(arm, kind, n, N, defect=None, seed=None, poison=True):
    """the check's verdict on one emulated call; the block arm's scratch first takes a call with y scaled by 1e6, as in the worker"""
    want_arm, Z = K.route_expect(kind, n, N, fma=arm == FMA)
    assert want_arm == arm, (arm, kind, n, N)
    seed = K.case_seed(kind, n, N) if seed is None else seed
    obs, tpos, y = K.make_inputs(n, N, seed, 37.0)
    sc = _scratch(kind, n, Z)
    if arm == BLK and poison:
        o2, t2, y2 = K.make_inputs(n, N, seed + 1, 37.0e6)
        K.emulate_gram(kind, n, o2, t2, y2, arm, Z, sc)
    G = K.emulate_gram(kind, n, obs, tpos, y, arm, Z, sc, defect)
    R, B, b = K.gram_reference(kind, n, obs, tpos, y)
    return K.gram_check(G, R, B, N, b, K.TILE[arm])


HONEST = [(MFMA, 2, 1, 1), (MFMA, 2, 4, 33), (MFMA, 1, 24, 4097), (MFMA, 0, 5, 32), (BLK, 2, 18, 33), (BLK, 1, 25, 2049),
          (FMA, 2, 10, 4097), (FMA, 1, 65, 31), (FMA, 1, 59, 8193), (MFMA, 2, 3, 6000)]


@pytest.mark.parametrize("arm,kind,n,N", HONEST)
def test_honest_emulation_passes_with_room(arm, kind, n, N):
    res = _run(arm, kind, n, N)
    print("[ridge checks] %-50s ratio %.3f at %s" % (K.case_name(arm, kind, n, N, {}), res["ratio"], res["at"]))
    assert K.gram_ok(res), res
    assert res["ratio"] < 0.25, res                         # an honest summation order leaves room: the bar of 1 is not met by luck


def test_inputs_hold_what_the_cases_are_about():
    obs, tpos, y = K.make_inputs(17, 4097, 5)
    for v in K.PLANTS:
        assert np.any((obs == v) & (np.signbit(obs) == np.signbit(v))), v
    assert np.sum(np.abs(obs) > 10.0) > 100                 # randn * 4: ~1.2 % beyond the clip
    assert set(K.TPOS_HEAD) <= set(tpos[:4].tolist()) and tpos.max() == 2500 and np.sum(tpos == 0) > 10
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(y))
    assert K.make_inputs(1, 1, 3)[0].shape == (1, 1) and K.make_tpos(1)[0] == 2500
    assert np.finfo(np.longdouble).nmant >= 63


# (arm, kind, n, smallest N at which the defect can occur, a larger N); n = 17 at N = 1 holds all six planted values
PLANTED = {
    "drop_last": (MFMA, 2, 17, 1, 4097),
    "row32_twice": (MFMA, 2, 17, 33, 4097),
    "tpos_off": (MFMA, 2, 17, 1, 2049),
    "obs_fp32": (FMA, 2, 17, 1, 4097),
    "no_clip": (MFMA, 2, 17, 1, 2049),
    "tau3": (FMA, 1, 59, 1, 4097),
    "mirror": (MFMA, 1, 11, 1, 2049),                       # 17 augmented columns: the first shape with an off-diagonal tile
    "stale": (BLK, 2, 18, 1, 2049),
    "swap_y_const": (BLK, 1, 25, 1, 2049),
}


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_planted_gram_defect_is_flagged(defect):
    arm, kind, n, N0, N1 = PLANTED[defect]
    for N in (N0, N1):
        assert K.gram_ok(_run(arm, kind, n, N)), (defect, N)
        res = _run(arm, kind, n, N, defect)
        print("[ridge checks] %-14s N %-5d ratio %.3g symmetric %s" % (defect, N, res["ratio"], res["symmetric"]))
        assert not K.gram_ok(res), (defect, N, res)
        if defect not in ("mirror",):
            assert res["ratio"] > 1.0, (defect, N, res)     # by the bound itself, not by the symmetry check alone


def test_mirror_defect_shows_in_both_checks_on_each_arm():
    for arm, kind, n, N in ((MFMA, 1, 11, 33), (BLK, 2, 18, 33), (FMA, 2, 10, 33)):
        res = _run(arm, kind, n, N, "mirror")
        assert res["ratio"] > 1.0 and not res["symmetric"], (arm, res)


def test_stale_partials_need_the_preceding_call_to_show():
    """why the worker runs a call with y * 1e6 before every block-arm case: on a fresh (zero) block the defect is invisible"""
    assert K.gram_ok(_run(BLK, 2, 18, 33, "stale", poison=False))
    assert not K.gram_ok(_run(BLK, 2, 18, 33, "stale"))


def test_not_finite_and_asymmetric_results_are_flagged():
    obs, tpos, y = K.make_inputs(3, 33, 1)
    R, B, b = K.gram_reference(2, 3, obs, tpos, y)
    G = np.asarray(R, np.float64)
    assert K.gram_ok(K.gram_check(G, R, B, 33, b, 16))
    for bad in (np.nan, np.inf):
        H = G.copy(); H[2, 5] = H[5, 2] = bad
        res = K.gram_check(H, R, B, 33, b, 16)
        assert not res["finite"] and res["ratio"] == np.inf and res["at"] in ([2, 5], [5, 2]), res
    H = G.copy(); H[7, 1] = np.nextafter(H[7, 1], np.inf)
    res = K.gram_check(H, R, B, 33, b, 16)
    assert not res["symmetric"] and not K.gram_ok(res) and res["ratio"] <= 1.0


@pytest.mark.parametrize("kind,n,N", [(1, 1, 1), (2, 33, 129), (2, 128, 65), (1, 65, 1000)])
def test_predict_check_passes_the_honest_sum_and_flags_defects(kind, n, N):
    obs, tpos, _ = K.make_inputs(n, N, K.case_seed(kind, n, N))
    coef = K.make_coef(kind, n, 9000 + n)
    ref, S = K.predict_reference(kind, n, obs, tpos, coef)
    F = K.num_features(kind, n)
    res = K.predict_check(K.emulate_predict(kind, n, obs, tpos, coef), ref, S, F)
    print("[ridge checks] predict kind %d n %d N %d ratio %.3f" % (kind, n, N, res["ratio"]))
    assert K.predict_ok(res) and res["ratio"] < 0.25, res
    for defect in ("coef_shift", "fp32_acc"):
        bad = K.predict_check(K.emulate_predict(kind, n, obs, tpos, coef, defect), ref, S, F)
        assert not K.predict_ok(bad), (defect, bad)


def test_features_check_flags_a_wrong_entry():
    n, N = 17, 257
    obs, tpos, _ = K.make_inputs(n, N, 11)
    tau = tpos.astype(np.float64) / 1000.0
    good = np.concatenate([np.clip(obs, -10, 10) / 10.0] + [(tau ** k)[:, None] for k in range(1, 5)], axis=1).astype(np.float32)
    assert K.features_ok(K.features_check(good, obs, tpos, n))
    bad = good.copy(); bad[5, 3] = np.nextafter(bad[5, 3], np.float32(2))
    assert K.features_check(bad, obs, tpos, n)["obs_bad"] == 1
    bad = good.copy(); bad[:, :n] = np.float32(np.float32(np.clip(obs, -10, 10)) / np.float32(10))      # the division in fp32
    assert K.features_check(bad, obs, tpos, n)["obs_bad"] > 0
    bad = good.copy(); bad[0, n + 3] = bad[0, n + 2]                                                     # tau^3 for tau^4 at tau 2.5
    assert K.features_check(bad, obs, tpos, n)["time_bad"] == 1
    bad = good.copy(); bad[3, n] = np.nextafter(np.float32(1), np.float32(0))                            # tpos 1000 must give exactly 1
    assert K.features_check(bad, obs, tpos, n)["exact_bad"] == 1
    zero = good.copy(); zero[:, :n][obs == 0.0] = np.float32(0.0)                                              # -0.0 must stay -0.0
    assert K.features_check(zero, obs, tpos, n)["obs_bad"] == 1


def test_case_lists_hold_every_shape_of_the_matrix():
    arms = {a: [(k, n, N, bool(env)) for arm, k, n, N, env, Z, s in K.GRAM_CASES if arm == a] for a in (MFMA, BLK, FMA)}
    assert len(arms[MFMA]) == 9 * 4 + 6 + 1 and len(arms[BLK]) == 4 * 6 + 2 + 1 and len(arms[FMA]) == 7 * 7 + 1
    for arm, k, n, N, env, Z, s in K.GRAM_CASES:
        want = K.route_expect(k, n, N, bool(env))
        assert want[0] == arm and (Z is None or want[1] == Z), (arm, k, n, N)
    assert len(K.PREDICT_CASES) == 2 * 6 * 5 + 1 and len(K.FEATURE_CASES) == 10
    assert [K.predict_threads(n) for n in (32, 33, 64, 65, 128)] == [256, 128, 128, 64, 64]
