"""The checks of tests/test_gpu_samplepath_matrix.py can fail, and pass what they should (CPU only).  tests/_samplepath_cases.py
emulates the sample-path kernels of csrc/vecops.h in NumPy: k_traj_scan's 256 segments with thread 0 chaining the carries, in
fp64; the statistics as NumPy's fp64 sums over what the 512 x 256 grid reads; the casts and the float32 step as the NumPy
expressions include/mjx.h names.  The honest emulations pass with room; each planted defect is flagged at the smallest size at
which it can occur."""
import numpy as np
import pytest

from tests import _samplepath_cases as K

_REF = {}


def _edge_refs():
    """the long-double references of a few configurations on the batch of every edge length, formed once"""
    if not _REF:
        off = K.offsets_of(K.EDGE_LENS)
        N = int(off[-1])
        c0 = [K.SCAN0_CONFIGS[i] for i in (3, 4, 1)]         # (0.995, mixed), (1, positive), (0.5, positive)
        x0 = [K.scan_input(dist, N, 100 + i) for i, (g, dist) in enumerate(c0)]
        _REF["off"], _REF["c0"], _REF["x0"] = off, c0, x0
        _REF["r0"] = K.scan0_references([(x, g) for x, (g, dist) in zip(x0, c0)], off)
        c1 = [K.SCAN1_CONFIGS[i] for i in (0, 4)]            # (0.995, 0.97) scale 1; (0.99, 1) scale 1e6, mixed rewards
        in1 = [(K.scan_input(dist, N, 200 + i), K.baseline_input(N, sc, 200 + i), K.flags_for(fl, len(K.EDGE_LENS)), ga, la)
               for i, (ga, la, fl, sc, dist) in enumerate(c1)]
        _REF["in1"] = in1
        _REF["r1"] = K.scan1_references(in1, off)
    return _REF


def _scan0(T, g, dist="normal", defect=None, lens=None, start=0, seed=1):
    off = K.offsets_of((T,) if lens is None else lens, start)
    x = K.scan_input(dist, int(off[-1]), seed)
    ref, A = K.scan0_reference(x, off, g)
    buf = K.emulate_scan(K.new_out(int(off[-1])), 0, x, None, off, None, g, None, defect)
    return K.scan_check(buf, off, ref, A, 4)


def _scan1(lens, gamma, lam, flags, defect=None, seed=2, scale=1.0):
    off = K.offsets_of(lens)
    N = int(off[-1])
    r, b = K.scan_input("normal", N, seed), K.baseline_input(N, scale, seed)
    term = None if flags is None else np.asarray(flags, np.uint8)
    buf = K.emulate_scan(K.new_out(N), 1, r, b, off, term, gamma, lam, defect)
    if lam < 0 or lam > 1 or np.isnan(lam):
        return K.diff_check(buf, off, r, b)
    ref, A = K.scan1_reference(r, b, off, term, gamma, lam)
    return K.scan_check(buf, off, ref, A, 6)


def test_references_are_long_double_and_the_layouts_hold_every_edge():
    assert np.finfo(np.longdouble).nmant >= 63
    assert set(K.SCAN_LENGTHS) == set(K.EDGE_LENS) and K.EDGE_LENS[0] == 0 and K.EDGE_LENS[-1] == 0 and 0 in K.EDGE_LENS[1:-1]
    assert -(-65537 // 256) == 257
    assert sorted({g for g, d in K.SCAN0_CONFIGS}) == [0.0, 0.5, 0.9, 0.995, 1.0] and {d for g, d in K.SCAN0_CONFIGS} == set(K.DISTS)
    assert {(c[0], c[1]) for c in K.SCAN1_CONFIGS} == {(0.995, 0.97), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5), (0.99, 1.0)}
    assert {c[2] for c in K.SCAN1_CONFIGS} == set(K.FLAGS) and {c[3] for c in K.SCAN1_CONFIGS} == {1.0, 1e6}
    f = K.flags_for("pattern", 16)
    assert not np.array_equal(f[:-2], f[2:]) and 0 < f.sum() < 16
    lens = K.many_lens()
    assert len(lens) == K.MANY and set(lens.tolist()) == {0, 1, 2, 3}
    steps = (len(K.SCAN0_CONFIGS) + len(K.SCAN1_CONFIGS)) * sum(K.EDGE_LENS) + 2 * int(lens.sum()) + 2 * sum(K.SHIFTED_LENS)
    assert steps < 1.15e6, steps                             # the long-double loops stay short
    a = K.cast_input(257)
    assert all(np.any((a == v) & (np.signbit(a) == np.signbit(v))) for v in K.CAST_PLANTS[:-1]) and np.isnan(a).sum() == 2
    assert np.isnan(a[-1]) or a[-1] == 0.0                   # a planted value sits on the last element
    got = {(m, r): K.step_policy(m, r) for m in K.STEP_M for r in K.STEP_RESIDUES}
    for (m, r), (n, h, d) in got.items():
        assert d == K.num_params(n, h, m) and d % 256 == r and 256 < d < 1024, (m, r, n, h, d)


def test_scan_ld_is_the_sequential_recurrence():
    x = K.scan_input("normal", 11, 3)
    off = np.array([2, 2, 7, 11])
    ref, A = K.scan0_reference(x, off, 0.9)
    for lo, hi in ((2, 7), (7, 11)):
        run, runa = K.LD(0), K.LD(0)
        for t in range(hi - 1, lo - 1, -1):
            run = K.LD(x[t]) + K.LD(0.9) * run
            runa = abs(K.LD(x[t])) + K.LD(0.9) * runa
            assert ref[t] == run and A[t] == runa
    assert np.all(ref[:2] == 0)
    bn = K.next_baseline(np.arange(1.0, 10.0), np.array([0, 3, 3, 9]), np.array([1, 1, 0], np.uint8), np.float64)
    assert bn.tolist() == [2, 3, 0, 5, 6, 7, 8, 9, 9]


def test_honest_segmented_scan_passes_with_room_on_every_edge_length():
    R = _edge_refs()
    off, N = R["off"], int(R["off"][-1])
    for (g, dist), x, (ref, A) in zip(R["c0"], R["x0"], R["r0"]):
        res = K.scan_check(K.emulate_scan(K.new_out(N), 0, x, None, off, None, g, None), off, ref, A, 4)
        print("[samplepath checks] mode 0 g %-5g %-8s ratio %.3f traj %d t %d" % (g, dist, res["ratio"], res["traj"], res["t"]))
        assert K.scan_ok(res) and res["ratio"] < 0.3, res
    for (r, b, term, ga, la), (ref, A) in zip(R["in1"], R["r1"]):
        res = K.scan_check(K.emulate_scan(K.new_out(N), 1, r, b, off, term, ga, la), off, ref, A, 6)
        print("[samplepath checks] mode 1 gamma %g lambda %g ratio %.3f traj %d t %d" % (ga, la, res["ratio"], res["traj"], res["t"]))
        assert K.scan_ok(res) and res["ratio"] < 0.3, res
        for lam in K.SCAN2_LAMBDAS:
            assert K.diff_ok(K.diff_check(K.emulate_scan(K.new_out(N), 1, r, b, off, term, ga, lam), off, r, b))


def test_single_trajectories_and_a_shifted_first_offset_pass():
    for T in K.SCAN_LENGTHS[:-1]:
        for g in (0.0, 0.995, 1.0):
            assert K.scan_ok(_scan0(T, g, "mixed")), (T, g)
    assert K.scan_ok(_scan0(None, 0.995, lens=K.SHIFTED_LENS, start=K.SHIFTED_START))
    assert K.scan_ok(_scan1((0, 3, 257, 0, 2), 0.995, 0.97, (1, 0, 1, 1, 0)))
    assert K.scan_ok(_scan1((0, 3, 257, 0, 2), 0.995, 0.97, None))


@pytest.mark.parametrize("T", [2, 257])
def test_a_dropped_carry_is_flagged_at_the_first_seam_and_the_first_long_segment(T):
    assert K.scan_ok(_scan0(T, 0.995))
    res = _scan0(T, 0.995, defect="carry_dropped")
    assert res["ratio"] > 1.0 and res["unwritten"] == 0, res
    assert K.scan_ok(_scan0(1, 0.995, defect="carry_dropped"))          # T = 1 has no seam: 2 is the smallest


def test_a_carry_weight_one_power_short_is_flagged():
    for T in (257, 3):                                                    # segments of two elements; of one (g^0 for g)
        assert _scan0(T, 0.995, defect="pw_short")["ratio"] > 1.0, T
    assert K.scan_ok(_scan0(2, 0.995, defect="pw_short"))                # the last segment's weight only ever multiplies a zero carry


def test_wrong_bootstrap_flag_factor_and_mode_are_flagged():
    lens, flags = (3, 1, 257, 2), (1, 0, 0, 1)
    assert K.scan_ok(_scan1(lens, 0.995, 0.97, flags))
    for defect in ("bootstrap_swapped", "flag_neighbour", "gamma_for_gl"):
        res = _scan1(lens, 0.995, 0.97, flags, defect)
        print("[samplepath checks] %-18s ratio %.3g traj %d t %d" % (defect, res["ratio"], res["traj"], res["t"]))
        assert res["ratio"] > 1.0, (defect, res)
    # the smallest batch: one trajectory of one step shows the bootstrap, two show the neighbour's flag, two steps the factor
    assert _scan1((1,), 0.995, 0.97, (1,), "bootstrap_swapped")["ratio"] > 1.0
    assert _scan1((1,), 0.995, 0.97, (0,), "bootstrap_swapped")["ratio"] > 1.0
    assert _scan1((1, 1), 0.995, 0.97, (1, 0), "flag_neighbour")["ratio"] > 1.0
    assert _scan1((2,), 0.995, 0.97, (0,), "gamma_for_gl")["ratio"] > 1.0
    assert K.scan_ok(_scan1(lens, 0.9, 0.0, flags))
    assert _scan1(lens, 0.9, 0.0, flags, "mode2_for_lam0")["ratio"] > 1.0
    assert _scan1((1,), 0.9, 0.0, (0,), "mode2_for_lam0")["ratio"] > 1.0
    # ... and the difference served where the scan is due the other way round: mode 2 checked bit by bit
    off = K.offsets_of(lens)
    r, b = K.scan_input("normal", int(off[-1]), 5), K.baseline_input(int(off[-1]), 1.0, 5)
    buf = K.emulate_scan(K.new_out(int(off[-1])), 1, r, b, off, np.array(flags, np.uint8), 0.9, 0.0)
    assert K.diff_check(buf, off, r, b)["bad"] > 0


def test_misplaced_trajectories_are_flagged():
    lens = (0, 1)                                                         # the smallest batch with an empty trajectory and a successor
    assert K.scan_ok(_scan0(None, 0.9, lens=lens))
    res = _scan0(None, 0.9, lens=lens, defect="empty_shifts")
    assert res["unwritten"] == 1 and res["guard_touched"] == 1 and not K.scan_ok(res), res
    res = _scan0(None, 0.9, lens=(2, 0, 3, 4), defect="empty_shifts")
    assert not K.scan_ok(res) and res["ratio"] > 1.0, res
    res = _scan0(None, 0.9, lens=(1,), start=1, defect="offset0_ignored")
    assert res["unwritten"] == 1 and res["outside_touched"] == 1, res
    res = _scan0(None, 0.9, lens=K.SHIFTED_LENS, start=K.SHIFTED_START, defect="offset0_ignored")
    assert res["unwritten"] > 0 and res["outside_touched"] > 0 and not K.scan_ok(res), res
    assert not K.diff_ok(K.diff_check(K.emulate_scan(K.new_out(3), 1, np.ones(3), np.ones(3), np.array([1, 3]), None, 0.9, -1.0,
                                                     "offset0_ignored"), np.array([1, 3]), np.ones(3), np.ones(3)))


def test_scan_check_flags_nan_and_a_nonzero_error_where_the_bound_is_zero():
    off = K.offsets_of((4,))
    x = np.array([1.0, 0.0, 0.0, 0.0])
    ref, A = K.scan0_reference(x, off, 0.5)
    buf = K.emulate_scan(K.new_out(4), 0, x, None, off, None, 0.5, None)
    assert K.scan_ok(K.scan_check(buf, off, ref, A, 4))
    bad = buf.copy(); K.body(bad)[2] = 1e-300
    assert K.scan_check(bad, off, ref, A, 4)["ratio"] == np.inf
    bad = buf.copy(); K.body(bad)[0] = np.nan
    assert K.scan_check(bad, off, ref, A, 4)["ratio"] == np.inf
    bad = buf.copy(); bad[0] ^= 1
    assert K.scan_check(bad, off, ref, A, 4)["guard_touched"] == 1


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("mu", K.STATS_MU)
def test_numpy_sums_pass_the_statistics_check_with_room(mu):
    for N in K.STATS_N:
        x = K.stats_input(N, mu)
        for shift in (0.0, float(np.sum(x) / N) if N else 1.5):
            res = K.stats_check(K.emulate_stats(x, shift), x, shift)
            assert K.stats_ok(res) and max(res["s"], res["q"]) < 0.3, (N, mu, shift, res)
        if N:
            assert K.std_rel_error(K.emulate_stats(x, float(np.sum(x) / N))[1], x) <= 1e-12, N
    assert K.emulate_stats(np.zeros(0), 0.0).tolist() == [0.0, 0.0, 0.0]
    assert not K.stats_ok(K.stats_check(np.array([0.0, 1e-300, 0.0]), np.zeros(0), 0.0))     # N = 0: exactly zero
    assert not K.stats_ok(K.stats_check(np.array([0.0, 0.0, 1.0]), np.zeros(0), 0.0))


def test_planted_statistics_defects_are_flagged():
    for mu in K.STATS_MU:
        for defect, N in (("partial0_dropped", 1), ("partial511_dropped", 131072), ("tail_dropped", 131073)):
            x = K.stats_input(N, mu)
            for shift in (0.0, float(np.sum(x) / N)):
                res = K.stats_check(K.emulate_stats(x, shift, defect), x, shift)
                if N == 1 and shift != 0.0:                   # v = 0: nothing to drop
                    continue
                assert res["s"] > 1.0 and res["q"] > 1.0, (defect, mu, shift, res)
        x = K.stats_input(131072, mu)
        assert K.stats_ok(K.stats_check(K.emulate_stats(x, 0.0, "tail_dropped"), x, 0.0))      # no tail yet at one grid pass
        for N in (1, 257):
            x = K.stats_input(N, mu) + 0.5
            shift = float(np.sum(x) / N) - 0.25
            res = K.stats_check(K.emulate_stats(x, shift, "q_unshifted"), x, shift)
            assert res["s"] <= 1.0 and res["q"] > 1.0, (N, mu, res)
    x = K.stats_input(300001, 1e8)                          # the unshifted second pass is what the shift is there against
    assert K.std_rel_error(K.emulate_stats(x, 0.0)[1] - np.sum(x) ** 2 / len(x), x) > 1e-12


# ---------------------------------------------------------------- casts
def test_numpy_casts_pass_and_rounding_defects_are_flagged_at_the_planted_values():
    for size in K.SMALL_SIZES:
        a = K.cast_input(size)
        buf = K.new_out(size, 4)
        K.body(buf)[:] = K.emulate_cast(a)
        assert K.bits_ok(K.bits_check(buf, K.cast_expect(a))), size
    a = K.CAST_PLANTS
    want = K.cast_expect(a)
    assert np.isinf(want[a == 3.4028235677973366e38]) and want[a == 2.0 ** -150] == 0 and want[a == 2.0 ** -150 * (1 + 2.0 ** -52)] > 0
    assert want[a == 1 + 2.0 ** -24] == 1 and want[a == 1 + 3 * 2.0 ** -24] == np.float32(1 + 2.0 ** -22)
    assert 1 + 2.0 ** -24 + 2.0 ** -53 == 1 + 2.0 ** -24 and want[a == 1 + 2.0 ** -24 + 2.0 ** -52] == np.float32(1 + 2.0 ** -23)
    for defect, values in (("truncate", (1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -52, 3.4028235677973366e38, 1e39,
                                        -(2.0 ** -150) * (1 + 2.0 ** -52))),
                           ("flush", (1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -150) * (1 + 2.0 ** -52)))):
        buf = K.new_out(len(a), 4)
        K.body(buf)[:] = K.emulate_cast(a, defect)
        res = K.bits_check(buf, want)
        assert not K.bits_ok(res), defect
        got = K.body(buf)
        for v in values:
            i = int(np.nonzero(a == v)[0][0])
            assert got[i].view(np.uint32) != want[i].view(np.uint32), (defect, v)
        assert got[a == 1 + 2.0 ** -24] == 1                 # this tie rounds down either way: the one above it tells
    one = np.array([1 + 3 * 2.0 ** -24])                    # the smallest size
    buf = K.new_out(1, 4)
    K.body(buf)[:] = K.emulate_cast(one, "truncate")
    assert K.bits_check(buf, K.cast_expect(one))["bad"] == 1
    buf = K.new_out(3, 4)                                     # -0.0 against 0.0, an unwritten element against NaN, NaN against NaN
    K.body(buf)[:2] = (0.0, np.nan)
    res = K.bits_check(buf, np.array([-0.0, np.nan, np.nan], np.float32))
    assert res["bad"] == 2 and [f[0] for f in res["first"]] == [0, 2]


def test_whiten_expression_passes_and_a_missing_eps_is_flagged():
    for variant in K.WHITEN_VARIANTS:
        for size in K.SMALL_SIZES:
            a, mean, std, eps = K.whiten_input(size, variant)
            want = K.whiten_expect(a, mean, std, eps)
            buf = K.new_out(size, 4)
            K.body(buf)[:] = want
            assert K.bits_ok(K.bits_check(buf, want)) and np.all(np.isfinite(want))
            with np.errstate(all="ignore"):
                K.body(buf)[:] = ((a - mean) / std).astype(np.float32)
            if size > 1 or variant == "mean1e8":                 # (one element is its own mean: 0 / x)
                assert K.bits_check(buf, want)["bad"] > 0, (variant, size)
    a, mean, std, eps = K.whiten_input(257, "mean1e8")
    buf = K.new_out(257, 4)
    K.body(buf)[:] = ((a.astype(np.float32) - np.float32(mean)) / np.float32(std + eps))      # the subtraction in fp32
    assert K.bits_check(buf, K.whiten_expect(a, mean, std, eps))["bad"] > 200


# ---------------------------------------------------------------- steps
def _step(m, residue, alpha, variant, defect=None):
    n, h, d = K.step_policy(m, residue)
    theta, x = K.step_input(d, m, variant, 10 * d + variant)
    buf = K.emulate_step(K.new_out(d, 4), theta, x, alpha, d - m, defect=defect)
    return K.bits_check(buf, K.step_expect(theta, x, alpha, d - m)), d


def test_exact_float32_step_passes_and_the_plants_sit_where_they_should():
    for m in K.STEP_M:
        for residue in K.STEP_RESIDUES:
            for alpha in K.STEP_ALPHAS + tuple(K.npg_alpha(g) for g in K.NPG_GDOTX):
                for variant in range(K.STEP_VARIANTS):
                    res, d = _step(m, residue, alpha, variant)
                    assert K.bits_ok(res), (m, residue, alpha, variant, res)
    mls = np.float32(K.MIN_LOG_STD)
    seen = set()
    for variant in range(4):
        theta, x = K.step_input(300, 1, variant, variant)
        v = K.step_expect(theta, x, -0.3, 299)
        seen.add(int(np.sign(float(theta[299]) - float(mls))))
        assert v[299] == max(theta[299], mls) and v[298] == mls - 1 and not np.any(np.isnan(v))
    assert seen == {-1, 0, 1}
    theta, x = K.step_input(300, 8, 1, 1)
    assert sorted(np.sign(theta[292:296].astype(np.float64) - float(mls)).tolist()) == [-1, -1, 0, 1] and np.any(x[296:] != 0)
    assert K.npg_alpha(0.0) == np.sqrt(0.05 / 1e-20) and K.npg_alpha(-3.7) == K.npg_alpha(3.7) and np.isfinite(np.float32(K.npg_alpha(1e-300)))


def test_planted_step_defects_are_flagged():
    res, d = _step(8, 255, -0.3, 4, "fma")
    print("[samplepath checks] fused multiply-add: %d of %d elements differ" % (res["bad"], d))
    assert 0.03 * d < res["bad"] < 0.16 * d, res             # one element in seven here; about 8 % in a CG step (csrc/vecops.h step_add)
    for m in K.STEP_M:
        for residue in K.STEP_RESIDUES:
            for alpha in K.STEP_ALPHAS:
                assert _step(m, residue, alpha, 0, "clamp_early")[0]["bad"] == 1, (m, residue, alpha)       # oS - 1 lies below the floor
    # the clamp beginning one late shows where the first log_std entry ends below the floor: variants 0 and 1 plant one there
    for m in K.STEP_M:
        for variant in (0, 1):
            assert _step(m, 0, 0.0, variant, "clamp_late")[0]["bad"] == 1, (m, variant)
        assert _step(m, 0, 0.0, 2, "clamp_late")[0]["bad"] == 0              # exactly at the floor: nothing to see
    for m in K.STEP_M:
        res, d = _step(m, 1, -0.3, 0, "last_unwritten")
        assert d % 256 == 1 and res["bad"] == 1 and res["first"][0][0] == d - 1, res
