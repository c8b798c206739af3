"""The checks of tests/test_gpu_plan_matrix.py can fail, and pass what they should (CPU only).  tests/_plan_cases.py emulates
k_plan_rollout's data movement in NumPy fp32 (the staged image with feat()'s column map and the padding to HW and NS, the tiles the
launched waves own, the lane's action slots and state registers through unit_of, the tail's read of the state before its write, the
guarded store) with a plain fp32 chain standing in for route 0, and the four scoring kernels in fp64 with their fixed summation orders.
The honest emulations pass every check the GPU tests apply, with the same bars from the same fixture and the same derived bounds; each
planted defect is flagged at the case named for it, and where the check is a bar the defect exceeds it at least ten times.  Also, from
the fp64 oracle and the reference's yardsticks alone: the route and the instance of every case, and the input condition that keeps the
per-column measure from dividing by noise (every compared column reaches 1e-3, no state exceeds 1e3)."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _plan_cases as C  # noqa: E402

_PLAIN, _HONEST, _SHONEST = {}, {}, {}
TEN = 10.0


# ---------------------------------------------------------------------------- rollout
def _runner(defect):
    def run(route, name, mem, s0, actions):
        if route == 0:
            key = (name, actions.shape, s0.ndim)
            if key not in _PLAIN:
                _PLAIN[key] = C.plain_fp32(name, mem, s0, actions)
            return _PLAIN[key]
        return C.emulate(name, mem, s0, actions, defect)
    return run


def _yard(name):
    return C.yard(name) if name in C.STEPPED else (None, None)


def _verdict(name, defect=None):
    if defect is None and name in _HONEST:
        return _HONEST[name]
    rec = C.measure(name, _runner(defect))
    out = (C.checks(name, rec, *_yard(name)), rec)
    if defect is None:
        _HONEST[name] = out
    return out


def test_fixture_holds_an_fp32_sized_yardstick_for_every_stepped_case():
    G = np.load(C.FIXTURE)
    assert sorted(G.files) == sorted([p + c for c in C.STEPPED for p in ("pstep_", "pfree_")])
    for key in G.files:
        assert G[key].dtype == np.float64 and G[key].shape == () and 1e-9 < float(G[key]) < 1e-5, key


@pytest.mark.parametrize("case", C.ORDER)
def test_case_is_on_route_1_with_the_instance_it_is_here_for(case):
    """mjx_plan_route (arithmetic alone; the library loads without a device) answers 1, as the restated arithmetic does, and the
    instance is the one the case table names"""
    from mjrl_amd import _lib
    lib = _lib.load()
    ds = C.sizes(case)
    assert lib.mjx_plan_route((ctypes.c_int * len(ds))(*ds), len(ds), C.CASES[case]["m"]) == 1 and C.route(case) == 1
    assert C.instance(case) == C.CASES[case]["inst"]


def test_the_axes_the_cases_are_here_for():
    c, lay = C.CASES, {k: C.layout(k) for k in C.CASES}
    assert c["r1"]["n"] == lay["r1"]["n8"] and c["r1"]["m"] == lay["r1"]["m8"]
    assert [lay[k]["m8"] // 8 for k in ("r3", "r4", "r8", "r9")] == [3, 4, 4, 4]
    assert all(c[k]["dh"][0] < c[k]["dh"][1] for k in ("r3", "r6", "r8", "f3", "g1")) and c["r4"]["dh"] == (64, 32)
    assert c["r5"]["n"] == 32 and c["r5"]["flags"] == 0 and c["r7"]["n"] == 33 and c["r7"]["m"] == 1 and c["r2"]["m"] == 1
    assert (c["r9"]["n"], c["r9"]["m"]) == (64, 32) and C.plan_lds_floats("r9") == max(C.plan_lds_floats(k) for k in c) == 38848
    assert sorted({c[k]["flags"] for k in C.ORDER}) == [0, 1, 3, 5, 7]
    assert C.zero_column("r10") >= 32 and c["r10"]["act"] == C.TANH and C.instance("r10")[1] == 2
    assert {C.instance(k) for k in C.ORDER} == {(hb, nb) for hb in (1, 2, 3, 4) for nb in (1, 2)}          # all eight
    assert c["g1"]["K"] == 5 and (417 + 127) // 128 == 4 and 417 - 32 * 13 == 1 and c["g2"]["rows"] == (1,) and c["g2"]["H"] == 1
    for k in C.ORDER:                                    # one out_scale entry exactly 0 beside +-0.4 wherever a second column exists
        z, mem = C.zero_column(k), C.cached_case(k)[0]
        n, din = c[k]["n"], c[k]["n"] + c[k]["m"]
        for tr in mem["trs"]:
            zeros = np.nonzero(tr[2 * din + n:] == 0)[0]
            assert list(zeros) == ([] if z is None else [z]) and (z is None or abs(tr[2 * din + z]) == np.float32(0.4))


@pytest.mark.parametrize("case", C.STEPPED)
def test_input_condition_holds_from_the_oracle_and_the_reference_alone(case):
    """every compared column's largest |reference| is at least 1e-3 (per member, per run: the step references formed from the fp64
    free-running states, and the free-running states themselves), and no state exceeds 1e3 within H steps"""
    c = C.CASES[case]
    mem, data = C.cached_case(case)
    cols = C.compared_columns(case)
    for key, (s0, actions) in data.items():
        free = C.free_reference(case, key)
        assert np.max(np.abs(free)) < C.CEIL_STATE
        for k in range(c["K"]):
            tops = [np.min(np.max(np.abs(r[..., cols].reshape(-1, len(cols))), 0)) for r in (C.step_reference(free[k], actions, mem, k), free[k][:, 1:])]
            print(case, key, k, "smallest column top %.3e, largest |state| %.3e" % (min(tops), np.max(np.abs(free[k]))))
            assert min(tops) >= C.FLOOR_TOP


@pytest.mark.parametrize("case", C.ORDER)
def test_honest_emulation_passes_every_check(case):
    ok, rec = _verdict(case)
    print("\n".join(rec["runs"]), rec["routes"], _yard(case))
    assert all(ok.values()), ok
    assert rec["calls"] == 2 * len(C.CASES[case]["rows"]) * len(C.CASES[case]["s0"])


def _flagged(case, defect, check, over=False):
    """the honest emulation passes `check`, the defective one fails it; over: the defect's one-step error on route 1 exceeds its bar
    at least ten times"""
    ok, rec = _verdict(case, defect)
    print(case, defect, ok, rec["step"], rec["free"], rec["unwritten"], rec["guard"])
    assert _verdict(case)[0][check] is True
    assert ok[check] is False, (case, defect, ok)
    if over:
        assert rec["step"]["1"] >= TEN * C.MARGIN * C.yard(case)[0], rec["step"]


@pytest.mark.parametrize("case", ["r3", "r6", "r8"])
def test_w2_staged_with_the_row_stride_h2(case):
    _flagged(case, "w2_stride", "mfma", True)


def test_action_part_placed_at_column_n():
    _flagged("r3", "act_col_n", "mfma", True)


def test_fourth_slot_group_dropped():
    _flagged("r4", "drop_q3", "mfma", True)


@pytest.mark.parametrize("case", C.STEPPED)
def test_next_steps_actions_not_refreshed(case):
    _flagged(case, "stale_actions", "mfma", True)


def test_residual_added_from_the_overwritten_block():
    _flagged("r8", "residual_overwritten", "mfma", True)


def test_mask_skipped_in_block_1():
    _flagged("r10", "mask_skip_b1", "masked")
    rec = _verdict("r10", "mask_skip_b1")[1]                 # (the column is left out of the one-step error: only the exact check sees it there)
    assert rec["step"]["1"] < C.MARGIN * C.yard("r10")[0]


def test_affine_applied_under_flags_0():
    _flagged("r5", "affine_forced", "mfma", True)


@pytest.mark.parametrize("case", ["r1", "r9", "g1"])
def test_s0_stride_ignored(case):
    _flagged(case, "s0_stride", "s0")


def test_member_k_reading_member_0s_transforms():
    _flagged("g1", "member0_tr", "mfma", True)


@pytest.mark.parametrize("case", C.ORDER)
def test_store_from_a_lane_beyond_n_reaches_the_guard(case):
    assert any(r % 32 for r in C.CASES[case]["rows"])        # (every case has a partial tile)
    _flagged(case, "store_no_valid", "written")
    assert _verdict(case, "store_no_valid")[1]["guard"] > 0


@pytest.mark.parametrize("case", [c for c in C.ORDER if max(C.CASES[c]["rows"]) > 32])
def test_tile_no_wave_owns_leaves_nan(case):
    _flagged(case, "tile_unowned", "written")
    rec = _verdict(case, "tile_unowned")[1]
    assert rec["unwritten"] > 0 and rec["guard"] == 0


# ---------------------------------------------------------------------------- scoring
def _emu_runner(defect):
    def run(name, mode, obs, rew, acts, c):
        return C.emu_score(obs, rew, acts, c, mode, defect)
    return run


def _sverdict(name, defect=None):
    if defect is None and name in _SHONEST:
        return _SHONEST[name]
    rec = C.score_measure(name, _emu_runner(defect))
    out = (C.score_checks(rec), rec)
    if defect is None:
        _SHONEST[name] = out
    return out


@pytest.mark.parametrize("case", C.SCORE_ORDER)
def test_honest_scoring_emulation_stays_inside_the_bounds(case):
    ok, rec = _sverdict(case)
    print("\n".join(rec["runs"]))
    assert all(ok.values()), ok


@pytest.mark.parametrize("case", C.SCORE_ORDER)
def test_numpys_own_fp64_evaluation_stays_inside_the_same_bounds(case):
    rec = C.score_measure(case, lambda name, mode, obs, rew, acts, c: C.numpy_score(obs, rew, acts, c, mode))
    print("\n".join(rec["runs"]))
    ok = C.score_checks(rec)
    assert ok["R"] and ok["S"] and ok["seq"] and ok["written"], ok


def test_the_edges_the_scoring_cases_are_here_for():
    s = C.SCORE_CASES
    assert [s[k]["K"] * s[k]["N"] for k in ("t1023", "t1024", "t1025")] == [1023, 1024, 1025]
    assert [s[k]["N"] for k in ("n255", "t1024", "n257")] == [255, 256, 257]
    assert [s[k]["H"] * s[k]["n"] for k in ("hn63", "hn64", "hn65")] == [63, 64, 65]
    p = s["maxw15"]["plant"]
    assert p >= 1024 and ((p % 1024) >> 6) == 15 and p < s["maxw15"]["K"] * s["maxw15"]["N"]
    assert s["maxT"]["plant"] == s["maxT"]["K"] * s["maxT"]["N"] - 1 and s["max0"]["plant"] == 0
    assert all("reference" in C.score_modes(k) for k in s)
    obs, rew, acts = C.score_inputs("kap800")
    R = C.score_ld(obs, rew, acts, s["kap800"], "none")[0]
    assert float(np.ptp(R)) > 5.0                        # scores spread over several units


def _sflagged(case, defect, keys):
    ok, rec = _sverdict(case, defect)
    print(case, defect, ok, rec["runs"])
    assert all(_sverdict(case)[0].values())
    for key in keys:
        assert ok[key] is False and not rec[key] < TEN, (case, defect, key, rec[key])


def test_sample_std_where_the_population_std_belongs():
    _sflagged("gamh", "sample_std", ["R"])


def test_gamma_to_the_t_plus_1():
    _sflagged("gamh", "gamma_t1", ["R"])


def test_index_modes_swapped():
    _sflagged("gamh", "idx_swapped", ["R"])


@pytest.mark.parametrize("case", ["maxT", "maxw15"])
def test_maximum_over_the_first_1024_scores_only(case):
    _sflagged(case, "max_1024", ["S"])


@pytest.mark.parametrize("case,keys", [("t1025", ["seq"]), ("n257", ["seq"]), ("hn65", ["R"])])
def test_strided_partial_sum_stopped_after_one_pass(case, keys):
    _sflagged(case, "one_pass", keys)


@pytest.mark.parametrize("case", ["gamh", "kap800"])
def test_1e_6_left_out_of_the_denominator(case):
    _sflagged(case, "no_1e6", ["seq"])


def test_members_weights_not_summed():
    _sflagged("gamh", "k0_only", ["seq"])


def test_zz_cpu_work_of_the_matrix_stays_under_30_s():
    """oracle, honest emulations and bounds of all cases (more than the GPU worker does on the CPU), timed afresh"""
    t = time.time()
    C._CASE.clear(); C._FREE.clear(); C._SIN.clear(); _PLAIN.clear(); _HONEST.clear(); _SHONEST.clear()
    for name in C.ORDER:
        _verdict(name)
    for name in C.SCORE_ORDER:
        _sverdict(name)
    print("%.1f s" % (time.time() - t))
    assert time.time() - t < 30.0
