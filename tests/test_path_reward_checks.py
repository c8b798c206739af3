"""The checks of tests/test_gpu_path_reward_matrix.py can fail, and pass what they should (CPU only).  tests/_path_reward_cases.py
emulates k_path_rewards' data movement in NumPy fp32 (the staged image, the host's grid, the tiles per wave, the lane's feature and
action-slot selection, the guarded store); a plain fp32 chain stands in for route 0.  The honest emulation passes every check the GPU
tests apply, with the same bars from the same fixture; each planted defect is flagged at the case named for it.  Also the
conditions that keep a comparison from being empty, from the fp64 oracle alone: the route, the spread of the rewards, and how far
the rewards move when the s' transform, the reward activation or a dynamics flag is taken wrong.

One planted defect cannot show in the outputs and is flagged by the walk alone: with `tile += gridDim.x` in place of
`4 gridDim.x` every tile is still computed (several times over, by several waves, to the same values), so the emulation reports the
tiles its waves really walked and the check compares them with the host's arithmetic.  On the device only the arithmetic is known."""
import ctypes
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _path_reward_cases as C  # noqa: E402

_PLAIN, _HONEST = {}, {}
FLOOR_SPREAD, FLOOR_MOVE = 0.05, 1e-3


def _runner(defect):
    def run(route, name, mem, obs, act):
        if route == 0:
            key = (name, obs.shape[1], act.ndim)
            if key not in _PLAIN:
                _PLAIN[key] = C.plain_fp32(name, mem, obs, act)
            return _PLAIN[key] + (0,)
        b32, b64, w = C.emulate(name, mem, obs, act, C.CUS, defect)
        run.walked[str(obs.shape[1])] = w
        return b32, b64, 1
    run.walked = {}
    return run


def _verdict(name, defect=None):
    if defect is None and name in _HONEST:
        return _HONEST[name]
    run = _runner(defect)
    rec = C.measure(name, run, C.CUS)
    out = (C.checks(name, rec, C.kref(name), run.walked), rec)
    if defect is None:
        _HONEST[name] = out
    return out


def test_fixture_holds_an_fp32_sized_yardstick_for_every_case():
    G = np.load(C.FIXTURE)
    assert sorted(G.files) == sorted("kref_" + c for c in C.CASES)
    for c in C.CASES:
        assert G["kref_" + c].dtype == np.float64 and 1e-8 < float(G["kref_" + c]) < 1e-6, c


@pytest.mark.parametrize("case", C.ORDER)
def test_case_is_served_by_the_instance_and_image_it_is_here_for(case):
    """mjx_path_rewards_route (arithmetic alone; the library loads without a device) answers 1, and the instance and the image are the
    ones the case table names"""
    from mjrl_amd import _lib
    lib = _lib.load()
    ints = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
    ds, rs = C.sizes(case)
    assert lib.mjx_path_rewards_route(ints(ds), len(ds), ints(rs), len(rs)) == 1
    assert C.instance(case) == C.CASES[case]["inst"]
    assert round(C.image_kib(case), 1) == C.CASES[case]["kib"] and C.image_kib(case) <= 160.0


def test_the_axes_the_cases_are_here_for():
    c, lay = C.CASES, {k: C.layout(k)[2] for k in C.CASES}
    assert [lay[k]["m8"] // 8 for k in ("a2", "a3", "a4", "a10")] == [3, 4, 4, 4]                    # action slot groups beyond the second
    assert (lay["a2"]["g1b"], lay["a2"]["g2b"]) == (4, 1) and (lay["a3"]["g1b"], lay["a3"]["g2b"]) == (1, 4)
    assert c["a5"]["n"] == lay["a5"]["n8"] and c["a5"]["m"] == lay["a5"]["m8"] and c["a5"]["rh"] == (128, 128)
    assert c["a6"]["rh"] == (1, 1) and (c["a6"]["n"], c["a6"]["m"]) == (1, 1)
    assert C.instance("a7")[2] == 2 and c["a7"]["rh"][1] == 1
    assert c["a8"]["n"] == 32 and c["a8"]["flags"] == 0 and c["a9"]["n"] == 33 and c["a9"]["m"] == 1
    assert (c["a10"]["n"], c["a10"]["m"]) == (64, 32) and c["a4"]["kib"] > 158
    assert sorted({c[k]["flags"] for k in C.AXIS}) == [0, 1, 3, 5, 7]
    assert all(c[k]["dact"] != c[k]["ract"] for k in ("a2", "a3", "a7"))
    assert all(C.masked_column(k) is not None for k in C.CASES if c[k]["flags"] & C.MASK)
    assert c["g3"]["K"] * c["g3"]["rows"][0] > 2 ** 20 and c["g2"]["K"] > C.CUS
    for k, want in C.WALK_AT_256.items():
        assert tuple(C.walk_numbers(C.walk(c[k]["rows"][0], c[k]["K"], 256))) == want, k


@pytest.mark.parametrize("case", C.ORDER)
def test_conditions_hold_from_the_oracle_alone(case):
    """rewards that spread (a dead unit would make every row equal), transforms whose s' columns matter, activations and flags
    that matter: per member, >= 1e-3 of the largest reward.  [the smallest spread is 0.158 of max |r| (one of g2's 300 members); a6's two members 0.45 at seed 7166; the
    smallest move 3.5e-3 (g2, the mask flag cleared)]  With n = 1 and the mask on (a6) the only output column is multiplied by 0, so
    no affine can move it: that one condition cannot hold there and is left out."""
    c = C.CASES[case]
    mem = C.cached_case(case)[0]
    ref = C.reference(case)
    what = ["sp_as_s"] + (["ract_dact"] if c["dact"] != c["ract"] else []) + [b for b in (C.AFF, C.MASK, C.RES) if c["flags"] & b]
    if c["n"] == 1 and c["flags"] & C.MASK:
        what.remove(C.AFF)       # a6: the only output column is the masked one, and no affine moves a column that is multiplied by 0
    for (rows, mode), r in ref.items():
        top = np.max(np.abs(r), axis=1)
        if rows >= 32:
            spread = np.ptp(r, axis=1) / top
            print(case, rows, mode, "spread %.3f" % spread.min())
            assert spread.min() >= FLOOR_SPREAD
            for w in what:
                moved = np.max(np.abs(C.oracle(case, C.variant(mem, w), rows, mode) - r), axis=1) / top
                print(case, rows, mode, w, "moves the rewards by %.2e" % moved.min())
                assert moved.min() >= FLOOR_MOVE, w


@pytest.mark.parametrize("case", C.ORDER)
def test_honest_emulation_passes_every_check(case):
    ok, rec = _verdict(case)
    print("\n".join(rec["runs"]), rec["routes"], rec["walk"])
    assert all(ok.values()), ok
    assert rec["err"]["1"] < 2.0 * C.kref(case)              # ... with room: the bar is 3 x


def _flagged(case, defect, check):
    ok, rec = _verdict(case, defect)
    print(case, defect, ok, rec["err"], rec["unwritten"], rec["guard"])
    assert _verdict(case)[0][check] is True
    assert ok[check] is False, (case, defect, ok)


@pytest.mark.parametrize("case", C.GEOM)
def test_loop_body_run_once_per_wave_leaves_rows_unwritten(case):
    _flagged(case, "once", "written")
    assert _verdict(case, "once")[1]["guard"] == 0


def test_stride_of_one_workgroup_shows_in_the_walk_alone():
    _flagged("g1", "stride1", "walk")
    ok = _verdict("g1", "stride1")[0]
    assert ok["mfma"] and ok["written"]                      # (every tile is still computed, several times over)


@pytest.mark.parametrize("case", C.ORDER)
def test_s_prime_under_the_s_columns(case):
    _flagged(case, "sp_under_s", "mfma")


@pytest.mark.parametrize("case", ["a2", "a3", "a7"])
def test_ract_taken_from_dact(case):
    _flagged(case, "ract_from_dact", "mfma")


@pytest.mark.parametrize("case", ["a2", "a3", "a4", "a10"])
def test_action_slot_groups_beyond_the_second_dropped(case):
    _flagged(case, "drop_q2", "mfma")


@pytest.mark.parametrize("case", C.ORDER)
def test_action_stride_of_the_other_mode(case):
    for mode, defect in (("own", "own_as_shared"), ("shared", "shared_as_own")):
        if mode in C.CASES[case]["modes"]:
            _flagged(case, defect, "mfma")


def test_v2_read_with_the_instance_stride():
    _flagged("a3", "v2_stride", "mfma")


@pytest.mark.parametrize("case", ["a2", "a3"])
def test_block_guards_replaced_by_the_instance_block_count(case):
    _flagged(case, "guards_rb", "mfma")


@pytest.mark.parametrize("case,defect", [("a4", "ignore_mask"), ("a5", "ignore_mask"), ("a1", "ignore_mask"), ("a4", "ignore_affine"),
                                         ("a5", "ignore_affine"), ("a1", "ignore_affine"), ("a4", "ignore_residual"), ("a1", "ignore_residual"),
                                         ("a8", "flags_on")])
def test_mask_affine_and_residual_each_ignored_or_forced(case, defect):
    _flagged(case, defect, "mfma")


@pytest.mark.parametrize("case", C.AXIS + ["g1"])
def test_store_without_valid_reaches_the_guard(case):
    _flagged(case, "store_no_valid", "written")
    assert _verdict(case, "store_no_valid")[1]["guard"] > 0


def test_zz_cpu_work_of_the_matrix_stays_under_30_s():
    """oracle, honest emulation and yardstick subset of all cases (what the GPU worker does on the CPU), timed afresh"""
    t = time.time()
    C._CASE.clear(); C._REF.clear(); _PLAIN.clear(); _HONEST.clear()
    for name in C.ORDER:
        _verdict(name)
    print("%.1f s" % (time.time() - t))
    assert time.time() - t < 30.0
