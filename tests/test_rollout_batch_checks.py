"""CPU checks of the device-resident model rollouts (csrc/rollout_batch.h; tests/_rollout_batch_cases.py): the route function against
mjx_plan_route and the restated arithmetic, the NumPy emulation of mjx_rollout_pack against the reference's loop restated
(model_accel_npg.py:137-155), the truncation limits the cases fix from the fp64 oracle, and the public surface the resident route adds.
No GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import _plan_cases as C  # noqa: E402
import _rollout_batch_cases as B  # noqa: E402
from tests._worker_dev import ints as _ints  # noqa: E402


def _lib():
    from mjrl_amd._lib import load
    return load()


@pytest.mark.parametrize("name", C.ORDER)
def test_route_agrees_with_plan_route_on_the_plan_cases(name):
    lib, ds = _lib(), C.sizes(name)
    got = lib.mjx_rollout_disagreement_route(_ints(ds), len(ds))
    assert got == lib.mjx_plan_route(_ints(ds), len(ds), C.CASES[name]["m"]) == B.route(ds) == 1


@pytest.mark.parametrize("ds", B.UNSERVED)
def test_route_is_generic_on_unserved_shapes(ds):
    lib = _lib()
    assert lib.mjx_rollout_disagreement_route(_ints(ds), len(ds)) == lib.mjx_plan_route(_ints(ds), len(ds), ds[0] - ds[-1]) == B.route(ds) == 0


@pytest.mark.parametrize("ds", B.BAD)
def test_route_refuses_bad_sizes(ds):
    assert _lib().mjx_rollout_disagreement_route(_ints(ds), len(ds)) < 0 and B.route(ds) < 0


def test_entries_refuse_bad_arguments_without_a_device():
    """MJX_ERR_ARG (-1) before any device work: null blocks, a negative count, both or neither reward block"""
    lib = _lib()
    ds = (8, 32, 32, 6)
    one = ctypes.c_void_p(8)
    assert lib.mjx_rollout_disagreement(None, one, 1, 2, 1, _ints(ds), 4, one, one, 0, 7, one, None, None) == -1
    assert lib.mjx_rollout_disagreement(one, one, -1, 2, 1, _ints(ds), 4, one, one, 0, 7, one, None, None) == -1
    assert lib.mjx_rollout_disagreement(one, one, 1, 2, 1, _ints(ds), 4, one, one, 2, 7, one, None, None) == -1
    args = lambda r32, r64, P=1: (one, one, r32, r64, None, P, 2, 6, 2, 0.5, 4, 0.0, one, one, one, one, one, one, None, None, None)  # noqa: E731
    assert lib.mjx_rollout_pack(*args(one, one)) == -1
    assert lib.mjx_rollout_pack(*args(None, None)) == -1
    assert lib.mjx_rollout_pack(*args(one, None, P=-1)) == -1
    route = ctypes.c_int(-5)                                    # P = 0 and H = 1: MJX_OK without a launch, the route reported
    assert lib.mjx_rollout_disagreement(one, one, 0, 6, 2, _ints(ds), 4, one, one, 0, 7, one, ctypes.byref(route), None) == 0 and route.value == 1
    assert lib.mjx_rollout_disagreement(one, one, 3, 1, 2, _ints(ds), 4, one, one, 0, 7, one, ctypes.byref(route), None) == 0 and route.value == 1


@pytest.mark.parametrize("name", sorted(B.PACK_CASES))
def test_pack_emulation_equals_the_reference_loop(name):
    """every packed array and the lengths.  `terminated` is compared where H >= 4: below, the reference's max(4, T) exceeds the path
    and its flag says "terminated" for a path it kept whole -- paths it never sees, since its length filter drops H < 5"""
    c = B.pack_case(name)
    P, H, _ = c["obs"].shape
    err = c["err"] if c["err"] is not None else np.zeros((P, H - 1), np.float32)
    emu = B.emu_pack(c["obs"], c["act"], c["rew"], c["err"], c["lim"], c["min_len"], c["truncate_reward"])
    ref = B.reference_loop(c["obs"], c["act"], c["rew"], err, c["lim"], c["truncate_reward"])
    off = emu["off"]
    assert [len(p["rewards"]) for p in ref] == list(np.diff(off))
    for key, mine in (("observations", emu["obs"]), ("actions", emu["act"])):
        np.testing.assert_array_equal(np.concatenate([p[key] for p in ref]), mine)
    got = np.concatenate([p["rewards"] for p in ref])
    assert got.dtype == c["rew"].dtype
    np.testing.assert_array_equal(got.astype(np.float64), emu["rew"])
    if H >= 4:
        assert [int(p["terminated"]) for p in ref] == list(emu["term"])
    np.testing.assert_array_equal(emu["tpos"], np.concatenate([np.arange(t) for t in np.diff(off)]))
    assert emu["rows"] == off[-1] <= P * H


def test_pack_cases_cover_what_they_claim():
    v = {name: B.emu_pack(**{k: c[k] for k in ("obs", "act", "rew", "err", "lim", "min_len", "truncate_reward")})
         for name, c in ((n, B.pack_case(n)) for n in B.PACK_CASES)}
    assert set(v["p257"]["first"]) == {-1, 0, 1, 2, 6} and np.all(v["all"]["first"] >= 0) and np.all(v["none"]["first"] < 0)
    assert np.all(v["null"]["first"] < 0) and v["null"]["rows"] == 33 * 6
    c = B.pack_case("p257")
    assert np.isnan(c["err"]).any() and (c["err"] == np.float32(B.PACK_LIM)).any()
    assert v["h2"]["rows"] == 9 * 2 and not v["h2"]["term"].any() and v["h3"]["rows"] == 9 * 3
    assert v["p20000"]["rows"] > 2 ** 16


@pytest.mark.parametrize("case", B.limited(), ids=B.dis_id)
def test_disagreement_cases_fix_a_limit_by_the_rule(case):
    mem, obs, act = B.dis_data(case)
    err = B.oracle_err(mem, obs, act)
    lim = B.fix_lim(err)                                   # (asserts the rule's conditions)
    v = B.first_violation(err, lim)
    P, H = err.shape[0], err.shape[1] + 1
    assert P / 4 <= np.sum(v >= 0) <= 3 * P / 4 and (v == H - 2).any() and (v < 0).any() and ((v >= 0) & (v < 3)).any()
    e = np.sort(err.ravel())
    i = np.searchsorted(e, lim)
    assert e[i] / e[i - 1] >= 1.05 and abs(lim - np.sqrt(e[i] * e[i - 1])) <= 1e-12 * lim


def test_the_limited_cases_are_those_with_31_paths_or_more():
    assert len(B.limited()) == 80 and {c[2] for c in B.limited()} == {2, 5, 6} and all(c[1] < 5 for c in B.dis_cases() if c not in B.limited())


def test_every_net_meets_every_member_count_and_shape():
    cases = B.dis_cases()
    assert len(cases) == len(B.NETS) * len(B.SHAPES)
    for net in B.NETS:
        assert {c[3] for c in cases if c[0] == net} == set(B.KS)
    assert {C.instance(n) for n in B.NETS} == {(a, b) for a in (1, 2, 3, 4) for b in (1, 2)}
    assert {C.CASES[n]["flags"] for n in B.NETS} == {0, 1, 3, 5, 7}


def test_yardsticks_are_recorded_for_every_case():
    G = np.load(B.FIXTURE)
    for case in B.dis_cases():
        assert 0 <= float(G["d_" + B.dis_id(case)]) < 1e-4
    assert 0 < float(G["e2e_roll"]) < 1e-4


def test_end_to_end_case_fixes_its_limit():
    o = B.e2e_oracle()
    v = B.first_violation(o["err"], o["lim"])
    assert 30 <= np.sum(v >= 0) <= 90 and (v == B.E2E["H"] - 2).any() and ((v >= 0) & (v < 3)).any()


def test_resident_is_opt_in():
    from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG
    from mjrl_amd.utils import ingest
    assert inspect.signature(ModelAccelNPG.__init__).parameters["resident"].default is False
    assert inspect.signature(ModelAccelNPG.train_step).parameters["resident"].default is None
    assert callable(ModelAccelNPG.train_step_info) and callable(ingest.register_device_batch)
