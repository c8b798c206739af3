"""The wide plan rollout without a GPU: mjx_plan_rollout_wide_route's table, the documented LDS layout, mjx_plan_rollout_wide's routes
at N = 0 / H = 0 and its argument errors (the library builds here and these paths need no device), the calls MPCPolicy makes (the
recorder of tests/test_model_accel_calls_cpu.py in the library's place), the conditions on the fixture (tests/golden/plan_wide.npz,
tests/golden/make_golden_plan_wide.py), and the GPU checks themselves on an fp32 NumPy emulation of the kernel's data movement: it
passes every check the GPU worker runs, and each of four planted defects is flagged by them (tests/test_plan_checks.py's method)."""
import ctypes
import os
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _plan_wide_cases as C  # noqa: E402
from tests._worker_dev import ints as _ints  # noqa: E402
from tests.test_model_accel_calls_cpu import Recorder, stubbed  # noqa: E402

G = np.load(C.FIXTURE)


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from mjrl_amd import _lib
    return _lib.load()


def test_wide_route_table():
    lib = _lib()

    def route(ds, m=None):
        return lib.mjx_plan_rollout_wide_route(_ints(ds), len(ds), ds[0] - ds[-1] if m is None else m)

    for name in C.ORDER:
        assert route(C.sizes(name)) == 1 == C.served(C.sizes(name)), name
    assert route([13, 256, 256, 11]) == 1
    assert route([23, 1, 1, 17]) == 1
    # not served
    assert route([13, 257, 256, 11]) == 0 and route([13, 256, 257, 11]) == 0
    assert route([13, 256, 11]) == 0                                      # one hidden layer
    assert route([13, 256, 256, 256, 11]) == 0                            # three
    assert route([67, 256, 256, 65]) == 0                                 # n = 65
    assert route([76, 256, 256, 11]) == 0                                 # m = 65
    assert route([128, 256, 256, 64]) == 1 and route([127, 256, 256, 64]) == 1      # n + m = 128 ...
    assert route([129, 256, 256, 65]) == 0 and route([129, 256, 256, 64]) == 0      # ... and 129 (n = 65; m = 65)
    for ds in ([13, 257, 256, 11], [13, 256, 11], [67, 256, 256, 65], [76, 256, 256, 11], [129, 256, 256, 64]):
        assert C.served(ds) == 0
    # bad sizes
    assert route([13, 256, 0, 11]) < 0
    assert route([11, 256, 256, 11]) < 0                                  # no action
    assert route([13, 256, 256, 11], m=3) < 0                             # act_dim does not fit
    assert route([13, 256, 256, 11], m=0) < 0
    assert route([13]) < 0
    # ... and mjx_plan_route's answers are what they were
    assert lib.mjx_plan_route(_ints([13, 256, 256, 11]), 4, 2) == 0
    assert lib.mjx_plan_route(_ints([23, 256, 256, 17]), 4, 6) == 0
    assert lib.mjx_plan_route(_ints(C.sizes("q7")), 4, 6) == 1
    for name in C.ORDER:
        ds = C.sizes(name)
        assert lib.mjx_plan_route(_ints(ds), 4, C.CASES[name]["m"]) == C.NARROW_ROUTE[name], name


def test_documented_layout():
    """include/mjx.h: n + pad8(n + m) + pad32(h1) + pad32(h2) + pad32(n) rows of 36 floats, then h1 + h2 + 5 n + 2 m floats; at most
    114 432 bytes"""
    with open(os.path.join(ROOT, "include", "mjx.h")) as f:
        text = f.read()
    assert "pad32(h1) + pad32(h2) + pad32(n) rows of 36 floats (S, XD, H1, H2, Z3), then h1 + h2 + 5 n + 2 m floats" in text
    assert "at most 114 432 bytes" in text
    assert 4 * C.lds_floats(64, 64, 256, 256) == 114432 <= C.LDS_MAX
    assert C.lds_floats(64, 64, 256, 256) == 36 * 768 + 960
    assert C.lds_floats(11, 2, 256, 256) == 36 * (11 + 16 + 256 + 256 + 32) + 571
    assert C.lds_floats(1, 1, 129, 1) == 36 * (1 + 8 + 160 + 32 + 32) + 137


def test_wide_entry_routes_and_argument_errors_touch_nothing():
    """bad arguments return MJX_ERR_ARG before any device work (this test has no device); N == 0 or H == 0 returns MJX_OK and the
    route: 2 on a served shape, mjx_plan_route's answer under MJX_PLAN_WIDE=0, 0 under MJX_PLAN_MFMA=0"""
    lib = _lib()
    buf = (ctypes.c_float * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ds = [8, 256, 256, 6]
    route = ctypes.c_int(-7)

    def call(s0=p, s0s=0, N=5, H=3, K=2, acts=p, ds=ds, dP=p, dtr=p, act=0, flags=7, obs=p):
        return lib.mjx_plan_rollout_wide(s0, s0s, N, H, K, acts, _ints(ds), len(ds), dP, dtr, act, flags, obs, ctypes.byref(route), None)

    for bad in (dict(s0=None), dict(acts=None), dict(dP=None), dict(dtr=None), dict(obs=None), dict(s0s=5), dict(N=-1), dict(H=-1),
                dict(K=0), dict(K=65536), dict(act=2), dict(flags=8), dict(flags=-1), dict(ds=[8, 256, 0, 6]), dict(ds=[6, 256, 256, 6]),
                dict(ds=[8])):
        assert call(**bad) == -1, bad
        assert route.value == -7 and not any(buf), bad
    assert call(N=0) == 0 and route.value == 2
    assert call(N=0, s0s=6) == 0 and route.value == 2
    assert call(H=0) == 0 and route.value == 2
    assert call(N=0, ds=[8, 64, 64, 6]) == 0 and route.value == 2         # served when called directly
    assert call(N=0, ds=[8, 257, 256, 6]) == 0 and route.value == 0       # not served by either kernel
    assert call(N=0, ds=[8, 64, 64, 64, 6]) == 0 and route.value == 0
    for switch, chained in (("MJX_PLAN_WIDE", 1), ("MJX_PLAN_MFMA", 0)):
        os.environ[switch] = "0"
        try:                                                              # the switches are read per call
            assert call(N=0) == 0 and route.value == 0
            assert call(H=0) == 0 and route.value == 0
            assert lib.mjx_plan_route(_ints([8, 64, 64, 6]), 4, 2) == 1
            assert call(N=0, ds=[8, 64, 64, 6]) == 0 and route.value == chained
        finally:
            os.environ.pop(switch)
        assert call(N=0) == 0 and route.value == 2
    # a null route_out is allowed; the narrow entry is what it was (unknown flag bits are not its business)
    assert lib.mjx_plan_rollout_wide(p, 0, 0, 3, 2, p, _ints(ds), 4, p, p, 0, 7, p, None, None) == 0
    assert lib.mjx_plan_rollout(p, 0, 0, 3, 2, p, _ints(ds), 4, p, p, 0, 8, p, None) == 0
    assert lib.mjx_plan_rollout(None, 0, 0, 3, 2, p, _ints(ds), 4, p, p, 0, 7, p, None) == -1
    assert not any(buf)


# ---- the calls MPCPolicy makes, recorded
def _planner_calls(hidden, reward, force_narrow=False, wide=True):
    from mjrl_amd.algos.model_accel import model_learning_mpc as P
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    n, m, N, H = 6, 2, 5, 3
    models = [D.WorldModel(n, m, hidden_size=hidden, seed=k, learn_reward=True) for k in range(2)]

    class Inner:
        def compute_path_rewards(self, paths):
            paths["rewards"] = -paths["observations"][..., 0].astype(np.float64)

    env = types.SimpleNamespace(observation_dim=n, action_dim=m, env=types.SimpleNamespace(env=Inner()))
    rec = Recorder()
    narrow = lambda *a: False
    with stubbed(rec), mock.patch.object(P, "wide_rows_shape", narrow if force_narrow else P.wide_rows_shape), \
            mock.patch.object(D, "wide_rows_shape", narrow if force_narrow else D.wide_rows_shape):
        pol = P.MPCPolicy(env=env, plan_horizon=H, plan_paths=N, fitted_model=models, reward=reward, wide=wide)
        np.random.seed(3)
        pol.get_action(np.arange(n) / 8.0)
        last = pol.last_routes()
    return rec.calls, last


@pytest.mark.parametrize("reward", ["learned", "env"])
def test_mpc_policy_calls_the_wide_entries_for_wide_members_only(reward):
    today = ["mjx_cast_f64_f32", "mjx_plan_rollout"] + (["mjx_path_rewards"] if reward == "learned" else []) + ["mjx_plan_score"]
    wide = [{"mjx_plan_rollout": "mjx_plan_rollout_wide", "mjx_path_rewards": "mjx_path_rewards_wide"}.get(e, e) for e in today]
    calls, last = _planner_calls((256, 256), reward)
    assert [c[0] for c in calls] == wide
    assert last == dict(rollout=1, rewards=1 if reward == "learned" else None)       # (the recorder's routes, handed through)
    narrow_calls, narrow_last = _planner_calls((256, 256), reward, force_narrow=True)
    assert [c[0] for c in narrow_calls] == today
    assert narrow_last == dict(rollout=None, rewards=1 if reward == "learned" else None)
    # the wide rollout receives mjx_plan_rollout's arguments in order, then route_out, then the stream
    w, nrw = calls[1], narrow_calls[1]
    assert len(w) == len(nrw) + 1 and w[1:14] == nrw[1:14] and w[14] == "byref" and w[15] is None and nrw[14] is None
    assert w[7] == [8, 256, 256, 6] and w[2:6] == [0, 5, 3, 2]
    if reward == "learned":
        assert calls[2][2:] == narrow_calls[2][2:]                        # (all but obs, which the recorder moves for entries it knows)
    for hidden in ((32, 32), (128, 128), (64, 128)):
        assert [c[0] for c in _planner_calls(hidden, reward)[0]] == today, hidden
    assert [c[0] for c in _planner_calls((129, 64), reward)[0]] == wide
    # a planner built without the keyword makes today's calls on every shape, with today's arguments
    plain_calls, plain_last = _planner_calls((256, 256), reward, wide=False)
    assert plain_calls == narrow_calls and plain_last == narrow_last


def test_route_answers_with_and_without_the_keyword():
    """route() / reward_route() answer 2 for wide members of a planner built with wide=True, under the switches as they stand; a
    planner built as before answers what it did (0 at 256 wide), and narrower members keep their answers either way"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    _lib()
    env = types.SimpleNamespace(observation_dim=6, action_dim=2, env=types.SimpleNamespace(env=None))

    def planner(hidden, **kw):
        models = [WorldModel(6, 2, hidden_size=hidden, seed=k, learn_reward=True) for k in range(2)]
        return MPCPolicy(env=env, plan_horizon=3, plan_paths=5, fitted_model=models, reward='learned', **kw)

    pol = planner((256, 256), wide=True)
    assert (pol.route(), pol.reward_route()) == (2, 2) and pol.last_routes() is None
    for switches, want in ((("MJX_PLAN_WIDE",), (0, 2)), (("MJX_PATH_REWARDS_WIDE",), (2, 0)), (("MJX_PLAN_MFMA", "MJX_PATH_REWARDS_MFMA"), (0, 0))):
        for name in switches:
            os.environ[name] = "0"
        try:
            assert (pol.route(), pol.reward_route()) == want, switches
        finally:
            for name in switches:
                os.environ.pop(name)
    assert (planner((256, 256)).route(), planner((256, 256)).reward_route()) == (0, 0)
    for kw in (dict(), dict(wide=True)):
        assert (planner((64, 64), **kw).route(), planner((64, 64), **kw).reward_route()) == (1, 1)
    assert planner((300, 300), wide=True).route() == 0                    # wide, but not served


def test_fixture_has_every_key_and_fp32_sized_yardsticks():
    """float64 scalars only; the reference's own fp32 steps lie a few roundings from fp64 on every case"""
    want = {"pstep_" + name for name in C.STEPPED} | {"pfree_f1", "mpc_R", "mpc_seq", "mpc_R_env", "mpc_seq_env"}
    assert set(G.files) == want
    assert "q8" not in C.STEPPED and C.CASES["q8"]["H"] == 1 and len(C.STEPPED) == 8
    for key in sorted(G.files):
        assert G[key].dtype == np.float64 and G[key].shape == ()
        print(key, float(G[key]))
        assert 1e-9 < float(G[key]) < (1e-5 if key == "pfree_f1" else 2e-6), key


# ---- the GPU checks on the emulation
def _emulated(defect=None):
    def runner(rt, name, mem, s0, actions):
        if rt == "0":
            return C.plain_fp32(name, mem, s0, actions)
        return C.emulate(name, mem, s0, actions, defect)
    return runner


@pytest.mark.parametrize("name", C.ORDER)
def test_emulation_passes_every_check(name):
    rec = C.measure(name, _emulated())
    for line in rec["runs"]:
        print(line)
    ok = C.checks(name, rec, C.yard(name) if C.CASES[name]["H"] > 1 else None)
    assert all(ok.values()), ok
    assert rec["calls"] == 2 * len(C.CASES[name]["s0"])
    if C.CASES[name]["H"] > 1:
        assert not rec["same_bits"]                                       # two summation orders never agree to the bit


# defect -> (a case that shows it, the checks that must flag it)
PLANTED = {
    "actions_ahead": ("q1", ("wide", "routes")),
    "member0_tr": ("q3", ("wide", "routes")),
    "residual_overwritten": ("q6", ("wide", "routes")),
    "store_no_valid": ("q1", ("written",)),
}


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_planted_defect_is_flagged(defect):
    name, flagged = PLANTED[defect]
    rec = C.measure(name, _emulated(defect))
    ok = C.checks(name, rec, C.yard(name))
    print(defect, name, ok, rec["err"], rec["routes"], rec["unwritten"], rec["guard"])
    for check in flagged:
        assert ok[check] is False or ok[check] == False, (defect, check)      # noqa: E712
    assert ok["generic"]                                                  # (the stand-in for route 0 carries no defect)
