"""The wide policy rollout's host side without a GPU: mjx_policy_rollout_wide_route's table, mjx_policy_rollout_wide's routes at N = 0
and its argument errors (the library builds here and these paths need no device), sampling.wide_rollout_shape and the call
rollout_models_device makes (a recorder in the library's place, as tests/test_model_accel_calls_cpu.py has one), and the conditions
on the fixture (tests/golden/rollout_wide.npz, tests/golden/make_golden_rollout_wide.py)."""
import contextlib
import ctypes
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refine_oracle as F  # noqa: E402
import _rollout_wide_cases as W  # noqa: E402
from tests._worker_dev import ints as _ints  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "rollout_wide.npz"))
LDS_MAX = 160 * 1024


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from mjrl_amd import _lib
    return _lib.load()


def _pad(d, to):
    return (d + to - 1) // to * to


def _wide_floats(n, m, h1, h2, p1, p2):
    """the documented layout (include/mjx.h): rows of 36 floats, then the biases and transforms"""
    rows = n + _pad(n + m, 8) + max(_pad(h1, 32) + _pad(h2, 32) + _pad(n, 32), _pad(n, 8) + _pad(p1, 32) + _pad(p2, 32) + _pad(m, 32))
    return 36 * rows + p1 + p2 + h1 + h2 + 7 * n + 6 * m


def test_wide_route_table():
    lib = _lib()

    def route(pol, dyn):
        return lib.mjx_policy_rollout_wide_route(_ints(pol), len(pol), _ints(dyn), len(dyn))

    assert route([11, 64, 64, 2], [13, 256, 256, 11]) == 1
    for name, (n, m, dh, ph, *_rest) in W.WCASES.items():
        assert route([n] + list(ph) + [m], [n + m] + list(dh) + [n]) == 1, name
    assert route([11, 256, 256, 2], [13, 256, 256, 11]) == 1
    assert route([17, 64, 64, 6], [23, 64, 64, 17]) == 1                 # the chained route serves it too ...
    assert lib.mjx_policy_rollout_route(_ints([17, 64, 64, 6]), 4, _ints([23, 64, 64, 17]), 4) == 1
    assert route([17, 1, 1, 6], [23, 1, 1, 17]) == 1
    # not served
    assert route([11, 64, 64, 2], [13, 257, 256, 11]) == 0
    assert route([11, 64, 64, 2], [13, 256, 257, 11]) == 0
    assert route([11, 257, 64, 2], [13, 256, 256, 11]) == 0
    assert route([11, 64, 257, 2], [13, 256, 256, 11]) == 0
    assert route([11, 64, 2], [13, 256, 256, 11]) == 0                   # one hidden layer
    assert route([11, 64, 64, 64, 2], [13, 256, 256, 11]) == 0           # three
    assert route([11, 64, 64, 2], [13, 256, 11]) == 0
    assert route([11, 64, 64, 2], [13, 256, 256, 256, 11]) == 0
    assert route([65, 64, 64, 2], [67, 256, 256, 65]) == 0               # n = 65
    assert route([11, 64, 64, 65], [76, 256, 256, 11]) == 0              # m = 65
    assert route([64, 64, 64, 64], [128, 256, 256, 64]) == 1             # n + m = 128 ...
    assert route([64, 64, 64, 63], [127, 256, 256, 64]) == 1
    assert route([65, 64, 64, 64], [129, 256, 256, 65]) == 0             # ... and 129
    # the largest layout there is fits by arithmetic
    assert 4 * _wide_floats(64, 64, 256, 256, 256, 256) == 127232 <= LDS_MAX
    # bad sizes
    assert route([11, 0, 64, 2], [13, 256, 256, 11]) < 0
    assert route([11, 64, 64, 2], [13, 256, 0, 11]) < 0
    assert route([10, 64, 64, 2], [13, 256, 256, 11]) < 0                # a policy that does not fit the dynamics net
    assert route([11, 64, 64, 3], [13, 256, 256, 11]) < 0
    assert route([11, 64, 64, 2], [11, 256, 256, 11]) < 0                # no action
    assert route([11], [13, 256, 256, 11]) < 0
    # ... and mjx_policy_rollout_route's answer for the 256-wide pair is what it was
    assert lib.mjx_policy_rollout_route(_ints([11, 64, 64, 2]), 4, _ints([13, 256, 256, 11]), 4) == 0
    assert lib.mjx_policy_rollout_route(_ints([17, 64, 64, 6]), 4, _ints([23, 256, 256, 17]), 4) == 0


def test_wide_entry_routes_and_argument_errors_touch_nothing():
    """bad arguments return MJX_ERR_ARG before any device work (this test has no device); N == 0 or H == 0 returns MJX_OK and the
    route: 2 on a served shape, mjx_policy_rollout_route's answer under MJX_POLICY_ROLLOUT_WIDE=0, 0 under MJX_POLICY_ROLLOUT_MFMA=0"""
    lib = _lib()
    buf = (ctypes.c_float * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ps, ds = [6, 32, 32, 2], [8, 256, 256, 6]
    route = ctypes.c_int(-7)

    def call(s0=p, s0s=0, N=5, H=3, K=2, ps=ps, pP=p, ptr=p, nz=p, nzs=0, ds=ds, dP=p, dtr=p, act=0, flags=7, alo=p, ahi=p, slo=p, shi=p,
             obs=p, ao=p):
        return lib.mjx_policy_rollout_wide(s0, s0s, N, H, K, _ints(ps), len(ps), pP, ptr, nz, nzs, _ints(ds), len(ds), dP, dtr, act, flags,
                                           alo, ahi, slo, shi, obs, ao, ctypes.byref(route), None)

    for bad in (dict(s0=None), dict(pP=None), dict(ptr=None), dict(dP=None), dict(dtr=None), dict(obs=None), dict(ao=None),
                dict(s0s=5), dict(nzs=7), dict(nzs=5 * 3 * 2 + 1), dict(alo=None), dict(ahi=None), dict(slo=None), dict(shi=None),
                dict(N=-1), dict(H=-1), dict(K=0), dict(act=2), dict(flags=8), dict(ps=[5, 32, 32, 2]), dict(ps=[6, 32, 32, 3]),
                dict(ds=[8, 256, 0, 6]), dict(ps=[6, 0, 32, 2])):
        assert call(**bad) == -1, bad
        assert route.value == -7 and not any(buf), bad
    assert call(N=0) == 0 and route.value == 2
    assert call(N=0, s0s=6, nzs=0, nz=None, alo=None, ahi=None, slo=None, shi=None) == 0 and route.value == 2
    assert call(H=0, nzs=0) == 0 and route.value == 2
    assert call(N=0, ds=[8, 64, 64, 6]) == 0 and route.value == 2        # served when called directly
    assert call(N=0, ds=[8, 257, 256, 6]) == 0 and route.value == 0      # not served by either kernel
    assert call(N=0, ps=[6, 32, 2], ds=[8, 64, 64, 6]) == 0 and route.value == 0
    for switch, chained in (("MJX_POLICY_ROLLOUT_WIDE", 1), ("MJX_POLICY_ROLLOUT_MFMA", 0)):
        os.environ[switch] = "0"
        try:                                                             # the switches are read per call
            assert call(N=0) == 0 and route.value == 0
            assert lib.mjx_policy_rollout_route(_ints(ps), 4, _ints([8, 64, 64, 6]), 4) == 1
            assert call(N=0, ds=[8, 64, 64, 6]) == 0 and route.value == chained
        finally:
            os.environ.pop(switch)
        assert call(N=0) == 0 and route.value == 2
    assert not any(buf)


def test_wide_rollout_shape_table():
    from mjrl_amd.algos.model_accel.sampling import wide_rollout_shape as wide
    assert wide((11, 64, 64, 2), (13, 256, 256, 11))
    assert wide((11, 64, 64, 2), (13, 129, 64, 11)) and wide((11, 64, 64, 2), (13, 64, 129, 11))
    assert wide((11, 65, 64, 2), (13, 64, 64, 11)) and wide((11, 64, 65, 2), (13, 64, 64, 11))
    assert wide((11, 128, 128, 2), (13, 64, 64, 11))
    assert wide([11, 64, 64, 2], [13, 300, 300, 11])                     # (the entry decides what is served; this is the dispatch only)
    assert not wide((11, 64, 64, 2), (13, 128, 128, 11))
    assert not wide((11, 64, 64, 2), (13, 64, 64, 11))
    assert not wide((6, 16, 16, 2), (8, 16, 48, 6))                      # small ragged shapes keep their call
    assert not wide((11, 64, 2), (13, 256, 256, 11)) and not wide((11, 64, 64, 64, 2), (13, 256, 256, 11))
    assert not wide((11, 64, 64, 2), (13, 256, 11)) and not wide((11, 64, 64, 2), (13, 256, 256, 256, 11))
    for name, (n, m, dh, ph, *_rest) in W.WCASES.items():
        assert wide((n,) + ph + (m,), (n + m,) + dh + (n,)), name


# ---- the call rollout_models_device makes, recorded
class _Ptr:
    def __init__(self, t):
        self.t = t


class _Recorder:
    """logs (entry name, arguments) of every mjx_* call; every route comes back as 1"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("mjx_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            for a in args:
                if hasattr(a, "_obj") and not isinstance(a, _Ptr):
                    a._obj.value = 1
            return 0
        return entry


@contextlib.contextmanager
def _stubbed(rec):
    import importlib
    with contextlib.ExitStack() as stack:
        for name in ("nn_dynamics", "sampling", "model_accel_npg"):
            mod = importlib.import_module("mjrl_amd.algos.model_accel." + name)
            for attr, val in (("_device", lambda: torch.device("cpu")), ("_stream", lambda dev: None), ("load", lambda: rec),
                              ("ptr", lambda t: None if t is None else _Ptr(t))):
                if hasattr(mod, attr):
                    stack.enter_context(mock.patch.object(mod, attr, val))
        yield


def _plain(a):
    if isinstance(a, _Ptr):
        return ("tensor", str(a.t.dtype), tuple(a.t.shape), a.t.detach().cpu().numpy().tobytes())
    if isinstance(a, ctypes.Array):
        return [int(v) for v in a]
    if hasattr(a, "_obj"):
        return "byref"
    return a


def _device_call(hidden, force_narrow):
    """rollout_models_device on two members of the given width -> (entry name, plain arguments, info)"""
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    from mjrl_amd.algos.model_accel import sampling as S
    from mjrl_amd.policies.gaussian_mlp import MLP
    n, m, N, H = 6, 2, 5, 3
    models = [D.WorldModel(n, m, hidden_size=hidden, seed=k) for k in range(2)]
    pol = MLP(types.SimpleNamespace(observation_dim=n, action_dim=m, horizon=10), hidden_sizes=(32, 32), seed=2)
    rng = np.random.RandomState(5)
    s0, noise = rng.randn(N, n).astype(np.float32), torch.from_numpy(rng.randn(H, N, m).astype(np.float32))
    rec, info = _Recorder(), {}
    with _stubbed(rec), mock.patch.object(S, "wide_rollout_shape", (lambda p, d: False) if force_narrow else S.wide_rollout_shape):
        S.rollout_models_device(models, pol, s0, H, noise, a_min=-1.0, a_max=1.0, info=info)
    assert len(rec.calls) == 1, [c[0] for c in rec.calls]
    name, args = rec.calls[0]
    plain = [_plain(a) for a in args]
    for i in (21, 22):                                                    # the output blocks are torch.empty: dtype and shape only
        plain[i] = plain[i][:3]
    return name, plain, info


def test_rollout_models_device_calls_the_wide_entry_for_wide_nets_only():
    name, args, info = _device_call((256, 256), False)
    assert name == "mjx_policy_rollout_wide" and info["route"] == 1       # (the recorder's route, handed through)
    narrow_name, narrow_args, _ = _device_call((256, 256), True)
    assert narrow_name == "mjx_policy_rollout"
    assert len(args) == len(narrow_args) == 25 and args == narrow_args    # the argument list mjx_policy_rollout would have received
    assert args[5] == [6, 32, 32, 2] and args[11] == [8, 256, 256, 6] and args[1:5] == [6, 5, 3, 2]
    assert _device_call((32, 32), False)[0] == "mjx_policy_rollout"


def test_refine_route_asks_the_wide_route_function_for_wide_shapes():
    from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    _lib()
    spec = types.SimpleNamespace(observation_dim=6, action_dim=2, horizon=10)

    def agent(dh, ph):
        models = [WorldModel(6, 2, hidden_size=dh, seed=k) for k in range(2)]
        return ModelAccelNPG(learned_model=models, env=None, policy=MLP(spec, hidden_sizes=ph, seed=3), baseline=LinearBaseline(spec),
                             normalized_step_size=0.05, seed=1, refine=True, reward_function=lambda p: p)

    assert agent((256, 256), (32, 32)).refine_route() == 2
    assert agent((64, 64), (128, 128)).refine_route() == 2
    assert agent((64, 64), (32, 32)).refine_route() == 1
    assert agent((300, 300), (32, 32)).refine_route() == 0                # wide, but not served


def test_fixture_has_every_key_and_fp32_sized_yardsticks():
    """the reference's own fp32 steps lie a few roundings from fp64 on every case (the H = 1 case stores s0 only: 0), and the tight
    bounds clamp at least a tenth of the fp64 rollout's actions and states (stored shares, and recomputed)"""
    want = {"kfree_act", "kfree_obs"} | {"share_" + name for name in W.TIGHT}
    for name in W.WCASES:
        want |= {"kya_" + name, "kys_" + name}
    assert set(G.files) == want
    for name in sorted(W.WCASES):
        ya, ys = float(G["kya_" + name]), float(G["kys_" + name])
        print(name, ya, ys)
        assert 1e-9 < ya < 2e-6 and 0.0 <= ys < 2e-6
        assert (ys == 0.0) == (W.WCASES[name][8] == 1)
        c = W.wide_case(name)
        assert (c["bounds"] is not None) == (name in W.TIGHT)
        if c["bounds"] is not None:
            sa, ss = F.clamped_shares(c, *F.free_rollout(c))
            assert sa >= 0.1 and ss >= 0.1, (name, sa, ss)
            assert np.allclose(G["share_" + name], [sa, ss], atol=1e-12) and np.all(G["share_" + name] >= 0.1)
    assert float(G["kys_w8"]) == 0.0 and W.WCASES["w8"][8] == 1
    assert 1e-9 < float(G["kfree_obs"]) < 1e-5 and 1e-9 < float(G["kfree_act"]) < 1e-5
