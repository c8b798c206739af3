"""Planning on learned rewards, host side (no GPU): the fp64 restatement of the learned-reward chain (tests/_mpc_learned_oracle.py)
against the unmodified reference's fixture (tests/golden/mpc_learned.npz, tests/golden/make_golden_mpc_learned.py), the route table
of mjx_path_rewards_route, the argument errors of mjx_path_rewards, and MPCPolicy's `reward` keyword."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
from tests._worker_dev import ints as _ints  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "mpc_learned.npz"))


@pytest.mark.parametrize("case", sorted(L.PLAN_CASES))
def test_fixture_weights_are_neither_degenerate_nor_flat(case):
    """the conditions cap: weights on one trajectory, or the same weight on all, would let a wrong reward through"""
    N, H, kappa, omega, fc, gamma = L.PLAN_CASES[case]
    for c in range(L.CALLS):
        e = M.ess(M.weights(G["%s_%d_R" % (case, c)], kappa))
        assert e == pytest.approx(float(G["%s_%d_ess" % (case, c)]))
        assert 5.0 <= e <= 0.5 * L.PK * N
    assert L.PLAN_CASES["la"][3] == 0.0         # only the rewards move case la's weights


# The reference's own distance from the fp64 restatement, measured per case over the three calls (the figures are printed):
#   member rewards, max |dr| / max |r|:   la 3.5e-7   lb 5.1e-7
#   R, max |dR| / max |R|:                la 2.8e-7   lb 1.1e-7
#   planned sequence, relative L2:        la 3.3e-7   lb 2.8e-7
# Bars: a reward is the end of two fp32 nets on an fp32 rollout of up to 16 steps, each correct to a few roundings of the largest
# reward: 32 roundings (32 x 2^-24 = 1.9e-6).  R is tests/test_mpc_cpu.py's bar, 16 roundings of max |R| (9.5e-7): it sums H <= 16 such
# rewards, each rounded once more to fp32 by the reference under NumPy 2 (gamma ** t * np.float32 stays fp32).  The sequence bar is
# the project's TOL_STEP.
BAR_REWARDS, BAR_R, TOL_STEP = 1.9e-6, 9.5e-7, 1e-5


@pytest.mark.parametrize("case", sorted(L.PLAN_CASES))
def test_fp64_restatement_reproduces_the_references_learned_reward_planning(case):
    from mjrl_amd.algos.model_accel.model_learning_mpc import perturbed_action_batch
    N, H, kappa, omega, fc, gamma = L.PLAN_CASES[case]
    mem = L.fixture_members(G)
    np.random.seed(900 + sorted(L.PLAN_CASES).index(case))
    for c in range(L.CALLS):
        key = "%s_%d_" % (case, c)
        assert np.array_equal(G[key + "obs"], L.call_obs(case, c))
        actions = perturbed_action_batch(N, G[key + "seq_in"], list(fc))
        assert np.random.rand() == float(G[key + "after"])
        r = L.plan(G[key + "obs"], actions, mem, kappa, gamma, omega)
        e_rew = L.rel_max(r["rewards"], G[key + "rewards"])
        e_R = float(np.max(np.abs(r["R"] - G[key + "R"])) / np.max(np.abs(G[key + "R"])))
        e_seq = M.rel_l2(r["seq"], np.concatenate([G[key + "action"][None], G[key + "seq_out"][:-1]]))
        print("case %s call %d: rewards %.2e  R %.2e  sequence %.2e" % (case, c, e_rew, e_R, e_seq))
        assert G[key + "rewards"].dtype == np.float32 and G[key + "rewards"].shape == (L.PK, N, H)
        assert e_rew < BAR_REWARDS
        assert e_R < BAR_R
        assert e_seq < TOL_STEP
        assert np.array_equal(G[key + "seq_out"][-1], np.zeros(L.PM))


def test_kernel_yardsticks_are_fp32_sized():
    """the reference's fp32 chain on the kernel cases' inputs lies a few roundings from fp64: a yardstick far from that would make
    the GPU bars (3 x each) meaningless"""
    for name in L.KCASES:
        assert 2.0 ** -25 < float(G["kref_" + name]) < 32 * 2.0 ** -24, name


def test_path_rewards_route_table():
    """mjx_path_rewards_route is arithmetic alone: 1 where a k_path_rewards instance holds BOTH nets in LDS"""
    from mjrl_amd import _lib
    lib = _lib.load()

    def route(ds, rs):
        return lib.mjx_path_rewards_route(_ints(ds), len(ds), _ints(rs), len(rs))

    assert route([23, 64, 64, 17], [40, 100, 100, 1]) == 1            # 133.7 KiB
    assert route([23, 128, 128, 17], [40, 100, 100, 1]) == 0          # 200.2 KiB
    assert route(L.DYN_SIZES, L.REW_SIZES) == 1
    for name, (n, m, dh, rh, act, flags, K) in L.KCASES.items():
        assert route((n + m,) + dh + (n,), (2 * n + m,) + rh + (1,)) == 1, name
    assert route([8, 96, 96, 6], [14, 100, 100, 1]) == 1              # 140.6 KiB
    assert route([8, 128, 128, 6], [14, 64, 64, 1]) == 1              # reward widths <= 64: the narrow instance beside 128 x 128
    assert route([8, 128, 128, 6], [14, 65, 64, 1]) == 0              # one unit more: the wide instance, which 128 x 128 does not have
    assert route([8, 64, 64, 6], [14, 1, 1, 1]) == 1
    assert route([8, 64, 64, 64, 6], [14, 100, 100, 1]) == 0          # three dynamics layers
    assert route([8, 64, 64, 6], [14, 100, 100, 100, 1]) == 0         # three reward layers
    assert route([8, 64, 64, 6], [14, 200, 100, 1]) == 0              # reward width 200
    assert route([8, 64, 64, 6], [14, 100, 129, 1]) == 0
    assert route([8, 100, 100, 6], [14, 100, 100, 1]) == 0            # dynamics widths that are no multiples of 32
    assert route([8, 256, 256, 6], [14, 100, 100, 1]) == 0
    assert route([67, 64, 64, 65], [132, 100, 100, 1]) == 0           # n = 65
    assert route([66, 64, 64, 64], [130, 64, 64, 1]) == 1             # n = 64: 108.9 KiB
    assert route([66, 64, 64, 64], [130, 100, 100, 1]) == 0           # ... 193.6 KiB
    assert route([23, 96, 32, 17], [40, 36, 72, 1]) == 1              # ragged widths are padded per layer (64, 96): 107.0 KiB
    assert route([8, 64, 64, 6], [15, 100, 100, 1]) < 0               # the reward net's input is not [s, a, s']
    assert route([8, 64, 64, 6], [14, 100, 100, 2]) < 0               # ... its output not a scalar
    assert route([6, 64, 64, 6], [12, 100, 100, 1]) < 0               # no action
    assert route([8, 64, 0, 6], [14, 100, 100, 1]) < 0
    assert route([8], [14, 100, 100, 1]) < 0


def test_path_rewards_argument_errors_touch_nothing():
    """bad arguments return MJX_ERR_ARG before any device work (this test has no device); rows == 0 returns MJX_OK and the route"""
    from mjrl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ds, rs = [8, 64, 64, 6], [14, 100, 100, 1]
    route = ctypes.c_int(-7)

    def call(obs=p, act=p, stride=0, rows=5, K=2, ds=ds, dP=p, dtr=p, dact=0, dflags=7, rs=rs, rP=p, rtr=p, ract=0, r32=p, r64=None):
        return lib.mjx_path_rewards(obs, act, stride, rows, K, _ints(ds), len(ds), dP, dtr, dact, dflags, _ints(rs), len(rs), rP, rtr, ract,
                                    r32, r64, ctypes.byref(route), None)

    for bad in (dict(obs=None), dict(act=None), dict(dP=None), dict(dtr=None), dict(rP=None), dict(rtr=None), dict(r32=None, r64=None),
                dict(rows=-1), dict(K=0), dict(stride=7), dict(dact=2), dict(ract=-1), dict(dflags=8), dict(rs=[15, 100, 100, 1]),
                dict(rs=[14, 100, 100, 2]), dict(ds=[8, 64, 0, 6]), dict(ds=[6, 64, 64, 6], rs=[12, 100, 100, 1])):
        assert call(**bad) == -1, bad
        assert route.value == -7 and not any(buf), bad
    assert call(rows=0) == 0 and route.value == 1
    assert call(rows=0, ds=[8, 256, 256, 6]) == 0 and route.value == 0
    os.environ["MJX_PATH_REWARDS_MFMA"] = "0"
    try:
        assert call(rows=0, r32=None, r64=p) == 0 and route.value == 0      # the switch is read per call
    finally:
        os.environ.pop("MJX_PATH_REWARDS_MFMA")
    assert call(rows=0) == 0 and route.value == 1


def _models(learn=(True, True)):
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    return [WorldModel(6, 2, hidden_size=(32, 32), seed=k, learn_reward=lr) for k, lr in enumerate(learn)]


def test_reward_keyword():
    """'env' is the default and today's planner; 'learned' needs a reward net in every member and never looks at env.env.env"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    kw = dict(plan_horizon=5, plan_paths=7)
    assert MPCPolicy(env=M.plan_env(6, 2), fitted_model=_models((False, False)), **kw).reward == 'env'
    with pytest.raises(ValueError):
        MPCPolicy(env=M.plan_env(6, 2), fitted_model=_models((True, False)), reward='learned', **kw)
    with pytest.raises(ValueError):
        MPCPolicy(env=M.plan_env(6, 2), fitted_model=_models((False,))[0], reward='learned', **kw)
    with pytest.raises(ValueError):
        MPCPolicy(env=M.plan_env(6, 2), fitted_model=_models(), reward='model', **kw)
    pol = MPCPolicy(env=L.plan_env_no_rewards(6, 2), fitted_model=_models(), reward='learned', **kw)
    assert pol.reward == 'learned' and pol.last_rewards() is None and pol.last_scores() is None
    assert pol.route() == 1 and pol.reward_route() == 1
    assert MPCPolicy(env=L.plan_env_no_rewards(6, 2), fitted_model=_models((True,))[0], reward='learned', **kw).reward_route() == 1
    assert MPCPolicy(env=M.plan_env(6, 2), fitted_model=_models(), **kw).reward_route() is None
    pol._pack, pol._last = ("key", object()), (object(), object(), object())
    q = pickle.loads(pickle.dumps(pol))
    assert q._pack is None and q._last is None and q.reward == 'learned' and q.reward_route() == 1


def test_pack_key_changes_after_a_reward_refit(monkeypatch):
    """on reward='learned' the device copy also holds the reward nets: the key must change after fit_reward with the transforms
    kept (the write-back goes through p.data.copy_), after new reward transforms and after an in-place edit of a reward parameter,
    and it must hold the tensors it names.  On 'env' the reward nets are not part of the key.  (The fit runs with the library call
    stubbed out: its host side, write-back included, is what is under test.)"""
    import types
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    models = _models()
    pol = MPCPolicy(env=L.plan_env_no_rewards(6, 2), plan_horizon=5, plan_paths=7, fitted_model=models, reward='learned')
    env_pol = MPCPolicy(env=M.plan_env(6, 2), plan_horizon=5, plan_paths=7, fitted_model=models)
    keys, env_key = [pol._pack_key("cpu")[0]], env_pol._pack_key("cpu")[0]
    assert pol._pack_key("cpu")[0] == keys[0]

    def changed():
        k = pol._pack_key("cpu")[0]
        ok = all(k != prev for prev in keys)
        keys.append(k)
        return ok

    monkeypatch.setattr(D, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(D, "_stream", lambda dev: None)
    monkeypatch.setattr(D, "load", lambda: types.SimpleNamespace(mjx_dyn_fit_adam=lambda *a: 0))
    monkeypatch.setattr(D, "ensemble_forward", lambda nets, x, dev=None: torch.zeros((len(nets), x.shape[-2], nets[0].layer_sizes[-1])))
    s, a, sp, r = L.reward_fit_data(64, 3)
    net = models[1].reward_net
    versions = [p._version for p in net.parameters()]
    models[1].fit_reward(s, a, r, 32, 1, set_transformations=False)
    assert [p._version for p in net.parameters()] == versions       # the case the key has to see without torch's help
    assert changed(), "fit_reward(set_transformations=False)"
    assert env_pol._pack_key("cpu")[0] == env_key                   # the env planner's copy holds no reward net
    net.set_transformations(net.s_shift, net.s_scale, net.a_shift, net.a_scale, 0.5, 2.0)
    assert changed(), "new output transforms (plain numbers)"
    net.s_scale.mul_(2.0)
    assert changed(), "in-place edit of a reward transform tensor"
    with torch.no_grad():
        next(models[0].reward_net.parameters()).add_(1.0)
    assert changed(), "in-place edit of a reward parameter"
    key, held = pol._pack_key("cpu")
    assert all(any(t is h for h in held) for t in net.parameters())
    assert len(held) == 2 * (6 + 6) + 2 * (6 + 4)
