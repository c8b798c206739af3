"""The policy rollout's host side and ModelAccelNPG's refinement keywords without a GPU: conditions on the fixture
(tests/golden/refine.npz, tests/golden/make_golden_refine.py), mjx_policy_rollout_route's table, mjx_policy_rollout's argument
errors (the library builds here and these paths need no device), and the constructor / get_action surface."""
import ctypes
import os
import pickle
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mpc_learned_oracle as L  # noqa: E402
import _mpc_oracle as M  # noqa: E402
import _refine_oracle as F  # noqa: E402
from tests._worker_dev import ints as _ints  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "refine.npz"))
TOL_STEP = 1e-5
LDS_MAX = 160 * 1024


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from mjrl_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", sorted(F.RCASES))
def test_fixture_weights_are_neither_degenerate_nor_flat(case):
    """5 <= ESS <= 0.5 K N on every call (the condition tests/test_mpc_learned_cpu.py puts on its fixture)"""
    N, H, ph, kappa, omega, gamma = F.RCASES[case]
    for c in range(F.RCALLS):
        key = "%s_%d_" % (case, c)
        e = M.ess(M.weights(G[key + "R"], kappa))
        assert abs(e - float(G[key + "ess"])) < 1e-9 * e
        assert 5.0 <= e <= 0.5 * L.PK * N, (case, c, e)


@pytest.mark.parametrize("case", sorted(F.RCASES))
def test_fp64_restatement_reproduces_the_references_refined_action(case):
    """_refine_oracle.refined (fp64 on the reference's fp32 inputs and torch's noise) against the reference's own pieces: the
    action within TOL_STEP (relative L2) -- and, so that a GPU result has room, within a third of it -- and R within
    tests/test_mpc_cpu.py's R bar (16 fp32 roundings of max |R|).  Measured: action 2.1e-7 .. 1.3e-6, R 8.6e-8 .. 3.9e-7, the rollouts' states at most 2.0e-7 of the largest."""
    import torch
    from mjrl_amd.algos.model_accel.sampling import draw_rollout_noise
    N, H, ph, kappa, omega, gamma = F.RCASES[case]
    mem = L.fixture_members(G)
    pol_sizes = (L.PN,) + tuple(ph) + (L.PM,)
    pol_tr = np.concatenate([np.zeros(L.PN), np.ones(L.PN), np.zeros(L.PM), np.ones(L.PM)])
    for c in range(F.RCALLS):
        key = "%s_%d_" % (case, c)
        assert np.array_equal(G[key + "obs"], F.rcall_obs(case, c)) and int(G[key + "seed"]) == F.rcall_seed(case, c)
        torch.manual_seed(int(G[key + "seed"]))
        noise = draw_rollout_noise(1, H, N, L.PM)[0].numpy()
        assert torch.randn(1).item() == float(G[key + "after"])           # the reference's stream position after the call
        r = F.refined(G[key + "obs"], noise, G[case + "_pol_params"], pol_sizes, pol_tr, mem, kappa, gamma, omega)
        e_a = M.rel_l2(r["action"], G[key + "action"])
        e_R = float(np.max(np.abs(r["R"] - G[key + "R"])) / np.max(np.abs(G[key + "R"])))
        e_o = F.rel_max(G[key + "roll_obs"], r["obs"])
        print("case %s call %d: action %.2e  R %.2e  rollout states %.2e" % (case, c, e_a, e_R, e_o))
        assert e_a < TOL_STEP / 3
        assert e_R < 9.5e-7
        assert e_o < 1e-5


def test_kernel_yardsticks_are_fp32_sized():
    """the reference's own fp32 steps lie a few roundings from fp64 on every kernel case (an H = 1 case stores s0 only: 0), and
    the tight bounds clamp at least a tenth of the fp64 rollout's actions and states"""
    for name in sorted(F.KCASES):
        ya, ys = float(G["kya_" + name]), float(G["kys_" + name])
        print(name, ya, ys)
        assert 1e-9 < ya < 2e-6 and 0.0 <= ys < 2e-6
        assert (ys == 0.0) == (F.KCASES[name][8] == 1)
        c = F.kernel_case(name)
        if c["bounds"] is not None:
            sa, ss = F.clamped_shares(c, *F.free_rollout(c))
            assert sa >= 0.1 and ss >= 0.1, (name, sa, ss)
    assert 1e-9 < float(G["kfree_obs"]) < 1e-5 and 1e-9 < float(G["kfree_act"]) < 1e-5


def _plan_floats(HB, NB, n, m):
    HW, K1 = 32 * HB, (n + 7) // 8 * 8 + (m + 7) // 8 * 8
    return HW * (K1 + 4) + HW * (HW + 4) + 32 * NB * (HW + 4) + 2 * HW + 32 * NB + 2 * K1 + 3 * 32 * NB


def _pol_floats(p1, p2, n, NB):
    P1, P2, n8 = (p1 + 31) // 32 * 32, (p2 + 31) // 32 * 32, (n + 7) // 8 * 8
    return P1 * (n8 + 4) + P2 * (P1 + 4) + 32 * (P2 + 4) + P1 + P2 + 32 + 2 * n8 + 5 * 32 + 2 * 32 * NB


def test_policy_rollout_route_table():
    lib = _lib()

    def route(pol, dyn):
        return lib.mjx_policy_rollout_route(_ints(pol), len(pol), _ints(dyn), len(dyn))

    assert route([17, 64, 64, 6], [23, 64, 64, 17]) == 1
    assert route([17, 1, 1, 6], [23, 64, 64, 17]) == 1
    assert route([17, 65, 64, 6], [23, 64, 64, 17]) == 0
    assert route([17, 64, 65, 6], [23, 64, 64, 17]) == 0
    assert route([17, 128, 128, 6], [23, 64, 64, 17]) == 0
    assert route([17, 64, 6], [23, 64, 64, 17]) == 0                  # one hidden layer
    assert route([17, 64, 64, 64, 6], [23, 64, 64, 17]) == 0          # three
    assert route([17, 64, 64, 6], [23, 256, 256, 17]) == 0
    assert route([17, 64, 64, 6], [23, 64, 48, 17]) == 0              # a dynamics net mjx_plan_route does not serve
    for pol in ([64, 1, 1, 32], [64, 32, 32, 32], [64, 64, 64, 32]):
        assert route(pol, [96, 128, 128, 64]) == 0                    # the dynamics image alone is 155 392 bytes; no policy image fits in the 8 448 left
    assert 4 * _plan_floats(4, 2, 64, 32) == 155392
    # every kernel case of the GPU tests is served, by the instance its comment names
    for name, (n, m, dh, ph, *_rest) in F.KCASES.items():
        assert route([n] + list(ph) + [m], [n + m] + list(dh) + [n]) == 1, name
    # the documented formula decides: 128 x 128 dynamics beside a 64 x 64 policy over n = 1 .. 64 crosses LDS_MAX
    seen = set()
    for m in (6, 32):
        for n in range(1, 65):
            NB = (n + 31) // 32
            fits = 4 * (_plan_floats(4, NB, n, m) + _pol_floats(64, 64, n, NB)) <= LDS_MAX
            assert route([n, 64, 64, m], [n + m, 128, 128, n]) == (1 if fits else 0), (n, m)
            seen.add(fits)
    assert seen == {True, False}
    n_over = min(n for n in range(1, 65) if 4 * (_plan_floats(4, (n + 31) // 32, n, 32) + _pol_floats(64, 64, n, (n + 31) // 32)) > LDS_MAX)
    assert route([n_over - 1, 64, 64, 32], [n_over - 1 + 32, 128, 128, n_over - 1]) == 1       # just under
    assert route([n_over, 64, 64, 32], [n_over + 32, 128, 128, n_over]) == 0                   # just over
    # a policy that does not fit the dynamics net's n and m, and malformed sizes
    assert route([16, 64, 64, 6], [23, 64, 64, 17]) < 0
    assert route([17, 64, 64, 5], [23, 64, 64, 17]) < 0
    assert route([17, 64, 64, 6], [17, 64, 64, 17]) < 0               # no action
    assert route([17, 0, 64, 6], [23, 64, 64, 17]) < 0
    assert route([17], [23, 64, 64, 17]) < 0


def test_policy_rollout_argument_errors_touch_nothing():
    """bad arguments return MJX_ERR_ARG before any device work (this test has no device); N == 0 returns MJX_OK and the route"""
    lib = _lib()
    buf = (ctypes.c_float * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ps, ds = [6, 32, 32, 2], [8, 64, 64, 6]
    route = ctypes.c_int(-7)

    def call(s0=p, s0s=0, N=5, H=3, K=2, ps=ps, pP=p, ptr=p, nz=p, nzs=0, ds=ds, dP=p, dtr=p, act=0, flags=7, alo=p, ahi=p, slo=p, shi=p,
             obs=p, ao=p):
        return lib.mjx_policy_rollout(s0, s0s, N, H, K, _ints(ps), len(ps), pP, ptr, nz, nzs, _ints(ds), len(ds), dP, dtr, act, flags,
                                      alo, ahi, slo, shi, obs, ao, ctypes.byref(route), None)

    for bad in (dict(s0=None), dict(pP=None), dict(ptr=None), dict(dP=None), dict(dtr=None), dict(obs=None), dict(ao=None),
                dict(s0s=5), dict(nzs=7), dict(nzs=5 * 3 * 2 + 1), dict(alo=None), dict(ahi=None), dict(slo=None), dict(shi=None),
                dict(N=-1), dict(H=-1), dict(K=0), dict(act=2), dict(flags=8), dict(ps=[5, 32, 32, 2]), dict(ps=[6, 32, 32, 3]),
                dict(ds=[8, 64, 0, 6]), dict(ps=[6, 0, 32, 2])):
        assert call(**bad) == -1, bad
        assert route.value == -7 and not any(buf), bad
    assert call(N=0) == 0 and route.value == 1
    assert call(N=0, s0s=6, nzs=0, nz=None, alo=None, ahi=None, slo=None, shi=None) == 0 and route.value == 1
    assert call(H=0, nzs=0) == 0 and route.value == 1
    assert call(N=0, ds=[8, 256, 256, 6]) == 0 and route.value == 0
    assert call(N=0, ps=[6, 32, 2]) == 0 and route.value == 0
    os.environ["MJX_POLICY_ROLLOUT_MFMA"] = "0"
    try:
        assert call(N=0) == 0 and route.value == 0                    # the switch is read per call
    finally:
        os.environ.pop("MJX_POLICY_ROLLOUT_MFMA")
    assert call(N=0) == 0 and route.value == 1


def _agent(**kw):
    from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    spec = types.SimpleNamespace(observation_dim=6, action_dim=2, horizon=10)
    pol = MLP(spec, hidden_sizes=(32, 32), seed=3, init_log_std=-0.5)
    models = [WorldModel(6, 2, hidden_size=(64, 64), seed=k, learn_reward=True) for k in range(2)]
    return ModelAccelNPG(learned_model=models, env=None, policy=pol, baseline=LinearBaseline(spec), normalized_step_size=0.05, seed=1,
                         **kw), pol


def test_refine_keywords_and_unrefined_get_action():
    """refine_gamma / refine_omega construct (defaults 1.0 and 0.0); refine=False still hands policy.get_action's value on and
    consumes NumPy's stream as it does; the route answer needs no device; a pickle carries no device blocks"""
    agent, pol = _agent(refine=True, refine_gamma=0.9, refine_omega=2.0, kappa=3.0, plan_horizon=4, plan_paths=9)
    assert (agent.refine, agent.refine_gamma, agent.refine_omega, agent.kappa, agent.plan_horizon, agent.plan_paths) == (True, 0.9, 2.0, 3.0, 4, 9)
    assert agent.refine_route() == 1 and agent.last_scores() is None
    plain, pol2 = _agent()
    assert (plain.refine, plain.refine_gamma, plain.refine_omega) == (False, 1.0, 0.0)
    o = np.random.RandomState(0).randn(6)
    np.random.seed(5)
    got = plain.get_action(o)
    after = np.random.rand()
    np.random.seed(5)
    want = pol2.get_action(o)
    assert np.random.rand() == after
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1]['mean'], want[1]['mean'])
    agent._refine_pack, agent._refine_last = ("key", object(), []), (object(), object(), 1)
    q = pickle.loads(pickle.dumps(agent))
    assert q._refine_pack is None and q._refine_last is None and q.refine_omega == 2.0 and q.refine_route() == 1
    agent.invalidate()
    assert agent._refine_pack is None
