"""MPC planning, host side (no GPU), against the unmodified reference's fixtures (tests/golden/mpc.npz,
tests/golden/make_golden_mpc.py): the vectorised action draw and NumPy's stream after it, the fp64 restatement of get_action
(tests/_mpc_oracle.py) against the reference's scores and sequences, sample_paths / evaluate_policy, the drop-in binding, the
route table of mjx_plan_route and pickling of an MPCPolicy."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mpc_oracle as M  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "mpc.npz"))


def _members(case):
    """(thetas, transforms) of the case's members: stored (a, b) or rebuilt from their seeds and proved equal by sample and sum"""
    n, m = M.CASES[case][:2]
    if case in M.FITTED:
        return [G["fit_%d_params" % k] for k in range(3)], [M.packed(G["fit_%d_tr" % k], n, m) for k in range(3)]
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    ths, trs = [], []
    for k, wm in enumerate(M.init_members(WorldModel, torch, case)):
        th = M.flat_params(wm.dynamics_net)
        assert np.array_equal(th[M.sample_idx(th.size)], G["%s_m%d_psample" % (case, k)]), (case, k)
        assert float(np.sum(th.astype(np.float64))) == float(G["%s_m%d_psum" % (case, k)]), (case, k)
        ths.append(th)
        trs.append(M.packed(M.flat_transforms(wm.dynamics_net), n, m))
    return ths, trs


@pytest.mark.parametrize("case", sorted(M.CASES))
def test_fixture_weights_are_not_degenerate(case):
    """softmax weights that collapse onto one trajectory would make every sequence comparison empty"""
    kappa = M.CASES[case][6]
    for c in range(M.CALLS):
        assert float(G["%s_%d_ess" % (case, c)]) >= 5.0
        assert M.ess(M.weights(G["%s_%d_R" % (case, c)], kappa)) >= 5.0


@pytest.mark.parametrize("case", sorted(M.CASES))
def test_vectorised_action_draw_is_the_references_bit_for_bit(case):
    """one np.random.normal(size=(N, H, m)) + the filter over N == N calls of generate_perturbed_actions, and the stream ends
    where the reference's ends (the next np.random.rand() after each of the three chained calls)"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import perturbed_action_batch
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
    np.random.seed(500 + sorted(M.CASES).index(case))
    for c in range(M.CALLS):
        key = "%s_%d_" % (case, c)
        state = np.random.get_state()
        act = perturbed_action_batch(N, G[key + "seq_in"], list(fc))
        assert act.shape == (N, H, m) and act.dtype == np.float64
        flat = act.ravel()
        assert np.array_equal(flat[M.sample_idx(flat.size)], G[key + "act_sample"])
        assert float(flat.sum()) == float(G[key + "act_sum"])
        assert np.random.rand() == float(G[key + "after"])
        after = np.random.get_state()
        np.random.set_state(state)                      # ... and the restatement's N separate draws give the same numbers
        assert np.array_equal(M.perturbed_actions(N, G[key + "seq_in"], list(fc)), act)
        np.random.set_state(after)


def test_vectorised_action_draw_with_odd_counts_and_vector_sigma():
    """odd numbers of normals per call: NumPy's cached second Gaussian crosses the call boundaries"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import perturbed_action_batch
    base = np.random.RandomState(1).randn(3, 1)
    for fc in ([0.7, 0.25, 0.5, 0.25], [np.array([0.3]), 1.0, 0.0, 0.0]):
        np.random.seed(9)
        a = M.perturbed_actions(5, base, fc)
        ra = np.random.rand()
        np.random.seed(9)
        b = perturbed_action_batch(5, base, fc)
        assert np.array_equal(a, b) and np.random.rand() == ra


# the reference's own distance from the fp64 restatement, measured per case over the three calls (make_golden_mpc.py's run):
#   planned sequence, relative L2:   a 3.2e-7  b 1.6e-7  c 3.1e-6  d 7.0e-7  e 1.7e-6  f 2.3e-7  g 1.0e-9
#   R, max |dR| / max |R|:           a 7.3e-8  b 1.1e-7  c 2.1e-7  d 1.7e-7  e 1.2e-7  f 2.4e-7  g 1.3e-8
# The sequence bar is the project's TOL_STEP for an update direction; the R bar is 16 fp32 roundings (16 x 2^-24 = 9.5e-7): R sums
# H <= 32 fp32-computed rewards and an fp32 np.std, each correct to a few roundings of max |R|.
@pytest.mark.parametrize("case", sorted(M.CASES))
def test_fp64_restatement_reproduces_the_references_scores_and_sequences(case):
    from mjrl_amd.algos.model_accel.model_learning_mpc import perturbed_action_batch
    n, m, hid, K, N, H, kappa, omega, fc, activation, residual, gamma = M.CASES[case]
    ths, trs = _members(case)
    sizes = (n + m,) + tuple(hid) + (n,)
    act_code, flags = (1 if activation == "tanh" else 0), (7 if residual else 3)
    np.random.seed(500 + sorted(M.CASES).index(case))
    for c in range(M.CALLS):
        key = "%s_%d_" % (case, c)
        actions = perturbed_action_batch(N, G[key + "seq_in"], list(fc))
        np.random.rand()
        r = M.plan(G[key + "obs"], actions, ths, sizes, trs, act_code, flags, kappa, gamma, omega)
        obs = r["obs"].reshape(K, -1)
        assert np.max(np.abs(obs[:, M.sample_idx(obs.shape[1])] - G[key + "obs_sample"])) <= 1e-5 * max(1.0, np.max(np.abs(obs)))
        ref_seq = np.concatenate([G[key + "action"][None], G[key + "seq_out"][:-1]])
        e_seq = M.rel_l2(r["seq"], ref_seq)
        e_R = float(np.max(np.abs(r["R"] - G[key + "R"])) / np.max(np.abs(G[key + "R"])))
        print("case %s call %d: sequence %.2e  R %.2e" % (case, c, e_seq, e_R))
        assert e_seq < 1e-5                         # [3.1e-6]
        assert e_R < 9.5e-7                         # [2.4e-7]
        assert np.array_equal(G[key + "seq_out"][-1], np.zeros(m))          # the warm-start shift appends the mean


def _check_paths(prefix, paths, after):
    ref = M.flatten_paths(prefix, paths, after)
    names = [k for k in G.files if k.startswith(prefix + "_")]
    assert sorted(ref) == sorted(names)
    for k in names:
        a, b = ref[k], G[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert np.array_equal(a, b), k


@pytest.mark.parametrize("name,eval_mode,as_list", M.SAMPLE_RUNS)
def test_sample_paths_against_the_reference(name, eval_mode, as_list):
    """arrays, `terminated`, key sets, env_infos (nested) and NumPy's stream afterwards; eval_mode on / off, array- and
    list-valued get_action"""
    from mjrl_amd.algos.model_accel.sampling import sample_paths
    paths, after = M.run_sample_paths(sample_paths, name, eval_mode, as_list)
    assert {bool(p["terminated"]) for p in paths} == {True, False} or name != "sp_eval_arr"
    _check_paths(name, paths, after)


@pytest.mark.parametrize("name,real_step,noise,as_list", M.EVAL_RUNS)
def test_evaluate_policy_against_the_reference(name, real_step, noise, as_list):
    from mjrl_amd.algos.model_accel.sampling import evaluate_policy
    paths, after = M.run_evaluate_policy(evaluate_policy, name, real_step, noise, as_list)
    _check_paths(name, paths, after)


def test_dropin_binds_mpc_and_real_environment_sampling():
    code = (
        "import sys, types; sys.path.insert(0, %r)\n"
        "for name in ('mjrl', 'mjrl.algos', 'mjrl.baselines', 'mjrl.policies', 'mjrl.utils'):\n"
        "    mod = types.ModuleType(name); mod.__path__ = []; sys.modules[name] = mod\n"
        "from mjrl_amd import dropin; n = len(dropin.install())\n"
        "from mjrl.algos.model_accel.sampling import sample_paths, evaluate_policy\n"
        "from mjrl.algos.model_accel.model_learning_mpc import MPCPolicy\n"
        "mod = sys.modules['mjrl.algos.model_accel.model_learning_mpc']\n"
        "print(n, sample_paths.__module__, evaluate_policy.__module__, MPCPolicy.__module__, mod.__name__)\n"
    ) % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["13", "mjrl_amd.algos.model_accel.sampling", "mjrl_amd.algos.model_accel.sampling",
                                "mjrl_amd.algos.model_accel.model_learning_mpc",
                                "mjrl_amd.algos.model_accel.model_learning_mpc"], r.stdout


def test_plan_route_table():
    """mjx_plan_route is arithmetic alone: the fixture cases' routes, and the generic route for three hidden layers, widths that
    are not multiples of 32 or exceed 128, and states wider than 64"""
    from mjrl_amd import _lib
    lib = _lib.load()

    def route(sizes, m):
        return lib.mjx_plan_route((ctypes.c_int * len(sizes))(*sizes), len(sizes), m)

    for case, (n, m, hid, *_rest) in M.CASES.items():
        assert route([n + m, *hid, n], m) == M.ROUTES[case], case
    assert route([8, 64, 64, 64, 6], 2) == 0
    assert route([8, 100, 100, 6], 2) == 0
    assert route([8, 160, 160, 6], 2) == 0
    assert route([8, 64, 160, 6], 2) == 0
    assert route([67, 64, 64, 65], 2) == 0
    assert route([66, 64, 64, 64], 2) == 1
    assert route([96, 128, 128, 64], 32) == 1          # the largest image: 155.4 KiB
    assert route([97, 128, 128, 64], 33) == 0          # more actions than a lane keeps ahead
    assert route([8, 32, 32, 6], 2) == 1
    assert route([8, 64, 64, 6], 3) < 0                 # sizes[0] != n + act_dim
    assert route([8, 64, 0, 6], 2) < 0
    assert route([8], 2) < 0


def test_mpc_policy_pickles_without_a_device():
    """run_model_learning_mpc.py pickles the policy: the device cache is dropped, everything else survives"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    models = [WorldModel(6, 2, hidden_size=(32, 32), seed=k) for k in range(2)]
    pol = MPCPolicy(env=M.plan_env(6, 2), plan_horizon=5, plan_paths=7, kappa=2.0, gamma=0.9, mean=np.array([0.1, -0.2]),
                    filter_coefs=[0.3, 0.25, 0.8, 0.0], fitted_model=models, omega=1.5)
    pol._pack = ("key", object())
    pol._last = (object(), object())
    q = pickle.loads(pickle.dumps(pol))
    assert q._pack is None and q._last is None and pol._pack is not None
    assert np.array_equal(q.act_sequence, np.ones((5, 2)) * np.array([0.1, -0.2])) and np.array_equal(q.init_act_sequence, q.act_sequence)
    assert (q.plan_horizon, q.num_traj, q.kappa, q.gamma, q.omega, q.warmstart, q.n, q.m) == (5, 7, 2.0, 0.9, 1.5, True, 6, 2)
    assert q.reference_indexing is True and q.route() == 1
    for a, b in zip(q.fitted_model, models):
        assert np.array_equal(M.flat_params(a.dynamics_net), M.flat_params(b.dynamics_net))


def test_numpy_scoring_methods_follow_the_reference_expressions():
    """score_trajectory / score_trajectory_ensemble stay callable: both index settings against the restatement"""
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    rng = np.random.RandomState(4)
    K, N, H, n = 3, 5, 4, 2
    obs = rng.randn(K, N, H, n)
    rew = rng.randn(K, N, H)
    models = [WorldModel(n, 1, hidden_size=(32, 32), seed=k) for k in range(K)]
    for ref_idx in (True, False):
        pol = MPCPolicy(env=M.plan_env(n, 1), plan_horizon=H, plan_paths=N, gamma=0.9, fitted_model=models, omega=2.0,
                        reference_indexing=ref_idx)
        paths_list = [dict(observations=obs[k], rewards=rew[k]) for k in range(K)]
        paths = dict(rewards=rew.reshape(K * N, H))
        got = pol.score_trajectory_ensemble(paths, paths_list)
        assert np.allclose(got, M.scores(obs, rew, 2.0, 0.9, ref_idx), rtol=1e-13, atol=1e-13)
        assert np.allclose(pol.score_trajectory(paths), M.scores(obs, rew, 2.0, 0.9, ensemble=False), rtol=1e-13, atol=1e-13)
    assert not np.allclose(M.scores(obs, rew, 2.0, 0.9, True), M.scores(obs, rew, 2.0, 0.9, False))


def test_pack_key_sees_every_write_path_of_the_package(monkeypatch):
    """The planner's device copy of the members is keyed by MPCPolicy._pack_key.  It must change after the package's own fit
    with the transforms kept (the write-back goes through p.data.copy_, which leaves p._version as it was), after set_params,
    set_transformations and in-place edits of a parameter or a transform tensor -- and hold the tensors it names.  The fit runs
    here with the library call stubbed out (no device): its host side, write-back included, is what is under test."""
    import types
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    from mjrl_amd.algos.model_accel.model_learning_mpc import MPCPolicy
    models = [D.WorldModel(6, 2, hidden_size=(32, 32), seed=k) for k in range(2)]
    pol = MPCPolicy(env=M.plan_env(6, 2), plan_horizon=5, plan_paths=7, fitted_model=models)
    keys = [pol._pack_key("cpu")[0]]
    assert pol._pack_key("cpu")[0] == keys[0]                       # stable while nothing changes

    def changed():
        k = pol._pack_key("cpu")[0]
        ok = all(k != prev for prev in keys)
        keys.append(k)
        return ok

    monkeypatch.setattr(D, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(D, "_stream", lambda dev: None)
    monkeypatch.setattr(D, "load", lambda: types.SimpleNamespace(mjx_dyn_fit_adam=lambda *a: 0))
    s, a, sp = M.fit_data(64, 6, 2, 3)
    net = models[1].dynamics_net
    versions = [p._version for p in net.parameters()]
    tr_ids = [id(t) for t in net.get_params()["transforms"]]
    models[1].fit_dynamics(s, a, sp, 32, 1, set_transformations=False)
    assert [p._version for p in net.parameters()] == versions       # the case the key has to see without torch's help
    assert [id(t) for t in net.get_params()["transforms"]] == tr_ids
    assert changed(), "fit_dynamics(set_transformations=False)"
    net._apply_out_transforms = False
    D.fit_model(net, (torch.from_numpy(s), torch.from_numpy(a)), torch.from_numpy(sp), models[1].dynamics_opt, None, 32, 1)
    net._apply_out_transforms = True
    assert changed(), "fit_model"
    net.set_params(net.get_params())
    assert changed(), "set_params"
    net.set_transformations(*net.get_params()["transforms"])
    assert changed(), "set_transformations with the same tensors"
    net.out_scale.mul_(2.0)
    assert changed(), "in-place edit of a transform tensor"
    with torch.no_grad():
        next(models[0].dynamics_net.parameters()).add_(1.0)
    assert changed(), "in-place edit of a parameter"
    net.nonlinearity = torch.tanh
    assert changed(), "activation"
    key, held = pol._pack_key("cpu")
    assert len(held) == 2 * (6 + 6) and all(any(t is h for h in held) for t in net.parameters())
