"""The wide passes over stored rollouts without a GPU (csrc/rows_wide.h): the two route functions over a table, the LDS float count
against a restatement, the narrow route functions' unchanged answers at 256 wide, the entries' routes on empty calls and their
argument errors (the library builds here and these paths need no device), nn_dynamics.wide_rows_shape, the calls ModelAccelNPG makes
(the recorder of tests/test_model_accel_calls_cpu.py in the library's place), and the conditions on the cases and their fixture
(tests/_rows_wide_cases.py, tests/golden/rows_wide.npz)."""
import ctypes
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rollout_batch_cases as B  # noqa: E402
import _rows_wide_cases as W  # noqa: E402
from tests._worker_dev import ints as _ints  # noqa: E402
from tests.test_model_accel_calls_cpu import Recorder, stubbed  # noqa: E402

LDS_MAX = 160 * 1024


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from mjrl_amd import _lib
    return _lib.load()


def _routes(lib):
    def dis(ds):
        return lib.mjx_rollout_disagreement_wide_route(_ints(ds), len(ds))

    def rew(ds, rs):
        return lib.mjx_path_rewards_wide_route(_ints(ds), len(ds), _ints(rs), len(rs))
    return dis, rew


def test_wide_route_tables():
    lib = _lib()
    dis, rew = _routes(lib)
    # served: the reference's configs, every case, shapes the narrow routes serve too, the smallest and the largest
    assert dis([13, 256, 256, 11]) == 1 and rew([13, 256, 256, 11], [24, 100, 100, 1]) == 1
    assert dis([23, 256, 256, 17]) == 1 and rew([23, 256, 256, 17], [40, 100, 100, 1]) == 1
    for net in W.NETS:
        assert dis(W.dyn_sizes(net)) == 1, net
    for name in W.RCASES:
        assert rew(W.dyn_sizes(W.RCASES[name][0]), W.rew_sizes(name)) == 1, name
    assert dis([23, 64, 64, 17]) == 1 and lib.mjx_rollout_disagreement_route(_ints([23, 64, 64, 17]), 4) == 1
    assert rew([23, 64, 64, 17], [40, 100, 100, 1]) == 1
    assert lib.mjx_path_rewards_route(_ints([23, 64, 64, 17]), 4, _ints([40, 100, 100, 1]), 4) == 1
    assert dis([2, 1, 1, 1]) == 1 and rew([2, 1, 1, 1], [3, 1, 1, 1]) == 1
    assert dis([128, 256, 256, 64]) == 1 and rew([128, 256, 256, 64], [192, 256, 256, 1]) == 1      # n + m = 128
    assert dis([127, 256, 256, 64]) == 1
    # not served
    for ds in ([13, 257, 256, 11], [13, 256, 257, 11], [13, 256, 11], [13, 256, 256, 256, 11], [67, 256, 256, 65], [76, 256, 256, 11],
               [129, 256, 256, 65]):
        assert dis(ds) == 0, ds
        n, m = ds[-1], ds[0] - ds[-1]
        assert rew(ds, [2 * n + m, 100, 100, 1]) == 0, ds
    assert rew([13, 256, 256, 11], [24, 257, 100, 1]) == 0 and rew([13, 256, 256, 11], [24, 100, 257, 1]) == 0
    assert rew([13, 256, 256, 11], [24, 100, 1]) == 0 and rew([13, 256, 256, 11], [24, 100, 100, 100, 1]) == 0
    # bad sizes
    for ds in ([11, 256, 256, 11], [10, 256, 256, 11], [13], [13, 0, 256, 11]):
        assert dis(ds) < 0, ds
        assert rew(ds, [24, 100, 100, 1]) < 0, ds
    assert rew([13, 256, 256, 11], [23, 100, 100, 1]) < 0                # a reward net that does not fit the dynamics net
    assert rew([13, 256, 256, 11], [24, 100, 100, 2]) < 0
    assert rew([13, 256, 256, 11], [24, 0, 100, 1]) < 0 and rew([13, 256, 256, 11], [24]) < 0
    # the arithmetic restated
    table = [([13, 256, 256, 11], [24, 100, 100, 1]), ([13, 257, 256, 11], [24, 100, 100, 1]), ([129, 256, 256, 65], [194, 1, 1, 1]),
             ([13, 256, 256, 11], [24, 100, 1]), ([11, 8, 8, 11], [24, 8, 8, 1]), ([96, 100, 200, 64], [160, 256, 256, 1])]
    for ds, rs in table:
        assert dis(ds) == W.wide_route(ds) and rew(ds, rs) == W.wide_route(ds, rs), (ds, rs)


def test_lds_float_count_and_its_maximum():
    """rows_wide_lds_floats restated (include/mjx.h documents it): two regions of 68-float rows, then the staged vectors; the most any
    served shape takes is 512 rows = 139 264 bytes of tiles plus 8 460 bytes of vectors"""
    assert 4 * 68 * 512 == 139264
    assert W.lds_floats(64, 64, 256, 256, 256, 256) == 68 * 512 + 2115
    assert 4 * W.lds_floats(64, 64, 256, 256, 256, 256) == 139264 + 8460 <= LDS_MAX
    assert W.lds_floats(11, 2, 256, 256) == 68 * 512 + 256 + 256 + 11 + 26 + 22
    assert W.lds_floats(11, 2, 256, 256, 100, 100) == 68 * 512 + 571 + 100 + 200 + 1 + 50
    assert W.lds_floats(17, 6, 160, 96, 33, 130) == 68 * (160 + 160) + 160 + 96 + 17 + 46 + 34 + 33 + 260 + 1 + 82
    assert W.lds_floats(1, 1, 1, 1) == 68 * 64 + 1 + 1 + 1 + 4 + 2 and W.lds_floats(64, 32, 1, 1, 1, 1) == 68 * (64 + 160) + 712
    best = max(W.lds_floats(n, m, h, h, g, g) for n, m in ((64, 64), (64, 32), (1, 1)) for h in (1, 256) for g in (0, 1, 256))
    assert 4 * best == 139264 + 8460
    # the library's own route arithmetic agrees wherever the count decides (it never does below 256 wide: everything fits)
    lib = _lib()
    dis, rew = _routes(lib)
    for n, m, h1, h2, g1, g2 in ((64, 64, 256, 256, 256, 256), (1, 1, 1, 1, 1, 1), (17, 6, 160, 96, 33, 130)):
        assert 4 * W.lds_floats(n, m, h1, h2, g1, g2) <= LDS_MAX and rew([n + m, h1, h2, n], [2 * n + m, g1, g2, 1]) == 1
        assert dis([n + m, h1, h2, n]) == 1


def test_narrow_routes_at_256_wide_are_what_they_were():
    lib = _lib()
    for n, m in ((11, 2), (17, 6), (6, 2)):
        ds, rs = [n + m, 256, 256, n], [2 * n + m, 100, 100, 1]
        assert lib.mjx_rollout_disagreement_route(_ints(ds), 4) == 0
        assert lib.mjx_path_rewards_route(_ints(ds), 4, _ints(rs), 4) == 0


def test_wide_entries_on_empty_calls_and_argument_errors_touch_nothing():
    """bad arguments return MJX_ERR_ARG before any device work (this test has no device); empty work returns MJX_OK and the route: 2
    on a served shape, the narrow route's answer under the _WIDE switch, 0 under the _MFMA switch"""
    lib = _lib()
    buf = (ctypes.c_float * 8192)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    route = ctypes.c_int(-7)
    wide_ds, narrow_ds, rs = [8, 256, 256, 6], [8, 64, 64, 6], [14, 100, 100, 1]

    def dis(obs=p, act=p, P=3, H=4, K=2, ds=wide_ds, dP=p, dtr=p, dact=0, flags=7, err=p):
        return lib.mjx_rollout_disagreement_wide(obs, act, P, H, K, _ints(ds), len(ds), dP, dtr, dact, flags, err, ctypes.byref(route), None)

    def rew(obs=p, act=p, stride=0, rows=5, K=2, ds=wide_ds, dP=p, dtr=p, dact=0, flags=7, rs=rs, rP=p, rtr=p, ract=0, r32=p, r64=p):
        return lib.mjx_path_rewards_wide(obs, act, stride, rows, K, _ints(ds), len(ds), dP, dtr, dact, flags, _ints(rs), len(rs), rP, rtr, ract,
                                         r32, r64, ctypes.byref(route), None)

    for bad in (dict(obs=None), dict(act=None), dict(dP=None), dict(dtr=None), dict(err=None), dict(P=-1), dict(H=-1), dict(K=0), dict(dact=2),
                dict(flags=8), dict(ds=[6, 256, 256, 6]), dict(ds=[8, 0, 256, 6]), dict(ds=[8])):
        assert dis(**bad) == -1, bad
        assert route.value == -7 and not any(buf), bad
    for bad in (dict(obs=None), dict(act=None), dict(dP=None), dict(dtr=None), dict(rP=None), dict(rtr=None), dict(r32=None, r64=None),
                dict(rows=-1), dict(stride=7), dict(K=0), dict(dact=2), dict(ract=2), dict(flags=8), dict(rs=[13, 100, 100, 1]),
                dict(rs=[14, 100, 100, 2]), dict(ds=[8, 0, 256, 6]), dict(rs=[14, 0, 100, 1])):
        assert rew(**bad) == -1, bad
        assert route.value == -7 and not any(buf), bad
    # empty work: no launch, the route reported
    for empty in (dict(P=0), dict(H=1), dict(H=0)):
        assert dis(**empty) == 0 and route.value == 2, empty
        assert dis(ds=narrow_ds, **empty) == 0 and route.value == 2       # served when called directly
        assert dis(ds=[8, 257, 256, 6], **empty) == 0 and route.value == 0
        assert dis(ds=[8, 64, 6], **empty) == 0 and route.value == 0
    assert rew(rows=0) == 0 and route.value == 2
    assert rew(rows=0, r32=None) == 0 and route.value == 2 and rew(rows=0, r64=None) == 0 and route.value == 2
    assert rew(rows=0, ds=narrow_ds) == 0 and route.value == 2
    assert rew(rows=0, ds=[8, 257, 256, 6]) == 0 and route.value == 0
    assert rew(rows=0, rs=[14, 300, 100, 1]) == 0 and route.value == 0
    for call, kw, switches in ((dis, dict(P=0), ("MJX_ROLLOUT_DISAGREE_WIDE", "MJX_ROLLOUT_DISAGREE_MFMA")),
                               (rew, dict(rows=0), ("MJX_PATH_REWARDS_WIDE", "MJX_PATH_REWARDS_MFMA"))):
        for switch, chained in zip(switches, (1, 0)):
            os.environ[switch] = "0"
            try:                                                          # the switches are read per call
                assert call(**kw) == 0 and route.value == 0               # nothing narrower serves 256 wide
                assert call(ds=narrow_ds, **kw) == 0 and route.value == chained
            finally:
                os.environ.pop(switch)
            assert call(**kw) == 0 and route.value == 2
    assert not any(buf)


def test_wide_rows_shape_table():
    from mjrl_amd.algos.model_accel.nn_dynamics import wide_rows_shape as wide
    assert wide((13, 256, 256, 11)) and wide((13, 256, 256, 11), (24, 100, 100, 1))
    assert wide((13, 129, 64, 11)) and wide((13, 64, 129, 11)) and wide([13, 300, 300, 11])     # (the entry decides what is served)
    assert not wide((13, 128, 128, 11)) and not wide((13, 64, 64, 11), (24, 100, 100, 1))
    assert not wide((13, 64, 64, 11), (24, 256, 256, 1))                 # a wide reward net alone keeps its call
    assert not wide((8, 16, 48, 6))
    assert not wide((13, 256, 11)) and not wide((13, 256, 256, 256, 11))
    assert not wide((13, 256, 256, 11), (24, 100, 1)) and not wide((13, 256, 256, 11), (24, 100, 100, 100, 1))
    for net in ("n1", "n2", "n3", "n4", "n5"):
        assert wide(W.dyn_sizes(net)), net
    assert not wide(W.dyn_sizes("n6"))                                   # (the geometry case calls the entry directly)


# ---- the calls ModelAccelNPG makes, recorded
def _agent(hidden):
    from mjrl_amd.algos.model_accel.model_accel_npg import ModelAccelNPG
    from mjrl_amd.algos.model_accel.nn_dynamics import WorldModel
    from mjrl_amd.baselines.linear_baseline import LinearBaseline
    from mjrl_amd.policies.gaussian_mlp import MLP
    spec = types.SimpleNamespace(observation_dim=6, action_dim=2, horizon=10)
    models = [WorldModel(6, 2, hidden_size=hidden, learn_reward=True, seed=k) for k in range(2)]
    pol = MLP(spec, hidden_sizes=(32, 32), seed=3, init_log_std=-0.5)
    return ModelAccelNPG(learned_model=models, env=None, policy=pol, baseline=LinearBaseline(spec), normalized_step_size=0.05, seed=1,
                         refine=True, kappa=2.0, plan_horizon=4, plan_paths=8)


class _OnDevice(torch.Tensor):
    """a CPU tensor that answers is_cuda as a device tensor does (rollout_disagreement_device and pack_rollouts_device assert it)"""
    is_cuda = property(lambda self: True)


def _recorded(hidden, force_narrow):
    """_resident_paths and get_refined_action on two members of the given width -> the transcript of their device calls"""
    from mjrl_amd.algos.model_accel import model_accel_npg as A
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    from mjrl_amd.algos.model_accel import sampling as S
    from mjrl_amd.utils import ingest
    from unittest import mock
    agent = _agent(hidden)
    rec = Recorder()
    rng = np.random.RandomState(9)
    torch.manual_seed(5)

    def disagreement(models, obs_d, act_d, **kw):
        return D.rollout_disagreement_device(models, obs_d.as_subclass(_OnDevice), act_d.as_subclass(_OnDevice), **kw)

    def pack(obs_d, *a, **kw):
        return S.pack_rollouts_device(obs_d.as_subclass(_OnDevice), *a, **kw)

    with stubbed(rec), mock.patch.object(D, "wide_rows_shape", (lambda *a: False) if force_narrow else D.wide_rows_shape), \
            mock.patch.object(A, "rollout_disagreement_device", disagreement), mock.patch.object(A, "pack_rollouts_device", pack):
        agent._step_info = {}
        noise = torch.from_numpy(rng.randn(2, 4, 8, 2).astype(np.float32))
        try:
            agent._resident_paths(rng.randn(8, 6), 4, noise, None, 0.5, -1.0)
        finally:
            ingest.drop_shared_batch()
        agent.get_refined_action(rng.randn(6))
    return rec.calls


def test_model_accel_npg_reaches_the_wide_entries_for_wide_members_only():
    wide, narrow = _recorded((256, 256), False), _recorded((256, 256), True)
    names = [c[0] for c in wide]
    assert [c[0] for c in narrow].count("mjx_path_rewards") == 2 and [c[0] for c in narrow].count("mjx_rollout_disagreement") == 1
    assert names.count("mjx_path_rewards_wide") == 2 and names.count("mjx_rollout_disagreement_wide") == 1
    assert "mjx_path_rewards" not in names and "mjx_rollout_disagreement" not in names
    # the arguments the narrow entries would have received, call by call
    assert len(wide) == len(narrow)
    for g, w in zip(wide, narrow):
        assert g[0] in (w[0], w[0] + "_wide"), (g[0], w[0])
        if g[0] != w[0]:                                                 # (the recorder writes its stand-in values for the entries it knows: what
            assert g[1:] == w[1:], (g[0], w[0])                          # later calls read differs, what these two read does not)
    dis = wide[names.index("mjx_rollout_disagreement_wide")]
    assert len(dis) == 15 and dis[3:6] == [16, 4, 2] and dis[6] == [8, 256, 256, 6]
    rew = wide[names.index("mjx_path_rewards_wide")]
    assert len(rew) == 21 and rew[3:6] == [32 * 2, 32, 2] and rew[6] == [8, 256, 256, 6] and rew[12] == [14, 100, 100, 1]
    # 64-wide members reach the narrow entries only
    names64 = [c[0] for c in _recorded((64, 64), False)]
    assert not any(nm.endswith("_wide") for nm in names64)
    assert names64.count("mjx_path_rewards") == 2 and names64.count("mjx_rollout_disagreement") == 1


# ---- the cases and their fixture
def test_cases_cover_the_edges_the_kernels_have():
    rows = {r for c in W.RCASES.values() for r in c[4]}
    assert {1, 63, 64, 65, 129} <= rows
    assert {W.NETS[c[0]][2] for c in W.RCASES.values()} >= {(256, 256), (160, 96), (100, 200), (129, 1)}
    assert {c[1] for c in W.RCASES.values()} >= {(100, 100), (256, 256), (1, 1), (33, 130)}
    nm = {W.NETS[c[0]][:2] for c in W.RCASES.values()}
    assert (64, 32) in nm and (1, 1) in nm and any(n + m == 128 for n, m in nm)
    assert {W.NETS[c[0]][4] for c in W.RCASES.values()} >= {0, 1, 3, 5, 7}
    assert {c[3] for c in W.RCASES.values()} >= {1, 2, 3}
    assert any(W.NETS[c[0]][3] != c[2] for c in W.RCASES.values())
    assert all(set(c[5]) == {"shared", "own"} for k, c in W.RCASES.items() if k != "rg")
    assert W.tiles_walked(330, 64) == (4, 6, 2)                           # the geometry cases: six tiles over four workgroups
    assert W.RCASES["rg"][3:5] == (64, (330,)) and W.dis_cases()[-1][1:] == (66, 5, 64)
    cases = W.dis_cases()
    assert len(set(cases)) == len(cases) == 21
    assert {c[3] for c in cases} >= {1, 2, 3} and {c[0] for c in cases} == set(W.NETS)
    assert {63, 64, 65, 129} <= {c[1] * c[2] for c in cases} and {63, 64, 65, 129} <= {c[1] * (c[2] - 1) for c in cases}
    assert any(c[2] == 2 for c in cases)
    assert any(c[1] * c[2] > 64 and 64 % c[2] for c in cases)             # a path boundary inside a tile
    assert any(64 % c[2] == 0 and c[1] * c[2] >= 64 for c in cases)       # a path's last row on a tile edge
    assert len(W.limited()) == 9 and all(c[1] >= 31 for c in W.limited())
    for net, (n, m, dh, act, flags, seed) in W.NETS.items():
        col = W.masked_column(net)
        assert (col is not None) == bool(flags & W.MASK)
        if col is not None:
            for tr in W.members(net, 2)["trs"]:
                assert tr[2 * (n + m) + n + col] == 0.0 and abs(tr[2 * (n + m) + col]) == np.float32(0.4)


def test_fixture_has_every_key_and_fp32_sized_yardsticks():
    G = np.load(W.FIXTURE)
    assert set(G.files) == {"r_" + name for name in W.RCASES} | {"d_" + W.dis_id(c) for c in W.dis_cases()}
    for key in G.files:
        assert 0.0 <= float(G[key]) < 1e-4, key
    for name in W.RCASES:
        assert W.ryard(name) > 0
    for case in W.dis_cases():
        assert W.dyard(case) >= 2.0 ** -24


def test_masks_and_residuals_move_the_oracle_and_the_limits_cut_as_required():
    """what tests/golden/make_golden_rows_wide.py asserts, repeated from the oracle alone"""
    for name in W.RORDER:
        mem = W.rcase(name)[0]
        for bit in (W.MASK, W.RES):
            if mem["dflags"] & bit:
                for (rows, mode), ref in W.rreference(name).items():
                    assert B.row_err(W.roracle(name, W.without_flag(mem, bit), rows, mode), ref) > W.MOVES, (name, bit, rows, mode)
    for case in W.dis_cases():
        mem, obs, act = W.dis_data(case)
        ref = B.oracle_err(mem, obs, act)
        for bit in (W.MASK, W.RES):
            if mem["flags"] & bit:
                assert B.row_err(B.oracle_err(dict(mem, flags=mem["flags"] & ~bit), obs, act), ref) > W.MOVES, (case, bit)
        if case in W.limited():
            cut, clamped, whole, P = W.truncation_shares(ref, B.fix_lim(ref))
            assert P / 4 <= cut <= 3 * P / 4 and clamped >= 1 and whole >= 1, (case, cut, clamped, whole)


def test_tile_rows_entry_names_the_shipped_tile():
    assert _lib().mjx_rows_wide_tile_rows() == W.TILE == 64


def test_fp32_torch_restatement_of_the_rewards_is_the_references_distance_from_fp64():
    """_rows_wide_cases.torch_rewards32 (the yardstick's subject of the end-to-end GPU check) against _mpc_learned_oracle.ensemble_rewards:
    it is the arithmetic of the unmodified reference's fp32 chain, so on a case of the fixture it lies no further from fp64 than the
    fixture's yardstick (the largest over the case's row sets and action modes), and not at 0"""
    for name in ("r2", "r4", "r1"):
        mem, data = W.rcase(name)
        for (rows, mode), want in W.rreference(name).items():
            obs, shared, own = data[rows]
            act = np.broadcast_to(shared, (obs.shape[0],) + shared.shape) if mode == "shared" else own
            e = B.row_err(W.torch_rewards32(mem, obs, act), want)
            print(name, rows, mode, e, W.ryard(name))
            assert 0 < e <= W.ryard(name), (name, rows, mode, e)


def test_a_sequential_fp32_mean_misses_the_bar_at_n64_and_the_fp64_sum_does_not():
    """why k_rollout_disagree_wide sums its mean in fp64 (csrc/rows_wide.h): on s' rounded CORRECTLY to fp32 from the fp64 oracle,
    d and d * d in fp32, a sum over c = 0 .. n - 1 in index order taken in fp32 is over the case's bar at n = 64 (4.81e-7 against
    3.52e-7 on n5_P129_H2_K1 -- the figure the first build of the kernel measured on the MI355X), the same sum taken in fp64 is
    well inside it.  The bar is MARGIN x the fixture's yardstick, as in the GPU test"""
    case = ("n5", 129, 2, 1)
    mem, obs, act = W.dis_data(case)
    want = B.oracle_err(mem, obs, act)
    P, H, n = obs.shape
    s, a, sn = obs[:, :-1].reshape(-1, n), act[:, :-1].reshape(P * (H - 1), -1), obs[:, 1:].reshape(-1, n)
    d = sn - np.float32(B.predict64(mem, 0, s, a))
    sq = (d * d).astype(np.float32)
    seq32 = np.cumsum(sq, axis=1, dtype=np.float32)[:, -1] / np.float32(n)
    sum64 = np.float32(sq.astype(np.float64).sum(1) / n)
    bar = W.MARGIN * W.dyard(case)
    e32, e64 = B.row_err(seq32.reshape(P, H - 1), want), B.row_err(sum64.reshape(P, H - 1), want)
    print("fp32 in index order %.3e, fp64 %.3e, bar %.3e" % (e32, e64, bar))
    assert n == 64 and e32 > bar and e64 < bar / 3
