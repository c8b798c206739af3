"""The reward-net ensemble fit, host side (no GPU): the route table of mjx_reward_fit_route, the LDS layout of the ensemble
kernel for ragged widths against the arithmetic written out, the host-side index draws of fit_world_models against
fit_permutations called in the driver's order (indices and the state NumPy's global stream is left in), and the argument checks
of mjx_reward_fit_ensemble, which refuse before any device work."""
import ctypes

import numpy as np
import pytest

from tests._reward_fit_cases import CASES, MAX_CASE, ROUTE0

ERR_ARG = -1


def _lib():
    from mjrl_amd import _lib
    return _lib.load()


def _route(sizes, batch):
    return _lib().mjx_reward_fit_route((ctypes.c_int * len(sizes))(*sizes), len(sizes), batch)


def test_reward_fit_route_table(monkeypatch):
    """arithmetic alone: exactly two hidden layers, each width 1 .. 256, batch 1 .. 64, d_in <= 128, d_out <= 64 -- one landmark
    on each side of every limit; MJX_REWARD_FIT_ENS does not change the answer"""
    for env in (None, "0"):
        if env is not None:
            monkeypatch.setenv("MJX_REWARD_FIT_ENS", env)
        assert _route([24, 100, 100, 1], 64) == 1
        assert _route([9, 33, 36, 1], 32) == 1
        assert _route([5, 1, 1, 1], 1) == 1
        assert _route([128, 256, 256, 64], 64) == 1
        assert _route([129, 256, 256, 64], 64) == 0
        assert _route([128, 257, 256, 64], 64) == 0 and _route([128, 256, 257, 64], 64) == 0
        assert _route([128, 256, 256, 65], 64) == 0
        assert _route([128, 256, 256, 64], 65) == 0 and _route([24, 100, 100, 1], 65) == 0
        assert _route([24, 100, 1], 64) == 0
        assert _route([24, 100, 100, 100, 1], 64) == 0
        assert _route([24, 100, 100, 1], 0) == ERR_ARG
        assert _route([24, 100, 100, 1], -3) == ERR_ARG
        assert _route([13], 16) == ERR_ARG
        assert _route([24, 0, 100, 1], 16) == ERR_ARG
    for name, sizes, batch, _ in CASES + [MAX_CASE]:
        assert _route(sizes, batch) == 1, name
    for name, sizes, batch, _, env in ROUTE0:
        assert _route(sizes, batch) == (1 if env == "0" else 0), name


def _layout(sizes, batch):
    info = (ctypes.c_int64 * 4)()
    rc = _lib().mjx_dyn_fit_ens_layout((ctypes.c_int * len(sizes))(*sizes), len(sizes), batch, info)
    return rc, list(info)


@pytest.mark.parametrize("sizes, batch", [([24, 100, 100, 1], 64), ([24, 100, 100, 1], 16), ([14, 100, 100, 1], 33), ([9, 33, 36, 1], 32),
                                          ([5, 31, 7, 1], 8), ([5, 1, 1, 1], 1), ([10, 100, 72, 3], 32), ([128, 255, 250, 1], 64),
                                          ([128, 225, 256, 64], 64), ([13, 256, 256, 11], 64), ([10, 64, 96, 8], 32), ([128, 256, 256, 64], 64)])
def test_layout_bytes_for_ragged_and_aligned_widths(sizes, batch):
    """H1, H2 and Z3 as [unit][sample] tiles: the unit rows of each padded to the next multiple of 32, the samples to 32 or 64
    with a row stride of 4 more; the gathered inputs (rows padded to 8) beside them while 160 KiB, less the kernel's 320 B of
    static LDS, holds both.  For multiples of 32 that is (h1 + h2 + ZR) rows: the bytes before ragged widths were served."""
    pad32 = lambda d: -(-d // 32) * 32
    din, h1, h2, dout = sizes
    st = (64 if batch > 32 else 32) + 4
    tiles = (pad32(h1) + pad32(h2) + pad32(dout)) * st * 4
    xtile = -(-din // 8) * 8 * st * 4
    in_lds = tiles + xtile + 8 * 8 + 64 * 4 <= 160 * 1024
    rc, info = _layout(sizes, batch)
    assert rc == 0
    assert info == [tiles + (xtile if in_lds else 0), int(in_lds), st, xtile // 4]
    if h1 % 32 == 0 and h2 % 32 == 0:
        assert info[0] == (h1 + h2 + pad32(dout)) * st * 4 + (xtile if in_lds else 0)
    assert info[0] + 320 <= 160 * 1024


def test_layout_cases_cover_both_homes_of_the_inputs():
    assert _layout([24, 100, 100, 1], 64)[1][1] == 1
    assert _layout(MAX_CASE[1], MAX_CASE[2])[1][1] == 0          # rw_max_b64: the inputs live in scratch
    assert _layout([24, 300, 100, 1], 64)[0] == ERR_ARG          # not a shape of the kernel
    assert _layout([24, 100, 100, 1], 0)[0] == ERR_ARG


@pytest.mark.parametrize("K, N, batch, epochs, max_steps", [(3, 100, 32, 3, 1e4), (4, 400, 64, 2, 1e4), (3, 50, 7, 5, 12), (2, 10, 16, 3, 1e4),
                                                             (1, 33, 33, 3, 1e10)])
def test_world_model_fit_indices_draw_what_the_driver_draws(K, N, batch, epochs, max_steps, capsys):
    """member 0's dynamics permutations, member 0's reward permutations, member 1's dynamics permutations, ...: the indices of
    2 K fit_permutations calls in the driver's order and the stream left in their state -- with max_steps cutting every fit
    short (one message per fit), and with no step at all (batch > N)"""
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    np.random.seed(11)
    want = [(D.fit_permutations(N, batch, epochs, max_steps), D.fit_permutations(N, batch, epochs, max_steps)) for _ in range(K)]
    state = np.random.get_state()
    said = capsys.readouterr().out
    np.random.seed(11)
    dyn, rew = D.world_model_fit_indices(K, N, batch, epochs, max_steps, True)
    after = np.random.get_state()
    assert capsys.readouterr().out == said
    assert all(np.array_equal(a, b) for a, b in zip(state, after))
    for which, (idx, num_steps, ran) in enumerate((dyn, rew)):
        assert (num_steps, ran) == want[0][which][1:]
        assert idx.dtype == np.int32 and idx.shape == (K, ran * num_steps * batch)
        for k in range(K):
            assert np.array_equal(idx[k], want[k][which][0])
    if K > 1 and dyn[0].size:
        assert not np.array_equal(dyn[0][0], rew[0][0]) and not np.array_equal(rew[0][0], dyn[0][1])
    if max_steps == 12:
        assert dyn[2] == 2 and said.count("Terminating early") == 2 * K       # 7 steps an epoch: the second epoch reaches 12


def test_world_model_fit_indices_without_learned_rewards_is_ensemble_fit_indices():
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    np.random.seed(5)
    want = D.ensemble_fit_indices(3, 100, 32, 3, 1e4)
    state = np.random.get_state()
    np.random.seed(5)
    dyn, rew = D.world_model_fit_indices(3, 100, 32, 3, 1e4, False)
    assert rew is None
    assert np.array_equal(dyn[0], want[0]) and dyn[1:] == want[1:]
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))


def test_reward_fit_refuses_bad_arguments_before_any_device_work():
    lib = _lib()
    sizes = (ctypes.c_int * 4)(24, 100, 100, 1)
    blk = (ctypes.c_float * 16)()              # never read: every call below is refused by its arguments
    p = ctypes.cast(blk, ctypes.c_void_p)
    s0 = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    neg = (ctypes.c_int64 * 4)(0, 0, -1, 0)
    route = ctypes.c_int(-9)

    def call(x=p, y=p, N=400, K=4, in_tr=p, out_tr=p, act=0, params=p, m=p, v=p, step0=s0, idx=p, steps=5, batch=32, loss=p, sz=sizes, nsz=4,
             xs=0, ys=0):
        return lib.mjx_reward_fit_ensemble(x, xs, y, ys, N, K, sz, nsz, in_tr, out_tr, act, params, m, v, step0, idx, steps, batch, 1e-3, 1e-5,
                                           loss, ctypes.byref(route), None)

    before = (ctypes.c_int64 * 2)()
    lib.mjx_process_state(before)
    for kw in (dict(x=None), dict(y=None), dict(in_tr=None), dict(out_tr=None), dict(params=None), dict(m=None), dict(v=None),
               dict(step0=None), dict(step0=neg), dict(idx=None), dict(loss=None), dict(K=0), dict(K=-1), dict(batch=401), dict(batch=0),
               dict(N=0), dict(steps=-1), dict(nsz=1), dict(act=2), dict(xs=-1), dict(ys=-1)):
        assert call(**kw) == ERR_ARG, kw
    assert route.value == -9                              # "touch nothing"
    assert call(steps=0) == 0 and route.value == 1        # MJX_OK without a launch
    assert call(steps=0, batch=65) == 0 and route.value == 0
    assert call(steps=0, idx=None, loss=None) == 0
    after = (ctypes.c_int64 * 2)()
    lib.mjx_process_state(after)
    assert after[0] == before[0]                    # no entry reached the HIP runtime
