"""The ensemble fit, host side (no GPU): the route table of mjx_dyn_fit_route, the host-side index draw of fit_ensemble against
K successive fit_permutations calls (indices and the state NumPy's global stream is left in), and the argument checks of
mjx_dyn_fit_ensemble, which refuse before any device work."""
import ctypes

import numpy as np
import pytest

from tests._dyn_ensemble_cases import CASES, ROUTE0, XSCR_CASE


def _lib():
    from mjrl_amd import _lib
    return _lib.load()


def _route(sizes, batch, tmode=2):
    return _lib().mjx_dyn_fit_route((ctypes.c_int * len(sizes))(*sizes), len(sizes), batch, tmode)


def test_fit_route_table():
    """arithmetic alone: exactly two hidden layers, widths multiples of 32 from 32 to 256, batch <= 64, d_in <= 128,
    d_out <= 64, target modes 1 and 2"""
    for name, sizes, batch, _, tmode in CASES + [XSCR_CASE]:
        assert _route(sizes, batch, tmode) == 1, name
    for name, sizes, batch, _, tmode, _env in ROUTE0[:-1]:          # (the last one is route 0 by MJX_DYN_FIT_ENS only)
        assert _route(sizes, batch, tmode) == 0, name
    # widths
    assert _route([13, 32, 32, 11], 16) == 1
    assert _route([13, 256, 256, 11], 16) == 1
    assert _route([13, 32, 256, 11], 16) == 1 and _route([13, 256, 32, 11], 16) == 1
    assert _route([13, 288, 288, 11], 16) == 0
    assert _route([13, 256, 288, 11], 16) == 0 and _route([13, 288, 256, 11], 16) == 0
    assert _route([13, 48, 48, 11], 16) == 0
    assert _route([13, 64, 48, 11], 16) == 0 and _route([13, 48, 64, 11], 16) == 0
    assert _route([24, 100, 100, 20], 16) == 0
    # batch
    assert _route([13, 64, 64, 11], 1) == 1
    assert _route([13, 64, 64, 11], 64) == 1
    assert _route([13, 64, 64, 11], 65) == 0
    # input and output widths
    assert _route([128, 64, 64, 11], 16) == 1
    assert _route([129, 64, 64, 11], 16) == 0
    assert _route([128, 64, 64, 64], 16) == 1
    assert _route([128, 64, 64, 65], 16) == 0
    # depth
    assert _route([13, 64, 11], 16) == 0
    assert _route([13, 64, 64, 11], 16) == 1
    assert _route([13, 64, 64, 64, 11], 16) == 0
    # target modes
    assert _route([13, 64, 64, 11], 16, 0) == 0
    assert _route([13, 64, 64, 11], 16, 1) == 1
    assert _route([13, 64, 64, 11], 16, 2) == 1
    # bad sizes
    assert _route([13, 64, 0, 11], 16) < 0
    assert _route([13], 16) < 0
    assert _route([13, 64, 64, 11], 0) < 0
    assert _route([13, 64, 64, 11], 16, 3) < 0


@pytest.mark.parametrize("K, N, batch, epochs, max_steps", [(4, 400, 64, 2, 1e4), (3, 100, 16, 25, 1e4), (3, 50, 7, 5, 12), (1, 33, 33, 3, 1e10),
                                                             (2, 10, 16, 3, 1e4)])
def test_ensemble_fit_indices_draw_what_the_loop_draws(K, N, batch, epochs, max_steps, capsys):
    """member 0's permutations, then member 1's, ...: the indices of K successive fit_permutations calls, and the stream left in
    their state -- with max_steps cutting every member short (one message per member), and with no step at all (batch > N)"""
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    np.random.seed(11)
    want = [D.fit_permutations(N, batch, epochs, max_steps) for _ in range(K)]
    state = np.random.get_state()
    said = capsys.readouterr().out
    np.random.seed(11)
    idx, num_steps, ran = D.ensemble_fit_indices(K, N, batch, epochs, max_steps)
    after = np.random.get_state()
    assert capsys.readouterr().out == said
    assert all(np.array_equal(a, b) for a, b in zip(state, after))
    assert (num_steps, ran) == want[0][1:]
    assert idx.dtype == np.int32 and idx.shape == (K, ran * num_steps * batch)
    for k in range(K):
        assert np.array_equal(idx[k], want[k][0])
    if max_steps == 12:
        assert ran == 2 and said.count("Terminating early") == K       # 7 steps an epoch: the second epoch reaches 12


def test_ensemble_fit_refuses_bad_arguments_before_any_device_work():
    lib = _lib()
    sizes = (ctypes.c_int * 4)(13, 64, 64, 11)
    blk = (ctypes.c_float * 16)()              # never read: every call below is refused by its arguments
    p = ctypes.cast(blk, ctypes.c_void_p)
    s0 = (ctypes.c_int64 * 4)(0, 0, 0, 0)
    route = ctypes.c_int(-9)

    def call(x=p, y=p, N=400, K=4, in_tr=p, out_tr=p, params=p, m=p, v=p, step0=s0, idx=p, steps=5, batch=32, loss=p, sz=sizes, nsz=4):
        return lib.mjx_dyn_fit_ensemble(x, 0, y, 0, N, K, sz, nsz, in_tr, out_tr, 2, 0, params, m, v, step0, idx, steps, batch, 1e-3, 1e-5,
                                        loss, ctypes.byref(route), None)

    before = (ctypes.c_int64 * 2)()
    lib.mjx_process_state(before)
    for kw in (dict(x=None), dict(y=None), dict(in_tr=None), dict(out_tr=None), dict(params=None), dict(m=None), dict(v=None),
               dict(step0=None), dict(idx=None), dict(loss=None), dict(K=0), dict(K=-1), dict(batch=401), dict(batch=0), dict(N=0),
               dict(steps=-1), dict(nsz=1)):
        assert call(**kw) == -1, kw                      # MJX_ERR_ARG
    assert route.value == -9                              # "touch nothing"
    assert call(steps=0) == 0 and route.value == 1        # MJX_OK without a launch
    assert call(steps=0, idx=None, loss=None) == 0
    after = (ctypes.c_int64 * 2)()
    lib.mjx_process_state(after)
    assert after[0] == before[0]                    # no entry reached the HIP runtime
