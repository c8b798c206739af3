"""mjx_linear_route, host side (no GPU): which update serves a LinearPolicy shape -- route 1, the Gram route of
csrc/linear_policy.h, for no hidden layer with n <= 63 and m <= 32; route 0 for everything else and under MJX_LINEAR_GRAM=0."""
import ctypes

import pytest

ERR_ARG = -1


def _lib():
    from mjrl_amd import _lib
    return _lib.load()


def _route(n, m, hidden=()):
    out = (ctypes.c_int32 * 4)()
    assert _lib().mjx_linear_route(n, m, (ctypes.c_int * max(len(hidden), 1))(*hidden), len(hidden), out) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("n", [1, 6, 31, 32, 63])
@pytest.mark.parametrize("m", [1, 17, 32])
def test_gram_route_and_its_layout(n, m):
    """route 1 with NP = n + 1 padded to 32 or 64, the LDS bytes of LinLayout's own arithmetic (two [W | b] images and four
    wave tiles of 32 x (NP + 4), 2 NP column and 5 x 32 action values), and chains of 1024 rows at the most"""
    NP = 32 if n + 1 <= 32 else 64
    assert _route(n, m) == [1, NP, 4 * (6 * 32 * (NP + 4) + 2 * NP + 5 * 32), 1024]


@pytest.mark.parametrize("n,m,hidden", [(64, 6, ()), (17, 33, ()), (17, 6, (32,)), (17, 6, (64, 64))])
def test_everything_else_is_route_0(n, m, hidden):
    assert _route(n, m, hidden) == [0, 0, 0, 0]


def test_switch_and_arguments(monkeypatch):
    lib, out = _lib(), (ctypes.c_int32 * 4)()
    monkeypatch.setenv("MJX_LINEAR_GRAM", "0")
    assert _route(17, 6) == [0, 0, 0, 0]                   # read per call
    monkeypatch.delenv("MJX_LINEAR_GRAM")
    assert _route(17, 6)[0] == 1
    assert lib.mjx_linear_route(17, 6, None, 0, None) == ERR_ARG
    assert lib.mjx_linear_route(17, 6, None, 1, out) == ERR_ARG
    assert lib.mjx_linear_route(0, 6, None, 0, out) == ERR_ARG
    assert lib.mjx_linear_route(17, 6, (ctypes.c_int * 1)(0), 1, out) == ERR_ARG
    assert lib.mjx_linear_moments(None, None, None) == ERR_ARG and lib.mjx_npg_update_linear(None, 10, 1e-4, 1e-10, 0.05, float("nan"), -3.0,
                                                                                             None, None, None, None, None, None) == ERR_ARG
