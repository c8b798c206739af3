"""mjx_linear_route_wide, host side (no GPU): route 2, the wide Gram route of csrc/linear_policy_wide.h, for no hidden layer
with 64 <= n <= 127 and m <= 32; mjx_linear_route's answer for everything else and under MJX_LINEAR_GRAM_WIDE=0."""
import ctypes

import pytest

ERR_ARG = -1


def _lib():
    from mjrl_amd import _lib
    return _lib.load()


def _route(n, m, hidden=(), entry="mjx_linear_route_wide"):
    out = (ctypes.c_int32 * 4)()
    assert getattr(_lib(), entry)(n, m, (ctypes.c_int * max(len(hidden), 1))(*hidden), len(hidden), out) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("n", [63, 64, 95, 96, 127, 128])
@pytest.mark.parametrize("m", [1, 32, 33])
def test_wide_route_and_its_layout(n, m):
    """route 2 with NP = 96 up to n = 95 and 128 beyond, the LDS bytes of pass 1's own arithmetic (one [W | b] image and four
    wave tiles of 32 x (NP + 4), 2 NP column and 5 x 32 action values) within 160 KiB, chains of 1024 rows at the most"""
    if 64 <= n <= 127 and m <= 32:
        NP = 96 if n <= 95 else 128
        lds = 4 * (5 * 32 * (NP + 4) + 2 * NP + 5 * 32)
        assert lds <= 163840 and _route(n, m) == [2, NP, lds, 1024]
    else:
        assert _route(n, m) == _route(n, m, entry="mjx_linear_route")
        assert _route(n, m)[0] == (1 if n == 63 and m <= 32 else 0)


def test_hidden_layer_switches_and_arguments(monkeypatch):
    lib, out = _lib(), (ctypes.c_int32 * 4)()
    assert _route(111, 8, (64,)) == [0, 0, 0, 0]
    monkeypatch.setenv("MJX_LINEAR_GRAM_WIDE", "0")        # read per call
    assert _route(111, 8) == [0, 0, 0, 0] and _route(17, 6)[0] == 1
    monkeypatch.delenv("MJX_LINEAR_GRAM_WIDE")
    monkeypatch.setenv("MJX_LINEAR_GRAM", "0")
    assert _route(111, 8) == [0, 0, 0, 0] and _route(17, 6) == [0, 0, 0, 0]
    monkeypatch.delenv("MJX_LINEAR_GRAM")
    assert _route(111, 8)[0] == 2
    assert lib.mjx_linear_route_wide(111, 8, None, 0, None) == ERR_ARG
    assert lib.mjx_linear_route_wide(111, 8, None, 1, out) == ERR_ARG
    assert lib.mjx_linear_route_wide(0, 8, None, 0, out) == ERR_ARG
    nan = float("nan")
    assert lib.mjx_linear_moments_wide(None, None, None) == ERR_ARG
    assert lib.mjx_npg_update_linear_wide(None, 10, 1e-4, 1e-10, 0.05, nan, -3.0, None, None, None, None, None, None) == ERR_ARG
    assert lib.mjx_trpo_update_linear_wide(None, 10, 1e-4, 1e-10, 0.05, 0.025, 100, -3.0, None, None, None, None, None, None) == ERR_ARG
