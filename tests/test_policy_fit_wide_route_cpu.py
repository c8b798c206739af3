"""The route ladder of mjx_policy_minibatch_adam_wide, host side (no GPU): mjx_policy_fit_wide_route answers {route, H, bytes} by
arithmetic alone -- 1 = k_policy_fit where mjx_policy_fit_route serves, 2 = k_policy_fit_wide (csrc/policy_fit_wide.h) from its own
layout struct, 0 = per-step launches -- under MJX_POLICY_FIT_WIDE and MJX_NO_POLICY_FIT, both read per call."""
import ctypes

import pytest

from tests._worker_dev import ints as _ints

ERR_ARG, LDS_MAX = -1, 160 * 1024
MODES = ((0, 1), (1, 1), (2, 1), (2, 0))         # (loss, old_tracks_new); the last keeps a second parameter image in LDS
# the last B served at (48, 32, 64 x 64), from the layout's arithmetic: without the old network's image B 64 takes 144 800 bytes; with
# it B 32 takes 145 056 and B 36 (48 padded rows) more than 160 KiB
LAST_B = {(0, 1): (64, 144800), (1, 1): (64, 144800), (2, 1): (64, 144800), (2, 0): (32, 145056)}


def _route(n, m, hidden, B, loss=0, old_tracks_new=0, wide=True):
    from mjrl_amd import _lib
    lib, out = _lib.load(), (ctypes.c_int32 * 3)()
    entry = lib.mjx_policy_fit_wide_route if wide else lib.mjx_policy_fit_route
    assert entry(n, m, _ints(hidden), len(hidden), B, loss, old_tracks_new, out) == 0
    return [int(x) for x in out][:3 if wide else 2]


@pytest.fixture
def default_switches(monkeypatch):
    monkeypatch.delenv("MJX_NO_POLICY_FIT", raising=False)
    monkeypatch.delenv("MJX_POLICY_FIT_WIDE", raising=False)
    return monkeypatch


def test_ladder_and_last_b_landmarks(default_switches):
    old = _route(11, 3, (64, 64), 64, wide=False)
    assert old[0] == 64 and _route(11, 3, (64, 64), 64) == [1] + old
    for n, m, H, B in ((39, 28, 32, 64), (33, 3, 32, 8), (11, 17, 64, 8), (64, 3, 64, 8)):
        r = _route(n, m, (H, H), B)
        assert r[:2] == [2, H] and 0 < r[2] <= LDS_MAX and _route(n, m, (H, H), B, wide=False) == [0, 0], (n, m, H, B, r)
    for n, m, hidden, B in ((65, 3, (64, 64), 8), (11, 33, (64, 64), 8), (11, 3, (128, 128), 8), (39, 28, (64, 32), 8), (39, 28, (32, 32), 68),
                            (39, 28, (32, 32), 10), (39, 28, (32,), 8), (39, 28, (), 8)):
        assert _route(n, m, hidden, B) == [0, 0, 0], (n, m, hidden, B)
    for (loss, otn), (last, nbytes) in LAST_B.items():
        assert _route(48, 32, (64, 64), last, loss, otn) == [2, 64, nbytes], (loss, otn)
        assert _route(48, 32, (64, 64), last + 4, loss, otn) == [0, 0, 0], (loss, otn)


@pytest.mark.parametrize("H, B, modes", [(32, 64, MODES), (64, 32, MODES[:3])])
def test_must_serve_table(default_switches, H, B, modes):
    # every n <= 48, m <= 32: route 2 wherever the older trainer does not take the shape, and never the launches
    for loss, otn in modes:
        for n in range(1, 49):
            for m in range(1, 33):
                r = _route(n, m, (H, H), B, loss, otn)
                want = 1 if _route(n, m, (H, H), B, loss, otn, wide=False)[0] else 2
                assert r[:2] == [want, H] and r[2] <= LDS_MAX, (n, m, loss, otn, r)


def test_switches_and_arguments(default_switches):
    mp = default_switches
    mp.setenv("MJX_POLICY_FIT_WIDE", "0")
    assert _route(39, 28, (32, 32), 64) == [0, 0, 0] and _route(11, 3, (64, 64), 64)[0] == 1
    mp.delenv("MJX_POLICY_FIT_WIDE")
    mp.setenv("MJX_NO_POLICY_FIT", "1")
    assert _route(39, 28, (32, 32), 64) == [0, 0, 0] and _route(11, 3, (64, 64), 64) == [0, 0, 0]
    mp.delenv("MJX_NO_POLICY_FIT")
    assert _route(39, 28, (32, 32), 64)[0] == 2
    from mjrl_amd import _lib
    lib, out, h2 = _lib.load(), (ctypes.c_int32 * 3)(), _ints((32, 32))
    assert lib.mjx_policy_fit_wide_route(39, 28, h2, 2, 64, 0, 0, None) == ERR_ARG
    assert lib.mjx_policy_fit_wide_route(39, 28, None, 2, 64, 0, 0, out) == ERR_ARG
    assert lib.mjx_policy_minibatch_adam_wide(None, 0, None, None, None, None, 1, 32, None, None, None, None, 0, None, None, 0, 1e-3, 0.2,
                                              None, None, None) == ERR_ARG
