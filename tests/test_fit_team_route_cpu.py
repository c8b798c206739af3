"""mjx_mlp_fit_route for minibatches of 128 .. 512 rows (no GPU): the team trainer (csrc/mlp_fit_team.h) takes 128 x 128 at batch
128, 192 .. 512 while the two-halves layout fits LDS, with register-resident moments; everything else keeps its route."""
import ctypes

import pytest

from tests._worker_dev import ints

LAUNCHES, TEAM, SITE_LAUNCHES, SITE_TEAM = 0, 4, 4, 13
NONE = [LAUNCHES, 0, 0, 0, 0, SITE_LAUNCHES]
SWITCHES = ("MJX_MLP_FIT_LAUNCHES", "MJX_FIT_WIDE", "MJX_FIT_REGMOM", "MJX_FIT_ONEPASS", "MJX_FIT_TEAM")


def _route(d_in, batch, N=None, hidden=(128, 128), epochs=1):
    from mjrl_amd import _lib
    out = (ctypes.c_int32 * 6)()
    assert _lib.load().mjx_mlp_fit_route(d_in, ints(hidden), len(hidden), batch, 4 * batch if N is None else N, epochs, out) == 0
    return [int(x) for x in out]


@pytest.fixture
def env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("d_in,nf1", [(9, 1), (43, 2)])
@pytest.mark.parametrize("batch", [128, 192, 256, 512])
def test_team_rows(env, d_in, nf1, batch):
    r = _route(d_in, batch)
    assert r[:4] == [TEAM, nf1, 1, batch // 64] and 0 < r[4] <= 160 * 1024 and r[5] == SITE_TEAM, r
    assert _route(d_in, batch, N=2 * batch)[0] == TEAM and _route(d_in, batch, N=2 * batch - 1) == NONE      # one step / none


def test_rows_that_keep_the_launch_route(env):
    for batch in (96, 160, 576):
        assert _route(9, batch) == NONE, batch
    assert _route(55, 128)[:2] == [TEAM, 2] and _route(56, 128) == NONE
    assert _route(9, 256, hidden=(64, 64)) == NONE and _route(9, 256, epochs=0) == NONE


@pytest.mark.parametrize("switch,value", [("MJX_FIT_TEAM", "0"), ("MJX_FIT_REGMOM", "0"), ("MJX_MLP_FIT_LAUNCHES", "1")])
def test_switches_send_the_team_rows_to_launches(env, switch, value):
    assert _route(24, 256)[0] == TEAM
    env.setenv(switch, value)
    assert _route(24, 256) == NONE


def test_team_switch_leaves_batch_64_alone(env):
    ds = (1, 23, 24, 31, 32, 55, 56, 97, 768, 769)
    base = [_route(d, 64) for d in ds]
    env.setenv("MJX_FIT_TEAM", "0")
    assert [_route(d, 64) for d in ds] == base
