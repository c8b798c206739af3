"""The team ensemble fit, host side (no GPU): the route table of mjx_dyn_fit_team_route, nn_dynamics.team_fit_shape against it,
the entry fit_ensemble picks, and -- from the fp64 oracle alone -- that the data recipe of tests/_dyn_fit_team_cases.py leaves at
most ILL_SHARE of any case's parameters below the gradient floor (the GPU test leaves those out of its comparison)."""
import ctypes

import numpy as np
import pytest

from tests import _dyn_oracle as O
from tests._dyn_fit_team_cases import CASES, GRAD_FLOOR, ILL_SHARE, LR, WD, member_data


def _route(sizes, batch, tmode=2, K=4):
    from mjrl_amd import _lib
    return _lib.load().mjx_dyn_fit_team_route((ctypes.c_int * len(sizes))(*sizes), len(sizes), batch, tmode, K)


# sizes, batch, target mode -> G; the last column: whether team_fit_shape takes the sizes.  It knows the widths alone and, of the
# served ones, takes the teams of four: a team of two lost to the one-workgroup kernel where it was measured (64 x 64)
TABLE = [([13, 64, 64, 11], 16, 2, 2, False), ([13, 128, 128, 11], 16, 2, 4, True), ([13, 192, 192, 11], 16, 1, 2, False),
         ([13, 256, 256, 11], 64, 2, 4, True), ([13, 128, 256, 11], 64, 2, 4, True), ([13, 128, 192, 11], 64, 2, 2, False),
         ([13, 96, 96, 11], 16, 2, 0, False), ([13, 64, 96, 11], 16, 2, 0, False), ([13, 64, 64, 64, 11], 16, 2, 0, False),
         ([13, 320, 320, 11], 16, 2, 0, False), ([13, 128, 128, 11], 65, 2, 0, True), ([13, 128, 128, 11], 16, 0, 0, True),
         ([13, 64, 0, 11], 16, 2, -1, False), ([13], 16, 2, -1, False), ([13, 128, 128, 11], 0, 2, -1, True), ([13, 128, 128, 11], 16, 3, -1, True)]


@pytest.mark.parametrize("sizes, batch, tmode, G, py", TABLE)
def test_team_route_table(sizes, batch, tmode, G, py):
    from mjrl_amd.algos.model_accel.nn_dynamics import team_fit_shape
    assert _route(sizes, batch, tmode) == G
    assert team_fit_shape(sizes) == py


@pytest.mark.parametrize("hidden, team, entry", [((128, 128), False, "mjx_dyn_fit_ensemble"), ((128, 128), True, "mjx_dyn_fit_ensemble_team"),
                                                 ((96, 96), True, "mjx_dyn_fit_ensemble")])
def test_fit_ensemble_picks_the_entry(monkeypatch, hidden, team, entry):
    from mjrl_amd.algos.model_accel import nn_dynamics as D
    seen = []
    monkeypatch.setattr(D, "_fit_members", lambda *args: seen.append(args[8]) or [[], []])
    models = [D.WorldModel(6, 2, hidden_size=hidden, seed=k) for k in range(2)]
    s, a = np.zeros((40, 6), np.float32), np.zeros((40, 2), np.float32)
    D.fit_ensemble(models, s, a, s, 16, 1, set_transformations=False, team=team)
    D.fit_world_models(models, s, a, s, None, 16, 1, set_transformations=False, team=team)
    assert seen == [entry, entry]


@pytest.mark.parametrize("name, sizes, batch, act, tmode, K, G", CASES)
def test_recipe_keeps_the_comparison_full(name, sizes, batch, act, tmode, K, G):
    assert _route(sizes, batch, tmode, K) == G and _route(sizes, batch, tmode, 0) < 0
    for k in range(K):
        th, tr, x, y, idx = member_data(name, sizes, batch, k)
        g1 = np.zeros(th.size)
        O.adam_steps(th, sizes, tr, x, y, idx[:batch], batch, act, tmode, LR, WD, g_first=g1)
        assert np.mean(g1 < GRAD_FLOOR) <= ILL_SHARE, (name, k, float(np.mean(g1 < GRAD_FLOOR)))
