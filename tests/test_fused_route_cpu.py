"""mjx_fused_route, host side (no GPU): which fused instance would serve a shape, read from the one instance table of
csrc/fused_host.h without a context or a device."""
import ctypes

from tests.test_gpu_fused_matrix import INSTANCES

ERR_ARG = -1
FIRST_N_OFF_64 = 24     # 64 x 64 with up to 8 actions: 23 observations need 161 888 bytes of LDS, 24 more than 160 KiB


def _lib():
    from mjrl_amd import _lib
    return _lib.load()


def _route(n, m, hidden):
    out = (ctypes.c_int32 * 4)()
    rc = _lib().mjx_fused_route(n, m, (ctypes.c_int * max(len(hidden), 1))(*hidden), len(hidden), out)
    assert rc == 0, rc
    return [int(x) for x in out]


def test_fused_route_table():
    """mjx_fused_route is arithmetic alone: every shape of the fused matrix gets the instance it is named for, with an
    accumulator-order slab; the layer-wise route (all four outputs 0) for one or three hidden layers, unequal or wide layers, more
    actions or observations than the 32 x 32 instances take, and the first observation count at which the 64 x 64 layout with up to
    8 actions no longer fits LDS; null pointers are argument errors"""
    for variant, npc, hid, shapes in INSTANCES:
        for n, m in shapes:
            v, c, dr, nbytes = _route(n, m, hid)
            assert (v, c) == (variant, npc), (hid, n, m, v, c)
            assert dr > 0 and dr % 4 == 0, (hid, n, m, dr)
            assert 0 < nbytes <= 160 * 1024, (hid, n, m, nbytes)
    assert _route(17, 16, (64, 64))[3] == 163840           # exactly at the limit
    for n, m, hid in [(17, 6, (64,)), (17, 6, (64, 64, 64)), (17, 6, (64, 32)), (17, 6, (32, 64)), (17, 6, (128, 128)),
                      (17, 33, (32, 32)), (64, 6, (32, 32)), (FIRST_N_OFF_64, 6, (64, 64))]:
        assert _route(n, m, hid) == [0, 0, 0, 0], (n, m, hid)
    assert _route(FIRST_N_OFF_64 - 1, 6, (64, 64))[0] == 1
    assert _route(17, 6, ())[0] == 0                        # no hidden layer: a null list is fine with n_hidden == 0
    lib = _lib()
    out = (ctypes.c_int32 * 4)()
    hid = (ctypes.c_int * 2)(64, 64)
    assert lib.mjx_fused_route(17, 6, hid, 2, None) == ERR_ARG
    assert lib.mjx_fused_route(17, 6, None, 2, out) == ERR_ARG
    assert lib.mjx_fused_route(0, 6, hid, 2, out) == ERR_ARG
    assert lib.mjx_fused_route(17, 6, (ctypes.c_int * 2)(64, 0), 2, out) == ERR_ARG
