"""The routes of the baseline, minibatch, dynamics and planning entries, host side (no GPU): mjx_bl_gram_route, mjx_mlp_fit_route,
mjx_policy_fit_route, mjx_dyn_fit_route and mjx_plan_route answer "which kernel serves this shape" by arithmetic alone, from the
tables of csrc/fit_host.h and csrc/model_host.h.  Every boundary below was read off the build before those headers existed
(the same conditions, then inline in mjx_mlp_fit_adam / mjx_policy_minibatch_adam), not off the tables."""
import ctypes

import pytest

from tests._worker_dev import ints as _ints

ERR_ARG = -1
LAUNCHES, HALVES, ONEPASS, WIDE = 0, 1, 2, 3       # out6[0] of mjx_mlp_fit_route
SITE_ONE_WG, SITE_WIDE, SITE_LAUNCHES = 2, 3, 4     # out6[5]: the scratch block of the route (ScratchSite, csrc/mjx.hip)
LAST_D_ONEPASS = 23        # the route's own rule, d_in <= 23 (the one-pass layout of 23 inputs takes 159 888 bytes of LDS)
LAST_D_NF1 = 31            # one 32-feature block of the input layer's weight gradient holds 31 inputs + the bias column
LAST_D_ONE_WG = 55         # two-halves layout: 55 inputs need 162 448 bytes, 56 more than 160 KiB (163 840)
LAST_D_WIDE = 768          # 16 workgroups x 48-feature slices
WIDE_BYTES = 159824        # the layout of one 48-feature slice, whatever d_in
LAST_B_OLD_NET = 16        # policy fit at n 63, m 16, H 64 with the old network's image in LDS: B 16 needs 149 120 bytes, B 20 too many
LAST_B_NO_OLD_NET = 48     # ... without it: B 48 needs 163 584 bytes, B 52 too many
SWITCHES = ("MJX_MLP_FIT_LAUNCHES", "MJX_FIT_WIDE", "MJX_FIT_REGMOM", "MJX_FIT_ONEPASS")


def _lib():
    from mjrl_amd import _lib
    return _lib.load()


def _mlp(d_in, hidden=(128, 128), batch=64, N=192, epochs=2):
    out = (ctypes.c_int32 * 6)()
    rc = _lib().mjx_mlp_fit_route(d_in, _ints(hidden), len(hidden), batch, N, epochs, out)
    assert rc == 0, rc
    return [int(x) for x in out]


def _policy(n, m, H, B, loss=0, old_tracks_new=0, hidden=None):
    hidden = (H, H) if hidden is None else hidden
    out = (ctypes.c_int32 * 2)()
    rc = _lib().mjx_policy_fit_route(n, m, _ints(hidden), len(hidden), B, loss, old_tracks_new, out)
    assert rc == 0, rc
    return [int(x) for x in out]


@pytest.fixture
def default_switches(monkeypatch):
    for name in SWITCHES + ("MJX_NO_POLICY_FIT",):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_mlp_fit_route_table(default_switches):
    """kind, NF1, REGMOM, workgroups, LDS bytes and scratch site over d_in at the reference's shape (128 x 128, batch 64)"""
    assert _mlp(LAST_D_ONEPASS) == [ONEPASS, 1, 1, 1, 159888, SITE_ONE_WG]
    assert _mlp(LAST_D_ONEPASS + 1) == [HALVES, 1, 1, 1, 147920, SITE_ONE_WG]
    assert _mlp(LAST_D_NF1) == [HALVES, 1, 1, 1, 151056, SITE_ONE_WG]
    assert _mlp(LAST_D_NF1 + 1) == [HALVES, 2, 1, 1, 149328, SITE_ONE_WG]
    assert _mlp(LAST_D_ONE_WG) == [HALVES, 2, 1, 1, 162448, SITE_ONE_WG]
    assert _mlp(LAST_D_ONE_WG + 1) == [WIDE, 2, 1, 2, WIDE_BYTES, SITE_WIDE]
    assert _mlp(96)[3] == 2 and _mlp(97)[3] == 3                       # ceil(d_in / 48) workgroups
    assert _mlp(LAST_D_WIDE) == [WIDE, 2, 1, 16, WIDE_BYTES, SITE_WIDE]
    assert _mlp(LAST_D_WIDE + 1) == [LAUNCHES, 0, 0, 0, 0, SITE_LAUNCHES]
    for d in range(1, 801):
        r = _mlp(d)
        want = ONEPASS if d <= LAST_D_ONEPASS else HALVES if d <= LAST_D_ONE_WG else WIDE if d <= LAST_D_WIDE else LAUNCHES
        assert r[0] == want, (d, r)
        # (G <= 16 is seen at 768 / 769; the route's d_in > 48 clause cannot be: 49 .. 55 inputs already take the one-workgroup route)
        assert (r[0] == WIDE) == (r[3] > 1) and r[4] <= 160 * 1024, (d, r)
        assert r[3] == (0 if want == LAUNCHES else 1 if want != WIDE else (d + 47) // 48), (d, r)


def test_mlp_fit_route_other_shapes_take_the_launch_route(default_switches):
    """anything but 128 x 128 at batch 64 with at least one step and one epoch"""
    none = [LAUNCHES, 0, 0, 0, 0, SITE_LAUNCHES]
    for d in (5, 40, 60):
        assert _mlp(d)[0] != LAUNCHES
        for hidden in ((64, 64), (128,), (128, 128, 128), (128, 64), (64, 128), ()):
            assert _mlp(d, hidden=hidden) == none, (d, hidden)
        for batch in (8, 32, 63, 65):
            assert _mlp(d, batch=batch, N=4096) == none, (d, batch)
        assert _mlp(d, N=64) == none and _mlp(d, N=127) == none           # N / 64 - 1 = 0 steps
        assert _mlp(d, N=128)[0] != LAUNCHES                               # one step
        assert _mlp(d, epochs=0) == none
        assert _mlp(d, epochs=1)[0] != LAUNCHES


def test_mlp_fit_switches_flip_their_rows_only(default_switches):
    """MJX_MLP_FIT_LAUNCHES=1: every row; MJX_FIT_WIDE=0: the wide rows; MJX_FIT_REGMOM=0: REGMOM everywhere and, with it, the one-pass
    rows (that trainer has register-resident moments only); MJX_FIT_ONEPASS=0: the one-pass rows.  Read per call."""
    ds = list(range(1, 70)) + [96, 97, 400, 768, 769]
    base = {d: _mlp(d) for d in ds}
    mp = default_switches
    mp.setenv("MJX_MLP_FIT_LAUNCHES", "1")
    for d in ds:
        assert _mlp(d) == [LAUNCHES, 0, 0, 0, 0, SITE_LAUNCHES], d
    mp.delenv("MJX_MLP_FIT_LAUNCHES")
    mp.setenv("MJX_FIT_WIDE", "0")
    for d in ds:
        assert _mlp(d) == ([LAUNCHES, 0, 0, 0, 0, SITE_LAUNCHES] if base[d][0] == WIDE else base[d]), d
    mp.delenv("MJX_FIT_WIDE")
    mp.setenv("MJX_FIT_REGMOM", "0")
    for d in ds:
        b = base[d]
        got = _mlp(d)
        if b[0] == ONEPASS:
            assert got[:4] == [HALVES, 1, 0, 1] and got[5] == SITE_ONE_WG, d
        else:
            assert got == (b if b[0] == LAUNCHES else b[:2] + [0] + b[3:]), d
    assert _mlp(5)[4] == 132240 and _mlp(LAST_D_ONEPASS)[4] == 144784       # the two-halves layouts of 5 and 23 inputs
    mp.delenv("MJX_FIT_REGMOM")
    mp.setenv("MJX_FIT_ONEPASS", "0")
    for d in ds:
        b = base[d]
        got = _mlp(d)
        assert (got == b) if b[0] != ONEPASS else (got[:4] == [HALVES, 1, 1, 1] and got[5] == SITE_ONE_WG), d
    assert _mlp(5)[4] == 132240 and _mlp(LAST_D_ONEPASS)[4] == 144784
    mp.delenv("MJX_FIT_ONEPASS")
    assert all(_mlp(d) == base[d] for d in ds)


def test_policy_fit_route_limits(default_switches):
    """H in {32, 64} twice; 8 <= B <= 64 in fours; n <= min(H, 63); m <= 16; the layout within 160 KiB, with and without the old
    network's parameter image (PPO whose old network does not track the new one)"""
    assert _policy(11, 3, 64, 64) == [64, 146592]
    assert _policy(11, 3, 32, 8) == [32, 33568]
    for hidden in ((128, 128), (16, 16), (64, 32), (32, 64), (64,), (64, 64, 64), ()):
        assert _policy(11, 3, 0, 64, hidden=hidden) == [0, 0], hidden
    for B in range(1, 70):
        assert (_policy(11, 3, 64, B)[0] == 64) == (B % 4 == 0 and 8 <= B <= 64), B
        assert (_policy(11, 3, 32, B)[0] == 32) == (B % 4 == 0 and 8 <= B <= 64), B
    assert _policy(63, 3, 64, 8)[0] == 64 and _policy(64, 3, 64, 8) == [0, 0]
    assert _policy(32, 3, 32, 8)[0] == 32 and _policy(33, 3, 32, 8) == [0, 0]
    assert _policy(11, 16, 64, 8)[0] == 64 and _policy(11, 17, 64, 8) == [0, 0]
    assert _policy(32, 16, 32, 64, loss=2) == [32, 105856] and _policy(32, 16, 32, 64, loss=2, old_tracks_new=1) == [32, 93952]
    for loss in (0, 1, 2):
        for otn in (0, 1):
            old_net = loss == 2 and not otn
            last = LAST_B_OLD_NET if old_net else LAST_B_NO_OLD_NET
            assert _policy(63, 16, 64, last, loss, otn) == [64, 149120 if old_net else 163584], (loss, otn)
            assert _policy(63, 16, 64, last + 4, loss, otn) == [0, 0], (loss, otn)
    default_switches.setenv("MJX_NO_POLICY_FIT", "1")
    assert _policy(11, 3, 64, 64) == [0, 0] and _policy(11, 3, 32, 8) == [0, 0]


def test_dyn_fit_and_plan_routes_still_answer(default_switches):
    """the two older read-only entries, through the same host header: a landmark on each side of every limit"""
    lib = _lib()

    def fit(sizes, batch, tmode=2):
        return lib.mjx_dyn_fit_route(_ints(sizes), len(sizes), batch, tmode)

    def plan(sizes, m):
        return lib.mjx_plan_route(_ints(sizes), len(sizes), m)

    assert fit([13, 256, 256, 11], 64) == 1 and fit([13, 288, 256, 11], 64) == 0 and fit([13, 48, 64, 11], 16) == 0
    assert fit([13, 64, 64, 11], 65) == 0 and fit([128, 64, 64, 64], 16) == 1 and fit([129, 64, 64, 11], 16) == 0
    assert fit([128, 64, 64, 65], 16) == 0 and fit([13, 64, 11], 16) == 0 and fit([13, 64, 64, 11], 16, 0) == 0
    assert fit([13, 64, 64, 11], 0) == ERR_ARG and fit([13, 64, 64, 11], 16, 3) == ERR_ARG and fit([13], 16) == ERR_ARG
    assert plan([8, 32, 32, 6], 2) == 1 and plan([96, 128, 128, 64], 32) == 1 and plan([97, 128, 128, 64], 33) == 0
    assert plan([8, 160, 160, 6], 2) == 0 and plan([8, 100, 100, 6], 2) == 0 and plan([67, 64, 64, 65], 2) == 0
    assert plan([8, 64, 64, 64, 6], 2) == 0 and plan([8, 64, 64, 6], 3) == ERR_ARG and plan([8], 2) == ERR_ARG


GRAM_MFMA, GRAM_BLK, GRAM_FMA = 0, 1, 2              # out6[0] of mjx_bl_gram_route


def _gram(kind, n, N=1000):
    out = (ctypes.c_int32 * 6)()
    rc = _lib().mjx_bl_gram_route(kind, n, N, out)
    assert rc == 0, rc
    return [int(x) for x in out]


def _feats(kind, n):
    return n + 4 if kind == 0 else n + 5 if kind == 1 else n + n * (n + 1) // 2 + 5


def test_gram_route_arms_by_shape(default_switches):
    """csrc/fit_host.h gram_route, read off its conditions: the one-workgroup matrix-core kernel while the augmented features fill at
    most 11 tiles of 16 (176 columns) and 32 n observations fit its 3 x 256 staging slots (n <= 24); the 128 x 128 block kernel while
    they fit its 8 x 256 slots (n <= 64); the FMA kernel beyond, and for every shape under MJX_GRAM_FMA=1 (read per call).
    out6 = {arm, Z, blocks a side, grid x, features a side of a reduce tile, bytes of LDS}."""
    default_switches.delenv("MJX_GRAM_FMA", raising=False)
    assert _feats(2, 17) + 1 == 176 and _feats(2, 18) + 1 == 195
    for kind in (0, 1, 2):
        for n in range(1, 140):
            FA = _feats(kind, n) + 1
            want = GRAM_MFMA if FA <= 176 and n <= 24 else GRAM_BLK if n <= 64 else GRAM_FMA
            r = _gram(kind, n)
            assert r[0] == want, (kind, n, r)
            if want == GRAM_MFMA:
                assert r[2:5] == [0, 1, 16], (kind, n, r)
            elif want == GRAM_BLK:
                nb = -(-FA // 128)
                assert r[2:5] == [nb, nb * (nb + 1) // 2, 128], (kind, n, r)
            else:
                nbt = -(-FA // 64)
                assert r[2:5] == [nbt, nbt * (nbt + 1) // 2, 64], (kind, n, r)
    # the landmarks by name: quadratic 17 / 18, linear and MLP features 24 / 25 and 64 / 65
    assert _gram(2, 17)[0] == GRAM_MFMA and _gram(2, 18)[0] == GRAM_BLK
    for kind in (0, 1):
        assert _gram(kind, 24)[0] == GRAM_MFMA and _gram(kind, 25)[0] == GRAM_BLK
    for kind in (0, 1, 2):
        assert _gram(kind, 64)[0] == GRAM_BLK and _gram(kind, 65)[0] == GRAM_FMA
    assert _gram(2, 64)[2:4] == [17, 153] and _gram(2, 18)[2:4] == [2, 3] and _gram(2, 21)[2:4] == [3, 6]      # 2150, 195, 258 columns
    assert _gram(2, 65)[2:4] == [35, 630]
    default_switches.setenv("MJX_GRAM_FMA", "1")
    for kind in (0, 1, 2):
        for n in (1, 3, 17, 18, 24, 25, 64, 65):
            assert _gram(kind, n)[0] == GRAM_FMA and _gram(kind, n)[4] == 64, (kind, n)
    default_switches.setenv("MJX_GRAM_FMA", "0")
    assert _gram(2, 17)[0] == GRAM_MFMA
    default_switches.delenv("MJX_GRAM_FMA")
    assert _gram(2, 17)[0] == GRAM_MFMA                      # read per call


def test_gram_route_sample_ranges(default_switches):
    """Z = clamp(ceil(N / per), 1, cap): 2048 rows a range and at most 512 on the one-workgroup arm; 2048 and ceil(768 / block pairs)
    on the block arm; 4096 and ceil(2048 / tile pairs) on the FMA arm"""
    mp = default_switches
    mp.delenv("MJX_GRAM_FMA", raising=False)

    def z(per, cap, N):
        return max(1, min(cap, -(-N // per)))

    Ns = (1, 2047, 2048, 2049, 4096, 4097, 8193, 2048 * 255 + 1, 2048 * 256, 2048 * 256 + 1, 2048 * 512, 2048 * 512 + 1, 4096 * 683 + 1,
          2000000, 10 ** 9, 2 ** 40)
    for N in Ns:
        assert _gram(2, 17, N)[1] == z(2048, 512, N) and _gram(1, 1, N)[1] == z(2048, 512, N), N
        assert _gram(1, 25, N)[1] == z(2048, 768, N), N                     # 31 columns: one diagonal block
        assert _gram(2, 18, N)[1] == z(2048, 256, N), N                     # 3 block pairs
        assert _gram(2, 21, N)[1] == z(2048, 128, N), N                     # 6 block pairs
        assert _gram(2, 64, N)[1] == z(2048, 6, N), N                       # 153 block pairs: ceil(768 / 153) = 6
        assert _gram(1, 65, N)[1] == z(4096, 683, N), N                     # 71 columns: 3 tile pairs, ceil(2048 / 3) = 683
        assert _gram(2, 65, N)[1] == z(4096, 4, N), N                       # 630 tile pairs
    assert _gram(2, 17, 2048)[1] == 1 and _gram(2, 17, 2049)[1] == 2 and _gram(2, 17, 4097)[1] == 3
    assert _gram(1, 1, 2000000)[1] == 512 and _gram(2, 18, 530000)[1] == 256
    mp.setenv("MJX_GRAM_FMA", "1")
    for N in Ns:
        assert _gram(2, 3, N)[1] == z(4096, 2048, N), N                     # 15 columns: one tile pair
        assert _gram(2, 17, N)[1] == z(4096, 342, N), N                     # 176 columns: 3 tiles a side, 6 pairs
        assert _gram(1, 59, N)[1] == z(4096, 683, N), N                     # 65 columns: 2 tiles a side, 3 pairs
    assert _gram(1, 58, 1)[2:4] == [1, 1] and _gram(1, 59, 1)[2:4] == [2, 3]


def test_gram_route_lds_bytes_at_the_ends_of_each_arm(default_switches):
    """one workgroup: 32 extended vectors of n + 7 doubles and 32 feature rows of 16 (T | 1); blocks: the vectors and two 32 x 144
    feature blocks; FMA: 32 x n observations and two 32 x 65 tiles (its 32 tau values are static)"""
    mp = default_switches
    mp.delenv("MJX_GRAM_FMA", raising=False)
    assert _gram(0, 1)[5] == 8 * (32 * 8 + 32 * 16 * 1)                     # 6 columns: one tile                      6 144
    assert _gram(2, 1)[5] == 8 * (32 * 8 + 32 * 16 * 1) == 6144
    assert _gram(2, 4)[5] == 8 * (32 * 11 + 32 * 16 * 3)                    # 20 columns: 2 tiles, stride 3 x 16
    assert _gram(2, 17)[5] == 8 * (32 * 24 + 32 * 16 * 11) == 51200         # the arm's last quadratic shape
    assert _gram(1, 24)[5] == 8 * (32 * 31 + 32 * 16 * 3) == 20224          # ... and last linear one
    assert _gram(1, 25)[5] == 8 * (32 * 32 + 2 * 32 * 144) == 81920         # first and last shape of the block arm
    assert _gram(2, 18)[5] == 8 * (32 * 25 + 2 * 32 * 144) == 80128
    assert _gram(2, 64)[5] == 8 * (32 * 71 + 2 * 32 * 144) == 91904
    assert _gram(1, 65)[5] == 8 * (32 * 65 + 2 * 32 * 65) == 49920          # first shape only the FMA arm serves
    assert _gram(1, 126)[5] == 65536                                        # the last it serves: 64 KiB exactly
    assert _gram(1, 127)[5] == 65792                                        # mjx_bl_gram refuses this one
    assert _gram(2, 65)[5] == 49920                                         # (whatever the feature count)
    mp.setenv("MJX_GRAM_FMA", "1")
    assert _gram(2, 1)[5] == 8 * (32 * 1 + 2 * 32 * 65) == 33536
    assert _gram(2, 17)[5] == 8 * (32 * 17 + 2 * 32 * 65) == 37632


def test_gram_route_refuses_bad_arguments(default_switches):
    lib = _lib()
    out6 = (ctypes.c_int32 * 6)()
    assert lib.mjx_bl_gram_route(2, 17, 1000, out6) == 0
    assert lib.mjx_bl_gram_route(2, 17, 1000, None) == ERR_ARG
    for kind, n, N in ((-1, 17, 1000), (3, 17, 1000), (2, 0, 1000), (2, -5, 1000), (2, 4097, 1000), (2, 17, 0), (2, 17, -1)):
        assert lib.mjx_bl_gram_route(kind, n, N, out6) == ERR_ARG, (kind, n, N)


def test_route_entries_refuse_bad_arguments_without_device_work(default_switches):
    lib = _lib()
    before = (ctypes.c_int64 * 2)()
    lib.mjx_process_state(before)
    assert lib.mjx_bl_gram_route(2, 17, 1000, (ctypes.c_int32 * 6)()) == 0 and lib.mjx_bl_gram_route(7, 17, 1000, None) == ERR_ARG
    out6, out2, hid = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 2)(), _ints((128, 128))
    assert lib.mjx_mlp_fit_route(5, hid, 2, 64, 192, 2, None) == ERR_ARG
    assert lib.mjx_mlp_fit_route(5, None, 2, 64, 192, 2, out6) == ERR_ARG
    assert lib.mjx_mlp_fit_route(5, None, 0, 64, 192, 2, out6) == 0             # no hidden layer: a null list is fine
    for kw in (dict(d_in=0), dict(n_hidden=-1), dict(batch=0), dict(N=0), dict(epochs=-1), dict(hid=_ints((128, 0)))):
        a = dict(d_in=5, hid=hid, n_hidden=2, batch=64, N=192, epochs=2); a.update(kw)
        assert lib.mjx_mlp_fit_route(a["d_in"], a["hid"], a["n_hidden"], a["batch"], a["N"], a["epochs"], out6) == ERR_ARG, kw
    h2 = _ints((64, 64))
    assert lib.mjx_policy_fit_route(11, 3, h2, 2, 64, 0, 0, None) == ERR_ARG
    assert lib.mjx_policy_fit_route(11, 3, None, 2, 64, 0, 0, out2) == ERR_ARG
    for kw in (dict(n=0), dict(m=0), dict(n_hidden=-1), dict(B=0), dict(loss=-1), dict(loss=3), dict(hid=_ints((64, -1)))):
        a = dict(n=11, m=3, hid=h2, n_hidden=2, B=64, loss=0); a.update(kw)
        assert lib.mjx_policy_fit_route(a["n"], a["m"], a["hid"], a["n_hidden"], a["B"], a["loss"], 0, out2) == ERR_ARG, kw
    after = (ctypes.c_int64 * 2)()
    lib.mjx_process_state(after)
    assert after[0] == before[0]                    # no entry reached the HIP runtime
