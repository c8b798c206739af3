"""The checks of tests/test_gpu_fit_matrix.py can fail: fp64 oracle results with the defects a wrong minibatch-Adam trainer would
leave behind are flagged at the bars that module uses, and the same results rounded to fp32 pass.  Also, from the oracle alone:
every case of the matrix is well posed (few ill-conditioned parameters; PPO rows on both branches of the clip, advantages of
both signs, no likelihood ratio within 1e-4 of a clip boundary).  CPU only."""
import numpy as np
import pytest

from tests import _dyn_oracle as O
from tests import _fit_cases as K
from tests import _fit_oracle as F
from tests.test_gpu_fit_matrix import BARS

LR, CLIP = K.LR, K.CLIP
# v formed with `1.0f - 0.999f` (1.3e-5 low) next to bias corrections from the double betas
V_MIXED = O.ADAM_TORCH[:3] + (float(np.float32(1.0) - np.float32(0.999)),) + O.ADAM_TORCH[4:]
# ... and what the MLP-baseline trainers compute on every route: fp32 betas in 1 - beta AND in the bias corrections
B1F, B2F = np.float32(0.9), np.float32(0.999)
MLP_KERNELS = (float(B1F), float(np.float32(1.0) - B1F), float(B2F), float(np.float32(1.0) - B2F), float(B1F), float(B2F))


def _r32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _flags(kind, got, ref, blocks, well, skip_moments=()):
    """the checks of the GPU module that fail for got = (params, m, v, losses) against ref"""
    bad = []
    if not F.worst(F.param_errors(got[0], ref[0], blocks, LR, well))[0] < BARS[kind + "_params_over_lr"]:
        bad.append("params")
    mb = [b for b in blocks if b[0] not in skip_moments]
    if not F.worst(F.moment_errors(got[1], ref[1], mb))[0] < BARS[kind + "_m"]:
        bad.append("m")
    if not F.worst(F.moment_errors(got[2], ref[2], mb))[0] < BARS[kind + "_v"]:
        bad.append("v")
    if not F.rel_losses(got[3], ref[3]) < BARS[kind + "_loss"]:
        bad.append("loss")
    return bad


def _bias_flag(kind, v, ref_v, blocks):
    """the second-moment bias check of the one-step runs"""
    return not F.worst(F.moment_bias(v, ref_v, blocks))[0] < BARS[kind + "_v_bias"]


def _cont_flag(kind, p, ref, blocks, well):
    return not F.worst(F.param_errors(p, ref, blocks, LR, well))[0] < BARS[kind + "_cont_over_lr"]


# ---------------------------------------------------------------- MLP baseline
D_IN = 97                     # three slices of W1: 48, 48 and 1 feature


def _mlp(wd=1e-3, one_step=False, **kw):
    th, x, y, perm, perm1 = K.mlp_data(D_IN, (128, 128), 64, 11)
    if one_step:
        return th, F.mlp_fit(th, D_IN, x[:128], y[:128], perm1, 128, 1, LR, wd, **kw)
    return th, F.mlp_fit(th, D_IN, x, y, perm, K.N_MLP, 2, LR, wd, **kw)


def test_mlp_rounded_results_pass_and_defects_are_flagged():
    g1 = np.zeros(128 * D_IN + 128 + 128 * 128 + 128 + 128 + 1)
    th, ref = _mlp(g_first=g1)
    well, blocks = g1 >= F.GRAD_FLOOR, F.mlp_blocks(D_IN)
    assert [b[0] for b in blocks] == ["W1[:, 0:48]", "W1[:, 48:96]", "W1[:, 96:97]", "b1", "W2", "b2", "W3", "b3"]
    assert np.mean(~well) < BARS["fit_ill_conditioned"]
    assert _flags("mlp", [_r32(a) for a in ref], ref, blocks, well) == []

    assert "params" in _flags("mlp", _mlp(wd=0.0)[1], ref, blocks, well)                  # weight decay dropped
    # 1.0f - 0.999f: the baseline trainers form v with it on every route and correct with the fp32 betas as well.  That is
    # self-consistent -- the steps stay within 1e-5 lr of torch's -- and it is in the measured bars of v: on this trainer the
    # coefficient is a property of the kernels, 1.3e-5 in v, which these checks therefore cannot flag (the policy's do, below)
    own = _mlp(coef=MLP_KERNELS)[1]
    assert F.worst(F.param_errors(own[0], ref[0], blocks, LR, well))[0] < 1e-5
    assert 1.2e-5 < F.worst(F.moment_errors(own[2], ref[2], blocks))[0] < 1.5e-5
    ref1 = _mlp(one_step=True)[1]
    assert not _bias_flag("mlp", _r32(ref1[2]), ref1[2], blocks)
    assert 1.2e-5 < F.worst(F.moment_bias(_mlp(one_step=True, coef=MLP_KERNELS)[1][2], ref1[2], blocks))[0] < 1.4e-5
    for name in ("W1[:, 48:96]", "W1[:, 96:97]", "b1", "b3"):                             # a block left at its start value
        ix = dict(blocks)[name]
        got = [a.copy() for a in ref]
        got[0][ix] = th[ix]
        assert _flags("mlp", got, ref, blocks, well) == ["params"], name
    got = [a.copy() for a in ref]                                                          # one moment wrong in the one-feature slice
    got[2][dict(blocks)["W1[:, 96:97]"][5]] *= 1.001
    assert _flags("mlp", got, ref, blocks, well) == ["v"]
    got = [a.copy() for a in ref]
    got[3][1] *= 1.0 + 1e-4                                                                # an epoch loss short of one minibatch's rounding
    assert _flags("mlp", got, ref, blocks, well) == ["loss"]


@pytest.mark.parametrize("s0", [0, 12])
def test_mlp_bias_correction_off_by_one_is_flagged(s0):
    """the continuation at t0 = 5 and 17: a second call that numbers its steps one too low or one too high"""
    th, x, y, perm, _ = K.mlp_data(D_IN, (128, 128), 64, 12)
    N, blocks = K.N_MLP, F.mlp_blocks(D_IN)
    p1, m1, v1, _ = F.mlp_fit(th, D_IN, x, y, perm[:N], N, 1, LR, 1e-3, t0=s0)
    g1 = np.zeros(th.size)
    ref = F.mlp_fit(p1, D_IN, x, y, perm[N:], N, 1, LR, 1e-3, m=m1, v=v1, t0=s0 + 5, g_first=g1)[0]
    well = g1 >= F.GRAD_FLOOR
    ok = F.mlp_fit(_r32(p1), D_IN, x, y, perm[N:], N, 1, LR, 1e-3, m=_r32(m1), v=_r32(v1), t0=s0 + 5)[0]
    assert not _cont_flag("mlp", _r32(ok), ref, blocks, well)
    for t0 in (s0 + 4, s0 + 6):
        bad = F.mlp_fit(p1, D_IN, x, y, perm[N:], N, 1, LR, 1e-3, m=m1, v=v1, t0=t0)[0]
        assert _cont_flag("mlp", bad, ref, blocks, well), t0
        assert not F.worst(F.param_errors(bad, ref, blocks, LR, well))[0] < BARS["mlp_params_over_lr"], t0


# ---------------------------------------------------------------- policy
n, m, HID, B = 17, 6, (64, 64), 64
O_D = n * 64 + 64 + 64 * 64 + 64 + 64 * m + m + m


def _pol(loss, track, steps=10, **kw):
    D = K.pol_data(n, m, HID, B, 21)
    am, av = K.pol_moments(D, m, loss)
    kw.setdefault("am", am)
    kw.setdefault("av", av)
    idx = kw.pop("idx", D["idx"][:steps * B])
    return D, F.policy_fit(kw.pop("theta", D["theta"]), n, m, HID, D["tr"], D["theta_old"], D["tr_old"], D["obs"], D["act"], D["adv"], idx, B,
                           loss, track, LR, CLIP, **kw)


@pytest.mark.parametrize("loss,track", K.MODES)
def test_policy_rounded_results_pass_and_defects_are_flagged(loss, track):
    g1 = np.zeros(O_D)
    D, ref = _pol(loss, track, g_first=g1)
    blocks = F.policy_blocks(n, m, HID)
    well = g1 >= F.GRAD_FLOOR
    skip = ("log_std",) if loss == 0 else ()
    if loss == 0:
        well[-m:] = True
    flags = lambda got: _flags("pol", got[:4], ref, blocks, well, skip)
    assert flags([_r32(a) for a in ref[:4]]) == []
    ref1 = _pol(loss, track, steps=1)[1]                                                   # 1.0f - 0.999f under double corrections: under the
    assert not _bias_flag("pol", _r32(ref1[2]), ref1[2], blocks)                          #  element-wise bar of v, found in the sums
    assert _bias_flag("pol", _r32(_pol(loss, track, steps=1, coef=V_MIXED)[1][2]), ref1[2], blocks)
    for name in ("b1", "b3") + (() if loss == 0 else ("log_std",)):                       # a block not updated
        ix = dict(blocks)[name]
        got = [a.copy() for a in ref[:4]]
        got[0][ix] = D["theta"][ix]
        assert flags(got) == ["params"], name
    if loss == 0:
        assert flags(_pol(loss, track, defect="mse_over_B")[1])                           # MSE normalised by 1 / B
        got = [a.copy() for a in ref[:4]]                                                  # Adam run over log_std with a zero gradient
        got[0][-m:] -= LR * 0.9 * D["am_ls"] / np.sqrt(D["av_ls"])
        assert np.sum(_r32(got[0])[-m:] != D["theta"][-m:]) == m and flags(got) == ["params"]
    if loss == 1:
        assert "params" in flags(_pol(loss, track, defect="no_log_std_grad")[1])          # log_std without its gradient
    if loss == 2:
        assert ref[4]["clipped"] > 0 and ref[4]["unclipped"] > 0
        assert "params" in flags(_pol(loss, track, defect="no_clip_mask")[1])             # the clip mask ignored
    got = [a.copy() for a in ref[:4]]
    got[3][7] += 1e-4 * max(1.0, abs(got[3][7]))                                           # one entry of the loss trace
    assert flags(got) == ["loss"]


@pytest.mark.parametrize("loss,track", K.MODES)
def test_policy_bias_correction_off_by_one_is_flagged(loss, track):
    """3 steps, then 9 from t0 = 3: a second call that numbers its steps from 2 or from 4"""
    D, (p1, m1, v1, _, _) = _pol(loss, track, steps=3)
    rest, blocks = D["idx"][3 * B:], F.policy_blocks(n, m, HID)
    g1 = np.zeros(O_D)
    ref = _pol(loss, track, theta=p1, am=m1, av=v1, t0=3, idx=rest, g_first=g1)[1][0]
    well = g1 >= F.GRAD_FLOOR
    if loss == 0:
        well[-m:] = True
    ok = _pol(loss, track, theta=_r32(p1), am=_r32(m1), av=_r32(v1), t0=3, idx=rest)[1][0]
    assert not _cont_flag("pol", _r32(ok), ref, blocks, well)
    for t0 in (2, 4):
        bad = _pol(loss, track, theta=p1, am=m1, av=v1, t0=t0, idx=rest)[1][0]
        assert _cont_flag("pol", bad, ref, blocks, well), t0


def test_guards():
    a = np.concatenate([np.arange(5.0), np.full(4, np.nan)])
    assert F.tail_intact(a, 5)
    b = a.copy(); b[5] = 0.0
    assert not F.tail_intact(b, 5)                         # a write behind the last parameter
    b = a.copy(); b[4] = np.nan
    assert not F.tail_intact(b, 5)                         # a real entry that is not finite


# ---------------------------------------------------------------- the cases themselves, from the oracle alone
def test_mlp_cases_are_well_posed():
    """few ill-conditioned parameters (measured: <= 1.5 % without weight decay -- ReLU units that are dead on a minibatch --,
    <= 0.03 % with it), and residuals of the first minibatch that do not cancel: the one-entry block b3 takes 2 mean e"""
    for name, d, _, _, hid, batch, wd, seed in K.MLP_CASES:
        th, x, y, perm, perm1 = K.mlp_data(d, hid, batch, seed)
        for N, pm in ((2 * batch, perm1), (K.N_MLP, perm)):
            g1 = np.zeros(th.size)
            F.mlp_fit(th, d, x[:N], y[:N], pm[:N], N, 1, LR, wd, hid, batch, g_first=g1)
            assert np.mean(g1 < F.GRAD_FLOOR) < BARS["fit_ill_conditioned"], (name, N)
            e = O.forward(th, F.mlp_sizes(d, hid), None, x[pm[:batch]], 0, 0)[:, 0] - y[pm[:batch]]
            assert abs(e.mean()) >= K.B3_CANCEL_FLOOR * np.abs(e).mean(), (name, N)


def test_policy_cases_are_well_posed():
    for n_, m_, hid, B_, env, _, seed in K.POL_CASES:
        D = K.pol_data(n_, m_, hid, B_, seed)
        assert np.any(np.sort(D["idx"][:B_])[1:] == np.sort(D["idx"][:B_])[:-1])          # a row twice inside the first minibatch
        for loss, track in K.MODES:
            am, av = K.pol_moments(D, m_, loss)
            g1 = np.zeros(D["theta"].size)
            st = F.policy_fit(D["theta"], n_, m_, hid, D["tr"], D["theta_old"], D["tr_old"], D["obs"], D["act"], D["adv"], D["idx"], B_, loss,
                              track, LR, CLIP, am, av, g_first=g1)[4]
            ill = np.mean(g1[:-m_] < F.GRAD_FLOOR) if loss == 0 else np.mean(g1 < F.GRAD_FLOOR)
            assert ill < BARS["fit_ill_conditioned"], (n_, m_, hid, B_, loss)
            if loss == 2:
                assert min(st["clipped"], st["unclipped"], st["adv_pos"], st["adv_neg"]) > 0 and st["near"] == 0, (n_, m_, hid, B_, track, st)
