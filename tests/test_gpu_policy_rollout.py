"""mjx_policy_rollout on the MI355X (csrc/policy_rollout.h): both routes step by step and free-running against the fp64 oracle, the
routes against each other, route 0's bits against mjx_model_rollout, and proof that route 1 runs its own kernel.  Every check
runs in ONE fresh worker process under a time limit (tests/_policy_rollout_worker.py); a worker that failed is not started again
-- the remaining tests fail with its output.  The worker asserts per call that no NaN of the pre-filled output blocks stays inside
and that the 64 guard elements behind each block are untouched.

The bars are 3x the reference's own fp32 error on the same quantity, measured by tests/golden/make_golden_refine.py exactly as the
worker measures the kernels (tests/golden/refine.npz: kya_ / kys_ per case, kfree_*); none is a multiple of anything the kernels
under test produced.  An H = 1 case stores s0 only, so its state yardstick is 0 and the stored state must be exact.  Measured on
the MI355X (route 1 / route 0, largest over the cases, as a share of the bar): action steps 0.42 / 0.43, state steps 0.49 / 0.40,
routes against each other 0.49, free-running 0.33 / 0.31."""
import os
import sys

import numpy as np
import pytest

from tests._worker_run import worker_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _refine_oracle as F  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "refine.npz"))


def _result():
    return worker_result("_policy_rollout_worker.py", 300, "policy rollout")


def _bars(name):
    return 3.0 * float(G["kya_" + name]), 3.0 * float(G["kys_" + name])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["1", "0"])
def test_rollout_step_by_step_against_fp64(route):
    """every case of _refine_oracle.KCASES (all eight <HB, NB> instances, each at H = 7 so that its dynamics half reaches a stored
    state; p9 at H = 1; rows 1, 31, 32, 33, 129; K 1 and 3; one state and
    (N, n); no, shared and per-member noise; no and tight bounds; five policy widths; m 1, 6, 9, 32; n 1, 17, 33, 64; ReLU / tanh;
    flags 7, 5, 3, 1, 0; a masked column): every stored action against the fp64 action step from the stored state, every stored
    state against the fp64 state step from the stored state and action before it"""
    r = _result()["step"][route]
    assert set(r) == set(F.KCASES)
    for name in sorted(r):
        (ea, es), (ba, bs) = r[name], _bars(name)
        print("route %s case %s: action %.2e of %.2e, state %.2e of %.2e" % (route, name, ea, ba, es, bs))
        assert ea <= ba and es <= bs, name


@pytest.mark.gpu
def test_free_running_rollouts_against_fp64():
    """H = 16 on one case per route against _dyn_oracle.rollout; the bar is 3x the reference's own free-running fp32 distance"""
    r = _result()["free"]
    for route in ("1", "0"):
        print(route, r[route])
        assert r[route][0] <= 3.0 * float(G["kfree_act"]) and r[route][1] <= 3.0 * float(G["kfree_obs"])


@pytest.mark.gpu
def test_routes_agree_on_every_served_case():
    """the two routes' free-running outputs against each other; the bar is the sum of the two routes' step bars for the case"""
    r = _result()["routes"]
    for name in sorted(F.KCASES):
        (ea, es), (ba, bs) = r[name], _bars(name)
        print("case %s: actions %.2e of %.2e, states %.2e of %.2e" % (name, ea, 2 * ba, es, 2 * bs))
        assert ea <= 2 * ba and es <= 2 * bs, name


@pytest.mark.gpu
def test_a_masked_output_column_is_exactly_zero():
    """case p2 (flags 3, out_scale 0 in one column): that column of every stored next state is exactly 0 on both routes"""
    assert _result()["masked_zero"] is True


@pytest.mark.gpu
def test_route_zero_is_model_rollout_bit_for_bit():
    """with per-member noise and (N, n) states against mjx_model_rollout; with one state and shared noise against the same call
    on inputs tiled and expanded by the caller, and against mjx_model_rollout on those"""
    assert _result()["bits"] == {"member": True, "tiled": True, "tiled_model": True}


@pytest.mark.gpu
def test_the_mfma_route_really_runs_its_own_kernel():
    """route_out agrees with mjx_policy_rollout_route on every case, is 0 under MJX_POLICY_ROLLOUT_MFMA=0, and the two routes'
    outputs are not bit-identical on at least one case"""
    r = _result()
    for name in F.KCASES:
        assert r["route_fn"][name] == 1 and r["route_out"][name] == [1, 0], name
    assert any(r["differ"].values())


@pytest.mark.gpu
def test_shared_noise_gives_every_member_the_same_first_action():
    r = _result()["shared"]
    assert r and all(r.values())
