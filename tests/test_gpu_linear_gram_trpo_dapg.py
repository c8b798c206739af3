"""TRPO and DAPG on the Gram route of LinearPolicy (csrc/linear_policy.h: the segmented first pass, the line search inside the
solve) against oracle/npg_oracle.py in fp64.  The cases run once, in tests/_linear_gram_trpo_dapg_worker.py; the bars are the
project's own (tests/test_gpu_operators.py:15-17, TOL_KL of tests/test_gpu_linear_gram.py).

Largest deviations seen on the MI355X: see DESIGN.md section 7g."""
import numpy as np
import pytest

from oracle import npg_oracle as O
from oracle import synth
from tests._cases import NpgCase
from tests._worker_run import worker_result
from tests.test_gpu_linear_gram import TOL_KL
from tests.test_gpu_operators import TOL_STEP, TOL_VPG, make_agent, rel

pytestmark = pytest.mark.gpu


def results():
    return worker_result("_linear_gram_trpo_dapg_worker.py", 240, "linear Gram TRPO / DAPG")


@pytest.mark.parametrize("case", ["1_1_33_1", "31_32_1024_40", "32_1_1025_31", "63_17_3000_1056", "17_6_4099_200"])
def test_dapg_vs_oracle(case):
    """(n, m, N_on, N_demo): route 1; x, step, gradient, KL and surr_before at the bars; G the bits of mjx_linear_moments on the
    on-policy prefix alone; padding exactly zero; two calls the same bits"""
    r = results()["dapg_" + case]
    print(case, r)
    assert r["route"] == 1 and r["rows"] == int(case.split("_")[2])
    assert r["x"] < TOL_STEP and r["step"] < TOL_STEP and r["grad"] < TOL_VPG and r["kl"] < TOL_KL and r["surr_before"] < 1e-6, r
    assert r["G_bits"] and r["pad"] == 0.0 and r["same_bits"], r


@pytest.mark.parametrize("case", ["1_1_33", "32_1_1025", "63_17_3000", "17_6_4099"])
def test_trpo_vs_oracle(case):
    """step_size = 2 kl_dist: route 1, the oracle's trial count, alpha / x / step at TOL_STEP, every trial's closed-form KL and the
    closing pass's batch KL at TOL_KL.  (margin: the fp64 oracle's own distance of every trial's KL from kl_dist, a condition on
    the inputs.)"""
    r = results()["trpo_" + case]
    print(case, r)
    assert r["margin"] > 1e-4, r
    assert r["route"] == 1 and r["accepted"] == 1.0 and r["trials"] == r["want_trials"], r
    assert r["alpha"] < TOL_STEP and r["x"] < TOL_STEP and r["step"] < TOL_STEP and r["ring"] < TOL_KL and r["kl"] < TOL_KL and r["surr_slots_nan"], r


def test_more_than_one_trial_and_the_zero_step():
    r = results()
    assert max(r["trpo_" + c]["want_trials"] for c in ("1_1_33", "32_1_1025", "63_17_3000", "17_6_4099")) > 1
    assert r["once"]["zero"] == dict(route=1, theta_same=True, accepted=0.0, trials=100.0), r["once"]["zero"]


def test_switch_off_and_twin_rank():
    r = results()["once"]
    assert r["trpo_off"] == dict(route=0, untouched=True) and r["dapg_off"] == dict(route=0, same=True), r
    t = r["twin"]
    assert t["route"] == 1 and t["calls"] == t["want"], t            # the moment block and the closing pass's 4 doubles: two rank sums
    assert t["theta"] < 1e-6 and t["x"] < 1e-6 and t["res"] < 1e-6, t


@pytest.mark.parametrize("algo", ["trpo", "dapg"])
def test_host_classes_on_the_fixture(algo):
    """TRPO / DAPG(gram=True) on the inputs of npg_cfg1_linear meet the fp64 oracle and report route 1; without the keyword the
    route is None and the parameters are those of gram=False, bit for bit"""
    from mjrl_amd.algos.dapg import DAPG
    from mjrl_amd.algos.trpo import TRPO
    c = NpgCase("npg_cfg1_linear")
    demos = synth.make_paths(3, 200, c.n, c.m, seed=7)
    th, o, a, w = (x.astype(np.float64) for x in (c.theta0, c.obs, c.act, c.adv_w))
    kw = dict(cg_iters=c.cg_iters, damping=float(np.float32(1e-4)), kl_dist=0.025)
    if algo == "trpo":
        cls, extra, ref = TRPO, {}, O.trpo_update(th.copy(), o, a, w, c.n, c.m, (), c.transforms(), **kw)
    else:
        do, da = (np.concatenate([p[k] for p in demos]).astype(np.float64) for k in ("observations", "actions"))
        cls, extra, ref = DAPG, dict(demo_paths=demos), O.dapg_update(th.copy(), o, a, w, do, da, c.n, c.m, (), c.transforms(), **kw)
    new = {}
    for key, g in [("gram", dict(gram=True)), ("off", dict(gram=False)), ("plain", {})]:
        agent, pol = make_agent(c, cls=cls, kl_dist=0.025, **extra, **g)
        agent.train_from_paths(c.paths)
        new[key], u = pol.get_param_values(), agent.last_update
        agent.engine.close()
        assert u["route"] == (1 if key == "gram" else None)
        if key == "gram":
            assert rel(new[key].astype(np.float64) - th, ref["new_params"] - th) < TOL_STEP
            assert abs(u["alpha"] - ref["alpha"]) < TOL_STEP * ref["alpha"] and abs(u["kl_dist"] - ref["kl"]) < TOL_KL * ref["kl"], (u, ref["alpha"], ref["kl"])
            assert algo == "dapg" or u["trials"] == ref["tries"]
    assert new["off"].tobytes() == new["plain"].tobytes()
