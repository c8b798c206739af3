"""The Gram route of the LinearPolicy NPG update (csrc/linear_policy.h: mjx_linear_moments, mjx_npg_update_linear) against
oracle/npg_oracle.py in fp64.  The cases run once, in tests/_linear_gram_worker.py; the bars are the project's own
(tests/test_gpu_operators.py:15-17, tests/test_gpu_parity.py for the update's scalars)."""
import numpy as np
import pytest

from tests._cases import NpgCase
from tests._worker_run import worker_result
from tests.test_gpu_operators import TOL_FVP, TOL_STEP, TOL_VPG, make_agent, rel

pytestmark = pytest.mark.gpu

TOL_KL = 1e-5
# (n, m, N): one feature and a two-row tail tile | NP exactly 32, the full action width | the first n with two feature blocks, one row
# past a chain | the largest shape | no transforms | several tiles per wave and several chains
CASES = ["1_1_33", "31_32_1500", "32_1_1025", "63_17_3000", "17_6_4099", "17_6_70001"]


def results():
    return worker_result("_linear_gram_worker.py", 240, "linear Gram")


@pytest.mark.parametrize("case", CASES)
def test_moments_vs_oracle(case):
    """F v formed in NumPy from the returned G, the gradient, the surrogate sum and the row count; padding exactly zero; two
    calls the same bits"""
    r = results()[case]
    print(case, r)
    assert r["fvp"] < TOL_FVP and r["vpg"] < TOL_VPG and r["surr"] < 1e-6, r
    assert r["rows"] == int(case.split("_")[2]) and r["tail"] == [0.0, 0.0] and r["pad"] == 0.0 and r["same_bits"], r


@pytest.mark.parametrize("case", CASES)
def test_update_vs_oracle(case):
    """route 1; x, the step and the scalars of results[] at the bars of tests/test_gpu_parity.py.  (The layer-wise update of
    the same case is printed beside it: the yardstick, not compared.)"""
    r = results()[case]
    g = r["gram"]
    print(case, "gram", g, "\n  layer-wise", r["layerwise"])
    assert r["route"] == 1
    assert g["x"] < TOL_STEP and g["step"] < TOL_STEP and g["grad"] < TOL_VPG, g
    assert g["surr_after"] < 2e-5 and g["kl"] < TOL_KL and g["surr_before"] < 1e-6 and g["alpha"] < 1e-5 and g["gx"] < 5e-5, g
    assert g["count"] == int(case.split("_")[2])


def test_clamp_constant_step_and_early_break():
    r = results()["once"]
    print(r)
    assert r["clamp"]["step"] < TOL_STEP and r["clamp"]["log_std"] == [0.25] * 6
    assert r["const_alpha"]["step"] < TOL_STEP and r["const_alpha"]["slot9"] == -7.0          # (what the slot held before the call)
    b = r["break"]
    assert b["above"] >= 10 and b["below"] >= 10 and b["oracle_is_k"] == 0.0 and min(b["one_less"], b["one_more"]) > 1e-3, b    # the oracle alone
    assert b["x"] < TOL_STEP, b


def test_switch_off_and_twin_rank():
    r = results()["once"]
    assert r["switch"] == dict(route=0, same=True)
    t = r["twin"]
    assert t["route"] == 1 and t["calls"] == t["want"], t            # the moment block and K3's 4 doubles: two rank sums
    assert t["theta"] < 1e-6 and t["x"] < 1e-6 and t["res"] < 1e-6, t


def test_host_class_on_the_fixture():
    """NPG(gram=True) on npg_cfg1_linear meets that fixture's bars (tests/test_gpu_parity.py:73-95) and reports route 1; the default
    reports None and leaves the parameters of an agent built without the keyword, bit for bit"""
    c = NpgCase("npg_cfg1_linear")
    new = {}
    for key, kw in [("gram", dict(gram=True)), ("off", dict(gram=False)), ("plain", {})]:
        agent, pol = make_agent(c, normalized_step_size=float(c.g["step"]), save_logs=True, **kw)
        agent.train_from_paths(c.paths)
        new[key], lg, route = pol.get_param_values(), agent.logger.get_current_log(), agent.last_update["route"]
        agent.engine.close()
        assert route == (1 if key == "gram" else None)
        if key == "gram":
            assert rel(new[key].astype(np.float64) - c.theta0, c.g["new_params"].astype(np.float64) - c.theta0) < TOL_STEP
            assert abs(lg["alpha"] - float(c.g["alpha"])) < 1e-5 * float(c.g["alpha"])
            assert abs(lg["kl_dist"] - float(c.g["kl"])) < TOL_KL * float(c.g["kl"]), ("kl", lg["kl_dist"], float(c.g["kl"]))
            assert abs(lg["surr_improvement"] - float(c.g["surr_improvement"])) < 2e-5
    assert new["off"].tobytes() == new["plain"].tobytes()
