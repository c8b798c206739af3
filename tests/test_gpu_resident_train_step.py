"""ModelAccelNPG.train_step(resident=True) on the MI355X against the host route (tests/_resident_step_worker.py, ONE fresh worker
process under a time limit; a worker that failed is not started again).  The case: (n, m) = (6, 2), K = 3, dynamics 64 x 64, reward
nets 100 x 100, policy 32 x 32, N = 40, H = 8, LinearBaseline, the truncation limit fixed on the CPU from the fp64 oracle
(tests/_rollout_batch_cases.py: e2e_oracle, fix_lim)."""
import pytest

from tests._worker_run import worker_result

DECLINES = ("termination_function", "members_differ", "mixed_rewards", "short_horizon", "distributed", "no_gpu")


def _result():
    return worker_result("_resident_step_worker.py", 300, "resident step")


@pytest.mark.gpu
def test_resident_step_equals_the_host_route_with_the_switches_off():
    """(a) all three route switches forced to 0, two agents from one seed and one RNG state: the paths array for array (observations,
    actions, rewards, lengths, terminated, returns, advantages), the statistics, the logged keys; the updated policy no further from
    the host route's than two host-route runs are from each other"""
    r = _result()
    assert r["a_info"]["resident"] is True and r["a_info"]["why"] is None and r["a_info"]["routes"] == dict(rollout=0, rewards=0, disagreement=0)
    assert r["a_host_info"]["resident"] is False and r["a_host_info"]["why"] == "resident=False"
    cut, paths, shortest, longest = r["a_truncated"]
    assert paths == 120 and 0 < cut < paths and shortest == 4 and longest == 8           # (the limit truncates some paths and clamps one)
    assert r["a_info"]["paths"] == paths and r["a_info"]["truncated"] == cut
    assert r["a_paths"] == []
    assert r["a_stats"][0] == r["a_stats"][1]
    assert r["a_keys"][0] == r["a_keys"][1]
    print("policy after the step: resident against host %.3e, host against host %.3e" % tuple(r["a_theta"]))
    assert r["a_theta"][0] <= r["a_theta"][1]


@pytest.mark.gpu
def test_resident_step_on_the_default_routes():
    """(b) every route is the MFMA one; lengths and terminated as with the switches off; the packed observations per column within
    6 x the fixture's rollout yardstick of the generic routes' (the sum of the two routes' bars)"""
    r = _result()
    assert r["b_info"]["routes"] == dict(rollout=1, rewards=1, disagreement=1)
    assert r["b_lens"] == [True, True]
    err, yard = r["b_obs"]
    print("packed observations, MFMA routes against generic: %.3e, bar %.3e" % (err, 6 * yard))
    assert err <= 6 * yard
    assert r["b_differs"]


@pytest.mark.gpu
def test_resident_step_uploads_nothing_of_the_batch_size():
    """(c) learned rewards: ingest.upload, PathStager.stage and PathStager.add_paths see no array with the batch's row count during the
    resident step (and do during the host step: the probe works)"""
    r = _result()
    rows, hits = r["c_resident"]
    assert rows > 0 and hits == []
    assert r["c_host"][1] > 0


@pytest.mark.gpu
def test_resident_step_reproduces_the_reference_fixture():
    """(d) tests/golden/model_accel.npz (host reward_function, ts_trunc): ts_lens, and ts_stats at the existing bar"""
    r = _result()
    assert r["d_info"]["resident"] is True and r["d_info"]["routes"]["rewards"] is None
    assert r["d_lens"]
    assert r["d_keys"][0] == r["d_keys"][1]
    print("statistics against the fixture: %.3e" % r["d_stats"])
    assert r["d_stats"] < 3e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name", DECLINES)
def test_declined_calls_take_the_host_route(name):
    """(e) resident: False with its why, and the host route's result"""
    e = _result()["e"][name]
    assert e["info"]["resident"] is False and e["info"]["why"] == e["why"]
    assert e["same"]


@pytest.mark.gpu
def test_the_default_is_the_host_route():
    r = _result()
    assert r["f_info"]["resident"] is False and r["f_info"]["why"] == "resident=False"
