"""The wide and the team trainer of the MLP baseline follow each other on the one exchange block and arrival counter they share
(csrc/fit_host.h fit_exchange), in ONE fresh worker process under a time limit (tests/_fit_exchange_worker.py): one thread, one
stream, wide fit A, team fit B, A again, B again, each from the same initial parameters and moments.

A: d_in 56 (the first width on the wide route -- up to 55 inputs one workgroup's LDS holds the layout; two workgroups), batch 64,
N 192 (two steps), one epoch.  B: d_in 9, batch 128 (a team of two),
N 384 (two steps), one epoch.  Both trainers give the same bits on repeated calls, so the two runs of A, and of B, agree bit for
bit in parameters, both moments and epoch losses -- whatever the other trainer left in the block and behind it in between."""
import pytest

from tests._worker_run import worker_result

pytestmark = pytest.mark.gpu


def test_wide_and_team_fits_alternate_on_one_exchange_block():
    r = worker_result("_fit_exchange_worker.py", 120, "fit exchange")
    kind_and_G = {k: [v[0], v[3]] for k, v in r["routes"].items()}
    assert kind_and_G == {"A": [3, 2], "B": [4, 2]}, r["routes"]                  # WIDE and TEAM, two workgroups each
    assert r["finite"] == {"A": [True, True], "B": [True, True]}, r["finite"]
    assert r["moved"] == {"A": True, "B": True}, r["moved"]
    assert r["bitwise"] == {"A": [True] * 4, "B": [True] * 4}, r["bitwise"]
