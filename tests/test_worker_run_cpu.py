"""tests/_worker_run.py and tests/_worker_dev.py on the CPU: throw-away workers (plain Python, no torch, no GPU) that append a line
to a counter file when they start, so "ran once" and "not started" are counted, not inferred."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _worker_dev as D
from tests import _worker_run as W

HEAD = "import os, sys, time\nopen(%r, 'a').write('x\\n')\n"
BODIES = {
    "two_results": "print('RESULT {\"v\": 1}')\nprint('noise')\nprint('RESULT {\"v\": 2}')\n",
    "exit1": "print('RESULT {\"v\": 1}')\nprint('the worker log')\nsys.exit(1)\n",
    "no_result": "print('the worker log')\n",
    "sleeps": "print('the worker log', flush=True)\ntime.sleep(30)\n",
    "exit139": "print('the worker log')\nsys.exit(139)\n",
    "healthy": "print('RESULT {\"v\": 3}')\n",
}


@pytest.fixture(autouse=True)
def fresh_latch():
    W.reset()
    yield
    W.reset()


@pytest.fixture
def worker(tmp_path):
    """name -> (script path, starts()): a throw-away worker and the number of times it started"""
    def make(name):
        counter = str(tmp_path / (name + ".count"))
        path = str(tmp_path / (name + ".py"))
        with open(path, "w") as f:
            f.write(HEAD % counter + BODIES[name])
        return path, lambda: len(open(counter).read().split()) if os.path.exists(counter) else 0
    return make


def _fails(call):
    with pytest.raises(pytest.fail.Exception) as e:
        call()
    return str(e.value)


def test_last_result_line_and_one_start(worker):
    path, starts = worker("two_results")
    assert W.worker_result(path, 30, "toy") == {"v": 2}
    assert W.worker_result(path, 30, "toy") == {"v": 2}
    assert starts() == 1 and W.tripped() is None


@pytest.mark.parametrize("name,limit,in_log,trips", [("exit1", 30, "exit 1\n", False), ("no_result", 30, "exit 0\n", False),
                                                      ("sleeps", 1, "timed out", True)], ids=["exit_1", "no_result_line", "time_limit"])
def test_failed_worker_is_kept_and_not_restarted(worker, name, limit, in_log, trips):
    path, starts = worker(name)
    first = _fails(lambda: W.worker_result(path, limit, "toy"))
    assert first.startswith("toy worker failed (not restarted):\n") and in_log in first and "the worker log" in first
    assert _fails(lambda: W.worker_result(path, limit, "toy")) == first
    assert starts() == 1
    assert (W.tripped() == "toy") is trips and (W.tripped() is None) is not trips


def test_missing_script_is_kept_too(tmp_path, monkeypatch):
    # (python itself starts and exits 2; an executable that does not exist is an OSError at start)
    first = _fails(lambda: W.worker_result(str(tmp_path / "absent.py"), 30, "toy"))
    assert first.startswith("toy worker failed (not restarted):\n") and "exit 2" in first and "absent.py" in first
    calls = []
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: calls.append(a))
    assert _fails(lambda: W.worker_result(str(tmp_path / "absent.py"), 30, "toy")) == first
    assert calls == [] and W.tripped() is None
    monkeypatch.undo()
    monkeypatch.setattr(sys, "executable", str(tmp_path / "no_such_python"))
    first = _fails(lambda: W.worker_result("other.py", 30, "toy"))
    assert first.startswith("toy worker failed (not restarted):\nnot started: ") and "no_such_python" in first
    monkeypatch.undo()
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: calls.append(a))
    assert _fails(lambda: W.worker_result("other.py", 30, "toy")) == first
    assert calls == [] and W.tripped() is None


def test_a_bad_exit_status_trips_the_latch_for_every_launcher(worker, tmp_path):
    bad, bad_starts = worker("exit139")
    good, good_starts = worker("healthy")
    assert "exit 139" in _fails(lambda: W.worker_result(bad, 30, "faulty"))
    assert W.tripped() == "faulty"
    msg = _fails(lambda: W.worker_result(good, 30, "toy"))
    assert msg.startswith("not started") and "faulty" in msg
    assert "faulty" in _fails(lambda: W.run_child([sys.executable, good], 30, "toy"))
    get = W.arm_runner(lambda arm, d: W.run_child([sys.executable, good], 30, arm), lambda arm: str(tmp_path))
    assert "faulty" in _fails(lambda: get("a"))
    assert (bad_starts(), good_starts()) == (1, 0)


@pytest.mark.parametrize("status,output,timed_out,trips", [(1, "AssertionError", False, False), (2, "", False, False), (-6, "", False, True),
                                                            (-11, "", False, True), (134, "", False, True), (139, "", False, True),
                                                            (137, "", False, True), (124, "", False, True), (None, "", True, True),
                                                            (1, "HIP error: an illegal memory access was encountered", False, True)],
                         ids=["exit_1", "exit_2", "signal_6", "signal_11", "exit_134", "exit_139", "exit_137", "exit_124", "time_limit", "fault_text"])
def test_what_trips_the_latch(status, output, timed_out, trips):
    W._trip_if_bad("toy", status, output, timed_out)
    assert (W.tripped() == "toy") is trips


def test_arm_runner_runs_each_arm_once_and_a_failed_arm_blocks_the_rest(worker, tmp_path):
    good, good_starts = worker("healthy")
    bad, bad_starts = worker("exit1")
    dirs = []

    def start(arm, out_dir):
        dirs.append(out_dir)
        W.run_child([sys.executable, bad if arm == "c" else good], 30, arm)
        return arm.upper()

    get = W.arm_runner(start, lambda arm: str(tmp_path / arm), "arm %s")
    assert [get("a"), get("b"), get("a"), get("b")] == ["A", "B", "A", "B"]
    assert good_starts() == 2 and dirs == [str(tmp_path / "a"), str(tmp_path / "b")]
    with pytest.raises(subprocess.CalledProcessError):
        get("c")
    for arm in ("c", "a", "d"):
        msg = _fails(lambda: get(arm))
        assert msg.startswith("not started: the arm c worker failed earlier in this module (") and "exit status 1" in msg
    assert (good_starts(), bad_starts()) == (2, 1) and W.tripped() is None


def test_run_child_environment(tmp_path, monkeypatch):
    out = str(tmp_path / "env.txt")
    code = "import os; open(%r, 'w').write(repr([os.environ.get(k) for k in ('MJX_T_SCRUBBED', 'MJX_T_ARM', 'MJX_T_OTHER')]))" % out
    monkeypatch.setenv("MJX_T_SCRUBBED", "1")
    monkeypatch.setenv("MJX_T_ARM", "parent")
    monkeypatch.setenv("MJX_T_OTHER", "kept")
    W.run_child([sys.executable, "-c", code], 30, "toy", scrub=("MJX_T_SCRUBBED", "MJX_T_ARM"), env={"MJX_T_ARM": "0"})
    assert open(out).read() == repr([None, "0", "kept"])
    with pytest.raises(subprocess.TimeoutExpired):
        W.run_child([sys.executable, "-c", "import time; time.sleep(30)"], 1, "slow")
    assert W.tripped() == "slow"


def test_switch_restores(monkeypatch):
    monkeypatch.setenv("MJX_T_SET", "before")
    monkeypatch.delenv("MJX_T_ABSENT", raising=False)
    with D.switch("MJX_T_SET", 1), D.switch("MJX_T_ABSENT", "0"), D.switch("MJX_T_ALONE", None):
        assert (os.environ["MJX_T_SET"], os.environ["MJX_T_ABSENT"]) == ("1", "0") and "MJX_T_ALONE" not in os.environ
    assert os.environ["MJX_T_SET"] == "before" and "MJX_T_ABSENT" not in os.environ
    with pytest.raises(ZeroDivisionError):
        with D.switch("MJX_T_SET", "2"), D.switch("MJX_T_ABSENT", "2"):
            1 / 0
    assert os.environ["MJX_T_SET"] == "before" and "MJX_T_ABSENT" not in os.environ


def test_device_helpers_on_cpu_tensors():
    cpu = torch.device("cpu")
    assert list(D.ints((np.int64(3), 4.0, True))) == [3, 4, 1]
    assert D.up(None) is None and D.up(np.arange(3), dev=cpu).dtype == torch.float32 and D.up(np.arange(3), None, dev=cpu).dtype == torch.int64
    kept = len(D.KEEP)
    t = D.up([1.0], keep=True, dev=cpu)
    assert len(D.KEEP) == kept + 1 and D.KEEP.pop() is t
    buf = D.nan_block(5, torch.float64, dev=cpu)
    assert buf.shape == (5 + D.GUARD,) and buf.dtype == torch.float64 and bool(torch.isnan(buf).all())
    n0 = D.CHECKED[0]
    with pytest.raises(AssertionError, match="toy: 5 elements never written"):
        D.checked_block(buf, 5, "toy")
    buf[:4] = 1.0
    with pytest.raises(AssertionError, match="toy: 1 elements never written"):
        D.checked_block(buf, 5, "toy")
    buf[:5] = torch.arange(5.0, dtype=torch.float64)
    got = D.checked_block(buf, 5, "toy")
    assert got.shape == (5,) and np.array_equal(got, np.arange(5.0))
    buf[5] = 0.0
    buf[5 + D.GUARD - 1] = 0.0
    with pytest.raises(AssertionError, match="toy: 2 guard elements touched"):
        D.checked_block(buf, 5, "toy")
    assert D.CHECKED[0] == n0 + 4
    a = np.array([0.0, 1.5, np.nan], np.float32)
    assert D.same_bits(a, a.copy()) and D.same_bits(torch.from_numpy(a), a) and D.same_bits(a.reshape(3, 1)[:, 0], a)
    assert not D.same_bits(a, np.array([-0.0, 1.5, np.nan], np.float32))          # equal values, other bits
    assert not D.same_bits(a, a.astype(np.float64)) and not D.same_bits(a, a.reshape(1, 3))
