"""The pytest side of the GPU worker tests: ONE fresh worker process per kernel family (or per arm of a family), under a time limit,
never started again once it failed -- and, across the whole pytest process, nothing started at all after a worker ended in a way
that may have left the card in a bad state (the latch below).  No torch and no GPU at import; not a plugin, not collected.

    worker_result(script, limit, what)      a worker that prints "RESULT {json}": its last payload
    run_child(argv, limit, ...)             one child under a limit with check=True and a scrubbed environment
    arm_runner(start, out_dir, what)        get(arm): a module's start(arm, out_dir) at most once per arm
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

_RUNS = {}              # (script, argv) -> (payload or None, log)
_TRIPPED = []           # [what]: the first worker that ended in a way that may have left the card bad
_BAD_STATUS = (134, 139, 137, 124)
_FAULT_TEXT = "illegal memory access"


def tripped():
    """the worker that tripped the process-wide latch, or None"""
    return _TRIPPED[0] if _TRIPPED else None


def reset():
    """forget every kept run and the latch (for the launcher's own tests)"""
    _RUNS.clear()
    del _TRIPPED[:]


def _gate():
    if _TRIPPED:
        pytest.fail("not started: the %s worker ended in a way that may have left the GPU in a bad state" % _TRIPPED[0])


def _trip_if_bad(what, returncode, output, timed_out=False):
    bad = timed_out or (returncode is not None and (returncode < 0 or returncode in _BAD_STATUS)) or _FAULT_TEXT in output
    if bad and not _TRIPPED:
        _TRIPPED.append(what)


def _text(x):
    return x.decode(errors="replace") if isinstance(x, bytes) else (x or "")


def worker_result(script, limit, what, argv=(), env=None):
    """-> the parsed payload of the last "RESULT " line of `python tests/<script> *argv`, run once per pytest process with cwd at
    the repository root.  A run that failed (a non-zero exit, no RESULT line, the time limit, an error at start) is kept: this
    call and every later one fail with its log."""
    key = (script, tuple(argv))
    if key not in _RUNS:
        _gate()
        try:
            p = subprocess.run([sys.executable, os.path.join(TESTS, script)] + list(argv), capture_output=True, text=True, timeout=limit,
                               cwd=ROOT, env=env)
            out = p.stdout + p.stderr
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            _RUNS[key] = (json.loads(line[-1][7:]) if p.returncode == 0 and line else None, "exit %d\n%s" % (p.returncode, out[-4000:]))
            _trip_if_bad(what, p.returncode, out)
        except subprocess.TimeoutExpired as e:
            _RUNS[key] = (None, "timed out: %s" % (_text(e.stdout) + _text(e.stderr))[-2000:])
            _trip_if_bad(what, None, "", timed_out=True)
        except (subprocess.SubprocessError, OSError) as e:
            _RUNS[key] = (None, "not started: %s: %s" % (type(e).__name__, e))
    r, log = _RUNS[key]
    if r is None:
        pytest.fail("%s worker failed (not restarted):\n" % what + log)
    return r


def run_child(argv, limit, what, scrub=(), env=None, cwd=None):
    """`argv` under `limit` seconds with check=True; its environment is os.environ minus the switch names in `scrub` plus `env`.
    Its output is passed on to this process's stdout / stderr when it ends.  Raises what subprocess.run raises; honours and feeds
    the latch."""
    _gate()
    e = {k: v for k, v in os.environ.items() if k not in scrub}
    e.update(env or {})
    p = None
    try:
        p = subprocess.run(argv, check=True, env=e, cwd=cwd, timeout=limit, capture_output=True, text=True)
    except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as err:
        p = err
        _trip_if_bad(what, getattr(err, "returncode", None), _text(err.stdout) + _text(err.stderr),
                     timed_out=isinstance(err, subprocess.TimeoutExpired))
        raise
    finally:
        if p is not None:
            sys.stdout.write(_text(p.stdout))
            sys.stderr.write(_text(p.stderr))


def arm_runner(start, out_dir, what="%s"):
    """-> get(arm): start(arm, out_dir(arm)) -> results, at most once per arm, on first use.  A worker that fails (an error, a
    fault, a timeout) is never started again: the failure is kept, and every later request -- for that arm or any other, since
    the GPU may be left in a bad state -- fails at once without starting a process.  `what` words the arm in that message."""
    cache, failed = {}, []

    def get(arm):
        if failed:
            pytest.fail("not started: the %s worker failed earlier in this module (%s)" % (what % failed[0][0], failed[0][1]))
        if arm not in cache:
            _gate()
            try:
                cache[arm] = start(arm, out_dir(arm))
            except (subprocess.SubprocessError, OSError) as e:
                failed.append((arm, e))
                raise
        return cache[arm]
    return get
