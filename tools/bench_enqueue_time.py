"""bench.py in this process with the host time of every mjx_npg_update call recorded: the time to the call's RETURN, before any
synchronisation -- what a change to libmjx's host side can move while the kernels stay the same.  The arguments go to bench.py
unchanged; after bench.py's JSON line a second one follows with the median over the timed steps (the warm-up calls are dropped).

    MJX_LIB=<libmjx.so> python tools/bench_enqueue_time.py --gpus 1 --steps 40 --warmup 5
"""
import json
import os
import runpy
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mjrl_amd import _lib  # noqa: E402

lib = _lib.load()
inner, calls = lib.mjx_npg_update, []


def timed(*args):
    t0 = time.perf_counter_ns()
    rc = inner(*args)
    calls.append(time.perf_counter_ns() - t0)
    return rc


lib.mjx_npg_update = timed          # (an attribute of the CDLL object: the engine's backend looks the entry up there per call)
steps = int(sys.argv[sys.argv.index("--steps") + 1])
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
us = sorted(1e-3 * t for t in calls[-steps:])
print(json.dumps({"npg_update_host_us_median": us[len(us) // 2], "npg_update_host_us_min": us[0], "npg_update_host_us_max": us[-1], "calls_timed": len(us),
                  "calls_in_all": len(calls), "lib": _lib.LIB_PATH}), flush=True)
