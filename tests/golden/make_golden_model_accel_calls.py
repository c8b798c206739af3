"""Records tests/golden/model_accel_calls.json: the transcript of every device call that the scenario of
tests/test_model_accel_calls_cpu.py makes, and the host state it leaves behind.  Run it on the commit whose marshalling is the
standard (the parent of a change to the host layer), never on the change itself; it needs neither a GPU nor libmjx.

    python tests/golden/make_golden_model_accel_calls.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_model_accel_calls_cpu as T  # noqa: E402

if __name__ == "__main__":
    out = T.scenario()
    with open(T.GOLDEN, "w") as f:
        f.write('{"calls":[\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in out["calls"]) + '\n],\n"after":')     # a call per line
        f.write(json.dumps(out["after"], separators=(",", ":")) + "}\n")
    print("%d device calls -> %s" % (len(out["calls"]), T.GOLDEN))
