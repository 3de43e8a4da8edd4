"""Generates tests/golden/upload_reuse.json: per script of tests/handle_life_scripts.py and per step, the step's label and the deltas of
the counters value_bytes_uploaded, edge_sorts and structure_builds on one live handle (f64, heuristics = 0), through walk() of
tests/test_gpu_upload_reuse.py -- what every upload reused.  Needs the GPU.  The numbers are a decision table, not floating point: they
were recorded on the setGraph that preceded csrc/ba_upload_plan.hpp, and a change of the library must reproduce them; record again only
when a script gains steps, at a commit whose reuse is trusted.  Run from the repo root: `python tests/golden/make_golden_upload_reuse.py`."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import handle_life_scripts as sc  # noqa: E402
import test_gpu_upload_reuse as t  # noqa: E402

if __name__ == "__main__":
    out = {name: t.walk(name) for name in sorted(sc.SCRIPTS)}
    with open(os.path.join(HERE, "upload_reuse.json"), "w") as f:
        f.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(v)) for k, v in out.items()) + "\n}\n")
