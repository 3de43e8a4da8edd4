"""What cuba_hip_set_graph refuses and what it reuses of the previous upload, without a GPU: host/test/upload_plan_test.cpp enumerates
every combination of the handle's sixteen boolean facts, the four call forms (one call, begin, ranged over a part, ranged over the whole
range), a graph with and without edges, the two hints and the outcome of the edge comparison -- 4 194 304 cases -- through planUpload
(csrc/ba_upload_plan.hpp), the function cuba_hip_solver::setGraph acts on, and checks the invariants listed in the program, each with the
defect it guards.

One-line mutants of the plan, each built once on a scratch copy (never committed), and the invariant that failed:
  lmOrderFits dropped from reuseSort                 "reuseSort implies sameEdges, devTopology, useDev and the landmark order a fresh upload
                                                     would choose"
  poseReorder dropped from keepPoseOrder             "keepPoseOrder implies poseReorder, reorderActive and reuseSort"
  lmOrderActive dropped from the host condition      "reuseHostSort implies hostTopoValid and no internal pose or landmark order"
  !valuesPartial dropped from keepValues             "keepValues implies promised values, reuseSort, sortedValuesValid, not valuesPartial"
The first three are defects that tests/test_gpu_handle_life.py found on the MI355X (reorder_options twice, orders); here they need no GPU.
The program was also run once under -fsanitize=address,undefined: clean."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")


def test_the_upload_plan_holds_its_invariants_in_every_case():
    subprocess.check_call(["make", "-C", HOST, "-s", "upload_plan_test"])
    out = subprocess.run([os.path.join(HOST, "upload_plan_test")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "4194304 cases, all invariants hold" in out.stdout
