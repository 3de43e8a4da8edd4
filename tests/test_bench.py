"""bench.py on one GPU: a plain run prints the headline line only, and --full (parity run, repeats, protocols, roofline ... before
and after the timed steps) leaves what the timed steps compute unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT

# what a plain run does not measure: the legs behind --full
FULL_ONLY = ("rank_parity", "repeats", "value_replay", "heuristics_off", "roofline", "reference_kernels_on_mi355x", "exact_solve",
             "shapes", "float32", "concurrent", "cpu_baseline", "chi2_max_rel_diff_vs_oracle", "contract_wall", "partitioned")


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "10", "--shape", "kitti07", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_times_the_same_steps(tmp_path):
    plain = run_bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["unit"] == "edge-iterations/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["steps"] == 20 and plain["warmup"] == 10 and plain["lm_trials"] == 20 and plain["value"] > 0
    assert plain["value"] == pytest.approx(plain["config"]["edges"] * 1e3 / plain["ms_per_step"], rel=1e-9)
    assert [k for k in FULL_ONLY if k in plain] == []
    full = run_bench("--full", "--no-shapes", "--no-concurrent", "--no-cpu-baseline", "--no-end-to-end", "--repeats", "1",
                     "--dump-outputs", str(tmp_path / "full"))
    assert full["rank_parity"][0]["chi2_max_rel_diff_vs_golden"] <= 1e-6 and full["repeats"]["blocks"] == 1
    assert "roofline" in full and "exact_solve" in full and "value_replay" in full
    # the timed steps start from the same perturbed estimates and return the same thing, bit for bit
    assert full["final_chi2"] == plain["final_chi2"] and full["pcg_iterations"] == plain["pcg_iterations"]
    assert sorted(plain["dump_outputs"]["arrays"]) == sorted(full["dump_outputs"]["arrays"])
    for name in plain["dump_outputs"]["arrays"]:
        assert np.array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")), name
