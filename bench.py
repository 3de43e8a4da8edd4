#!/usr/bin/env python3
"""bench.py -- headline benchmark: Levenberg-Marquardt bundle adjustment on a KITTI-00-shaped graph.

A "step" is one LM iteration (linearise + Schur + reduced solve + back-substitution + update +
re-evaluation) over the whole graph, with the graph resident in HBM; `value` = edges x steps / wall
(edge-iterations per second, the reading under which the reference's README numbers give 4.56 M/s on a GTX 1080
and 0.47 M/s for g2o).  Steps are taken as the reference's protocol takes them
(samples/sample_comparison_with_g2o.cpp:74-79, 303-307): a 1-iteration warm-up moves the estimates, then runs of
optimize(10) start from there -- but NOT from the very same estimate every time (round-3 verdict: three host heuristics of the
library -- carried-over first coarse inverse, repeat prediction of the PCG batch lengths, exact-length batch graphs -- are exact
only when a run replays the previous one).  Every timed run of `value` starts from its own seeded perturbation of the warm
state (1 cm on translations and landmarks, 0.05 deg on rotations: a sliding window that moved), prepared on the device before
the clock starts (cuba_hip_snapshot_state_slot) so that the timed region is still LM work only.  The replay figure of rounds
1-3 is reported beside it as `value_replay`, and `heuristics_off` prices the three heuristics under both protocols.

Next to `value` the line carries
  contract_wall  the SURVEY section 8(d) wall: initialize() + optimize(10) after the 1-iteration warm-up through the
                 C++ API (host flattening, PCIe upload, structure analysis and write-back inside), for an unchanged
                 and for a new topology, with E/wall (strict) and E x 10/wall;
  roofline       the dominant kernel against the 8 TB/s HBM peak, and `roofline.path`: the whole hot path,
                 B_alg(trial) x trials / t_hot against 8.0 and 6.3 TB/s;
  cpu_baseline   the CPU oracle (our g2o-faithful restatement -- "port", not g2o itself) on the host cores:
                 all cores (OpenMP build) and single thread, nproc printed.
  repeats        the timed block (exactly --steps steps, as `value`) five more times: median / min / max, so that a short
                 timed region is not one sample;
  shapes         every other single-GPU BASELINE.json configuration, driver-timed in the same invocation: kitti07
                 (configs[0], with the CPU path timed beside it), s2m (configs[2]), g4m (configs[4]'s graph on one GPU):
                 wall of 10 LM iterations (median / min / max of three runs under the same protocol), edge-iterations/s,
                 PCG iterations, chi2 max-rel-diff against the oracle (live for kitti07, the committed
                 tests/golden/baseline_shapes_chi2.json for all).

A plain run prints the headline only: it sets up, takes the warm-up iteration and the --warmup steps, times the --steps steps, writes
--dump-outputs if asked and prints the line (`value`, `ms_per_step` and the counters of the timed region).  Everything else named here
-- the parity check against the committed oracle trajectories (`rank_parity`), `repeats`, `value_replay`, `heuristics_off`, `roofline`,
`exact_solve`, `shapes`, `float32`, `concurrent`, `cpu_baseline`, `contract_wall`, the citation of the reference's kernels and, for N > 1,
the `partitioned` leg -- runs only with --full.

N = 1 : BASELINE.json configs[1] -- ba_kitti_00 shape (1332 poses / 133383 landmarks / 561116 edges,
        synthetic stand-in, seed 0), fp64, Huber kernels as in samples/sample_comparison_with_g2o.cpp:195-200.
N > 1 : configs[3] -- one independent KITTI-00-sized graph per GPU (seeds 100+rank), no data-path
        collective (weak scaling); launched by torchrun, one rank per GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # the oracle's OpenMP workers must not spin beside the GPU legs

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters")
LM_RUN = 10               # iterations per LM run (the reference protocol: optimize(10))


def algorithmic_bytes(fp, nblk, nc, upper=False):
    """Compulsory bytes per launch of each hot kernel. nc = coarse aggregates.
    upper: the three-launch PCG iteration on the upper-triangular storage (graphs beyond 1536 free poses): pcg_spmv = the SpMV that
    parks the transposed products, pcg_update = the row updates (pcg_rows_kernel), pcg_precond = the preconditioner launch."""
    E, Pf, Pt, Lf, Lt = fp.E, fp.Pf, fp.Pt, fp.Lf, fp.Lt
    Nc = int(round(6 * nc))
    edge_in = 40 * E                     # pose idx 4 + landmark idx 4 + 3 x 8 measurement + 8 information
    if upper:
        off = nblk - Pf                  # off-diagonal blocks
        return {
            "residual_chi2": edge_in + 24 * Lt + 96 * Pt,
            "linearize_schur": edge_in + (24 + 72) * Lf + 24 * (Lt - Lf) + 96 * Pt + 288 * nblk + 96 * Pf,
            "pcg_spmv": 288 * nblk + 8 * nblk + 48 * off + 4 * 48 * Pf,      # blocks once + (column, position) + parked products out + z, p in / p, q out
            "pcg_update": 48 * off + (4 + 2) * 48 * Pf,                      # parked products in + q, r, p, x in / r, x out
            "pcg_precond": 4 * Nc * ((Nc + 3) // 4 * 4) + 8 * Nc + (288 + 2 * 48) * Pf,   # fp32 coarse inverse + P^T r + block inverses, r in / z out
            "coarse_setup": 288 * nblk + 3 * 8 * Nc * Nc,
            "back_substitute": edge_in + (24 + 72 + 24) * Lf + (96 + 48) * Pt,
        }
    return {
        "residual_chi2": edge_in + 24 * Lt + 96 * Pt,
        "linearize_schur": edge_in + (24 + 72) * Lf + 24 * (Lt - Lf) + 96 * Pt + 288 * nblk + 96 * Pf,
        "pcg_spmv": 288 * nblk + 4 * 48 * Pf + 8 * (2 * nblk - Pf),     # blocks + z, p in / p, q out + (block, column) index pairs
        # two-level: fused update + restrict + preconditioner (one read of r, q, p, x, Minv, one of the coarse inverse -- stored in fp32,
        # rows padded to a multiple of 4 numbers: option precond_fp32, the fp64 library's default)
        "pcg_update": (288 + 6 * 48) * Pf if nc == 0 else (288 + 7 * 48) * Pf + 4 * Nc * ((Nc + 3) // 4 * 4),
        "pcg_precond": 8 * Nc * Nc + 8 * Nc + (288 + 2 * 48) * Pf,
        "coarse_setup": 288 * nblk + 3 * 8 * Nc * Nc,          # read Hsc once, write Ac, read+write it once more for the inverse
        "back_substitute": edge_in + (24 + 72 + 24) * Lf + (96 + 48) * Pt,
    }


def contract_wall_leg(shape, E, runs=5):
    """wall of initialize() + optimize(10) after a 1-iteration warm-up, through the C++ API
    (libcuda_bundle_adjustment.so -> C ABI), measured by the sample binary itself exactly where the reference's samples
    put their clock (samples/sample_comparison_with_g2o.cpp:74-79).  Host flattening, PCIe upload, structure analysis
    and write-back are inside."""
    import re
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host", "samples", "sample_ba_from_file")
    if not os.path.exists(exe):
        return None
    from cuba_amd.synth import synth_named
    res = {"protocol": "warm-up initialize()+optimize(1), then wall of initialize()+optimize(10) through the C++ API "
                       "(sample_ba_from_file); min and median of %d process runs" % runs, "iterations": LM_RUN}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "graph.json")
        synth_named(shape).to_json(path)
        for key, env in (("unchanged_topology", {}), ("new_topology", {"CUBA_HIP_NO_STRUCTURE_CACHE": "1"})):
            walls = []
            for _ in range(runs):
                r = subprocess.run([exe, path, str(LM_RUN), "1"], capture_output=True, text=True, timeout=600, env={**os.environ, **env})
                m = re.search(r"BA total\s*:\s*([0-9.eE+-]+)\s*\[sec\]", r.stdout)
                if r.returncode == 0 and m:
                    walls.append(float(m.group(1)))
            if not walls:
                res[key] = None
                continue
            best, med = min(walls), float(np.median(walls))
            res[key] = {"wall_ms": best * 1e3, "wall_ms_median": med * 1e3, "edges_per_s_strict": E / best,
                        "edge_iterations_per_s": E * LM_RUN / best}
    return res


def source_sha16():
    """Identity of the device-side sources the running library was built from -- every .hip / .hpp under csrc/, launch orders and
    block lists of ba_solver.hip / ba_structure.hip included (round-3 verdict: the Schur block order lives there) -- a PMC traffic
    file records the same at profiling time (scripts/pmc_traffic.py)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc")
    for f in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))):
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    return h.hexdigest()[:16]


# bench-line kernel key -> kernel names in the rocprofv3 outputs (template instantiations carry their arguments in the name)
PROFILE_NAMES = {"pcg_spmv": ["pcg_spmv_kernel", "pcg_spmv_row_kernel", "pcg_spmv_upper_kernel"], "pcg_update": ["pcg_rows_kernel", "pcg2_fused_kernel"],
                 "residual_chi2": ["residual_chi2_kernel"], "back_substitute": ["back_substitute_kernel"],
                 "linearize_schur": ["lm_pass_kernel<1", "schur_pass_kernel"], "pcg_precond": ["pcg2_fused_kernel|true>"]}


def newest_profile(pattern):
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), key=os.path.getmtime)
    return files[-1] if files else None


def reference_kernels_citation():
    """NOT measured by this run: the committed record of the reference's own kernels (its CUDA sources compiled for gfx950 as they are) timed by
    the reference's own stage timers on an MI355X beside this library's stage timers (tests/test_ref_lm.py::test_reference_stage_times_on_this_gpu
    writes it; bench.py only quotes the file)."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*reference_kernels_on_mi355x_stage_times.txt")))
    if not files:
        return None
    out = {"source": os.path.relpath(files[-1], ROOT), "measured_by_this_run": False,
           "what": "stages 2 Compute Error + 3 Build System + 4 Schur Complement + 7 Update Solution of initialize() + optimize(10), ms: "
                   "the reference's kernels on the MI355X | this library (stage timers on)"}
    shape = None
    for ln in open(files[-1]):
        m = re.match(r"\[(\w+)\]", ln)
        if m:
            shape = m.group(1)
        m = re.match(r"\s*kernel stages 2 \+ 3 \+ 4 \+ 7\s+([\d.]+) ms \|\s+([\d.]+) ms", ln)
        if m and shape:
            out[shape] = {"reference_kernels_ms": float(m.group(1)), "this_library_ms": float(m.group(2)),
                          "ratio": float(m.group(1)) / max(float(m.group(2)), 1e-9)}
    return out


def profile_evidence(shape, keys):
    """What the committed rocprofv3 outputs of this shape say about the bench line's kernels: HBM-side traffic per launch (PMC
    FETCH_SIZE / WRITE_SIZE, separate passes, profiles/*_<shape>_pmc_traffic.json: raw and fetch-doubled as MI355X_MICROARCH.md
    prescribes for gfx950) and the kernel-trace average duration (profiles/*_<shape>_kernel_stats.csv) -- so that the line can be
    recomputed without opening profiles/ (round-4 verdict).  A kernel key that stands for two kernels (linearise + Schur) gets sums;
    of several instantiations of one name the most-launched one counts."""
    import csv
    import re
    ev = {"pmc_file": None, "stats_file": None, "stale": None, "kernels": {}}
    # (the traffic file taken with THESE kernel sources if there is one -- file times do not survive a checkout --, else the newest; the
    # kernel-trace statistics of the same profiling round beside it)
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", f"*_{shape}_pmc_traffic.json")), key=lambda f: (os.path.getmtime(f), f))
    same = [f for f in cands if json.load(open(f)).get("kernel_source_sha16") == source_sha16()]
    pmc_path = (same or cands or [None])[-1]
    stats_path = newest_profile(f"*_{shape}_kernel_stats.csv")
    if pmc_path:
        twin = pmc_path.replace("_pmc_traffic.json", "_kernel_stats.csv")
        if os.path.exists(twin):
            stats_path = twin
    pk, sk = {}, {}
    if pmc_path:
        pj = json.load(open(pmc_path))
        pk = pj["kernels"]
        ev["pmc_file"] = os.path.basename(pmc_path)
        ev["stale"] = pj.get("kernel_source_sha16") != source_sha16()
    if stats_path:
        ev["stats_file"] = os.path.basename(stats_path)
        for row in csv.DictReader(open(stats_path)):
            nm = re.sub(r"\(.*", "", row["Name"]).replace("cubahip::", "").replace("void ", "").strip()
            sk[nm] = {"launches": int(row["Calls"]), "avg_ns": float(row["AverageNs"])}

    def find(table, name):
        # ("name|suffix": an instantiation picked by the end of its argument list -- the fused kernel's preconditioner-only form ends in "true>")
        name, _, suffix = name.partition("|")
        hits = [v for k, v in table.items() if (k == name or k.startswith(name + "<") or (name.endswith("<1") and k.startswith(name)))
                and (not suffix or k.endswith(suffix)) and not (not suffix and name == "pcg2_fused_kernel" and k.endswith("true>"))]
        return max(hits, key=lambda v: v["launches"]) if hits else None
    for key in keys:
        rec = {}
        names = PROFILE_NAMES.get(key, [])
        if key == "linearize_schur":
            groups = [[n] for n in names]                 # two kernels, both counted
        else:
            groups = [names]                             # alternatives: the one that ran
        pm = [next((f for f in (find(pk, n) for n in g) if f), None) for g in groups]
        if pm and all(pm):
            rec["traffic"] = sum(f["hbm_bytes_fetch_x2"] for f in pm)
            rec["traffic_raw"] = sum(f["hbm_bytes_raw"] for f in pm)
        stt = [next((f for f in (find(sk, n) for n in g) if f), None) for g in groups]
        if stt and all(stt):
            rec["rocprof_avg_ms"] = sum(f["avg_ns"] for f in stt) * 1e-6
        if rec:
            ev["kernels"][key] = rec
    return ev


def kernel_table(kt, alg, evidence):
    """per-kernel records of a roofline leg: HIP-event time, algorithmic bytes, achieved GB/s + the profile evidence"""
    table = {}
    for k, ms in kt.items():
        if ms <= 0 or k not in alg:
            continue
        rec = {"ms_per_launch": ms, "alg_bytes": alg[k], "achieved_GBs": alg[k] / (ms * 1e-3) / 1e9}
        e = evidence["kernels"].get(k, {})
        rec.update(e)
        if "traffic" in e:
            rec["traffic_over_alg"] = e["traffic"] / alg[k]
            rec["traffic_raw_over_alg"] = e["traffic_raw"] / alg[k]
        table[k] = rec
    return table


PERTURB = {"sigma_t_m": 0.01, "sigma_X_m": 0.01, "sigma_r_deg": 0.05}
HEURISTICS = ("heuristics",)


def perturbed_states(q, t, X, Pf, Lf, n, seed):
    """n seeded perturbations of an estimate (solver order: free vertices first): N(0, 1 cm) on free translations and landmarks,
    rotations of the free poses composed with exp(N(0, 0.05 deg)) -- the starts of the non-replay timed runs."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q2, t2, X2 = q.copy(), t.copy(), X.copy()
        t2[:Pf] += rng.normal(0, PERTURB["sigma_t_m"], (Pf, 3))
        X2[:Lf] += rng.normal(0, PERTURB["sigma_X_m"], (Lf, 3))
        dq = Rotation.from_rotvec(rng.normal(0, np.deg2rad(PERTURB["sigma_r_deg"]), (Pf, 3)))
        q2[:Pf] = (dq * Rotation.from_quat(q[:Pf])).as_quat()
        out.append((q2, t2, X2))
    return out


def prepare_slots(h, fp, warm, n, seed):
    """slot 0 = the warm state itself (replay protocol), slots 1..n = perturbed starts (uploaded and copied device-side, untimed)"""
    h.set_state(*warm); h.snapshot_state(0)
    for k, st in enumerate(perturbed_states(*warm, fp.Pf, fp.Lf, n, seed)):
        h.set_state(*st); h.snapshot_state(1 + k)
    h.restore_state(0)
    return n


DUMP_MAX_BYTES = 64 << 20


def timed_outputs(chi2, q, t, X):
    """What a caller of the timed path receives from its last LM run: the per-iteration chi2 and the estimates (solver row order).
    Landmarks beyond the dump budget are cut to a fixed, seeded sample of rows (their indices are dumped beside them)."""
    out = {"chi2": np.asarray(chi2, dtype=np.float64), "pose_q": q, "pose_t": t, "landmarks": X}
    room = DUMP_MAX_BYTES - sum(a.nbytes for k, a in out.items() if k != "landmarks")
    if X.nbytes > room:
        keep = room // (X.itemsize * X.shape[1] + 8)
        rows = np.sort(np.random.default_rng(0).choice(len(X), size=keep, replace=False))
        out["landmarks"], out["landmark_rows"] = X[rows], rows.astype(np.float64)
    return out


def write_outputs(path, outputs):
    os.makedirs(path, exist_ok=True)
    for name, a in outputs.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    return {"dir": path, "arrays": {k: list(a.shape) for k, a in outputs.items()}}


def fp32_bars():
    """FP32_TOL / FP32_MIN_ITERATIONS of tests/test_gpu_configs.py, read from the file (importing it would pull pytest fixtures in)"""
    import ast
    import re
    src = open(os.path.join(ROOT, "tests", "test_gpu_configs.py")).read()
    tol = ast.literal_eval(re.search(r"^FP32_TOL = (\{.*?\})", src, re.M).group(1))
    return tol, int(re.search(r"^FP32_MIN_ITERATIONS = (\d+)", src, re.M).group(1))


def exact_solve_probe(h):
    """The exact reduced solve (sparse tile Cholesky, csrc/ba_direct.hip; the seat of the reference's SparseLinearSolver::solve) on the damped
    system of the handle's current estimate: what the fallback costs when a solve needs it -- wall of cuba_hip_solve_reduced with
    "reduced_solver" = 1 (median of 5; the first call also pays ordering + symbolic analysis) and the increment against the PCG's at
    pcg_tol 1e-12.  Changes the handle's options: call it last."""
    import torch
    try:
        lam = 1e-5 * h.max_diagonal(); h.set_lambda(lam)
        h.set_option("pcg_tol", 1e-12); h.set_option("direct_fallback", 0); h.schur(); ok_pcg = h.solve_reduced(); x_pcg = h.array("xp")
        h.set_option("direct_fallback", 1); h.set_option("reduced_solver", 1)
        ts = []
        for _ in range(6):
            h.schur(); torch.cuda.synchronize(); t = time.perf_counter(); ok = h.solve_reduced(); ts.append(time.perf_counter() - t)
        x_ex = h.array("xp")
        return {"ms": float(np.median(ts[1:])) * 1e3, "first_call_ms_with_symbolic_phase": ts[0] * 1e3, "ok": bool(ok and ok_pcg),
                "increment_max_rel_diff_vs_pcg_tol_1e-12": float(np.abs(x_ex - x_pcg).max() / np.abs(x_pcg).max())}
    except Exception as e:   # noqa: BLE001
        return {"error": repr(e)[:200]}


def shapes_leg(rk, device_index, stream, names=("kitti07", "s2m", "g4m"), runs=3, cpu=True):
    """Driver-timed numbers for the single-GPU BASELINE configurations the headline shape is not: for each shape one parity run
    (10 LM iterations from the generator's initial guess, per-iteration chi2 against the oracle) and `runs` timed runs under the
    bench protocol (1-iteration warm-up, then optimize(10) from that state, graph resident)."""
    import torch
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import flatten
    from cuba_amd.synth import synth_named
    gpath = os.path.join(ROOT, "tests", "golden", "baseline_shapes_chi2.json")
    golden = json.load(open(gpath))["shapes"] if os.path.exists(gpath) else {}
    res, cpu_jobs = {}, []
    for name in names:
        try:
            fp = flatten(synth_named(name))
            h = HipSolver(fp, rk, device=device_index, stream=stream)
            got = h.optimize(LM_RUN)["chi2"]
            rec = {"poses": fp.Pt, "landmarks": fp.Lt, "edges": fp.E, "chi2_first": float(got[0]), "chi2_last": float(got[-1])}
            if name in golden and len(golden[name]["chi2"]) == len(got):
                ref = np.array(golden[name]["chi2"])
                rec["chi2_max_rel_diff_vs_golden"] = float(np.max(np.abs(got - ref) / ref))
            h.set_state(fp.q, fp.t, fp.Xw)
            h.optimize(1)                                    # the protocol's warm-up iteration
            q1, t1, X1 = h.state()
            nslots = prepare_slots(h, fp, (q1, t1, X1), runs + 1, seed=1000)

            def timed(slot):
                h.restore_state(slot)
                c0 = h.counters()
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = h.optimize(LM_RUN)["chi2"]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                if len(r) != LM_RUN:
                    raise RuntimeError(f"LM stopped after {len(r)} iterations")
                return dt, h.counters()["pcg_iterations"] - c0["pcg_iterations"]
            timed(nslots)                                    # untimed first run on the structure (hipGraph instantiation), its own start
            walls, iters = zip(*[timed(1 + k) for k in range(runs)])             # every timed run from its own perturbed start
            timed(0)
            replay, _ = zip(*[timed(0) for _ in range(runs)])                    # rounds 1-3 protocol: the same start every time
            med = float(np.median(walls))
            rec.update({"wall_ms_10iter": med * 1e3, "wall_ms_10iter_min": min(walls) * 1e3, "wall_ms_10iter_max": max(walls) * 1e3,
                        "wall_ms_10iter_replay": float(np.median(replay)) * 1e3,
                        "runs": runs, "edge_iterations_per_s": fp.E * LM_RUN / med, "pcg_iterations_per_run": int(np.median(iters)),
                        "hsc_blocks": h.counters()["hsc_blocks"], "coarse_dim": h.counters()["coarse_dim"],
                        "unconverged_solves": h.pcg_history()[1], "exact_solve_fallbacks": h.counter("exact_solve_fallbacks")})
            # roofline of this shape: HIP-event time of each hot kernel on the solver's stream, its algorithmic bytes, and what the
            # committed rocprofv3 outputs of the shape say (traffic, kernel-trace average).  The kernel named is the SpMV -- the one
            # bandwidth-bound kernel of the path on the large shapes -- whichever kernel has the largest share is given beside it.
            try:
                c = h.counters()
                kt = {k: v for k, v in h.time_kernels(reps=10).items() if v > 0}
                upper = kt.get("pcg_precond", 0) > 0 and kt.get("coarse_setup", 0) > 0        # (the two-launch iteration has no separate preconditioner launch)
                alg = algorithmic_bytes(fp, c["hsc_blocks"], c["coarse_dim"] / 6.0 if kt.get("coarse_setup", 0) > 0 else 0, upper=upper)
                ev = profile_evidence(name, list(kt))
                table = kernel_table(kt, alg, ev)
                it_per_run = int(np.median(iters))
                share = {"pcg_spmv": it_per_run, "pcg_update": it_per_run, "pcg_precond": it_per_run if upper else 0}
                dom = max(share, key=lambda k: share[k] * kt.get(k, 0))
                sp = table.get("pcg_spmv")
                if sp:
                    rec["roofline"] = {"bound": "hbm", "kernel": "pcg_spmv", "achieved": sp["achieved_GBs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                       "frac": sp["achieved_GBs"] / HBM_PEAK_GBS, "traffic": sp.get("traffic"), "alg_bytes_per_launch": sp["alg_bytes"],
                                       "ms_per_launch": sp["ms_per_launch"], "largest_share": dom, "iteration": "upper-triangle, three launches" if upper else "two launches",
                                       "traffic_source": ev["pmc_file"],
                                       "traffic_stale": ev["stale"], "rocprof_source": ev["stats_file"], "kernels": table}
            except Exception as e:   # noqa: BLE001
                rec["roofline"] = {"error": repr(e)[:200]}
            h.restore_state(0)
            rec["exact_solve"] = exact_solve_probe(h)
            if name == "kitti07" and cpu:
                cpu_jobs.append((name, fp, got, (q1, t1, X1)))
            h.close()
            res[name] = rec
        except Exception as e:   # noqa: BLE001  -- one shape failing must not take the line down
            res[name] = {"error": repr(e)[:300]}
    # the CPU legs come after every GPU timing: the OpenMP runtime's worker threads keep spinning for a while after a parallel
    # region and slow the launch-latency-bound GPU runs down (KITTI-07: 7.8 instead of 4.2 ms when timed after them)
    for name, fp, got, (q1, t1, X1) in cpu_jobs:
        try:
            rec = res[name]
            # BASELINE configs[0] is the CPU-path configuration: the oracle on the host cores, same graph, same protocol
            from oracle.oracle import OracleSolver
            ref = OracleSolver(fp, rk).optimize(LM_RUN)["chi2"]
            rec["chi2_max_rel_diff_vs_oracle"] = float(np.max(np.abs(got - ref) / ref))
            base = {}
            ncpu = os.cpu_count() or 1
            for threads in sorted({1, min(ncpu, 8), min(ncpu, 16), min(ncpu, 32)}):
                orc = OracleSolver(fp, rk, threads=threads)
                orc.build_structure()
                orc.set_state(q1, t1, X1)
                tc = time.perf_counter(); r = orc.optimize(LM_RUN); tc = time.perf_counter() - tc
                base["threads_%d" % orc.threads] = {"value": fp.E * len(r["chi2"]) / tc, "unit": "edges/s", "cores": orc.threads, "seconds": tc}
            best = max(base.values(), key=lambda b: b["value"])
            rec["cpu_baseline"] = {"value": best["value"], "unit": "edges/s", "cores": best["cores"], "kind": "port", "nproc": ncpu,
                                   "sample": "10 LM iterations of oracle/ba_oracle.cpp from the same warm state (structure analysis excluded)",
                                   "thread_sweep_edges_per_s": {k: v["value"] for k, v in base.items()},
                                   "single_thread_seconds": base["threads_1"]["seconds"]}
        except Exception as e:   # noqa: BLE001
            res[name]["cpu_baseline"] = {"error": repr(e)[:300]}
    return res


def float32_leg(rk, device_index, stream, names=("kitti00", "g4m"), runs=3):
    """BASELINE configs[4]'s "plus USE_FLOAT32 variant" (the reference: src/scalar.h:25-29, README "no significant speedup"): the all-fp32
    library (libcuba_hip_f32.so) under the bench protocol on the headline shape and on configs[4]'s graph -- wall of 10 LM iterations from
    perturbed starts, iterations actually run (an fp32 run may stop early), chi2 of a run from the generator's guess against the fp64 golden."""
    import torch
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import flatten
    from cuba_amd.synth import synth_named
    gpath = os.path.join(ROOT, "tests", "golden", "baseline_shapes_chi2.json")
    golden = json.load(open(gpath))["shapes"] if os.path.exists(gpath) else {}
    res = {}
    for name in names:
        try:
            fp = flatten(synth_named(name))
            h = HipSolver(fp, rk, device=device_index, stream=stream, precision="f32")
            got = h.optimize(LM_RUN)["chi2"]
            rec = {"edges": fp.E, "iterations_run": len(got), "chi2_last": float(got[-1]) if len(got) else None}
            if name in golden and len(got):
                ref = np.array(golden[name]["chi2"])[:len(got)]
                rec["chi2_max_rel_diff_vs_fp64_golden"] = float(np.max(np.abs(got - ref) / ref))
                # the stated fp32 bar of this shape (one table: tests/test_gpu_configs.py, FP32_TOL / FP32_MIN_ITERATIONS)
                bar, min_it = fp32_bars()
                if name in bar:
                    rec["chi2_bar"] = bar[name]; rec["min_iterations"] = min_it
                    rec["within_bar"] = bool(rec["chi2_max_rel_diff_vs_fp64_golden"] <= bar[name] and len(got) >= min_it)
            h.set_state(fp.q, fp.t, fp.Xw); h.optimize(1)
            nslots = prepare_slots(h, fp, h.state(), runs + 1, seed=1000)

            def timed(slot):
                h.restore_state(slot)
                torch.cuda.synchronize(); t = time.perf_counter(); r = h.optimize(LM_RUN)["chi2"]; torch.cuda.synchronize()
                return time.perf_counter() - t, len(r)
            timed(nslots)
            walls, its = zip(*[timed(1 + k) for k in range(runs)])
            rec.update({"wall_ms_10iter": float(np.median(walls)) * 1e3, "wall_ms_10iter_min": min(walls) * 1e3, "iterations_in_timed_runs": list(its),
                        "edge_iterations_per_s": fp.E * float(np.median(its)) / float(np.median(walls))})
            h.close()
            res[name] = rec
        except Exception as e:   # noqa: BLE001
            res[name] = {"error": repr(e)[:300]}
    return res


def concurrent_child(shape, counts=(2, 4), runs=5):
    """(child process of concurrent_leg) N handles on ONE GPU, one host thread each, every thread optimising its own copy of the graph"""
    import threading
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import flatten
    from cuba_amd.synth import synth_named
    rk = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))
    fp = flatten(synth_named(shape))
    hs = []
    for _ in range(max(counts)):
        h = HipSolver(fp, rk); h.optimize(1); h.snapshot_state(); h.optimize(LM_RUN); hs.append(h)

    def timed(h):
        ts, chi = [], None
        for _ in range(runs):
            h.restore_state(); t = time.perf_counter(); chi = h.optimize(LM_RUN)["chi2"]; ts.append(time.perf_counter() - t)
        return float(np.median(ts)), chi
    solo, chi_solo = timed(hs[0])
    out = {"shape": shape, "edges": fp.E, "graphs_env": os.environ.get("CUBA_HIP_GRAPHS", "0"), "solo_wall_ms_10iter": solo * 1e3,
           "solo_with_idle_handles_alive": len(hs), "runs_per_thread": runs, "groups": {}}
    for n in counts:
        group, res = hs[:n], [None] * n
        bar = threading.Barrier(n + 1)

        def work(i):
            bar.wait()
            res[i] = timed(group[i])
        th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
        [t.start() for t in th]
        bar.wait(); t0 = time.perf_counter()
        [t.join() for t in th]
        wall = time.perf_counter() - t0
        rate = n * runs * LM_RUN * fp.E / wall
        out["groups"][str(n)] = {"per_graph_wall_ms_10iter": [r[0] * 1e3 for r in res], "aggregate_edge_iterations_per_s": rate,
                                 "throughput_vs_one_graph": rate / (LM_RUN * fp.E / solo),
                                 "bit_identical_to_solo": bool(all(np.array_equal(r[1], chi_solo) for r in res))}
    # the same graphs as ONE batch from ONE thread (cuba_hip_optimize_batch: the PCG iterations of all graphs in one launch chain)
    from cuba_amd.capi import optimize_batch
    out["batch"] = {}
    for n in counts:
        group = hs[:n]
        ts, chis, batched = [], None, 0
        for _ in range(runs + 1):
            for h in group:
                h.restore_state()
            t = time.perf_counter(); chis, batched = optimize_batch(group, LM_RUN); ts.append(time.perf_counter() - t)
        wall = float(np.median(ts[1:]))
        rate = n * LM_RUN * fp.E / wall
        out["batch"][str(n)] = {"wall_ms_10iter_all_graphs": wall * 1e3, "aggregate_edge_iterations_per_s": rate, "throughput_vs_one_graph": rate / (LM_RUN * fp.E / solo),
                                "batched_reduced_solves": batched, "bit_identical_to_solo": bool(all(np.array_equal(c, chi_solo) for c in chis))}
    for h in hs:
        h.close()
    print("CONCURRENT " + json.dumps(out), flush=True)


def concurrent_leg(shape):
    """2 and 4 graphs of the bench shape optimised concurrently on ONE GPU from distinct host threads (include/cuba_hip.h: distinct handles
    may be driven from distinct threads; the reference's CudaBundleAdjustment objects are independent, include/cuda_bundle_adjustment.h:34-125
    -- ORB-SLAM's local and global BA).  Measured in child processes because the property is a process-wide one on this runtime: once a
    process has instantiated a hipGraph the kernel chains of two streams no longer overlap, so the leg runs both
    ways -- the default (hipGraphs are opt-in since round 6) and CUBA_HIP_GRAPHS=1."""
    import subprocess
    res = {}
    for label, env, shp, counts in (("default", {}, shape, "2,4"), ("graphs_on", {"CUBA_HIP_GRAPHS": "1"}, shape, "2,4"), ("kitti07_default", {}, "kitti07", "8")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--concurrent-child", "--shape", shp, "--concurrent-counts", counts],
                               capture_output=True, text=True, timeout=300, env={**os.environ, **env})
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("CONCURRENT ")), None)
            res[label] = json.loads(line[len("CONCURRENT "):]) if line else {"error": (r.stderr or r.stdout)[-300:]}
        except Exception as e:   # noqa: BLE001
            res[label] = {"error": repr(e)[:300]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline: parity against the committed oracle trajectories, repeats, "
                         "replay and heuristics-off protocols, roofline, exact solve, other shapes, fp32, concurrent handles, CPU "
                         "baseline, the C++-API wall and (N > 1) the landmark-partitioned leg")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the oracle parity leg")
    ap.add_argument("--no-end-to-end", action="store_true", help="with --full: skip the C++-API leg (the reference's sample protocol)")
    ap.add_argument("--no-shapes", action="store_true", help="with --full: skip the kitti07 / s2m / g4m legs (N = 1 only)")
    ap.add_argument("--repeats", type=int, default=5, help="with --full: further timed blocks of --steps steps for the median / min / max")
    ap.add_argument("--concurrent-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--concurrent-counts", default="2,4", help=argparse.SUPPRESS)
    ap.add_argument("--no-concurrent", action="store_true", help="with --full: skip the concurrent-handles leg (N = 1 only)")
    ap.add_argument("--partition", action="store_true",
                    help="N>1: ONE graph, landmark-partitioned over the ranks with an RCCL all-reduce of [Hsc|bsc|bp] "
                         "per trial (BASELINE config 5, strong scaling) instead of one independent graph per GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what their last LM run returned (rank 0: per-iteration chi2, pose and "
                         "landmark estimates) as DIR/<name>.npy, so that two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.concurrent_child:
        concurrent_child(args.shape, counts=tuple(int(v) for v in args.concurrent_counts.split(",")))
        return

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # one rank per GPU; the modulo only matters for dry runs of the N > 1 code path on a box with fewer GPUs
    # (CUBA_BENCH_BACKEND=gloo, several ranks sharing a device) -- RCCL itself needs distinct devices
    device_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(device_index)
    dist = None
    backend = os.environ.get("CUBA_BENCH_BACKEND", "nccl")
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group(backend)

    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import flatten
    from cuba_amd.synth import SHAPES, synth_named

    rk = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))
    partitioned = args.partition and world > 1
    seed = SHAPES[args.shape]["seed"] if (world == 1 or partitioned) else 100 + rank
    fp = flatten(synth_named(args.shape, seed=seed))
    if partitioned:
        # (the rank's upload: index arrays and estimates whole, measurements / information of its own landmarks' edges only)
        from cuba_amd.dist import landmark_ranges
        solver = HipSolver(None, rk, device=device_index, stream=torch.cuda.current_stream().cuda_stream)
        solver.set_graph(fp, landmark_range=landmark_ranges(fp.eL, fp.Lt, world)[rank])
    else:
        solver = HipSolver(fp, rk, device=device_index, stream=torch.cuda.current_stream().cuda_stream)
    comm = None
    native = None
    if partitioned:
        # native driver (libcuba_hip_dist.so): the LM loop in C++, RCCL collectives on the solver's stream; its communicator
        # is created from a unique id that rank 0 hands out through the torch process group.  CUBA_BENCH_BACKEND=gloo (dry
        # runs on a box with fewer GPUs than ranks) uses the torch group for the collectives instead.
        from cuba_amd.dist import NativeDist, TorchComm, rccl_unique_id
        if backend == "nccl":
            ids = [rccl_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ids, src=0)
            native = NativeDist(solver, fp, rank, world, unique_id=ids[0])
        else:
            native = NativeDist(solver, fp, rank, world, comm=TorchComm())

        def partitioned_optimize(_backend, _comm, n):
            return native.optimize(n)
    solver.build_structure()
    # ---- parity of THIS rank's graph before anything is timed: 10 iterations from the generator's initial guess against the committed
    # oracle trajectory (tests/golden: baseline_shapes_chi2.json for the shape's own seed, config4_seeds_chi2.json for the graphs
    # of the N > 1 weak mode, seeds 100 + rank) -- protocol of samples/sample_comparison_with_g2o.cpp:89-110, per graph
    def optimize(n):
        return partitioned_optimize(backend, comm, n) if partitioned else solver.optimize(n)["chi2"]

    def golden_chi2():
        try:
            if seed == SHAPES[args.shape]["seed"]:
                return json.load(open(os.path.join(ROOT, "tests", "golden", "baseline_shapes_chi2.json")))["shapes"][args.shape]["chi2"]
            if args.shape == "kitti00":
                return json.load(open(os.path.join(ROOT, "tests", "golden", "config4_seeds_chi2.json")))["seeds"][str(seed)]["chi2"]
        except (OSError, KeyError):
            pass
        return None
    parity = None
    if args.full:
        parity = {"rank": rank, "seed": seed, "chi2_max_rel_diff_vs_golden": None}
        gold = golden_chi2()
        got0 = optimize(LM_RUN)
        if gold is not None and len(gold) == len(got0):
            parity["chi2_max_rel_diff_vs_golden"] = float(np.max(np.abs(got0 - np.array(gold)) / np.array(gold)))
        parity["chi2_last"] = float(got0[-1]) if len(got0) else None
        solver.set_state(fp.q, fp.t, fp.Xw)
    # the reference protocol's warm-up: one LM iteration from the initial guess moves the estimates; the timed runs of
    # optimize(10) start from there (sample_comparison_with_g2o.cpp:303-307) -- each from its own perturbation of that estimate
    optimize(1)
    q0, t0, X0 = solver.state()
    repeats = max(0, args.repeats) if args.full else 0
    total_runs = (args.warmup + LM_RUN - 1) // LM_RUN + (1 + repeats) * ((args.steps + LM_RUN - 1) // LM_RUN)
    nslots = prepare_slots(solver, fp, (q0, t0, X0), max(2, min(48, total_runs)), seed=1000 + rank)
    next_slot = [0]

    def run_steps(k, replay=False):
        """k LM iterations as runs of LM_RUN iterations, each from its own perturbed start (replay: all from the warm state itself).
        Returns chi2 of the last run."""
        chi2, left = None, k
        while left > 0:
            n = min(LM_RUN, left)
            if replay:
                solver.restore_state(0)
            else:
                solver.restore_state(1 + next_slot[0] % nslots); next_slot[0] += 1
            chi2 = optimize(n)
            if len(chi2) != n:
                raise RuntimeError(f"LM stopped after {len(chi2)} of {n} iterations")
            left -= n
        return chi2

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(seconds):
        if dist is None:
            return seconds
        tt = torch.tensor([seconds], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    def timed_block(k, replay=False):
        fence()
        tb = time.perf_counter()
        chi2 = run_steps(k, replay)
        fence()
        return max_over_ranks(time.perf_counter() - tb), chi2

    def counters():
        c = solver.counters()
        c["coarse_inline_inversions"] = solver.counter("coarse_inline_inversions")
        c["pcg_graph_instantiations"] = solver.counter("pcg_graph_instantiations")
        c["exact_solve_fallbacks"] = solver.counter("exact_solve_fallbacks")
        c["late_decision_records"] = solver.counter("late_decision_records")
        if native is not None:
            c["lm_trials"] = native.counters()["lm_trials"]      # the native driver runs the trial loop, not the solver handle
        return c

    if args.warmup > 0:
        run_steps(args.warmup)
    c0 = counters()
    elapsed, chi2 = timed_block(args.steps)
    c1 = counters()
    outputs = timed_outputs(chi2, *solver.state()) if args.dump_outputs and rank == 0 else None

    if args.full:
        # the same block again, `--repeats` times (further perturbed starts): spread of the measurement (`value` stays the block above)
        block_ms = [timed_block(args.steps)[0] * 1e3 for _ in range(repeats)]

        # ---- the protocol of rounds 1-3 beside it (every run from the SAME estimate), and both protocols with the three replay-exact
        # heuristics switched off: what they are worth, in the driver's line
        run_steps(LM_RUN, replay=True)
        replay_s, _ = timed_block(args.steps, replay=True)
        for k in HEURISTICS:
            solver.set_option(k, 0)
        run_steps(LM_RUN)
        hoff_s, _ = timed_block(args.steps)
        run_steps(LM_RUN, replay=True)
        hoff_replay_s, _ = timed_block(args.steps, replay=True)
        for k in HEURISTICS:
            solver.set_option(k, 1)
        rank_parity = [parity]
        if dist is not None:
            rank_parity = [None] * world
            dist.all_gather_object(rank_parity, parity)

    pcg_iters = c1["pcg_iterations"] - c0["pcg_iterations"]
    trials = c1["lm_trials"] - c0["lm_trials"]
    E = fp.E
    graphs = 1 if partitioned else world
    value = E * args.steps * graphs / elapsed
    nblk = c1["hsc_blocks"]

    out = None
    if rank == 0 and args.full:
        # ---- roofline leg: per-kernel device time from HIP events on the solver's stream ------------
        solver.set_state(q0, t0, X0)
        kt = solver.time_kernels(reps=20)
        nc = 0 if kt["coarse_setup"] == 0 else c1["coarse_dim"] / 6.0        # algorithmic_bytes() takes the coarse dimension / 6
        alg = algorithmic_bytes(fp, nblk, nc, upper=kt.get("pcg_precond", 0) > 0 and kt.get("coarse_setup", 0) > 0)
        launches = {"residual_chi2": trials + args.steps, "linearize_schur": trials, "pcg_spmv": pcg_iters,
                    "pcg_update": pcg_iters, "back_substitute": trials, "pcg_precond": pcg_iters + trials,
                    "coarse_setup": c1["coarse_refreshes"] - c0["coarse_refreshes"]}
        kt = {k: v for k, v in kt.items() if v > 0}
        # the coarse inverse is rebuilt on a second stream under the PCG of an earlier trial: the
        # per-kernel table charges the work stream with the inversions the library COUNTED there (cuba_hip_get_counter
        # "coarse_inline_inversions"), the rest is off the timed path
        refreshes = launches["coarse_setup"]
        launches["coarse_setup"] = c1["coarse_inline_inversions"] - c0["coarse_inline_inversions"]
        share = {k: kt[k] * launches[k] for k in kt}
        dom = max(share, key=share.get)
        # measured HBM-side traffic (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; FETCH_SIZE doubled as MI355X_MICROARCH.md
        # prescribes for gfx950, the raw sum beside it) and the kernel-trace average duration of EVERY kernel of the table, from the
        # newest committed profiles of this shape (written by scripts/profile_round.sh).  They are profiles of an EARLIER run of this
        # command, so the traffic file is checked against the running build: it records the hash of the kernel sources it was taken
        # with (scripts/pmc_traffic.py); a file from other sources is still quoted but flagged `traffic_stale`.
        ev = profile_evidence(args.shape, list(kt))
        kernels = kernel_table(kt, alg, ev)
        for k in kernels:
            kernels[k]["launches"] = launches[k]
        if "coarse_setup" in kernels:
            kernels["coarse_setup"]["launches_on_second_stream"] = refreshes - launches["coarse_setup"]
        traffic = kernels[dom].get("traffic")
        traffic_stale = ev["stale"] if traffic is not None else None
        pmc_path = ev["pmc_file"] or ""
        # whole hot path: B_alg(trial) = 120 E3 + 96 E2 + 288 L + 2 * 288 nblk, achieved = B_alg x trials / t_hot.
        # The PCG's re-reads of the (L2 / Infinity-Cache resident) reduced matrix are deliberately NOT counted as HBM bytes.
        b_trial = 120 * fp.E3 + 96 * fp.E2 + 288 * fp.Lt + 2 * 288 * nblk
        path_gbs = b_trial * trials / elapsed / 1e9
        path = {"B_alg_per_trial": b_trial, "trials": trials, "t_hot_ms": elapsed * 1e3, "GBs": path_gbs,
                "frac_8.0": path_gbs / 8000.0, "frac_6.3": path_gbs / 6300.0,
                "pcg_iterations_per_trial": pcg_iters / max(trials, 1),
                "note": "latency-bound path: ~%d dependent kernel launches per trial, HBM roofline wall of the run would be %.2f ms"
                        % (round(2 * pcg_iters / max(trials, 1)) + 12, b_trial * trials / 6.3e12 * 1e3)}
        # headline fraction from the rocprofv3 kernel-trace average the committed profile reproduces (round-5 verdict); the live HIP-event
        # figure stays beside it (`frac_hip_events`, `achieved_hip_events`) and is the fallback when no profile of this shape is committed
        rp_ms = kernels[dom].get("rocprof_avg_ms")
        ach_events = kernels[dom]["achieved_GBs"]
        ach = alg[dom] / (rp_ms * 1e-3) / 1e9 if rp_ms else ach_events
        worst = max((k for k in kernels if "traffic_over_alg" in kernels[k]), key=lambda k: kernels[k]["traffic_over_alg"], default=None)
        roof = {"bound": "hbm", "kernel": dom, "achieved": ach, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "frac_source": "rocprof_avg_ms" if rp_ms else "hip_events",
                "achieved_hip_events": ach_events, "frac_hip_events": ach_events / HBM_PEAK_GBS, "traffic": traffic,
                "path_frac": path_gbs / HBM_PEAK_GBS,
                "worst_traffic_over_alg": kernels[worst]["traffic_over_alg"] if worst else None, "worst_traffic_kernel": worst,
                "alg_bytes_per_launch": alg[dom], "ms_per_launch": kt[dom], "rocprof_avg_ms": rp_ms,
                "traffic_source": os.path.basename(pmc_path) if traffic else None, "rocprof_source": ev["stats_file"],
                "traffic_stale": traffic_stale, "kernel_source_sha16": source_sha16(),
                "kernels": kernels, "path": path}
    if rank == 0:
        out = {
            "metric": "edges/sec (edge-iterations/s = E x LM iterations / wall, graph resident in HBM, every timed 10-iteration run from its own "
                      "perturbed start) + 10-iter LM wall-clock (contract_wall: initialize()+optimize(10) after warm-up, C++ API) on KITTI-00-shaped "
                      "graph; per-iter chi2 vs g2o-faithful oracle",
            "value": value, "unit": "edge-iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed * 1e3 / args.steps, "higher_is_better": True, "scaling": "strong" if partitioned else "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"ba_{args.shape}-shaped synthetic stereo graph, {LM_RUN}-iteration LM runs, Huber",
                       "poses": fp.Pt, "landmarks": fp.Lt, "edges": E, "graphs": graphs,
                       "parallelism": ("1 graph landmark-partitioned over %d GPUs, 1 all-reduce per trial" % world) if partitioned
                       else ("1 graph per GPU (no collective)" if world > 1 else "single GPU")},
            "wall_ms_total": elapsed * 1e3,
            "wall_ms_10iter": elapsed * 1e3 * LM_RUN / args.steps,
            "edges_per_s_strict_10iter": E * graphs / (elapsed * LM_RUN / args.steps),
            "pcg_iterations": pcg_iters, "pcg_iterations_enqueued": c1["pcg_iterations_enqueued"] - c0["pcg_iterations_enqueued"],
            "pcg_host_looks": c1["pcg_host_looks"] - c0["pcg_host_looks"], "coarse_refreshes": c1["coarse_refreshes"] - c0["coarse_refreshes"],
            "lm_trials": trials, "hsc_blocks": nblk, "schur_products": c1["schur_products"],
            "coarse_inline_inversions": c1["coarse_inline_inversions"] - c0["coarse_inline_inversions"],
            "exact_solve_fallbacks": c1["exact_solve_fallbacks"] - c0["exact_solve_fallbacks"],
            "late_decision_records": c1["late_decision_records"],      # (life of the handle: LM decision records fetched behind a stream synchronisation; 0 in normal operation)
            "pcg_graph_instantiations_in_timed_region": c1["pcg_graph_instantiations"] - c0["pcg_graph_instantiations"],
            "final_chi2": float(chi2[-1]),
            "protocol": {"timed_runs": "each optimize(%d) from its own seeded perturbation of the warm state" % LM_RUN, **PERTURB,
                         "distinct_starts": nslots},
        }
        if args.full:
            out.update({
                "value_replay": E * args.steps * graphs / replay_s, "ms_per_step_replay": replay_s * 1e3 / args.steps,
                "heuristics_off": {"options": {k: 0 for k in HEURISTICS}, "value": E * args.steps * graphs / hoff_s,
                                   "ms_per_step": hoff_s * 1e3 / args.steps, "value_replay": E * args.steps * graphs / hoff_replay_s,
                                   "ms_per_step_replay": hoff_replay_s * 1e3 / args.steps},
                "rank_parity": rank_parity,
                "repeats": ({"blocks": len(block_ms), "steps_per_block": args.steps, "ms_per_step_median": float(np.median(block_ms)) / args.steps,
                             "ms_per_step_min": min(block_ms) / args.steps, "ms_per_step_max": max(block_ms) / args.steps,
                             "value_median": E * args.steps * graphs / (float(np.median(block_ms)) * 1e-3)} if block_ms else None),
                "roofline": roof,
                "reference_kernels_on_mi355x": reference_kernels_citation() if world == 1 else None,
            })
        if outputs is not None:
            out["dump_outputs"] = write_outputs(args.dump_outputs, outputs)
    if rank == 0 and args.full:
        # the GPU side of the parity leg, then this handle goes: several live handles share the runtime's few hardware queues and
        # slow each other down (a KITTI-07-sized graph runs at half speed as the second handle of a process)
        got = None
        if world == 1 and not args.no_cpu_baseline:
            solver.restore_state()
            got = solver.optimize(min(LM_RUN, args.steps))["chi2"]
        if world == 1:
            try:
                solver.restore_state()
            except Exception:   # noqa: BLE001
                pass
            out["exact_solve"] = exact_solve_probe(solver)
            solver.close()
        # ---- the other single-GPU BASELINE configurations, driver-timed in the same line (before any CPU leg: see shapes_leg) ----
        if world == 1 and not args.no_shapes and args.shape == "kitti00":
            out["shapes"] = shapes_leg(rk, device_index, torch.cuda.current_stream().cuda_stream, cpu=not args.no_cpu_baseline)
            out["float32"] = float32_leg(rk, device_index, torch.cuda.current_stream().cuda_stream)
        if world == 1 and not args.no_concurrent:
            out["concurrent"] = concurrent_leg(args.shape)
        # ---- CPU baseline + parity leg (rank 0, N = 1 only): the oracle on the host cores ------------
        if world == 1 and not args.no_cpu_baseline:
            from oracle.oracle import OracleSolver
            n = min(LM_RUN, args.steps)
            base = {}
            ref = None
            # all-core leg: the atomic accumulation into shared Hsc blocks stops scaling (and on a two-socket host turns
            # negative) long before 256 threads, so a few thread counts are tried and the fastest is the one reported
            ncpu = os.cpu_count() or 1
            sweep = sorted({min(ncpu, c) for c in (8, 16, 32, 64, ncpu)} - {1})
            for label, threads in [("single_thread", 1)] + [("threads_%d" % c, c) for c in sweep]:
                orc = OracleSolver(fp, rk, threads=threads)
                orc.build_structure()
                orc.set_state(q0, t0, X0)
                tc = time.perf_counter()
                r = orc.optimize(n)
                tc = time.perf_counter() - tc
                if threads == 1:
                    ref = r                       # the single-thread library is the parity checker (fixed summation order)
                base[label] = {"value": E * len(r["chi2"]) / tc, "unit": "edges/s", "cores": orc.threads, "seconds": tc}
            m = min(len(got), len(ref["chi2"]))
            multi = {k: v for k, v in base.items() if k != "single_thread"}
            base["all_cores"] = max(multi.values(), key=lambda b: b["value"]) if multi else base["single_thread"]
            base["all_cores"]["thread_sweep_edges_per_s"] = {k: v["value"] for k, v in multi.items()}
            best = max(base["single_thread"], base["all_cores"], key=lambda b: b["value"])
            out["cpu_baseline"] = {"value": best["value"], "unit": "edges/s", "cores": best["cores"], "kind": "port",
                                   "nproc": os.cpu_count(),
                                   "sample": f"same graph and start as the GPU run, {len(ref['chi2'])} LM iterations of oracle/ba_oracle.cpp "
                                             "(our g2o-faithful CPU restatement with an exact sparse block Cholesky -- NOT g2o itself, "
                                             "which is not installable here); all_cores = OpenMP over edges/landmarks with a sequential "
                                             "factorisation (as g2o's OpenMP build); structure analysis excluded, as for the GPU",
                                   "single_thread": base["single_thread"], "all_cores": base["all_cores"]}
            out["chi2_max_rel_diff_vs_oracle"] = float(np.max(np.abs(got[:m] - ref["chi2"][:m]) / ref["chi2"][:m]))
        # ---- end-to-end leg (rank 0, N = 1): the reference's own protocol through the C++ API -- warm-up initialize() +
        # optimize(1), then wall of initialize() + optimize(10) with host flattening, upload and write-back inside
        # (samples/sample_comparison_with_g2o.cpp:74-79, 303-307).  Reported next to `value`, never as `value`.
        if world == 1 and not args.no_end_to_end:
            out["contract_wall"] = contract_wall_leg(args.shape, E)
    # ---- N > 1, independent-graphs mode: also measure BASELINE config 5's mode -- ONE graph of this shape, landmark-partitioned
    # over the ranks by the native driver with RCCL all-reduces -- and report it inside the same line as `partitioned`.  It is the
    # first place a multi-rank RCCL communicator of this library runs, so it is fenced: a watchdog on every rank prints the line
    # without it and exits if the leg has not finished in time; any exception just drops the object.
    if args.full and world > 1 and not partitioned and os.environ.get("CUBA_BENCH_PARTITION_LEG", "1") != "0":
        import threading
        solver.close()                 # (one live handle per process: see above)

        def give_up():
            if rank == 0 and out is not None:
                out["partitioned"] = {"error": "landmark-partitioned leg did not finish within its time limit"}
                print(json.dumps(out), flush=True)
            os._exit(0)
        watchdog = threading.Timer(float(os.environ.get("CUBA_BENCH_PARTITION_TIMEOUT", "150")), give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            res = partition_leg(args, dist, backend, rank, world, device_index, rk)
            if rank == 0 and out is not None:
                single = out["ms_per_step"] * LM_RUN        # one rank's own 10-iteration run of this shape, measured above
                res["single_gpu_wall_ms_10iter"] = single
                res["speedup_over_one_gpu"] = single / res["wall_ms_10iter"]
                ts = res.get("time_shares") or {}
                if ts.get("replicated_reduced_solve_ms"):
                    ts["amdahl_ceiling_speedup"] = single / ts["replicated_reduced_solve_ms"]
                out["partitioned"] = res
        except Exception as e:   # noqa: BLE001
            if rank == 0 and out is not None:
                out["partitioned"] = {"error": repr(e)[:300]}
        watchdog.cancel()
    if rank == 0 and out is not None:
        print(json.dumps(out), flush=True)
    solver.close()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def partition_leg(args, dist, backend, rank, world, device_index, rk):
    """BASELINE config 5's mode on the bench shape: every rank holds the whole graph (seed of the shape), the native driver
    (libcuba_hip_dist.so) restricts it to its landmark range and all-reduces [Hsc | bsc | bp] once per LM trial."""
    import torch
    from cuba_amd.capi import HipSolver
    from cuba_amd.dist import NativeDist, TorchComm, landmark_ranges, rccl_unique_id
    from cuba_amd.graph import flatten
    from cuba_amd.synth import synth_named
    fp = flatten(synth_named(args.shape))
    h = HipSolver(None, rk, device=device_index, stream=torch.cuda.current_stream().cuda_stream)
    h.set_graph(fp, landmark_range=landmark_ranges(fp.eL, fp.Lt, world)[rank])      # values of the rank's own landmarks' edges only
    if backend == "nccl":
        ids = [rccl_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ids, src=0)
        d = NativeDist(h, fp, rank, world, unique_id=ids[0])
    else:
        d = NativeDist(h, fp, rank, world, comm=TorchComm())
    # parity first: 10 iterations from the generator's initial guess against the committed oracle trajectory of this shape
    par = None
    try:
        gold = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "baseline_shapes_chi2.json")))["shapes"][args.shape]["chi2"])
        got = d.optimize(LM_RUN)
        if len(got) == len(gold):
            par = float(np.max(np.abs(got - gold) / gold))
    except (OSError, KeyError):
        pass
    h.set_state(fp.q, fp.t, fp.Xw)
    d.optimize(1)                                   # the protocol's warm-up iteration
    h.snapshot_state()
    d.optimize(LM_RUN)                              # untimed run (hipGraphs, RCCL channels)
    runs = 3
    dist.barrier(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(runs):
        h.restore_state()
        chi2 = d.optimize(LM_RUN)
    dist.barrier(); torch.cuda.synchronize()
    dt = time.perf_counter() - t
    tt = torch.tensor([dt], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    dt = float(tt.item())
    c = d.counters()
    # where a trial's time goes on this rank (one more run with the per-stage synchronising profile of the solver handle): the
    # replicated reduced solve is the Amdahl term of this mode, what no bucket covers is collectives + host turnaround
    share = None
    try:
        h.set_option("profile", 1.0)
        p0 = h.profile()
        h.restore_state()
        dist.barrier(); torch.cuda.synchronize()
        tp = time.perf_counter()
        d.optimize(LM_RUN)
        torch.cuda.synchronize()
        tp = time.perf_counter() - tp
        prof = {k: v - p0[k] for k, v in h.profile().items()}
        h.set_option("profile", 0.0)
        solve_s = prof["6: Numerical Decomposition"]
        local_s = prof["2: Compute Error"] + prof["3: Build System"] + prof["4: Schur Complement"] + prof["7: Update Solution"]
        share = {"profiled_run_ms": tp * 1e3, "replicated_reduced_solve_ms": solve_s * 1e3,
                 "replicated_reduced_solve": solve_s / tp, "partitioned_edge_and_landmark_work": local_s / tp,
                 "collectives_and_host": max(0.0, 1.0 - (solve_s + local_s) / tp),
                 "note": "shares of one profiled 10-iteration run on rank 0 (every stage synchronises, so the run is slower than the timed ones); "
                         "the reduced solve is replicated on every rank, so this mode cannot run faster than replicated_reduced_solve_ms: "
                         "amdahl_ceiling_speedup = single-GPU wall of the same shape / that time"}
    except Exception as e:   # noqa: BLE001
        share = {"error": repr(e)[:200]}
    res = {"workload": f"ONE ba_{args.shape}-shaped graph, landmark-partitioned over {world} ranks (native driver, "
                       f"{'RCCL' if backend == 'nccl' else backend} all-reduce of [Hsc|bsc|bp] per trial), {LM_RUN}-iteration LM runs",
           "scaling": "strong", "wall_ms_10iter": dt * 1e3 / runs, "value": fp.E * LM_RUN * runs / dt, "unit": "edges/s",
           "final_chi2": float(chi2[-1]), "iterations_done": int(len(chi2)), "chi2_max_rel_diff_vs_golden": par,
           "allreduce_elements_per_trial": int(h.reduction_buffer()[1]), "reduction_parts": d.reduction_parts()[0],
           "value_bytes_uploaded_rank0": h.counter("value_bytes_uploaded"), "value_bytes_whole_graph": 32 * int(fp.E), "time_shares": share}
    d.close(); h.close()
    return res




if __name__ == "__main__":
    main()
