"""ctypes binding of the C ABI (include/cuba_hip.h -> csrc/libcuba_hip.so).

This is plumbing for tests and bench.py: every call goes straight through the C ABI to the HIP
kernels.  There is no CPU fallback -- if the shared library is missing or no GPU is visible the
constructor raises.  The method names mirror CudaBlockSolver's stage methods
(/root/reference/src/cuda_bundle_adjustment.cpp:115-562).
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libcuba_hip.so")
LIB_PATH_F32 = os.path.join(CSRC, "libcuba_hip_f32.so")     # single-precision build (the reference's USE_FLOAT32 option)
HEADER = os.path.join(os.path.dirname(_HERE), "include", "cuba_hip.h")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)

ARRAY_IDS = dict(bp=0, bsc=1, xp=2, xl=3, lm_sys=4, hsc=5, state=6)
PROFILE_KEYS = (  # same strings as CudaBlockSolver::getTimeProfile (src/cuda_bundle_adjustment.cpp:545-562)
    "0: Initialize Optimizer", "1: Build Structure", "2: Compute Error", "3: Build System",
    "4: Schur Complement", "5: Symbolic Decomposition", "6: Numerical Decomposition", "7: Update Solution")
TRI_STATUS_NAMES = (  # CUBA_HIP_TRI_* of include/cuba_hip.h, in the order the statuses are decided
    "ok", "not_selected", "fixed", "few_observations", "low_parallax", "singular", "behind_camera", "chi2")
POSEREF_STATUS_NAMES = (  # CUBA_HIP_POSEREF_* of include/cuba_hip.h
    "ok", "not_selected", "fixed", "few_observations", "singular", "few_inliers")
POSELOC_STATUS_NAMES = (  # CUBA_HIP_POSELOC_* of include/cuba_hip.h
    "ok", "not_selected", "fixed", "few_observations", "no_solution", "few_inliers")


class CubaHipError(RuntimeError):
    pass


def build_library(force=False):
    """Compile csrc/*.hip for gfx950 (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))] + [HEADER]
    stale = not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale or not os.path.exists(LIB_PATH_F32):
        subprocess.check_call(["make", "-C", CSRC, "-s", "all"])
    return LIB_PATH


_libs = {}


def load_library(precision="f64"):
    path = {"f64": LIB_PATH, "f32": LIB_PATH_F32}[precision]
    path = os.environ.get("CUBA_HIP_LIB_" + precision.upper(), path)     # e.g. the stage-timestamp build (make libcuba_hip_trace.so)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise CubaHipError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    if os.environ.get("CUBA_HIP_NO_TORCH") != "1":
        # PyTorch wheels bundle their own libamdhip64; whichever HIP runtime is loaded first serves the whole
        # process.  Loading torch's first keeps torch.cuda (streams, torch.distributed/RCCL) usable next to this
        # library; the C ABI itself does not depend on torch.
        try:
            import torch  # noqa: F401
        except Exception:      # pragma: no cover
            pass
    lib = C.CDLL(path)
    H = C.c_void_p
    sig = {
        "cuba_hip_create": [C.c_int, C.POINTER(H)],
        "cuba_hip_destroy": [H],
        "cuba_hip_set_stream": [H, C.c_void_p],
        "cuba_hip_set_option": [H, C.c_char_p, C.c_double],
        "cuba_hip_set_graph": [H, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _ip, _ip, _u8p, _dp, _dp],
        "cuba_hip_set_graph_begin": [H, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _ip, _ip, _u8p, _dp, _dp],
        "cuba_hip_set_graph_end": [H],
        "cuba_hip_set_graph_partition": [H, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _ip, _ip, _u8p, _dp, _dp, C.c_int, C.c_int],
        "cuba_hip_set_robust_kernel": [H, C.c_int, C.c_int, C.c_double],
        "cuba_hip_build_structure": [H],
        "cuba_hip_compute_errors": [H, _dp],
        "cuba_hip_build_system": [H],
        "cuba_hip_max_diagonal": [H, _dp],
        "cuba_hip_set_lambda": [H, C.c_double],
        "cuba_hip_restore_diagonal": [H],
        "cuba_hip_schur": [H],
        "cuba_hip_schur_parts": [H, C.POINTER(C.c_int)],
        "cuba_hip_schur_part": [H, C.c_int, C.POINTER(C.c_size_t)],
        "cuba_hip_solve_reduced": [H, C.POINTER(C.c_int)],
        "cuba_hip_back_substitute": [H],
        "cuba_hip_solve": [H, C.POINTER(C.c_int)],
        "cuba_hip_update": [H],
        "cuba_hip_compute_scale": [H, C.c_double, _dp],
        "cuba_hip_push": [H],
        "cuba_hip_pop": [H],
        "cuba_hip_hint_unchanged": [H, C.c_int, C.c_int],
        "cuba_hip_chi_squares_begin": [H, _dp],
        "cuba_hip_chi_squares_end": [H],
        "cuba_hip_snapshot_state": [H],
        "cuba_hip_restore_state": [H],
        "cuba_hip_snapshot_state_slot": [H, C.c_int],
        "cuba_hip_restore_state_slot": [H, C.c_int],
        "cuba_hip_get_counter": [H, C.c_char_p, C.POINTER(C.c_int64)],
        "cuba_hip_optimize": [H, C.c_int, _dp, C.POINTER(C.c_int)],
        "cuba_hip_optimize_batch": [C.POINTER(H), C.c_int, C.c_int, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "cuba_hip_get_solution": [H, _dp, _dp, _dp],
        "cuba_hip_set_solution": [H, _dp, _dp, _dp],
        "cuba_hip_chi_squares": [H, _dp],
        "cuba_hip_get_profile": [H, _dp],
        "cuba_hip_get_counters": [H, C.POINTER(C.c_int64)],
        "cuba_hip_get_hsc_structure": [H, _ip, _ip, C.POINTER(C.c_int)],
        "cuba_hip_get_pcg_history": [H, _ip, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)],
        "cuba_hip_get_array": [H, C.c_int, _dp, C.POINTER(C.c_size_t)],
        "cuba_hip_time_kernels": [H, C.c_int, _dp],
        "cuba_hip_set_partition": [H, C.c_int, C.c_int],
        "cuba_hip_assemble": [H],
        "cuba_hip_max_diagonal_parts": [H, _dp, _dp],
        "cuba_hip_compute_scale_parts": [H, C.c_double, _dp, _dp],
        "cuba_hip_device_pointer": [H, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
        "cuba_hip_reduction_buffer": [H, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
        "cuba_hip_get_stream": [H, C.POINTER(C.c_void_p)],
        "cuba_hip_begin_run": [H],
        "cuba_hip_get_sizes": [H, C.POINTER(C.c_int)],
        "cuba_hip_evaluate_device": [H, C.c_double, C.c_int, C.POINTER(C.c_void_p)],
        "cuba_hip_compute_covariance": [H, _dp, _dp, C.POINTER(C.c_int)],
        "cuba_hip_get_covariance_blocks": [H, _dp],
        "cuba_hip_compute_covariance_pairs": [H, C.c_int, _ip, _ip, _ip, _ip, _dp, C.POINTER(C.c_int)],
        "cuba_hip_set_pose_priors": [H, C.c_int, _ip, _dp, _dp, _dp],
        "cuba_hip_prior_chi_squares": [H, _dp],
        "cuba_hip_set_relative_pose_edges": [H, C.c_int, _ip, _ip, _dp, _dp, _dp],
        "cuba_hip_relative_pose_chi_squares": [H, _dp],
        "cuba_hip_set_pose_factor_robust_kernels": [H, C.c_int, C.c_int, _ip, _dp],
        "cuba_hip_set_landmark_priors": [H, C.c_int, _ip, _dp, _dp, _ip, _dp],
        "cuba_hip_landmark_prior_chi_squares": [H, _dp],
        "cuba_hip_set_position_factors": [H, C.c_int, _ip, _dp, _dp, _dp, _ip, _dp],
        "cuba_hip_position_factor_chi_squares": [H, _dp],
        "cuba_hip_set_direction_factors": [H, C.c_int, _ip, _dp, _dp, _dp, _ip, _dp],
        "cuba_hip_direction_factor_chi_squares": [H, _dp],
        "cuba_hip_set_range_factors": [H, C.c_int, _ip, _dp, _dp, _dp, _dp, _ip, _dp],
        "cuba_hip_range_factor_chi_squares": [H, _dp],
        "cuba_hip_set_pose_range_factors": [H, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, _ip, _dp],
        "cuba_hip_pose_range_factor_chi_squares": [H, _dp],
        "cuba_hip_gate_edges": [H, _dp, C.c_int, C.c_int, C.POINTER(C.c_int64), _dp],
        "cuba_hip_set_edge_active": [H, _u8p],
        "cuba_hip_get_edge_active": [H, _u8p],
        "cuba_hip_landmark_active_edges": [H, _ip],
        "cuba_hip_triangulate_landmarks": [H, _u8p, C.c_int, C.c_double, _dp, C.c_int, _ip, C.POINTER(C.c_int64), _dp],
        "cuba_hip_refine_poses": [H, _u8p, C.c_int, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _ip, C.POINTER(C.c_int64), _ip, _dp, _dp, _dp, _u8p],
        "cuba_hip_localize_poses": [H, _u8p, C.c_int, C.c_uint64, _dp, C.c_int, C.c_int, _ip, C.POINTER(C.c_int64), _ip, _dp, _ip, _dp, _dp, _u8p],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.cuba_hip_host_alloc.argtypes = [C.c_size_t]
    lib.cuba_hip_host_alloc.restype = C.c_void_p
    lib.cuba_hip_host_free.argtypes = [C.c_void_p]
    lib.cuba_hip_host_free.restype = None
    lib.cuba_hip_debug_dense_inverse.argtypes = [C.c_int, C.c_int, _dp, _dp]
    lib.cuba_hip_debug_dense_inverse.restype = C.c_int
    lib.cuba_hip_debug_dense_solve.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int)]
    lib.cuba_hip_debug_dense_solve.restype = C.c_int
    lib.cuba_hip_debug_sparse_solve.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int32)]
    lib.cuba_hip_debug_sparse_solve.restype = C.c_int
    lib.cuba_hip_debug_selected_inverse.argtypes = [C.c_int, C.c_int, _dp, _dp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int32)]
    lib.cuba_hip_debug_selected_inverse.restype = C.c_int
    lib.cuba_hip_debug_sparse_plan.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32),
                                               C.c_size_t, C.POINTER(C.c_size_t)]
    lib.cuba_hip_debug_sparse_plan.restype = C.c_int
    lib.cuba_hip_debug_inverse_blocks.argtypes = [C.c_int, C.c_int, _dp, C.c_int, _ip, _ip, _dp, C.POINTER(C.c_int), C.c_int,
                                                  C.POINTER(C.c_int32)]
    lib.cuba_hip_debug_inverse_blocks.restype = C.c_int
    lib.cuba_hip_debug_pair_plan.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, _ip, _ip, C.c_int,
                                             C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
    lib.cuba_hip_debug_pair_plan.restype = C.c_int
    lib.cuba_hip_debug_pcg_config.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_size_t)]
    lib.cuba_hip_debug_pcg_config.restype = C.c_int
    lib.cuba_hip_debug_lm_script.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, _dp, C.POINTER(C.c_uint64), C.c_double, C.c_double, C.c_int, C.c_int,
                                             _ip, _dp, _ip, _dp, _ip, _dp, _ip, C.c_size_t, _dp, _dp]
    lib.cuba_hip_debug_lm_script.restype = C.c_int
    lib.cuba_hip_debug_lm_records.argtypes = [H, _dp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.cuba_hip_debug_lm_records.restype = C.c_int
    lib.cuba_hip_last_error.argtypes = [H]
    lib.cuba_hip_last_error.restype = C.c_char_p
    lib.cuba_hip_version.restype = C.c_char_p
    lib.cuba_hip_scalar_size.restype = C.c_int
    _libs[path] = lib
    return lib


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_ip) if a is not None else None


# ---- the factor setters' arguments as the C ABI takes them ------------------------------------------
def _index(a):
    """int32[n]: vertices in the solver numbering"""
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _rows(a, n, width=3):
    """float64[n, width], or None"""
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(n, width)


def _information(a, n, d):
    """float64[n, d, d], every block column-major: the transpose of the row-major reading (symmetric matrices: the two agree up to the
    symmetrisation the library applies)"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(n, d, d).transpose(0, 2, 1))


def _scalars(a, n):
    """float64[n], a scalar broadcast"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))


def _kernels(kind, delta, n):
    """(int32[n], float64[n]) of a set of n factors, scalars broadcast; either may be None (the library wants both or neither)"""
    if kind is not None:
        kind = np.ascontiguousarray(np.full(n, kind) if np.ndim(kind) == 0 else kind, dtype=np.int32).reshape(-1)
    if delta is not None:
        delta = np.ascontiguousarray(np.full(n, delta) if np.ndim(delta) == 0 else delta, dtype=np.float64).reshape(-1)
    if (kind is not None and kind.size != n) or (delta is not None and delta.size != n):
        raise ValueError("kind / delta differ in length from the set")
    return kind, delta


def dense_inverse(A, precision="f64", device=0):
    """The library's blocked Gauss-Jordan inversion (coarse level of the preconditioner) applied to an SPD matrix: test hook."""
    A = np.asfortranarray(A, dtype=np.float64)
    out = np.zeros_like(A, order="F")
    rc = load_library(precision).cuba_hip_debug_dense_inverse(int(device), A.shape[0], _d(A), _d(out))
    if rc != 0:
        raise CubaHipError(f"cuba_hip_debug_dense_inverse failed with status {rc}")
    return np.array(out)


LM_STATE = ("F", "lam", "nu", "halt", "trials", "accepted", "rej", "maxq", "tag_base")
LM_RECORD = ("Fhat", "scale", "rho", "lam", "F", "accepted", "halt", "tag")


def lm_script(trials, niter, F0=0.0, lam0=0.0, chi_slots=None, maxdiag_bits=None, tau=1e-5, tag_base=65536.0, scratch_count=1, precision="f64", device=0):
    """The decision kernels of a device-decided run on scripted partial sums (cuba_hip_debug_lm_script): test hook.
    trials: [(ok, a, b, c), ...] with a, b, c the partial-sum arrays of the landmark part of the denominator, of chi2 and of the pose part.
    chi_slots (16 numbers) and maxdiag_bits (64 uint64) given: the run starts on the device (launch_lm_run_init) instead of from F0, lam0.
    Returns (start, per_trial): start = dict(state, lam_scalar); per_trial = list of dict(state, record [dicts by name], lam_scalar,
    sums (a, b, c) or None, slots_zero, restored, untouched, absorbed, done, stop, rej_run, chi2 (or None), host_lam, host_F)."""
    n = len(trials)
    ok = np.ascontiguousarray([1 if t[0] else 0 for t in trials], dtype=np.int32)
    cols = []
    for k in (1, 2, 3):
        arrs = [np.asarray(t[k] if t[0] else [], dtype=np.float64).reshape(-1) for t in trials]
        off = np.zeros(n + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(x) for x in arrs])
        cols += [np.ascontiguousarray(np.concatenate(arrs + [np.zeros(1)])), off]
    start, out = np.zeros(10), np.zeros((max(n, 1), 32))
    on_device = chi_slots is not None
    if on_device:
        chi_slots = np.ascontiguousarray(chi_slots, dtype=np.float64).reshape(16)
        maxdiag_bits = np.ascontiguousarray(maxdiag_bits, dtype=np.uint64).reshape(64)
    rc = load_library(precision).cuba_hip_debug_lm_script(
        int(device), 1 if on_device else 0, float(F0), float(lam0), _d(chi_slots), maxdiag_bits.ctypes.data_as(C.POINTER(C.c_uint64)) if on_device else None,
        float(tau), float(tag_base), int(niter), n, _i(ok), _d(cols[0]), _i(cols[1]), _d(cols[2]), _i(cols[3]), _d(cols[4]), _i(cols[5]),
        int(scratch_count), _d(start), _d(out))
    if rc != 0:
        raise CubaHipError(f"cuba_hip_debug_lm_script failed with status {rc}")
    res = []
    for t in range(n):
        o = out[t]
        res.append(dict(state=dict(zip(LM_STATE, o[0:9].tolist())), record=dict(zip(LM_RECORD, o[9:17].tolist())), lam_scalar=float(o[17]),
                        sums=tuple(o[18:21].tolist()) if o[21] >= 0 else None, slots_zero=o[21] == 1, restored=o[22] == 1, untouched=o[23] == 1,
                        absorbed=int(o[24]), done=int(o[25]), stop=o[26] == 1, rej_run=int(o[27]), chi2=float(o[29]) if o[28] == 1 else None,
                        host_lam=float(o[30]), host_F=float(o[31])))
    return dict(state=dict(zip(LM_STATE, start[0:9].tolist())), lam_scalar=float(start[9])), res


_live = weakref.WeakSet()


@atexit.register
def _close_all():
    # destroy device objects (streams, graphs, buffers) while the HIP runtime is still alive: handles that
    # survive until interpreter teardown would be destroyed after the runtime's own static destructors
    for s in list(_live):
        s.close()


def dense_solve(A, b, precision="f64", device=0, slack=-1, with_stats=False):
    """The library's exact reduced solve (sparse tile Cholesky on the matrix cores, csrc/ba_direct.hip) applied to a symmetric
    matrix whose order is a multiple of 6 (6 x 6 blocks that are identically zero stay out of the pattern): test hook.
    Returns (x, not_positive_definite[, {tile columns, tiles, levels, slack}])."""
    A = np.asfortranarray(A, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    flag = C.c_int()
    stats = (C.c_int32 * 4)()
    rc = load_library(precision).cuba_hip_debug_sparse_solve(int(device), A.shape[0], _d(A), _d(b), _d(x), C.byref(flag), int(slack), stats)
    if rc != 0:
        raise CubaHipError(f"cuba_hip_debug_sparse_solve failed with status {rc}")
    if with_stats:
        return x, bool(flag.value), dict(zip(("tile_columns", "tiles", "levels", "slack"), (int(v) for v in stats)))
    return x, bool(flag.value)


def selected_inverse(A, slack=-1, precision="f64", device=0, with_stats=False):
    """The selected inversion behind HipSolver.covariance (csrc/ba_covariance.hip) applied to a symmetric matrix on dense_solve's block
    pattern: test hook.  Returns (sigma, not_positive_definite[, stats]); sigma holds A^-1 on the pattern's blocks and their mirrors, as
    the kernels extracted them (nothing symmetrised on the host), and zeros elsewhere."""
    A = np.asfortranarray(A, dtype=np.float64)
    sigma = np.zeros_like(A, order="F")
    flag = C.c_int()
    stats = (C.c_int32 * 4)()
    rc = load_library(precision).cuba_hip_debug_selected_inverse(int(device), A.shape[0], _d(A), _d(sigma), C.byref(flag), int(slack), stats)
    if rc != 0:
        raise CubaHipError(f"cuba_hip_debug_selected_inverse failed with status {rc}")
    sigma = np.array(sigma)
    if with_stats:
        return sigma, bool(flag.value), dict(zip(("tile_columns", "tiles", "levels", "slack"), (int(v) for v in stats)))
    return sigma, bool(flag.value)


def inverse_blocks(A, pairs, slack=-1, precision="f64", device=0, with_stats=False):
    """The kernels behind HipSolver.covariance_pairs applied to a symmetric matrix on dense_solve's block pattern: test hook.  pairs: (i, j)
    6 x 6 block indices, on or off the pattern.  Returns (blocks [n, 6, 6] = A^-1[6i:6i+6, 6j:6j+6], not_positive_definite[, stats])."""
    A = np.asfortranarray(A, dtype=np.float64)
    pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    bi, bj = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    out = np.zeros((len(pr), 36))
    flag = C.c_int()
    stats = (C.c_int32 * 4)()
    rc = load_library(precision).cuba_hip_debug_inverse_blocks(int(device), A.shape[0], _d(A), len(pr), bi.ctypes.data_as(_ip),
                                                               bj.ctypes.data_as(_ip), _d(out), C.byref(flag), int(slack), stats)
    if rc != 0:
        raise CubaHipError(f"cuba_hip_debug_inverse_blocks failed with status {rc}")
    blocks = out.reshape(-1, 6, 6).transpose(0, 2, 1).copy()
    if with_stats:
        return blocks, bool(flag.value), dict(zip(("tile_columns", "tiles", "levels", "slack"), (int(v) for v in stats)))
    return blocks, bool(flag.value)


PAIR_PLAN_ARRAYS = ("header", "pairs", "fwdPtr", "fwdCols", "bwdPtr", "bwdCols", "slotPtr", "slotCols", "fLvlPtr", "fRec", "fGather",
                    "bLvlPtr", "bRec", "bGather")


def pair_plan(row_ptr, col_ind, pairs, slack=-1, precision="f64"):
    """Symbolic phase of the pair solve behind HipSolver.covariance_pairs for pose pairs (i = left, j = right) on an upper-triangular
    block pattern (host only, no device): dict of the arrays of PairPlan in csrc/ba_kernels.hpp, all blocks in one chunk.  "pairs" holds
    {block, column, 0, 0} per pair; fRec / bRec {slot, tile column, first gather entry, entries}; fGather / bGather {tile, slot}."""
    lib = load_library(precision)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32); ci = np.ascontiguousarray(col_ind, dtype=np.int32)
    pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    bi, bj = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    ip = C.POINTER(C.c_int32)
    out = {}
    for which, name in enumerate(PAIR_PLAN_ARRAYS):
        n = C.c_size_t()
        args = (len(rp) - 1, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), int(slack), len(pr), bi.ctypes.data_as(_ip), bj.ctypes.data_as(_ip), which)
        rc = lib.cuba_hip_debug_pair_plan(*args, None, 0, C.byref(n))
        if rc != 0:
            raise CubaHipError(f"cuba_hip_debug_pair_plan failed with status {rc}")
        a = np.zeros(n.value, dtype=np.int32)
        rc = lib.cuba_hip_debug_pair_plan(*args, a.ctypes.data_as(ip), n.value, C.byref(n))
        if rc != 0:
            raise CubaHipError(f"cuba_hip_debug_pair_plan failed with status {rc}")
        out[name] = a
    h = out.pop("header")
    out.update(blocks=int(h[0]), slots=int(h[1]), fRecords=int(h[2]), fEntries=int(h[3]), bRecords=int(h[4]), bEntries=int(h[5]))
    return out


SPARSE_PLAN_ARRAYS = ("header", "posOfSeg", "colPtr", "rowIdx", "gPtr", "gather", "lvlPtr", "lvlTiles", "lvlColPtr", "lvlCols", "blkTile")


def sparse_plan(row_ptr, col_ind, slack=-1, precision="f64"):
    """Symbolic phase of the exact reduced solve for an upper-triangular block pattern (host only, no device): dict of the plan's arrays
    (SparseCholPlan in csrc/ba_kernels.hpp)."""
    lib = load_library(precision)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32); ci = np.ascontiguousarray(col_ind, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    out = {}
    for which, name in enumerate(SPARSE_PLAN_ARRAYS):
        n = C.c_size_t()
        rc = lib.cuba_hip_debug_sparse_plan(len(rp) - 1, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), int(slack), which, None, 0, C.byref(n))
        if rc != 0:
            raise CubaHipError(f"cuba_hip_debug_sparse_plan failed with status {rc}")
        a = np.zeros(n.value, dtype=np.int32)
        rc = lib.cuba_hip_debug_sparse_plan(len(rp) - 1, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), int(slack), which, a.ctypes.data_as(ip), n.value, C.byref(n))
        if rc != 0:
            raise CubaHipError(f"cuba_hip_debug_sparse_plan failed with status {rc}")
        out[name] = a
    h = out.pop("header")
    out.update(T=int(h[0]), nTiles=int(h[1]), nLevels=int(h[2]), slack=int(h[3]), entries=int(h[4]), nblk=int(h[5]))
    return out


SELINV_PLAN_ARRAYS = ("header", "stepPtr", "offRec", "colStepPtr", "cols", "gather")


def selinv_plan(row_ptr, col_ind, slack=-1, precision="f64"):
    """Symbolic phase of the selected inversion behind HipSolver.covariance, built on sparse_plan's factor pattern (host only, no
    device): dict of the arrays of SelInvPlan in csrc/ba_kernels.hpp.  Step s walks level nLevels - 1 - s of the elimination tree;
    offRec holds {tile, column, first gather entry, entries} per off-diagonal tile, gather {Sigma tile | bit 30 = stored transposed, tile
    of L_kj} per entry."""
    lib = load_library(precision)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32); ci = np.ascontiguousarray(col_ind, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    out = {}
    for which, name in enumerate(SELINV_PLAN_ARRAYS, start=11):
        n = C.c_size_t()
        rc = lib.cuba_hip_debug_sparse_plan(len(rp) - 1, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), int(slack), which, None, 0, C.byref(n))
        if rc != 0:
            raise CubaHipError(f"cuba_hip_debug_sparse_plan failed with status {rc}")
        a = np.zeros(n.value, dtype=np.int32)
        rc = lib.cuba_hip_debug_sparse_plan(len(rp) - 1, rp.ctypes.data_as(ip), ci.ctypes.data_as(ip), int(slack), which, a.ctypes.data_as(ip), n.value, C.byref(n))
        if rc != 0:
            raise CubaHipError(f"cuba_hip_debug_sparse_plan failed with status {rc}")
        out[name] = a
    h = out.pop("header")
    out.update(nLevels=int(h[0]), nOff=int(h[1]), entries=int(h[2]), products=int(h[3]) + (int(h[4]) << 31))
    return out


def optimize_batch(solvers, niter):
    """cuba_hip_optimize_batch: the LM runs of several HipSolver handles (one library, one device) in one launch chain.
    Returns ([chi2 per iteration of every handle], reduced solves that ran batched)."""
    n = len(solvers)
    lib = solvers[0].lib
    arr = (C.c_void_p * n)(*[s.h.value for s in solvers])
    chi2 = np.zeros((n, max(niter, 1)))
    done = (C.c_int * n)()
    batched = C.c_int()
    rc = lib.cuba_hip_optimize_batch(arr, n, int(niter), _d(chi2), done, C.byref(batched))
    if rc != 0:
        raise CubaHipError(f"cuba_hip_optimize_batch failed with status {rc}: {lib.cuba_hip_last_error(solvers[0].h).decode()}")
    return [chi2[i, :done[i]].copy() for i in range(n)], int(batched.value)


class HipSolver:
    """One bundle-adjustment problem on one GPU, driven through the C ABI."""

    def __init__(self, fp=None, robust=((0, 0.0), (0, 0.0)), device=0, stream=None, precision="f64", **options):
        self.lib = load_library(precision)
        self.scalar_size = self.lib.cuba_hip_scalar_size()
        self.h = C.c_void_p()
        rc = self.lib.cuba_hip_create(int(device), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise CubaHipError(f"cuba_hip_create failed with status {rc} (4 = no HIP device visible)")
        if stream is not None:
            self._ck(self.lib.cuba_hip_set_stream(self.h, C.c_void_p(int(stream))))
        for k, v in options.items():
            self.set_option(k, v)
        self.fp = None
        self._n_factors = {}
        _live.add(self)
        for et, (kind, delta) in enumerate(robust):
            self.set_robust_kernel(et, kind, delta)
        if fp is not None:
            self.set_graph(fp)

    def close(self):
        if getattr(self, "h", None):
            self.lib.cuba_hip_destroy(self.h)
            self.h = None

    __del__ = close

    def _ck(self, rc):
        if rc != 0:
            raise CubaHipError(f"status {rc}: {self.lib.cuba_hip_last_error(self.h).decode()}")

    def set_option(self, key, value):
        self._ck(self.lib.cuba_hip_set_option(self.h, key.encode(), float(value)))

    def set_robust_kernel(self, edge_type, kind, delta):
        self._ck(self.lib.cuba_hip_set_robust_kernel(self.h, int(edge_type), int(kind), float(delta)))

    def hint_unchanged(self, same_edges=True, same_values=False):
        """promise about the NEXT set_graph call only (cuba_hip_hint_unchanged)"""
        self._ck(self.lib.cuba_hip_hint_unchanged(self.h, int(bool(same_edges)), int(bool(same_values))))

    def set_graph(self, fp, two_step=False, landmark_range=None):
        """two_step: cuba_hip_set_graph_begin + cuba_hip_build_structure + cuba_hip_set_graph_end (what the C++ layer does: the
        measurements cross PCIe on a second stream while the structure analysis runs).
        landmark_range = (begin, end): cuba_hip_set_graph_partition -- the upload of one rank of a landmark partition, which sends the
        measurements and information of its own landmarks' edges only."""
        q, t, cam, Xw = (np.ascontiguousarray(a, dtype=np.float64) for a in (fp.q, fp.t, fp.cam, fp.Xw))
        eP = np.ascontiguousarray(fp.eP, dtype=np.int32)
        eL = np.ascontiguousarray(fp.eL, dtype=np.int32)
        eD = np.ascontiguousarray(fp.eDim, dtype=np.uint8)
        meas = np.ascontiguousarray(fp.meas, dtype=np.float64)
        om = np.ascontiguousarray(fp.omega, dtype=np.float64)
        if landmark_range is not None:
            self._ck(self.lib.cuba_hip_set_graph_partition(self.h, fp.Pt, fp.Pf, fp.Lt, fp.Lf, _d(q), _d(t), _d(cam), _d(Xw), len(eP),
                     eP.ctypes.data_as(_ip), eL.ctypes.data_as(_ip), eD.ctypes.data_as(_u8p), _d(meas), _d(om),
                     int(landmark_range[0]), int(landmark_range[1])))
            self._uploaded(fp)
            return
        fn = self.lib.cuba_hip_set_graph_begin if two_step else self.lib.cuba_hip_set_graph
        self._ck(fn(self.h, fp.Pt, fp.Pf, fp.Lt, fp.Lf, _d(q), _d(t), _d(cam), _d(Xw), len(eP),
                    eP.ctypes.data_as(_ip), eL.ctypes.data_as(_ip), eD.ctypes.data_as(_u8p), _d(meas), _d(om)))
        self._uploaded(fp)
        if two_step == "begin_only":                                 # (test hook: the arrays are kept alive by the caller of this method)
            self._pending_upload = (meas, om)
        elif two_step:
            self.build_structure()
            self._ck(self.lib.cuba_hip_set_graph_end(self.h))        # (meas / om stay referenced until here)

    def _uploaded(self, fp):
        """after a SUCCESSFUL upload (a refused one leaves the handle, and so the sizes of this object's output buffers, as they were)"""
        self.fp = fp
        self._n_factors = {}            # (every upload clears the pose priors, the relative-pose edges, the landmark priors, the position, the direction and both kinds of range factors)

    # ---- stages --------------------------------------------------------------------------------
    def build_structure(self): self._ck(self.lib.cuba_hip_build_structure(self.h))

    def compute_errors(self):
        v = C.c_double()
        self._ck(self.lib.cuba_hip_compute_errors(self.h, C.byref(v)))
        return v.value

    def build_system(self): self._ck(self.lib.cuba_hip_build_system(self.h))

    def max_diagonal(self):
        v = C.c_double()
        self._ck(self.lib.cuba_hip_max_diagonal(self.h, C.byref(v)))
        return v.value

    def set_lambda(self, lam): self._ck(self.lib.cuba_hip_set_lambda(self.h, float(lam)))
    def restore_diagonal(self): self._ck(self.lib.cuba_hip_restore_diagonal(self.h))
    def schur(self): self._ck(self.lib.cuba_hip_schur(self.h))

    def schur_parts(self):
        n = C.c_int()
        self._ck(self.lib.cuba_hip_schur_parts(self.h, C.byref(n)))
        return n.value

    def schur_part(self, part):
        """Part `part` of schur(); returns ((offset, count), (offset, count)): the ranges of the reduction buffer it completes."""
        r = (C.c_size_t * 4)()
        self._ck(self.lib.cuba_hip_schur_part(self.h, int(part), r))
        return (int(r[0]), int(r[1])), (int(r[2]), int(r[3]))

    def solve_reduced(self):
        ok = C.c_int()
        self._ck(self.lib.cuba_hip_solve_reduced(self.h, C.byref(ok)))
        return bool(ok.value)

    def back_substitute(self): self._ck(self.lib.cuba_hip_back_substitute(self.h))

    def solve(self):
        ok = C.c_int()
        self._ck(self.lib.cuba_hip_solve(self.h, C.byref(ok)))
        return bool(ok.value)

    def update(self): self._ck(self.lib.cuba_hip_update(self.h))

    def compute_scale(self, lam):
        v = C.c_double()
        self._ck(self.lib.cuba_hip_compute_scale(self.h, float(lam), C.byref(v)))
        return v.value

    def push(self): self._ck(self.lib.cuba_hip_push(self.h))
    def pop(self): self._ck(self.lib.cuba_hip_pop(self.h))
    def snapshot_state(self, slot=0): self._ck(self.lib.cuba_hip_snapshot_state_slot(self.h, int(slot)))
    def restore_state(self, slot=0): self._ck(self.lib.cuba_hip_restore_state_slot(self.h, int(slot)))

    def optimize(self, niter):
        chi2 = np.zeros(max(niter, 1))
        n = C.c_int()
        self._ck(self.lib.cuba_hip_optimize(self.h, int(niter), _d(chi2), C.byref(n)))
        return dict(chi2=chi2[:n.value])

    # ---- results -------------------------------------------------------------------------------
    def state(self):
        q, t, X = np.zeros((self.fp.Pt, 4)), np.zeros((self.fp.Pt, 3)), np.zeros((self.fp.Lt, 3))
        self._ck(self.lib.cuba_hip_get_solution(self.h, _d(q), _d(t), _d(X)))
        return q, t, X

    def set_state(self, q, t, X):
        q, t, X = (np.ascontiguousarray(a, dtype=np.float64) for a in (q, t, X))
        self._ck(self.lib.cuba_hip_set_solution(self.h, _d(q), _d(t), _d(X)))

    def chi_squares(self):
        out = np.zeros(self.fp.E)
        self._ck(self.lib.cuba_hip_chi_squares(self.h, _d(out)))
        return out

    # ---- edge gating (cuba_hip_gate_edges: g2o's setLevel / computeActiveErrors flow) ----------
    GATE_MODES = {"reclassify": 0, "only_remove": 1, "dry_run": 2}
    GATE_COUNTS = ("active_mono", "active_stereo", "gated_chi2_mono", "gated_chi2_stereo", "gated_depth", "changed")

    def gate_edges(self, chi2_max=(5.991, 7.815), positive_depth=True, mode="reclassify", with_chi2=False):
        """Classifies every reprojection edge on the device at the current estimate: active iff its omega |r|^2 (uploaded omega) is at most
        chi2_max[stereo] and -- positive_depth -- its point lies in front of the camera.  mode: "reclassify", "only_remove", "dry_run" (or
        the integer).  Returns the six counts by name; with_chi2: also "chi2", the ungated omega |r|^2 per edge in the caller's order."""
        E = self.fp.E if self.fp is not None else 0
        thr = np.ascontiguousarray(chi2_max, dtype=np.float64).reshape(2)
        counts = (C.c_int64 * 6)()
        chi = np.zeros(E) if with_chi2 else None
        self._ck(self.lib.cuba_hip_gate_edges(self.h, _d(thr), int(bool(positive_depth)), int(self.GATE_MODES.get(mode, mode)), counts,
                                              _d(chi) if with_chi2 else None))
        out = {k: int(v) for k, v in zip(self.GATE_COUNTS, counts)}
        if with_chi2:
            out["chi2"] = chi
        return out

    def set_edge_active(self, mask):
        """mask[E] in the caller's edge order (truthy = active); None: all edges active, the gate's storage is freed"""
        if mask is None:
            self._ck(self.lib.cuba_hip_set_edge_active(self.h, None))
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if self.fp is not None and m.shape != (self.fp.E,):
            raise ValueError(f"mask: expected {self.fp.E} entries")
        self._ck(self.lib.cuba_hip_set_edge_active(self.h, m.ctypes.data_as(_u8p)))

    def edge_active(self):
        """bool[E], caller's edge order; all True on a handle without a gate"""
        out = np.zeros(self.fp.E if self.fp is not None else 0, dtype=np.uint8)
        self._ck(self.lib.cuba_hip_get_edge_active(self.h, out.ctypes.data_as(_u8p)))
        return out.astype(bool)

    def landmark_active_edges(self):
        """int32[Lt], caller's landmark order: active edges per landmark"""
        out = np.zeros(self.fp.Lt if self.fp is not None else 0, dtype=np.int32)
        self._ck(self.lib.cuba_hip_landmark_active_edges(self.h, out.ctypes.data_as(_ip)))
        return out

    # ---- landmark triangulation (cuba_hip_triangulate_landmarks) --------------------------------
    def triangulate_landmarks(self, select=None, refine_iterations=5, min_parallax_deg=1.0, chi2_max=(5.991, 7.815), dry_run=False):
        """(Re-)triangulates the free landmarks on the device from their active reprojection edges and the current poses: a linear start,
        refine_iterations Gauss-Newton steps per landmark, acceptance tests (include/cuba_hip.h).  select: truthy[Lt] in the caller's
        landmark order, None = all.  Returns "status" (int32[Lt], indices into TRI_STATUS_NAMES), the eight counts by name, and "xyz"
        ([Lt, 3]: the accepted position of every "ok" landmark, the unchanged one of every other)."""
        Lt = self.fp.Lt if self.fp is not None else 0
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
            if sel.shape != (Lt,):
                raise ValueError(f"select: expected {Lt} entries")
        thr = np.ascontiguousarray(chi2_max, dtype=np.float64).reshape(2)
        status, xyz = np.zeros(Lt, dtype=np.int32), np.zeros((Lt, 3))
        counts = (C.c_int64 * len(TRI_STATUS_NAMES))()
        self._ck(self.lib.cuba_hip_triangulate_landmarks(self.h, sel.ctypes.data_as(_u8p) if sel is not None else None, int(refine_iterations),
                                                         float(min_parallax_deg), _d(thr), int(bool(dry_run)), status.ctypes.data_as(_ip), counts, _d(xyz)))
        out = {k: int(v) for k, v in zip(TRI_STATUS_NAMES, counts)}
        out["status"], out["xyz"] = status, xyz
        return out

    # ---- pose refinement with the landmarks held (cuba_hip_refine_poses) -----------------------------
    def refine_poses(self, select=None, rounds=4, iterations=10, robust_rounds=2, chi2_max=(5.991, 7.815), min_inliers=10, dry_run=False):
        """Refines the free poses on the device from their active reprojection edges with every landmark held: `rounds` outlier rounds of
        `iterations` Levenberg-Marquardt trials each, all inside one launch, the robust kernels in the first robust_rounds rounds
        (include/cuba_hip.h).  select: truthy[Pt] in the caller's pose order, None = all.  Returns "status" (int32[Pt], indices into
        POSEREF_STATUS_NAMES), the six counts by name, "inliers" (int32[Pt]), "chi2" ([Pt]), "q" ([Pt, 4]) and "t" ([Pt, 3]) (the refined
        pose of every "ok" pose, the unchanged one of every other) and "edge_inlier" (bool[E], the caller's edge order)."""
        Pt, E = (self.fp.Pt, self.fp.E) if self.fp is not None else (0, 0)
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
            if sel.shape != (Pt,):
                raise ValueError(f"select: expected {Pt} entries")
        thr = np.ascontiguousarray(chi2_max, dtype=np.float64).reshape(2)
        status, inliers = np.zeros(Pt, dtype=np.int32), np.zeros(Pt, dtype=np.int32)
        chi2, q, t, edge = np.zeros(Pt), np.zeros((Pt, 4)), np.zeros((Pt, 3)), np.zeros(E, dtype=np.uint8)
        counts = (C.c_int64 * len(POSEREF_STATUS_NAMES))()
        self._ck(self.lib.cuba_hip_refine_poses(self.h, sel.ctypes.data_as(_u8p) if sel is not None else None, int(rounds), int(iterations),
                                                int(robust_rounds), _d(thr), int(min_inliers), int(bool(dry_run)), status.ctypes.data_as(_ip), counts,
                                                inliers.ctypes.data_as(_ip), _d(chi2), _d(q), _d(t), edge.ctypes.data_as(_u8p)))
        out = {k: int(v) for k, v in zip(POSEREF_STATUS_NAMES, counts)}
        out.update(status=status, inliers=inliers, chi2=chi2, q=q, t=t, edge_inlier=edge.astype(bool))
        return out

    # ---- pose localisation from scratch (cuba_hip_localize_poses) -------------------------------------------
    def localize_poses(self, select=None, hypotheses=256, seed=0, chi2_max=(5.991, 7.815), min_inliers=10, dry_run=False):
        """Gives the free poses a value on the device from their active reprojection edges and the current landmarks alone, by a
        deterministic RANSAC of `hypotheses` three-point (P3P) samples per pose scored by MSAC; a pose's current value is never read (it may
        be NaN) (include/cuba_hip.h).  select: truthy[Pt] in the caller's pose order, None = all.  Returns "status" (int32[Pt], indices into
        POSELOC_STATUS_NAMES), the six counts by name, "inliers" (int32[Pt]), "cost" ([Pt], the winner's score), "winner" (int32[Pt],
        4 h + root, -1 for a pose that is not ok), "q" ([Pt, 4]) and "t" ([Pt, 3]) (the new pose of every "ok" pose, the unchanged one of
        every other) and "edge_inlier" (bool[E], the caller's edge order)."""
        Pt, E = (self.fp.Pt, self.fp.E) if self.fp is not None else (0, 0)
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select) != 0, dtype=np.uint8)
            if sel.shape != (Pt,):
                raise ValueError(f"select: expected {Pt} entries")
        thr = np.ascontiguousarray(chi2_max, dtype=np.float64).reshape(2)
        status, inliers, winner = np.zeros(Pt, dtype=np.int32), np.zeros(Pt, dtype=np.int32), np.zeros(Pt, dtype=np.int32)
        cost, q, t, edge = np.zeros(Pt), np.zeros((Pt, 4)), np.zeros((Pt, 3)), np.zeros(E, dtype=np.uint8)
        counts = (C.c_int64 * len(POSELOC_STATUS_NAMES))()
        self._ck(self.lib.cuba_hip_localize_poses(self.h, sel.ctypes.data_as(_u8p) if sel is not None else None, int(hypotheses),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, _d(thr), int(min_inliers), int(bool(dry_run)),
                                                  status.ctypes.data_as(_ip), counts, inliers.ctypes.data_as(_ip), _d(cost),
                                                  winner.ctypes.data_as(_ip), _d(q), _d(t), edge.ctypes.data_as(_u8p)))
        out = {k: int(v) for k, v in zip(POSELOC_STATUS_NAMES, counts)}
        out.update(status=status, inliers=inliers, cost=cost, winner=winner, q=q, t=t, edge_inlier=edge.astype(bool))
        return out

    def set_pose_priors(self, pose, q, t, info):
        """SE(3) pose priors (cuba_hip_set_pose_priors), replacing the handle's set: pose[n] in the solver numbering, q[n, 4] (x, y, z, w),
        t[n, 3], info[n, 6, 6] in the [omega, upsilon] order of the pose update (symmetric).  An empty pose list clears the set."""
        pose = _index(pose)
        n = len(pose)
        q, t, info = _rows(q, n, 4), _rows(t, n), _information(info, n, 6)
        self._ck(self.lib.cuba_hip_set_pose_priors(self.h, n, _i(pose), _d(q), _d(t), _d(info)))
        self._n_factors["prior"] = n

    def set_relative_pose_edges(self, pose_i, pose_j, q, t, info):
        """SE(3) relative-pose edges (cuba_hip_set_relative_pose_edges), replacing the handle's set: pose_i[n], pose_j[n] in the solver
        numbering, the measured T_j T_i^-1 as q[n, 4] (x, y, z, w) and t[n, 3], info[n, 6, 6] symmetric in [omega, upsilon] order;
        n = 0 clears."""
        pose_i, pose_j = _index(pose_i), _index(pose_j)
        n = int(pose_i.size)
        q, t, info = _rows(q, n, 4), _rows(t, n), _information(info, n, 6)
        if pose_j.size != n:
            raise ValueError("pose_i and pose_j differ in length")
        self._ck(self.lib.cuba_hip_set_relative_pose_edges(self.h, n, _i(pose_i), _i(pose_j), _d(q), _d(t), _d(info)))
        self._n_factors["relative_pose"] = n

    def set_pose_factor_robust_kernels(self, factor_type, kind, delta):
        """Robust kernels of the current pose priors (factor_type 0) or relative-pose edges (1), cuba_hip_set_pose_factor_robust_kernels:
        kind[n] (0 none, 1 Huber, 2 Tukey, 3 Cauchy) and delta[n] in the order the set was given; scalars broadcast to the set's size.
        Empty arrays clear the kernels of that type."""
        n = self._n_factors.get("prior" if factor_type == 0 else "relative_pose", 0)
        if np.ndim(kind) == 0:
            kind = np.full(n, kind)
        if np.ndim(delta) == 0:
            delta = np.full(n, delta)
        kind = np.ascontiguousarray(kind, dtype=np.int32).reshape(-1)
        delta = np.ascontiguousarray(delta, dtype=np.float64).reshape(-1)
        if kind.size != delta.size:
            raise ValueError("kind and delta differ in length")
        self._ck(self.lib.cuba_hip_set_pose_factor_robust_kernels(self.h, int(factor_type), int(kind.size), kind.ctypes.data_as(_ip), _d(delta)))

    def _factor_chi_squares(self, kind):
        """cuba_hip_<kind>_chi_squares: one number per factor of the set last given"""
        n = self._n_factors.get(kind, 0)
        out = np.zeros(max(n, 1))
        self._ck(getattr(self.lib, f"cuba_hip_{kind}_chi_squares")(self.h, _d(out)))
        return out[:n]

    def relative_pose_chi_squares(self):
        """r^T Omega r of every relative-pose edge at the current estimate, in the order they were given (0 with both ends fixed)"""
        return self._factor_chi_squares("relative_pose")

    def prior_chi_squares(self):
        """r^T Omega r of every prior at the current estimate, in the order they were given (0 for priors on fixed poses)"""
        return self._factor_chi_squares("prior")

    def set_landmark_priors(self, landmark, xyz, info, kind=None, delta=None):
        """Landmark position priors (cuba_hip_set_landmark_priors), replacing the handle's set: landmark[n] in the solver numbering,
        xyz[n, 3], info[n, 3, 3] symmetric; kind[n] (0 none, 1 Huber, 2 Tukey, 3 Cauchy) and delta[n] together or not at all (scalars
        broadcast).  An empty landmark list clears the set."""
        landmark = _index(landmark)
        n = int(landmark.size)
        xyz, info = _rows(xyz, n), _information(info, n, 3)
        kind, delta = _kernels(kind, delta, n)
        self._ck(self.lib.cuba_hip_set_landmark_priors(self.h, n, _i(landmark), _d(xyz), _d(info), _i(kind), _d(delta)))
        self._n_factors["landmark_prior"] = n

    def landmark_prior_chi_squares(self):
        """r^T Omega r of every landmark prior at the current estimate, in the order they were given (0 for priors on fixed landmarks)"""
        return self._factor_chi_squares("landmark_prior")

    def set_position_factors(self, pose, position, info, lever_arm=None, kind=None, delta=None):
        """Position factors on the poses (cuba_hip_set_position_factors; GNSS-style fixes), replacing the handle's set: pose[n] in the
        solver numbering, the measured world positions position[n, 3], info[n, 3, 3] symmetric, lever_arm[n, 3] (the measured point in
        the camera frame; None: the camera centre); kind[n] (0 none, 1 Huber, 2 Tukey, 3 Cauchy) and delta[n] together or not at all
        (scalars broadcast).  An empty pose list clears the set."""
        pose = _index(pose)
        n = int(pose.size)
        position, info, lever_arm = _rows(position, n), _information(info, n, 3), _rows(lever_arm, n)
        kind, delta = _kernels(kind, delta, n)
        self._ck(self.lib.cuba_hip_set_position_factors(self.h, n, _i(pose), _d(position), _d(lever_arm), _d(info), _i(kind), _d(delta)))
        self._n_factors["position_factor"] = n

    def position_factor_chi_squares(self):
        """r^T Omega r of every position factor at the current estimate, in the order they were given (0 for factors on fixed poses)"""
        return self._factor_chi_squares("position_factor")

    def set_direction_factors(self, pose, world_dir, measured_dir, info, kind=None, delta=None):
        """Direction factors on the poses (cuba_hip_set_direction_factors; gravity, compass, vanishing directions), replacing the handle's
        set: pose[n] in the solver numbering, the world vectors world_dir[n, 3], the same vectors as measured in the camera frame
        measured_dir[n, 3] (neither is normalised), info[n, 3, 3] symmetric; kind[n] (0 none, 1 Huber, 2 Tukey, 3 Cauchy) and delta[n]
        together or not at all (scalars broadcast).  An empty pose list clears the set."""
        pose = _index(pose)
        n = int(pose.size)
        world_dir, measured_dir, info = _rows(world_dir, n), _rows(measured_dir, n), _information(info, n, 3)
        kind, delta = _kernels(kind, delta, n)
        self._ck(self.lib.cuba_hip_set_direction_factors(self.h, n, _i(pose), _d(world_dir), _d(measured_dir), _d(info), _i(kind), _d(delta)))
        self._n_factors["direction_factor"] = n

    def direction_factor_chi_squares(self):
        """r^T Omega r of every direction factor at the current estimate, in the order they were given (0 for factors on fixed poses)"""
        return self._factor_chi_squares("direction_factor")

    def set_range_factors(self, pose, anchor, range, info, lever_arm=None, kind=None, delta=None):
        """Range factors on the poses (cuba_hip_set_range_factors; UWB-style distances to known anchors), replacing the handle's set:
        pose[n] in the solver numbering, the anchors' world positions anchor[n, 3], the measured distances range[n] (>= 0), the scalar
        informations info[n] (1 / sigma^2, >= 0), lever_arm[n, 3] (the ranging antenna in the camera frame; None: the camera centre);
        kind[n] (0 none, 1 Huber, 2 Tukey, 3 Cauchy) and delta[n] together or not at all (scalars broadcast).  An empty pose list clears
        the set."""
        pose = _index(pose)
        n = int(pose.size)
        anchor, range, info, lever_arm = _rows(anchor, n), _scalars(range, n), _scalars(info, n), _rows(lever_arm, n)
        kind, delta = _kernels(kind, delta, n)
        self._ck(self.lib.cuba_hip_set_range_factors(self.h, n, _i(pose), _d(anchor), _d(range), _d(lever_arm), _d(info), _i(kind), _d(delta)))
        self._n_factors["range_factor"] = n

    def range_factor_chi_squares(self):
        """info r^2 of every range factor at the current estimate, in the order they were given (0 for factors on fixed poses)"""
        return self._factor_chi_squares("range_factor")

    def set_pose_range_factors(self, pose_i, pose_j, range, info, lever_arm_i=None, lever_arm_j=None, kind=None, delta=None):
        """Range factors between two poses (cuba_hip_set_pose_range_factors; odometer distances, peer UWB ranging, rig baselines),
        replacing the handle's set: pose_i[n] != pose_j[n] in the solver numbering, the measured distances range[n] (>= 0), the scalar
        informations info[n] (1 / sigma^2, >= 0), lever_arm_i[n, 3] and lever_arm_j[n, 3] (the two points in their camera frames; None:
        the camera centre); kind[n] (0 none, 1 Huber, 2 Tukey, 3 Cauchy) and delta[n] together or not at all (scalars broadcast).  An
        empty pose list clears the set.  The free-free pairs are part of the topology, as the relative-pose edges'."""
        pose_i, pose_j = _index(pose_i), _index(pose_j)
        n = int(pose_i.size)
        if pose_j.size != n:
            raise ValueError("pose_i / pose_j differ in length")
        range, info, lever_arm_i, lever_arm_j = _scalars(range, n), _scalars(info, n), _rows(lever_arm_i, n), _rows(lever_arm_j, n)
        kind, delta = _kernels(kind, delta, n)
        self._ck(self.lib.cuba_hip_set_pose_range_factors(self.h, n, _i(pose_i), _i(pose_j), _d(range), _d(lever_arm_i), _d(lever_arm_j), _d(info),
                                                          _i(kind), _d(delta)))
        self._n_factors["pose_range_factor"] = n

    def pose_range_factor_chi_squares(self):
        """info r^2 of every range factor between two poses at the current estimate, in the order they were given (0 with both ends fixed)"""
        return self._factor_chi_squares("pose_range_factor")

    def chi_squares_two_step(self):
        """cuba_hip_chi_squares_begin / _end (the C++ layer does its write-back between the two)"""
        out = np.zeros(self.fp.E)
        self._ck(self.lib.cuba_hip_chi_squares_begin(self.h, _d(out)))
        self._ck(self.lib.cuba_hip_chi_squares_end(self.h))
        return out

    def profile(self):
        out = np.zeros(8)
        self._ck(self.lib.cuba_hip_get_profile(self.h, _d(out)))
        return dict(zip(PROFILE_KEYS, out.tolist()))

    def counters(self):
        c = (C.c_int64 * 8)()
        self._ck(self.lib.cuba_hip_get_counters(self.h, c))
        return dict(pcg_iterations=int(c[0]), lm_trials=int(c[1]), hsc_blocks=int(c[2]), schur_products=int(c[3]),
                    coarse_refreshes=int(c[4]), pcg_host_looks=int(c[5]), pcg_iterations_enqueued=int(c[6]), coarse_dim=int(c[7]))

    def counter(self, name):
        """one counter by name (cuba_hip_get_counter), e.g. "coarse_inline_inversions", "pcg_graph_instantiations"."""
        v = C.c_int64()
        self._ck(self.lib.cuba_hip_get_counter(self.h, name.encode(), C.byref(v)))
        return int(v.value)

    def pcg_history(self):
        """(iterations per reduced solve since set_graph [negative = stopped at max_iter], number of unconverged solves)."""
        n, bad = C.c_int(), C.c_int64()
        self._ck(self.lib.cuba_hip_get_pcg_history(self.h, None, 0, C.byref(n), C.byref(bad)))
        it = np.zeros(max(n.value, 1), dtype=np.int32)
        self._ck(self.lib.cuba_hip_get_pcg_history(self.h, it.ctypes.data_as(_ip), n.value, C.byref(n), C.byref(bad)))
        return it[:n.value], int(bad.value)

    def pcg_config(self):
        """The PCG configuration in force (cuba_hip_debug_pcg_config): a dict of agg, cl, nc, spmv_rows, upper, ell_m, ell_over,
        coarse_fp32, rows_ept, and pose_order (the caller's index of every free pose in the solver's internal order)."""
        cfg = (C.c_int32 * 9)()
        n = C.c_size_t()
        self._ck(self.lib.cuba_hip_debug_pcg_config(self.h, cfg, None, 0, C.byref(n)))
        order = np.zeros(max(n.value, 1), dtype=np.int32)
        self._ck(self.lib.cuba_hip_debug_pcg_config(self.h, cfg, order.ctypes.data_as(_ip), n.value, C.byref(n)))
        keys = ("agg", "cl", "nc", "spmv_rows", "upper", "ell_m", "ell_over", "coarse_fp32", "rows_ept")
        out = {k: int(v) for k, v in zip(keys, cfg)}
        out["pose_order"] = order[:n.value]
        return out

    def lm_records(self):
        """The ring of decision records of the last optimize() / optimize_batch() run (cuba_hip_debug_lm_records): [64, 8], record of
        trial k in row k % 64, columns LM_RECORD."""
        n = C.c_size_t()
        self._ck(self.lib.cuba_hip_debug_lm_records(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value)
        self._ck(self.lib.cuba_hip_debug_lm_records(self.h, _d(out), n.value, C.byref(n)))
        return out.reshape(-1, len(LM_RECORD))

    def array(self, name):
        n = C.c_size_t()
        self._ck(self.lib.cuba_hip_get_array(self.h, ARRAY_IDS[name], None, C.byref(n)))
        out = np.zeros(n.value)
        if n.value:
            self._ck(self.lib.cuba_hip_get_array(self.h, ARRAY_IDS[name], _d(out), C.byref(n)))
        return out

    def hsc_structure(self):
        nb = C.c_int()
        self._ck(self.lib.cuba_hip_get_hsc_structure(self.h, None, None, C.byref(nb)))
        rp, ci = np.zeros(self.fp.Pf + 1, dtype=np.int32), np.zeros(nb.value, dtype=np.int32)
        self._ck(self.lib.cuba_hip_get_hsc_structure(self.h, rp.ctypes.data_as(_ip), ci.ctypes.data_as(_ip), C.byref(nb)))
        return rp, ci

    def hsc(self):
        """(rowptr, colind, values[nblk,6,6] indexed [blk][row][col]) of the upper-triangular BSR."""
        rp, ci = self.hsc_structure()
        v = self.array("hsc").reshape(len(ci), 6, 6).transpose(0, 2, 1).copy()
        return rp, ci, v

    def covariance(self, landmarks=True, poses=True):
        """Marginal covariances at the current estimate (cuba_hip_compute_covariance; g2o's computeMarginals): the inverse of the undamped
        Gauss-Newton Hessian.  {"pose": [Pt, 6, 6] in the [omega, upsilon] tangent of the pose update, "landmark": [Lt, 3, 3] (None when
        landmarks=False), "not_positive_definite": bool}; fixed vertices get zero blocks, a matrix that is not positive definite leaves both
        at zero."""
        pose = np.zeros((self.fp.Pt, 6, 6)) if poses else None
        lm = np.zeros((self.fp.Lt, 3, 3)) if landmarks else None
        bad = C.c_int()
        self._ck(self.lib.cuba_hip_compute_covariance(self.h, _d(pose), _d(lm), C.byref(bad)))
        # (column-major 6 x 6 / 3 x 3 blocks: the transpose of the row-major reading -- the blocks are symmetric up to rounding)
        return {"pose": None if pose is None else pose.transpose(0, 2, 1).copy(),
                "landmark": None if lm is None else lm.transpose(0, 2, 1).copy(),
                "not_positive_definite": bool(bad.value)}

    def covariance_blocks(self):
        """values[nblk, 6, 6] ([blk][row][col]) of the marginal covariance on the reduced matrix's pattern, as hsc_structure() numbers the
        blocks, from the last covariance() call (cuba_hip_get_covariance_blocks)"""
        rp, ci = self.hsc_structure()
        out = np.zeros((len(ci), 6, 6))
        self._ck(self.lib.cuba_hip_get_covariance_blocks(self.h, _d(out)))
        return out.transpose(0, 2, 1).copy()

    VERTEX_KINDS = {"pose": 0, "landmark": 1}

    def covariance_pairs(self, pairs):
        """Covariance blocks of arbitrary vertex pairs (cuba_hip_compute_covariance_pairs): pairs = [(kind_a, i, kind_b, j), ...] with kinds
        "pose" / "landmark" and indices in the caller's numbering.  Returns ([array (dim_a, dim_b) per pair, [row][col], rows from a and
        columns from b], not_positive_definite); fixed vertices give zero blocks."""
        n = len(pairs)
        ka = np.zeros(max(n, 1), dtype=np.int32); ia = np.zeros_like(ka); kb = np.zeros_like(ka); ib = np.zeros_like(ka)
        for k, (a_kind, a, b_kind, b) in enumerate(pairs):
            ka[k] = self.VERTEX_KINDS.get(a_kind, -1) if isinstance(a_kind, str) else int(a_kind)
            kb[k] = self.VERTEX_KINDS.get(b_kind, -1) if isinstance(b_kind, str) else int(b_kind)
            ia[k], ib[k] = int(a), int(b)
        out = np.zeros((max(n, 1), 36))
        bad = C.c_int()
        self._ck(self.lib.cuba_hip_compute_covariance_pairs(self.h, n, ka.ctypes.data_as(_ip), ia.ctypes.data_as(_ip), kb.ctypes.data_as(_ip),
                                                            ib.ctypes.data_as(_ip), _d(out), C.byref(bad)))
        blocks = []
        for k in range(n):
            da, db = (6 if ka[k] == 0 else 3), (6 if kb[k] == 0 else 3)
            blocks.append(out[k, :da * db].reshape(db, da).T.copy())
        return blocks, bool(bad.value)

    def time_kernels(self, reps=20):
        out = np.zeros(7)
        self._ck(self.lib.cuba_hip_time_kernels(self.h, int(reps), _d(out)))
        return dict(zip(("residual_chi2", "linearize_schur", "pcg_spmv", "pcg_update", "back_substitute", "pcg_precond",
                         "coarse_setup"), out.tolist()))

    # ---- landmark-partitioned multi-GPU hooks ---------------------------------------------------
    def set_partition(self, lm_begin, lm_end):
        self._ck(self.lib.cuba_hip_set_partition(self.h, int(lm_begin), int(lm_end)))

    def assemble(self): self._ck(self.lib.cuba_hip_assemble(self.h))

    def max_diagonal_parts(self):
        a, b = C.c_double(), C.c_double()
        self._ck(self.lib.cuba_hip_max_diagonal_parts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def compute_scale_parts(self, lam):
        a, b = C.c_double(), C.c_double()
        self._ck(self.lib.cuba_hip_compute_scale_parts(self.h, float(lam), C.byref(a), C.byref(b)))
        return a.value, b.value

    def device_pointer(self, name):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.cuba_hip_device_pointer(self.h, ARRAY_IDS[name], C.byref(p), C.byref(n)))
        return p.value, n.value

    def reduction_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.cuba_hip_reduction_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value
