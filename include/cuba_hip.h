/*
 * cuba_hip.h -- C ABI of the MI355X (gfx950) bundle-adjustment hot path.
 *
 * This is the drop-in boundary: everything the reference's host layer (class CudaBlockSolver,
 * /root/reference/src/cuda_bundle_adjustment.cpp:73-673) asks of its device layer -- the 27 functions
 * of namespace cuba::gpu (src/cuda_block_solver.h:29-94) plus SparseLinearSolver::{initialize,solve}
 * (src/cuda_linear_solver.h:28-39) -- is reachable through the entry points below, one solver handle
 * per graph.  Plain pointers and sizes only; no C++/torch types.  Each entry point names the reference
 * interface it replaces.
 *
 * Conventions
 *   - every call returns a cuba_hip_status (0 = ok); nothing throws across the ABI;
 *     cuba_hip_last_error() gives the message of the last failure on that handle.
 *   - all array arguments are HOST pointers, caller-owned, only read/written during the call.
 *   - Scalar is fp64.  Quaternions are (x,y,z,w), poses are world->camera, small matrices
 *     column-major (as in the reference, src/cuda_block_solver.cu:79-105).
 *   - vertices arrive in "solver order": free poses first [0,Pf), then fixed [Pf,Pt); same for
 *     landmarks (that is what CudaBlockSolver::initialize produces, :142-200).  Edges may come in
 *     any order; per-edge outputs are returned in the caller's order.
 *   - a handle is bound to one device and one HIP stream; it is not re-entrant, distinct handles
 *     may be driven from distinct host threads.
 */
#ifndef CUBA_HIP_H_
#define CUBA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cuba_hip_solver cuba_hip_solver;

typedef enum cuba_hip_status
{
	CUBA_HIP_OK = 0,
	CUBA_HIP_ERR_INVALID_ARGUMENT = 1,
	CUBA_HIP_ERR_RUNTIME = 2,       /* a HIP runtime call failed (reference: CUDA_CHECK only prints, src/macro.h:22-27) */
	CUBA_HIP_ERR_STATE = 3,         /* call order violated (e.g. solve before set_graph) */
	CUBA_HIP_ERR_NO_DEVICE = 4
} cuba_hip_status;

/* robust kernel kinds / edge types: include/cuda_bundle_adjustment_types.h:143-148,213-218 */
enum { CUBA_HIP_ROBUST_NONE = 0, CUBA_HIP_ROBUST_HUBER = 1, CUBA_HIP_ROBUST_TUKEY = 2 };
enum { CUBA_HIP_EDGE_MONOCULAR = 0, CUBA_HIP_EDGE_STEREO = 1 };
/* vertex kinds of cuba_hip_compute_covariance_pairs */
enum { CUBA_HIP_VERTEX_POSE = 0, CUBA_HIP_VERTEX_LANDMARK = 1 };

/* profile buckets, same order and meaning as CudaBlockSolver::ProfileItem (src/cuda_bundle_adjustment.cpp:77-88).
   Bucket 5 ("symbolic decomposition") holds the reduced-system structure analysis, bucket 6
   ("numerical decomposition") the block-PCG solve that replaces cuSOLVER's factor+solve. */
enum { CUBA_HIP_PROFILE_ITEMS = 8 };

/* arrays retrievable with cuba_hip_get_array (introspection for parity tests) */
enum
{
	CUBA_HIP_ARRAY_BP = 0,      /* 6*Pf   gradient-side vector bp                  (d_bp_)      */
	CUBA_HIP_ARRAY_BSC = 1,     /* 6*Pf   reduced right-hand side                   (d_bsc_)     */
	CUBA_HIP_ARRAY_XP = 2,      /* 6*Pf   pose increments                           (d_xp_)      */
	CUBA_HIP_ARRAY_XL = 3,      /* 3*Lf   landmark increments                       (d_xl_)      */
	CUBA_HIP_ARRAY_LM_SYS = 4,  /* 9*Lf   per landmark: 6 unique entries (00,01,02,11,12,22) of Hll
	                                       (after cuba_hip_max_diagonal) or of inv(Hll+lambda I)
	                                       (after cuba_hip_schur), then bl (3)                   */
	CUBA_HIP_ARRAY_HSC = 5,     /* 36*nblk upper-triangular BSR values of Hsc (col-major 6x6);
	                                       after cuba_hip_max_diagonal the diagonal blocks hold Hpp */
	CUBA_HIP_ARRAY_STATE = 6    /* 7*Pt+3*Lt  [q | t | Xw] estimates (cuba_hip_device_pointer only)          */
};

/* ---- lifetime -------------------------------------------------------------------------------- */

/* Replaces: CudaBundleAdjustment::create() -> CudaBlockSolver construction (src/cuda_bundle_adjustment.cpp:905-908).
   Threads: a handle is not re-entrant; distinct handles may be driven from distinct host threads at once (the reference's
   CudaBundleAdjustment objects are independent too, include/cuda_bundle_adjustment.h:34-125).  Each handle owns one work stream, one
   low-priority side stream (coarse inversions) and one upload stream.  hipGraphs are OPT-IN (option "pcg_graph" = 1 or CUBA_HIP_GRAPHS=1
   in the environment; the handle then also owns a helper thread that calls hipGraphInstantiate / hipGraphExecDestroy in the background --
   relevant for callers that fork, or that capture with hipStreamCaptureModeGlobal): on this runtime a process that has ever instantiated a
   hipGraph no longer overlaps the kernel chains of two streams (two KITTI-00 graphs from two threads: 1.5 x one graph's throughput
   without graphs, 1.0 x with), while a lone handle is only ~2 % faster with them.  With graphs on, the library
   still stops using them while more than one handle is alive. */
int cuba_hip_create(int device, cuba_hip_solver** out);
int cuba_hip_destroy(cuba_hip_solver* s);
const char* cuba_hip_last_error(const cuba_hip_solver* s);
const char* cuba_hip_version(void);
/* 8 for libcuba_hip.so, 4 for libcuba_hip_f32.so (the reference's USE_FLOAT32 build option, src/scalar.h:25-29):
   element size of the device arrays behind cuba_hip_device_pointer / cuba_hip_reduction_buffer.  Host-side
   arguments of every entry point are double in both builds. */
int cuba_hip_scalar_size(void);

/* Page-locked host memory for the caller's staging arrays (what it passes to cuba_hip_set_graph / receives from
   cuba_hip_get_solution / cuba_hip_chi_squares): transfers from it run at full PCIe rate and asynchronously.  Falls back to malloc
   when no device is visible; cuba_hip_host_free releases either kind.  Optional -- any host pointer is accepted everywhere. */
void* cuba_hip_host_alloc(size_t bytes);
void cuba_hip_host_free(void* p);

/* Run on an existing hipStream_t (e.g. torch's current stream) instead of the handle's private one. */
int cuba_hip_set_stream(cuba_hip_solver* s, void* hip_stream);

/* Options (20).  Solver: "pcg_tol" (relative preconditioned-residual tolerance of the reduced solve, default 1e-7; fp32 build 1e-4),
   "pcg_max_iter" (default 4*6*Pf capped at 32768), "pcg_accept_unconverged" (default 0, see cuba_hip_get_pcg_history),
   "direct_fallback" (default 1: a reduced solve whose PCG uses up its iteration budget, breaks down, or follows such a solve in the
   same Levenberg-Marquardt run is solved EXACTLY on the device -- sparse tile Cholesky, csrc/ba_direct.hip: minimum-degree ordering
   and symbolic analysis once per structure at the first exact solve, numeric factorisation + triangular solves per solve, the three
   phases of SparseLinearSolver, /root/reference/src/cuda_linear_solver.cpp:278-348, 147-232, 386-415 -- and fails only on a
   non-positive pivot like the reference, :406-410; 0 = the solve is reported as failed instead), "reduced_solver" (default 0 = block
   PCG with that fallback; 1 = EVERY reduced solve is the exact one, the reference's behaviour), "direct_after" (PCG iterations before
   the hand-over; default 0 = automatic: Pf / 4 clamped to 128 ... 384 -- about twice what an exact solve costs --, at most
   pcg_max_iter; a function of the graph's size, so that the decision never depends on timing), "direct_max_tiles" (default 2^20: the fill of the factor, in 32 x 32 tiles of 5 poses x 5 poses,
   beyond which the exact solver is not used and the failure report stands; a 10 000-pose trajectory with loop closures needs 19 000),
   "direct_slack" (default -1 = automatic: multiple-elimination slack of the ordering, 0 / 2 / 4 / 8 by a cost model of levels and fill),
   "pcg_aggregate" (poses per coarse aggregate of the two-level preconditioner; -1 = automatic: max(6, Pf/55) below 1320 free poses,
   max(16, Pf/min(180, max(115, Pf/32))) above; 0 = block-Jacobi only), "coarse_linear" (default 1: constant + linear-in-pose-index
   coarse functions per aggregate, 12 unknowns each; 0 = constant only, 6 unknowns), "precond_fp32" (fp64 library only, default 1: the
   explicit coarse inverse is STORED in fp32 -- symmetrised, applied with fp64 accumulation; a solve whose PCG breaks down with it is
   repeated with fp64 storage, which the handle then keeps; 0 = fp64 storage), "mixed_precision" (fp64 library only, default 0; 1 =
   per-edge linearisation records and the per-edge arithmetic of the pose / block Schur passes in fp32, every sum over edges, the
   reduced system and the PCG in fp64 -- the reference's USE_FLOAT32 idea, src/scalar.h:25-29, applied where it is second-order for
   the objective).
   The coarse matrix of a trial is assembled and inverted on a second, low-priority stream under that trial's PCG and serves from a
   later trial on (every trial up to a coarse dimension of 512, every second up to 1024, every third beyond); only the first solve
   on a structure inverts in line.
   "heuristics" (default 1: two run-to-run memories, exact when a run repeats the previous one and harmless otherwise -- the first
   solve of an LM run starts with the coarse inverse the first solve of the PREVIOUS run on this structure had, same damping regime,
   while its own inversion runs on the second stream; and a run that has repeated the previous run solve for solve so far sizes its
   next batch of iterations from that run instead of extrapolating; 0 = neither, what bench.py's "heuristics_off" prices).
   "spmv_upper" (default -1 = automatic: on beyond 1536 free poses, where the PCG kernels are bound by bytes; 1 / 0 = on / off: the
   PCG iteration as three launches straight from the upper-triangular BSR storage -- SpMV with the transposed products parked per
   block, row updates + P^T r per aggregate, preconditioner -- instead of two launches on a row-ordered copy of both triangles).
   "reduction_chunks" (default 0 = automatic; landmark partitions only: number of block-row ranges the reduced matrix is produced -- and,
   by the multi-GPU driver, summed -- in, see cuba_hip_schur_part),
   "landmark_reorder" (default 1, takes effect with the next cuba_hip_set_graph -- also one that uploads the previous call's index arrays
   again, promised or not --: the free landmarks are renumbered internally by (first, last)
   observing pose of the internal pose order, so that landmark-major data inherit the trajectory's locality whatever the caller's ids are;
   every host-pointer entry point keeps the caller's landmark numbering; a landmark partition other than the whole range, and the host
   pipeline, use the caller's order),
   cuba_hip_optimize takes the decision of every trial -- gain ratio, acceptance, next damping -- on the device and enqueues the next
   trial without having seen it, a rejected trial being undone by a conditional restore launch, and runs back-substitution, update and
   evaluation of a trial as ONE pass over the edges (control flow of /root/reference/src/cuda_bundle_adjustment.cpp:816-851; a
   landmark partition and "profile" use the host loop over the stage kernels instead).
   Execution: "pcg_graph" (default 0, or 1 when the environment has CUBA_HIP_GRAPHS=1: PCG iterations are replayed as hipGraphs of
   4 ... 256 iterations and of the exact batch lengths that come back; opt-in since round 6 -- a lone handle gains ~2 %, a process
   that has instantiated a hipGraph no longer overlaps the kernel chains of several handles; see cuba_hip_create),
   "device_setup" (default 1: the edge sort of
   cuba_hip_set_graph and the whole symbolic analysis of cuba_hip_build_structure run on the GPU; 0 = the host pipeline, the
   independent cross-check of the tests; on a handle that holds a graph the analysis follows the option at once, the edge sort and
   with it the internal landmark order with the next cuba_hip_set_graph -- until then sums may differ from a fresh handle's in rounding), "pose_reorder" (default 1: when most blocks of the reduced matrix lie far off its diagonal
   in the caller's pose numbering -- arbitrary vertex ids --, the free poses are renumbered internally along the trajectory found by
   a strongest-neighbour walk over the co-visibility counts, which the aggregates of the preconditioner need; every host-pointer
   entry point keeps the caller's numbering, only cuba_hip_device_pointer / cuba_hip_reduction_buffer expose the internal one; 0 takes
   effect with the next cuba_hip_set_graph, which then starts from the caller's numbering also when it uploads the same index arrays),
   "profile" (0/1: per-stage synchronising wall-clock like the reference's get_time_point(), src/cuda_bundle_adjustment.cpp:43-47).
   Variants that were built, measured slower and removed again (first-generation Schur kernel with fp64 atomics, single-launch
   PCG iteration, speculative trial tail, in-line coarse refresh policy, CU-masked side stream, forcing term on the PCG tolerance)
   are documented with their numbers in DESIGN.md section 4 and profiles/. */
int cuba_hip_set_option(cuba_hip_solver* s, const char* key, double value);

/* ---- graph upload ---------------------------------------------------------------------------- */

/* Replaces: the SoA gather + uploads of CudaBlockSolver::initialize / buildStructure
   (src/cuda_bundle_adjustment.cpp:115-261, :319-354).
   q[4*Pt], t[3*Pt], cam[5*Pt] = (fx,fy,cx,cy,bf) per pose, Xw[3*Lt];
   edge_pose[E], edge_landmark[E] solver indices; edge_dim[E] in {2,3};
   meas[3*E] (third component ignored for monocular edges); omega[E] scalar information.
   Edges whose two ends are both fixed must already be removed (as the reference does, :204-243).
   A cuba_hip_set_graph[_begin / _partition] that is refused with CUBA_HIP_ERR_INVALID_ARGUMENT (bad counts, a null array, a bad landmark
   range, an edge index or dimension out of range, an edge between two fixed vertices) leaves the handle as it was: the previous graph, its
   factor sets, its mask and its snapshot slots stay in force; only a pending cuba_hip_hint_unchanged promise is consumed.  A previous
   graph whose cuba_hip_set_graph_begin is still open stays open: its meas / omega must stay valid until its cuba_hip_set_graph_end. */
int cuba_hip_set_graph(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf,
	const double* q, const double* t, const double* cam, const double* Xw,
	int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim,
	const double* meas, const double* omega);

/* The same upload in two steps, for a caller whose meas / omega arrays stay valid (and unchanged) until cuba_hip_set_graph_end: _begin
   returns once every other argument has been consumed, while the 32 bytes per edge of measurements and information may still be
   crossing PCIe on a second stream; the caller then typically calls cuba_hip_build_structure -- the symbolic analysis needs the index
   arrays only, so the transfer hides under it (0.7 ms of a 1.2 ms analysis at KITTI-00 size) -- and cuba_hip_set_graph_end, which
   waits for the transfer.  Any entry point that needs the values finishes the transfer itself; page-locked arrays
   (cuba_hip_host_alloc) are what makes the transfer asynchronous.  A cuba_hip_hint_unchanged promise covers _begin like set_graph. */
int cuba_hip_set_graph_begin(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf,
	const double* q, const double* t, const double* cam, const double* Xw,
	int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim,
	const double* meas, const double* omega);
int cuba_hip_set_graph_end(cuba_hip_solver* s);

/* A promise about the NEXT cuba_hip_set_graph call only (it is consumed by that call, successful or not):
   same_edges  != 0: edge_pose / edge_landmark / edge_dim and all five counts are identical to those of the previous successful call
                     (the library then skips its own comparison of the index arrays);
   same_values != 0: in addition meas and omega are bit-identical to the previous call's, so their 32 bytes per edge need not cross
                     PCIe again (the estimates q / t / cam / Xw are uploaded in any case).
   A host layer that re-walks its own graph anyway (the reference re-reads every edge in initialize(), src/cuda_bundle_adjustment.cpp:
   204-243) learns both facts for free while it copies; a caller that cannot vouch for them simply does not call this.  A wrong
   promise is not detected: the solver then works on the previous call's edges / values. */
int cuba_hip_hint_unchanged(cuba_hip_solver* s, int same_edges, int same_values);

/* Replaces: CudaBundleAdjustment::setRobustKernels (src/cuda_bundle_adjustment.cpp:781-784). */
int cuba_hip_set_robust_kernel(cuba_hip_solver* s, int edge_type, int kind, double delta);

/* Replaces: CudaBlockSolver::buildStructure (:263-366): gpu::buildHplStructure,
   HschurSparseBlockMatrix::constructFromVertices, gpu::findHschureMulBlockIndices and
   SparseLinearSolver::initialize (symbolic analysis).  Called implicitly if omitted. */
int cuba_hip_build_structure(cuba_hip_solver* s);

/* ---- per-iteration stages (same granularity as CudaBlockSolver's public methods) ---------------- */

/* Replaces: CudaBlockSolver::computeErrors -> gpu::computeActiveErrors x2 (:368-382). Total robust chi2. */
int cuba_hip_compute_errors(cuba_hip_solver* s, double* chi2);

/* Replaces: CudaBlockSolver::buildSystem -> gpu::constructQuadraticForm x2 (:384-410).
   Marks the current estimate as the linearisation point; the Jacobian products themselves are
   (re)computed inside cuba_hip_max_diagonal / cuba_hip_schur, nothing is materialised per edge. */
int cuba_hip_build_system(cuba_hip_solver* s);

/* Replaces: CudaBlockSolver::maxDiagonal -> gpu::maxDiagonal x2 (:412-418). */
int cuba_hip_max_diagonal(cuba_hip_solver* s, double* max_diag);

/* Replaces: CudaBlockSolver::setLambda / restoreDiagonal -> gpu::addLambda / gpu::restoreDiagonal
   (:420-430).  lambda is applied on the fly, so restore only forgets it. */
int cuba_hip_set_lambda(cuba_hip_solver* s, double lambda);
int cuba_hip_restore_diagonal(cuba_hip_solver* s);

/* CudaBlockSolver::solve (:432-481) in three separately callable parts (so a landmark-partitioned
   multi-GPU driver can all-reduce between them), and as one call:
     schur           gpu::computeBschure + gpu::computeHschure                        (:443-444)
     solve_reduced   gpu::convertHschureBSRToCSR + SparseLinearSolver::solve          (:452-453),
                     here a block-Jacobi preconditioned block PCG on the BSR matrix
     back_substitute gpu::schurComplementPost                                          (:463)
   *ok = 0 reports a numerical failure (non-SPD pivot / PCG breakdown), the reference's
   "factorize failed" path (src/cuda_linear_solver.cpp:406-410). */
int cuba_hip_schur(cuba_hip_solver* s);
int cuba_hip_solve_reduced(cuba_hip_solver* s, int* ok);
int cuba_hip_back_substitute(cuba_hip_solver* s);
int cuba_hip_solve(cuba_hip_solver* s, int* ok);

/* Replaces: CudaBlockSolver::update -> gpu::updatePoses + gpu::updateLandmarks (:483-492). */
int cuba_hip_update(cuba_hip_solver* s);

/* Replaces: CudaBlockSolver::computeScale -> gpu::computeScale (:494-500). sum x (lambda x + b). */
int cuba_hip_compute_scale(cuba_hip_solver* s, double lambda, double* scale);

/* Replaces: CudaBlockSolver::push / pop (:502-510). */
int cuba_hip_push(cuba_hip_solver* s);
int cuba_hip_pop(cuba_hip_solver* s);

/* A second, caller-controlled copy of the estimates on the device (push / pop above are the LM loop's own and are overwritten by
   every trial of cuba_hip_optimize): snapshot keeps [q | t | Xw] as they are now, restore brings them back with one device-to-device
   copy on the handle's stream -- repeated runs from one starting point (benchmarks, parameter sweeps) need no host round trip.
   No counterpart in the reference, whose callers re-upload through initialize(). */
int cuba_hip_snapshot_state(cuba_hip_solver* s);      /* = slot 0 */
int cuba_hip_restore_state(cuba_hip_solver* s);
/* The same with several copies (slot in [0, CUBA_HIP_SNAPSHOT_SLOTS)): a caller that re-optimises from a SET of starting points --
   a benchmark whose timed runs must not replay one another, a sweep over perturbations -- prepares them once and switches between
   them with one device-to-device copy each.  Copies are dropped by cuba_hip_set_graph and whenever the library changes its
   internal pose order ("pose_reorder"): restoring an absent slot is CUBA_HIP_ERR_STATE, never a silent mix-up of pose rows. */
enum { CUBA_HIP_SNAPSHOT_SLOTS = 64 };
int cuba_hip_snapshot_state_slot(cuba_hip_solver* s, int slot);
int cuba_hip_restore_state_slot(cuba_hip_solver* s, int slot);

/* ---- whole Levenberg-Marquardt run -------------------------------------------------------------- */

/* Replaces: the loop of CudaBundleAdjustmentImpl::optimize (src/cuda_bundle_adjustment.cpp:793-857)
   with identical control flow (tau = 1e-5, at most 10 trials per iteration, g2o's rho / lambda rules),
   executed inside the library to avoid per-stage host round trips.
   chi2_per_iter[niterations] receives BatchInfo::chi2 for each executed iteration, *n_done their count. */
int cuba_hip_optimize(cuba_hip_solver* s, int niterations, double* chi2_per_iter, int* n_done);

/* The same for SEVERAL handles at once, in one launch chain.  Replaces: independent CudaBundleAdjustment objects optimised side by
   side (include/cuda_bundle_adjustment.h:34-125 -- ORB-SLAM's local BA windows, BASELINE configs[3]'s independent graphs when they share
   a GPU).  Every handle runs its own Levenberg-Marquardt loop exactly as cuba_hip_optimize would -- its own damping, acceptance
   decisions (taken on the device, per graph), iteration counts and stopping -- and everything of a trial but the PCG iterations on its
   own stream; the PCG iterations of all graphs are issued as ONE chain of batched launches (the graph number is the launch grid's second
   dimension, the kernels' arguments come from a device table), so the host pays 2 launches per iteration for the batch instead of 2
   per graph.  Results are bit-identical to cuba_hip_optimize on each handle alone.  Graphs of one size class batch together (two-launch
   iteration with a two-level preconditioner, the same coarse-dimension and occupancy class, same "pcg_tol", same device, distinct
   streams, no "profile", no landmark partition); anything else is run one handle after the other, with the same results.
   handles[n] (distinct, n <= 64), chi2_per_iter[n * niterations] (row i = handle i; may be NULL), n_done[n];
   *batched_solves (optional) = reduced solves that ran as a batch (0: the fallback ran).  The calling thread drives all handles: do not
   use them from other threads meanwhile.  Errors are recorded on handles[0]. */
int cuba_hip_optimize_batch(cuba_hip_solver** handles, int n, int niterations, double* chi2_per_iter, int* n_done, int* batched_solves);

/* ---- results ------------------------------------------------------------------------------------ */

/* Replaces: CudaBlockSolver::finalize downloads (:512-526). */
int cuba_hip_get_solution(cuba_hip_solver* s, double* q, double* t, double* Xw);
int cuba_hip_set_solution(cuba_hip_solver* s, const double* q, const double* t, const double* Xw);

/* Replaces: CudaBlockSolver::getChiSqs -> gpu::computeChiSquares x2 (:528-543).
   Non-robust omega*|r|^2 per edge, in the caller's edge order.  omega is the information in force: 0 for an edge that is gated
   (cuba_hip_gate_edges, below; g2o's rule for an inactive edge).  The ungated value comes from cuba_hip_gate_edges. */
int cuba_hip_chi_squares(cuba_hip_solver* s, double* chi2_per_edge);
/* The same in two steps, for a caller that has host work of its own to do meanwhile (the C++ layer copies the estimates back into the
   caller's vertices): _begin enqueues the evaluation and the copy into chi2_per_edge (page-locked memory from cuba_hip_host_alloc, or the
   copy is not asynchronous) and returns; cuba_hip_chi_squares_end waits for it.  No other call on the handle in between. */
int cuba_hip_chi_squares_begin(cuba_hip_solver* s, double* chi2_per_edge);
int cuba_hip_chi_squares_end(cuba_hip_solver* s);

/* ---- edge gating ---------------------------------------------------------------------------------- */

/* Replaces: nothing of the reference -- g2o's setLevel(1) / computeActiveErrors flow of ORB-SLAM's local bundle adjustment (optimize(5),
   switch off every edge with chi2 > 5.991 / 7.815 or non-positive depth, optimize(10) on the rest) and pose optimisation (four rounds,
   edges come back when they recover), which the reference lacks: there a caller reads cuba_hip_chi_squares back, re-flattens the graph
   without the outliers and uploads a new topology.  Here a gated reprojection edge stays in the graph as an edge of zero information:
   no new sort, structure, symbolic analysis or exact-solver plan.  cuba_hip_compute_errors, cuba_hip_optimize[_batch], the stage calls
   and both covariance calls see the active edges only (g2o's activeChi2); cuba_hip_chi_squares reports 0 for a gated edge.

   cuba_hip_gate_edges classifies every edge on the device at the current estimate with its UPLOADED information omega: it stays active
   iff omega*|r|^2 <= chi2_max[stereo] and (require_positive_depth == 0 or its point's depth in the camera is > 0); a NaN fails both.
   chi2_max[2] = {monocular, stereo}, +inf = no chi2 test, NaN = CUBA_HIP_ERR_INVALID_ARGUMENT (as is an unknown mode).
   mode: CUBA_HIP_GATE_RECLASSIFY judges every edge afresh (gated edges can come back), CUBA_HIP_GATE_ONLY_REMOVE never re-admits a gated
   edge, CUBA_HIP_GATE_DRY_RUN changes nothing and only reports.
   counts[6] (optional): active monocular, active stereo, gated by chi2 monocular, gated by chi2 stereo, gated by depth (whatever its
   chi2), edges whose state changed (would change: dry run).  With ONLY_REMOVE an edge that stays gated although it passes both tests is
   in none of the first five.
   chi2_per_edge (optional): the UNGATED omega*|r|^2, caller's edge order.

   The mask outlives a cuba_hip_set_graph whose edge arrays (pose, landmark, dimension, count) are those of the previous call --
   promised by cuba_hip_hint_unchanged or found by the library's own comparison --: the live information is rebuilt from the newly uploaded
   one, and a same_values promise still means the uploaded information, never a gated zero.  Any other cuba_hip_set_graph drops the mask
   (all edges active, storage freed).  None of these calls touches the estimates, the snapshot slots or the counters structure_builds,
   graph_uploads, value_bytes_uploaded.  A handle that never calls them allocates and launches nothing for them.
   CUBA_HIP_ERR_STATE before cuba_hip_set_graph and on a landmark-partitioned handle (cuba_hip_set_partition, cuba_hip_set_graph_partition;
   a gated handle in turn refuses cuba_hip_set_partition).
   Known limit: a GATED edge whose point lies at depth exactly 0.0 in its camera still yields 0 * inf = NaN in the evaluation kernels. */
enum { CUBA_HIP_GATE_RECLASSIFY = 0, CUBA_HIP_GATE_ONLY_REMOVE = 1, CUBA_HIP_GATE_DRY_RUN = 2 };
int cuba_hip_gate_edges(cuba_hip_solver* s, const double chi2_max[2], int require_positive_depth, int mode, int64_t counts[6], double* chi2_per_edge);
/* g2o's setLevel per edge: active[E] in the caller's edge order, non-zero = active.  NULL: all active, the gate's storage is freed. */
int cuba_hip_set_edge_active(cuba_hip_solver* s, const uint8_t* active);
/* active[E] in the caller's edge order, 0 / 1; all 1 on a handle without a gate */
int cuba_hip_get_edge_active(cuba_hip_solver* s, uint8_t* active);
/* per_landmark[Lt] in the caller's landmark order: active edges of every landmark (ORB-SLAM culls map points left with fewer than two) */
int cuba_hip_landmark_active_edges(cuba_hip_solver* s, int32_t* per_landmark);

/* ---- landmark triangulation ---------------------------------------------------------------------- */

/* Replaces: nothing of the reference -- g2o's StructureOnlySolver<3> / ORB-SLAM's CreateNewMapPoints: the position a landmark has
   BEFORE it is optimised (new map points behind a keyframe, points whose edges were gated and came back, points behind a loop
   closure that moved the poses).  Without it a caller reads the poses back, triangulates on the host and uploads the points again.
   Here every free landmark is (re-)triangulated on the device from its ACTIVE reprojection edges (live information omega > 0: a gated
   edge is out) and the current pose estimates, all arithmetic in double in both libraries.  Per landmark, the first rule that applies:
     NOT_SELECTED       select given and select[l] == 0
     FIXED              a fixed landmark
     FEW_OBSERVATIONS   fewer than two active edges, none of them a stereo edge of positive disparity u - u_r
     LOW_PARALLAX       (only without such a stereo edge, and min_parallax_deg > 0) the mean of the unit viewing rays in the world
                        frame is longer than cos(min_parallax_deg / 2) -- two views: their angle is below min_parallax_deg
     SINGULAR           the linear start (below) or a refinement step met a non-positive determinant or a non-finite number
     BEHIND_CAMERA      at the final position an active edge has depth <= 0
     CHI2               at the final position an active edge has omega |r|^2 > chi2_max[stereo] (+inf: no such test)
     OK                 the landmark's position is replaced (dry_run != 0: nothing is written)
   Linear start: the rows (fx R0 + (cx - u) R2) X = -(fx t0 + (cx - u) t2), the same in v and -- stereo -- in u_r with bf on the right,
   weighted by omega, solved through the 3 x 3 normal equations; the landmark's current position is never read (it may be NaN).
   Refinement: refine_iterations (0 ... 16) Gauss-Newton steps on the landmark's robustified reprojection cost with the handle's robust
   kernels (cuba_hip_set_robust_kernel), the poses held.  Landmark priors (cuba_hip_set_landmark_priors) take NO part in any of this.
   Known limit: SINGULAR is a test of a determinant's sign.  Where a Tukey kernel gives every edge of a landmark but ONE monocular edge
   the weight 0, H has rank 2, its determinant is rounding noise (1e-16 of the diagonal's product) and whether such a landmark is reported
   as SINGULAR or as what the huge step leads to (CHI2, BEHIND_CAMERA) is not determined; it is rejected either way.
   select[Lt] (optional), status[Lt] (optional), xyz[3 Lt] (optional): the caller's landmark numbering; xyz receives the accepted position
   of every OK landmark (as the estimate holds it) and the unchanged current position of every other one.
   counts[CUBA_HIP_TRI_STATUSES] (optional): landmarks per status; they sum to Lt.
   Poses, unselected, fixed and rejected landmarks, the gate, the snapshot slots and the counters stay as they are; a covariance computed
   before is dropped when a position changed.  A handle that never calls this allocates and launches nothing for it.
   CUBA_HIP_ERR_INVALID_ARGUMENT: refine_iterations outside 0 ... 16, a NaN min_parallax_deg or threshold, chi2_max NULL.
   CUBA_HIP_ERR_STATE before cuba_hip_set_graph and on a landmark-partitioned handle. */
enum { CUBA_HIP_TRI_OK = 0, CUBA_HIP_TRI_NOT_SELECTED, CUBA_HIP_TRI_FIXED, CUBA_HIP_TRI_FEW_OBSERVATIONS,
       CUBA_HIP_TRI_LOW_PARALLAX, CUBA_HIP_TRI_SINGULAR, CUBA_HIP_TRI_BEHIND_CAMERA, CUBA_HIP_TRI_CHI2, CUBA_HIP_TRI_STATUSES };
int cuba_hip_triangulate_landmarks(cuba_hip_solver* s, const uint8_t* select, int refine_iterations, double min_parallax_deg,
	const double chi2_max[2], int dry_run, int32_t* status, int64_t counts[CUBA_HIP_TRI_STATUSES], double* xyz);

/* ---- pose refinement with the landmarks held -------------------------------------------------------- */

/* Replaces: nothing of the reference -- g2o's motion-only bundle adjustment with EdgeSE3ProjectXYZOnlyPose, ORB-SLAM's
   Optimizer::PoseOptimization, the PnP refinement of a relocalisation candidate: the value a POSE gets from the current landmarks (poses
   behind a loop closure or a map merge, new keyframes whose start is a motion-model guess, the poses of a window whose points were just
   re-triangulated) -- the mirror image of cuba_hip_triangulate_landmarks and the flow "pose optimisation (four rounds, edges come back
   when they recover)" of the gating section above.  Free and fixed landmarks are both HELD at their current estimate, so every free pose
   is a 6-parameter problem of its own: all its Levenberg-Marquardt trials and all its outlier rounds run inside one launch, each pose
   with a damping of its own, all arithmetic in double in both libraries.
   The only terms are the pose's reprojection edges of live information omega > 0 (a gated edge is out).  Pose priors, relative-pose
   edges, position, direction and range factors take NO part (as landmark priors take none in triangulation).
   Classification, at the start of round k = 0 ... rounds - 1 and once more behind the last round, at the pose's then-current value:
     round 0       an edge is in iff omega > 0 and its point's depth in the camera is > 0
     later, final  it must also satisfy omega |r|^2 <= chi2_max[stereo] (chi2_max = {monocular, stereo}; +inf: no chi2 test; a NaN fails)
   An edge that was out can come back (ORB-SLAM's rule).  The classification lives in a scratch byte per edge owned by this call: the
   handle's gate is neither read for it (beyond omega > 0) nor written -- pass edge_inlier to cuba_hip_set_edge_active for that.
   One round: lambda = 1e-5 max_k H_kk at the round's first linearisation, nu = 2, then `iterations` TRIALS, a fixed count without an
   early exit.  A trial:
     1. H = sum w' J^T J, b = sum w' J^T r, F = sum rho(omega |r|^2) over the round's edges; r = proj - meas, J the 2 x 6 or 3 x 6
        Jacobian -d r / d [omega; upsilon] for the left-multiplicative update T <- exp([omega; upsilon]) T (the convention of the pose
        update everywhere in this library), w' = omega rho'(omega |r|^2), rho the handle's robust kernels (cuba_hip_set_robust_kernel) in
        the rounds below robust_rounds and the identity kernel in the later ones (ORB-SLAM drops Huber after two rounds)
     2. (H + lambda I) d = b by a 6 x 6 LDL^T; a non-positive pivot or a non-finite number: SINGULAR
     3. T' = exp(d) T; the trial is rejected if an edge of the round has depth <= 0 at T' or F' is not finite
     4. otherwise gain = (F - F') / (d^T (lambda d + b)); gain > 0: accept, lambda <- lambda max(1/3, 1 - (2 gain - 1)^3), nu = 2;
        else (also for a NaN gain and a denominator of exactly 0) lambda <- lambda nu, nu <- 2 nu
   Per pose, the first rule that applies:
     NOT_SELECTED       select given and select[p] == 0
     FIXED              a fixed pose
     FEW_OBSERVATIONS   fewer than 3 edges in at round 0
     SINGULAR           step 2 of a trial
     FEW_INLIERS        fewer than max(3, min_inliers) edges in at a later round's start or at the final classification
     OK                 the pose is replaced (dry_run != 0: nothing is written)
   rounds 1 ... 4, iterations 1 ... 32, robust_rounds 0 ... rounds, min_inliers >= 0.
   select[Pt], status[Pt], inliers[Pt], chi2[Pt], q[4 Pt] (x, y, z, w), t[3 Pt]: the caller's pose numbering; edge_inlier[E]: the
   caller's edge order.  Every array argument but chi2_max is optional (NULL).
     q, t           the refined pose of every OK pose as the estimate holds it (also in a dry run), the unchanged current pose of every other
     inliers[p]     the edges in at the pose's last classification: the final one for OK poses (and FEW_INLIERS decided there); 0 for a
                    pose that is not selected or fixed
     chi2[p]        sum omega |r|^2 (without the robust kernel) over the final inliers; 0 for a pose that did not reach the final classification
     edge_inlier[e] the final classification for the edges of poses that reached it; for every other edge whether its live omega > 0
     counts[CUBA_HIP_POSEREF_STATUSES]   poses per status; they sum to Pt
   Landmarks, unselected, fixed and rejected poses, the gate, the snapshot slots, the handle's LM state and the counters stay as they
   are; a covariance computed before is dropped when a pose changed.  A handle that never calls this allocates and launches nothing for it.
   CUBA_HIP_ERR_INVALID_ARGUMENT: a count outside its range, a NaN threshold, chi2_max NULL.
   CUBA_HIP_ERR_STATE before cuba_hip_set_graph and on a landmark-partitioned handle. */
enum { CUBA_HIP_POSEREF_OK = 0, CUBA_HIP_POSEREF_NOT_SELECTED, CUBA_HIP_POSEREF_FIXED, CUBA_HIP_POSEREF_FEW_OBSERVATIONS,
       CUBA_HIP_POSEREF_SINGULAR, CUBA_HIP_POSEREF_FEW_INLIERS, CUBA_HIP_POSEREF_STATUSES };
int cuba_hip_refine_poses(cuba_hip_solver* s, const uint8_t* select, int rounds, int iterations, int robust_rounds, const double chi2_max[2],
	int min_inliers, int dry_run, int32_t* status, int64_t counts[CUBA_HIP_POSEREF_STATUSES], int32_t* inliers, double* chi2, double* q, double* t,
	uint8_t* edge_inlier);

/* ---- pose localisation from scratch: P3P RANSAC per pose ---------------------------------------------- */

/* Replaces: nothing of the reference -- the first half of ORB-SLAM's Tracking::Relocalization (PnP-RANSAC; cuba_hip_refine_poses is
   the second half, PoseOptimization): the value a POSE gets when there is no usable guess at all (a relocalisation after tracking loss,
   a keyframe joined from another map, a pose behind a wrong loop closure, a camera with only 2-D - 3-D matches) -- the counterpart of the
   triangulation's linear start.  An absolute pose per selected free pose from its active reprojection edges and the current landmarks
   only, by a deterministic RANSAC over a minimal three-point solver; the intended flow is localize_poses -> refine_poses -> optimize.
   All arithmetic in double in both libraries.  THE POSE'S CURRENT VALUE IS NEVER READ (it may be NaN).
   1. Usable edges: the pose's reprojection edges of live information omega > 0 (a gated edge is out).  Free and fixed landmarks are both
      held at their current estimate.  Pose factors, landmark priors and robust kernels take no part.  Fewer than 4: FEW_OBSERVATIONS.
   2. Sampling: hypothesis h = 0 ... hypotheses - 1 takes the three usable edges of smallest key K(seed, p, h, e), p and e the CALLER's
      pose and edge indices, a tie to the smaller e; the three enter the solver ordered by key (points 1, 2, 3).  With
        mix(x):  x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;  x ^= x >> 27;  x *= 0x94d049bb133111eb;  x ^= x >> 31     (mod 2^64)
        K = mix(mix(mix(mix(seed + 0x9e3779b97f4a7c15) + p) + h) + e)
      so the sample does not depend on pose_reorder, landmark_reorder, device_setup or the internal sort.  A fixed count, no early exit.
   3. Minimal solver (P3P, Grunert's law-of-cosines system reduced to a quartic in one depth ratio).  Every edge gives the unit bearing
      f = (x, y, 1) / sqrt(x^2 + y^2 + 1), x = (u - cx) / fx, y = (v - cy) / fy (a stereo edge: its left measurement only).  With the
      landmarks X_1, X_2, X_3:  a2 = |X_2 - X_3|^2, b2 = |X_1 - X_3|^2, c2 = |X_1 - X_2|^2, ca = f_2 . f_3, cb = f_1 . f_3, cg = f_1 . f_2,
      K = (a2 - c2) / b2, C = c2 / b2, and the distances s_1, s_2 = u s_1, s_3 = v s_1 of the points from the centre:
        N(v) = (K - 1) v^2 - 2 K cb v + (1 + K),   D(v) = 2 (cg - ca v),   W(v) = -C v^2 + 2 C cb v + (1 - C),    u = N / D
        quartic  N^2 - 2 cg N D + D^2 W = A_4 v^4 + ... + A_0  (the coefficients by multiplying out), divided by A_4:  v^4 + B v^3 + C' v^2 + D' v + E
        depressed with v = y - B / 4:  y^4 + p y^2 + q y + r;  resolvent  m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0, its LARGEST real
        root m in closed form (m = z - p / 3, z^3 + P z + Q: Cardano's cube roots for Q^2 / 4 + P^3 / 27 > 0, the cosine form otherwise), two
        Newton steps on the resolvent;  s = sqrt(2 m);  the two quadratics  y^2 - s y + (p / 2 + m + q / (2 s))  and
        y^2 + s y + (p / 2 + m - q / (2 s));  root index 0, 1: the first one's roots with + and - the square root of its discriminant, 2, 3:
        the second one's; a negative discriminant: no such roots.  Each root v: two Newton steps on the normalised quartic, then
        u = N(v) / D(v), s_1 = sqrt(b2 / (1 + v^2 - 2 v cb)), s_2 = u s_1, s_3 = v s_1, and two Newton steps (3 x 3, Cramer's rule) on
        the law-of-cosines system  s_2^2 + s_3^2 - 2 s_2 s_3 ca = a2,  s_1^2 + s_3^2 - 2 s_1 s_3 cb = b2,  s_1^2 + s_2^2 - 2 s_1 s_2 cg = c2
        itself: near a double root of the quartic the ratio N / D and the quartic's own polish lose digits that the system still holds.
      [R | t] (world -> camera) from two orthonormal triads: Y_i = s_i f_i; e_1 = unit(Y_2 - Y_1), e_3 = unit(e_1 x (Y_3 - Y_1)),
      e_2 = e_3 x e_1; g_1, g_2, g_3 likewise from X_1, X_2, X_3; R = e_1 g_1^T + e_2 g_2^T + e_3 g_3^T, t = Y_1 - R X_1.
      A candidate is discarded if a number in it is not finite, if one of s_1, s_2, s_3 is <= 0, if a triad has no normal -- the three
      points collinear or coincident to rounding, |e_1 x (Y_3 - Y_1)|^2 <= 1e-24 |Y_3 - Y_1|^2, likewise for X: what is left of such a
      normal is rounding noise, and a pose that merely turns about the points' line reprojects all three -- or if one of its own three
      edges has depth <= 0 or omega |r|^2 > chi2_max[dim] at [R | t] (r with 2 or 3 components, the edge's own): badly conditioned roots
      go this way.
   4. Score (MSAC): C = sum over ALL usable edges of min(omega |r_e|^2, chi2_max[dim_e]); an edge of depth <= 0 or with a chi2 that is not
      finite counts chi2_max[dim_e].
   5. Winner: the candidate of smallest C, a tie to the smaller 4 h + root.  None at all: NO_SOLUTION.  Fewer than max(4, min_inliers)
      usable edges with depth > 0 and omega |r|^2 <= chi2_max at the winner (the classification, at the winner's [R | t]): FEW_INLIERS.
      Otherwise OK: the winner's pose replaces the estimate, as a quaternion (Shepperd) normalised with w >= 0 and written once as the
      library's scalar type (dry_run != 0: nothing is written).
   Per pose, the first rule that applies: NOT_SELECTED (select given and select[p] == 0), FIXED, FEW_OBSERVATIONS, NO_SOLUTION,
   FEW_INLIERS, OK.  hypotheses 1 ... 4096; chi2_max = {monocular, stereo}, both finite and > 0 (the score needs them); min_inliers >= 0.
   select[Pt], status[Pt], inliers[Pt], cost[Pt], winner[Pt], q[4 Pt] (x, y, z, w), t[3 Pt]: the caller's pose numbering;
   edge_inlier[E]: the caller's edge order.  Every array argument but chi2_max is optional (NULL).
     q, t           the pose of every OK pose as the estimate holds it (also in a dry run), the unchanged current pose of every other
     winner[p]      4 h + root of an OK pose, -1 of every other
     inliers[p]     the classification's count at the winner (OK, FEW_INLIERS); the usable edges (FEW_OBSERVATIONS, NO_SOLUTION); 0 for a
                    pose that is not selected or fixed
     cost[p]        C of the winner (OK, FEW_INLIERS); 0 for every other pose
     edge_inlier[e] the classification at the winner for the edges of OK and FEW_INLIERS poses; for every other edge whether its live omega > 0
     counts[CUBA_HIP_POSELOC_STATUSES]   poses per status; they sum to Pt
   Landmarks, other poses, the gate, the snapshot slots, the handle's LM state and the counters stay as they are; a covariance computed
   before is dropped when a pose changed.  A handle that never calls this allocates and launches nothing for it.
   CUBA_HIP_ERR_INVALID_ARGUMENT: a count outside its range, chi2_max NULL, not finite or not positive.
   CUBA_HIP_ERR_STATE before cuba_hip_set_graph and on a landmark-partitioned handle. */
enum { CUBA_HIP_POSELOC_OK = 0, CUBA_HIP_POSELOC_NOT_SELECTED, CUBA_HIP_POSELOC_FIXED, CUBA_HIP_POSELOC_FEW_OBSERVATIONS,
       CUBA_HIP_POSELOC_NO_SOLUTION, CUBA_HIP_POSELOC_FEW_INLIERS, CUBA_HIP_POSELOC_STATUSES };
int cuba_hip_localize_poses(cuba_hip_solver* s, const uint8_t* select, int hypotheses, uint64_t seed, const double chi2_max[2], int min_inliers,
	int dry_run, int32_t* status, int64_t counts[CUBA_HIP_POSELOC_STATUSES], int32_t* inliers, double* cost, int32_t* winner, double* q, double* t,
	uint8_t* edge_inlier);

/* Replaces: CudaBlockSolver::getTimeProfile (:545-562). Seconds per bucket. */
int cuba_hip_get_profile(cuba_hip_solver* s, double seconds[CUBA_HIP_PROFILE_ITEMS]);

/* Counters of the last optimize / solve: [0] PCG iterations (total), [1] LM trials (total),
   [2] number of 6x6 blocks in upper-triangular Hsc, [3] number of Schur block products (nmul),
   [4] coarse-inverse refreshes of the two-level preconditioner, [5] host looks at the device stop flag,
   [6] PCG iterations enqueued (>= [0]: launches after convergence return at once), [7] dimension of the coarse
   system of the two-level preconditioner. */
int cuba_hip_get_counters(cuba_hip_solver* s, int64_t counters[8]);
/* One counter by name (totals since cuba_hip_set_graph): the eight above as "pcg_iterations", "lm_trials", "coarse_refreshes",
   "pcg_host_looks", "pcg_iterations_enqueued", plus "coarse_inline_inversions" (coarse inversions that ran on the work stream in front
   of a solve -- the others ran on the second stream under an earlier trial's PCG), "pcg_unconverged_solves",
   "pcg_graph_instantiations" (hipGraphs of PCG iteration batches built), "precond_fp32_fallbacks" (solves repeated with the fp64
   coarse inverse after the fp32-stored one broke the PCG down), "exact_solve_fallbacks" (reduced solves that went to the exact
   solver, see "direct_fallback"; 0 on well-conditioned graphs), "exact_solve_failures" (of these, the ones that met a non-positive pivot), "host_looks" (times the host waited for a device report:
   PCG batches + the LM decisions it had to see), "pcg_iterations_plain_launches" (iterations enqueued as plain launches although graphs
   are on: graph not instantiated yet), "batch_full_trials" / "batch_iteration_trials" (on handles[0] of cuba_hip_optimize_batch calls:
   rounds of LM trials it issued with every launch of the trial batched / with the PCG iterations batched only; a call that fell back
   to one handle after the other counts in neither), "graph_uploads" (successful cuba_hip_set_graph[_begin] calls in the
   life of the handle, never reset: a caller that keeps state about "what the device holds" -- the promises of cuba_hip_hint_unchanged --
   stores this number with it and distrusts its state when the two differ), "value_bytes_uploaded" (bytes of measurements and
   information that crossed PCIe in the life of the handle: 32 per edge and full upload, 36 per OWNED edge for cuba_hip_set_graph_partition),
   "edge_sorts" (edge sorts run in the life of the handle, on the host or on the device: one per upload that could not keep the previous
   sort, one more whenever the library changes its internal pose or landmark order on a live graph; like "structure_builds" it shows
   what an upload reused),
   "late_decision_records" (life of the handle: LM decision records that had not reached host memory when the report behind them had, and
   were fetched by a stream synchronisation instead; 0 in normal operation).
   Unknown name: CUBA_HIP_ERR_INVALID_ARGUMENT. */
int cuba_hip_get_counter(cuba_hip_solver* s, const char* name, int64_t* value);

/* PCG iteration count of every reduced solve since cuba_hip_set_graph, oldest first (at most `capacity` are written,
   *n_solves receives their number); a NEGATIVE entry is a solve that stopped at pcg_max_iter with the stop test
   unsatisfied, *n_unconverged counts those.  Such a solve is reported as a failure (*ok = 0 from
   cuba_hip_solve_reduced / cuba_hip_solve; cuba_hip_optimize rejects the trial and raises lambda) -- the role of
   the reference's "factorize failed" path, src/cuda_linear_solver.cpp:406-410 -- unless the option
   "pcg_accept_unconverged" = 1 asks for the best iterate to be used as an inexact step, or -- the default, "direct_fallback" = 1 --
   the exact solver takes the solve over (the entry then records the iterations the PCG had used; solves that went to the exact solver
   straight away are recorded as 0). */
int cuba_hip_get_pcg_history(cuba_hip_solver* s, int32_t* iterations, int capacity, int* n_solves, int64_t* n_unconverged);

/* ---- marginal covariances ------------------------------------------------------------------------ */

/* Marginal covariances at the handle's CURRENT estimate -- the capability of g2o's SparseOptimizer::computeMarginals (Ceres:
   Covariance); the reference has no counterpart.  The covariance is the inverse of the UNDAMPED Gauss-Newton Hessian, the matrix the LM
   loop factorises with lambda = 0: robust weights rho'(e) omega as in constructQuadraticForm (no rho'' term), fixed vertices eliminated.
   With S = Hpp - Hpl Hll^-1 Hlp the reduced matrix:
     pose marginal      the 6 x 6 diagonal block of S^-1, in the tangent coordinates [omega, upsilon] of the solver's own pose update
                        (the left-multiplicative se3 exponential of the reference's update, src/cuda_block_solver.cu:551-579);
     landmark marginal  Hll^-1 + Hll^-1 (sum_{p,q in obs(l)} W_pl^T S^-1_pq W_ql) Hll^-1, W_pl the 6 x 3 block of Hpl;
     cross blocks       S^-1_pq for every block (p, q) of the reduced matrix's upper-triangular pattern (cuba_hip_get_covariance_blocks);
     fixed poses / fixed landmarks: zero blocks.
   S is factorised with the exact reduced solver's ordering and inverted on the factor's pattern only (selected inversion): a second
   copy of the factor's tiles in device memory.  pose_cov [36 Pt], landmark_cov [9 Lt]: column-major blocks in the caller's numbering;
   NULL skips that output (a NULL landmark_cov skips the landmark pass).  A non-positive pivot returns CUBA_HIP_OK with
   *not_positive_definite = 1 and the outputs untouched.  The call changes nothing the LM path sees: a later cuba_hip_optimize runs bit for
   bit as if it had not happened.  Refusals (the handle stays usable): the fp32 library CUBA_HIP_ERR_INVALID_ARGUMENT (an fp32 inverse of a
   bundle-adjustment Hessian is not meaningful); a landmark-partitioned handle or no graph yet CUBA_HIP_ERR_STATE; a factor beyond
   "direct_max_tiles" or beyond free device memory CUBA_HIP_ERR_RUNTIME. */
int cuba_hip_compute_covariance(cuba_hip_solver* s, double* pose_cov, double* landmark_cov, int* not_positive_definite);
/* The cross blocks of the last cuba_hip_compute_covariance (g2o's computeMarginals block set), values[36 nblk], in the layout and
   numbering of cuba_hip_get_hsc_structure.  CUBA_HIP_ERR_STATE before a successful computation and after cuba_hip_set_graph. */
int cuba_hip_get_covariance_blocks(cuba_hip_solver* s, double* values);
/* Covariance blocks of ARBITRARY vertex pairs (g2o's computeMarginals with any block list): pair k is (kind_a[k], index_a[k]) against
   (kind_b[k], index_b[k]), kinds CUBA_HIP_VERTEX_POSE / CUBA_HIP_VERTEX_LANDMARK, indices in the caller's numbering; any two vertices, not
   only co-visible ones (the drift of the last pose against the first, loop-closure gating, pose-landmark and landmark-landmark terms).
   out[36 n]: pair k's dim(a) x dim(b) block of the inverse of the undamped Hessian (the matrix cuba_hip_compute_covariance inverts), rows
   from a, columns from b, column-major with leading dimension dim(a) (6 for a pose, 3 for a landmark); the rest of the 36 numbers is zero.
   A fixed vertex on either side gives a zero block.  The call is self-contained: it linearises at lambda = 0, factorises the reduced
   matrix S with the exact solver's plan and solves S X = C for the right-hand sides of the right vertices, on the elimination-tree paths
   the request touches only; it needs no earlier cuba_hip_compute_covariance.  The side with fewer distinct vertices
   is solved for (pose 0 against every pose: one right-hand-side block) and the blocks are transposed back.  Right-hand sides go in chunks
   sized against free device memory (option "covariance_workspace_mb" caps a chunk; 0 = automatic); a workspace above 64 MiB is freed at
   the end of the call.  A non-positive pivot returns CUBA_HIP_OK
   with *not_positive_definite = 1 and out untouched.  A later cuba_hip_optimize runs bit for bit as if the call had not happened.
   Refusals (the handle stays usable): those of cuba_hip_compute_covariance, a chunk of one block that does not fit
   CUBA_HIP_ERR_RUNTIME, and a bad kind or an index out of range CUBA_HIP_ERR_INVALID_ARGUMENT (checked before any device work).
   Counters "covariance_pairs_ns": the last call's time, "covariance_pairs_chunks": the chunks it ran in. */
int cuba_hip_compute_covariance_pairs(cuba_hip_solver* s, int n, const int32_t* kind_a, const int32_t* index_a, const int32_t* kind_b,
	const int32_t* index_b, double* out, int* not_positive_definite);

/* ---- SE(3) pose priors (g2o's unary pose edges; the reference has no counterpart) --------------------------------------------------
   A prior names pose `pose` (the caller's solver numbering, 0 <= pose < Pt), a prior pose Tbar = (q, t) (world -> camera, quaternion
   (x, y, z, w), normalised by the library) and a 6 x 6 information matrix Omega (symmetric, column-major, in the [omega, upsilon] order of
   the pose update T <- exp(d) T -- the tangent cuba_hip_compute_covariance reports in, so that Sigma^-1 of one window is a prior of the next).
     residual     r = log(T Tbar^-1) = [w ; V(w)^-1 (t - R Rbar^T tbar)], w = log(R Rbar^T)
     objective    r^T Omega r, or rho(r^T Omega r) under a robust kernel (cuba_hip_set_pose_factor_robust_kernels below); the LM objective F
                  (cuba_hip_optimize's chi2, cuba_hip_compute_errors, the gain ratio) is the robust edge sum plus the prior sum
     linearised   with J = J_l(r)^-1, the inverse left Jacobian of SE(3): Hpp += J^T Omega J, bp += -J^T Omega r (the convention
                  (H + lambda I) x = b of the rest of the ABI); in the reduced system the same terms land in the pose's diagonal block and in
                  bsc, and the maximum diagonal of lambda_0 = tau max diag(H) includes them.
   Several priors on one pose are summed in the caller's order; priors on fixed poses are accepted and ignored (chi2 0).  Every solve
   path honours them: the device-decision loop, the host loop (option "profile", graphs without free landmarks), both PCG forms, the exact
   solver, the fp32 library, mixed precision, the covariances (a prior makes a graph without a fixed pose invertible).
   cuba_hip_set_pose_priors replaces the whole set (n = 0 clears it): q[4 n], t[3 n], info[36 n].  Valid any time after cuba_hip_set_graph,
   which clears the set.  Non-finite values, an information matrix that is not symmetric (beyond 1e-9 of its largest entry; within it the
   two triangles are averaged) or a pose out of range: CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged.  Refused with
   CUBA_HIP_ERR_STATE: a landmark-partitioned handle (and cuba_hip_set_partition on a handle with priors, hence the multi-GPU driver) and a
   graph without edges.  Setting priors drops the run-to-run memories of option "heuristics" as a new graph does.  A handle with priors
   takes part in cuba_hip_optimize_batch through the path that batches the PCG iterations only (results stay bit-identical to solo runs).
   cuba_hip_prior_chi_squares: r^T Omega r of every prior at the current estimate, in the caller's order (to gate bad GPS or relocalisation
   priors, as cuba_hip_chi_squares serves for edges). */
int cuba_hip_set_pose_priors(cuba_hip_solver* s, int n, const int32_t* pose, const double* q, const double* t, const double* info);
int cuba_hip_prior_chi_squares(cuba_hip_solver* s, double* chi2_per_prior);

/* ---- SE(3) relative-pose edges (g2o's binary SE(3) edge: odometry, loop closures; the reference has no counterpart) ------------------
   An edge names two DIFFERENT poses i, j (the caller's solver numbering, 0 <= i, j < Pt), a measured relative pose Zbar = (q, t) of
   T_j T_i^-1 (world -> camera poses, so Zbar maps camera-i coordinates to camera-j coordinates; quaternion (x, y, z, w), normalised by the
   library) and a 6 x 6 information matrix Omega (symmetric, column-major, [omega, upsilon] order of the pose update T <- exp(d) T, the
   tangent cuba_hip_compute_covariance reports in).
     residual     r = log(T_j T_i^-1 Zbar^-1)
     objective    r^T Omega r, or rho(r^T Omega r) under a robust kernel (cuba_hip_set_pose_factor_robust_kernels below); the LM objective F
                  (cuba_hip_optimize's chi2, cuba_hip_compute_errors, the gain ratio) is the robust edge sum plus the prior sum plus the
                  relative-pose sum
     linearised   exactly under the solver's update: with M = T_j T_i^-1 = [R_M | t_M] and Ad(M) = [[R_M, 0], [[t_M]x R_M, R_M]],
                  J_j = dr/dd_j = J_l(r)^-1 and J_i = dr/dd_i = -J_l(r)^-1 Ad(M).  Hpp_ii += J_i^T Omega J_i, Hpp_jj += J_j^T Omega J_j,
                  Hpp_ij += J_i^T Omega J_j, bp_i += -J_i^T Omega r, bp_j += -J_j^T Omega r; the same terms in the reduced system (Hsc, bsc);
                  the maximum diagonal of lambda_0 includes them.
   Unlike a prior, an edge between two free poses owns an off-diagonal block of the reduced system: the set of distinct free-free pairs is
   part of the topology.  The structure is rebuilt (lazily, at the next call that needs it) exactly when that set differs from the one the
   current structure was built with -- new values on the same pairs, or cuba_hip_set_graph on an unchanged topology followed by the same
   pairs, keep it; cuba_hip_get_counter "structure_builds" counts the builds.
   With one end fixed the edge acts on the free end only (it equals a prior Zbar T_i on pose j); with both fixed it is accepted and
   ignored (chi2 0).  Several edges on one pair are summed in the caller's order.  A free pose held by relative-pose edges alone is legal.
   Every solve path honours the edges: the device-decision loop, the host loop, both PCG forms, the exact solver, the fp32 library, mixed
   precision, the covariances (a pair is a block of Hsc, so cuba_hip_get_covariance_blocks reports it).
   cuba_hip_set_relative_pose_edges replaces the whole set (n = 0 clears it): pose_i[n], pose_j[n], q[4 n], t[3 n], info[36 n].  Valid any
   time after cuba_hip_set_graph, which clears the set.  i == j, an index out of range, non-finite values or an information matrix that is
   not symmetric (beyond 1e-9 of its largest entry; within it the two triangles are averaged): CUBA_HIP_ERR_INVALID_ARGUMENT, the handle
   unchanged.  Refused with CUBA_HIP_ERR_STATE, the handle staying usable: a landmark-partitioned handle (and cuba_hip_set_partition on a
   handle with such edges, hence the multi-GPU driver) and a graph without reprojection edges.  Setting the edges drops the run-to-run
   memories of option "heuristics" as a new graph does.  A handle with such edges takes part in cuba_hip_optimize_batch through the path
   that batches the PCG iterations only (results stay bit-identical to solo runs).
   cuba_hip_relative_pose_chi_squares: r^T Omega r of every edge at the current estimate, in the caller's order (to gate loop closures). */
int cuba_hip_set_relative_pose_edges(cuba_hip_solver* s, int n, const int32_t* pose_i, const int32_t* pose_j, const double* q, const double* t,
	const double* info);
int cuba_hip_relative_pose_chi_squares(cuba_hip_solver* s, double* chi2_per_edge);

/* ---- robust kernels on the pose factors (g2o's setRobustKernel on those edges) -------------------------------------------------------
   Every pose prior (factor_type 0) and every relative-pose edge (factor_type 1) may carry a kernel (kind, delta) of its own.  With
   e = r^T Omega r, residual and Omega as above:
     objective    rho(e) in place of e: in the LM objective F, cuba_hip_compute_errors and the gain ratio
     linearised   with w Omega in place of Omega, w = rho'(e), in every term of the factor (J^T Omega J, the cross block, J^T Omega r into bp /
                  bsc); no second-order term -- the convention of the reprojection edges' kernels, and g2o's.  lambda_0 sees the weighted terms.
     kind 0  none     rho = e                                                               w = 1
          1  Huber    rho = e (e <= delta^2), 2 delta sqrt(e) - delta^2 beyond              w = 1, delta / sqrt(e)
          2  Tukey    rho = delta^2 / 3 (1 - (1 - e / delta^2)^3), delta^2 / 3 beyond       w = (1 - e / delta^2)^2, 0
          3  Cauchy   rho = delta^2 log1p(e / delta^2)                                      w = 1 / (1 + e / delta^2)
   (Cauchy exists for the pose factors only: cuba_hip_set_robust_kernel refuses kind 3.)
   kind[n], delta[n] are in the caller's order of the CURRENT set of that type; n is that set's count, or 0, which clears the kernels of the
   type.  The kernels belong to the set: cuba_hip_set_pose_priors / cuba_hip_set_relative_pose_edges (the replaced set is a new set) and
   cuba_hip_set_graph drop them.  Setting kernels never rebuilds the structure ("structure_builds" stays); it drops the run-to-run memories
   of option "heuristics" and invalidates cached covariance blocks, as a change of the factors' values does.  A handle that never sets a
   kernel (or sets kinds all 0) runs exactly the code and computes exactly the bits of a library without this entry point.
   Every solve path honours the kernels (those listed above, cuba_hip_optimize_batch included).  The covariance entry points report the
   inverse of the WEIGHTED Hessian at the current estimate: a factor that Tukey has given weight 0 contributes nothing, so a graph that
   depended on it for its gauge reports not_positive_definite.
   cuba_hip_prior_chi_squares / cuba_hip_relative_pose_chi_squares keep returning the plain r^T Omega r (what a caller gates on; w follows).
   CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged: n neither 0 nor the set's count, factor_type outside {0, 1}, a kind outside 0..3, a
   non-finite delta, delta <= 0 on a kind != 0. */
int cuba_hip_set_pose_factor_robust_kernels(cuba_hip_solver* s, int factor_type /* 0 priors, 1 relative-pose edges */, int n, const int32_t* kind,
	const double* delta);

/* ---- landmark position priors (g2o's unary XYZ prior edge; the reference has no counterpart) -----------------------------------------
   A prior names landmark `landmark` (the caller's solver numbering, 0 <= landmark < Lt), a position Xbar and a 3 x 3 information matrix
   Omega (symmetric, column-major), and optionally a robust kernel (kind, delta) of the pose factors' family (table above: 0 none, 1 Huber,
   2 Tukey, 3 Cauchy, the same formulas): surveyed ground-control points, points of a map of finite certainty, range-sensor points, the
   landmark half of a previous window's marginal, a weak depth prior on a landmark seen under almost no parallax.
     residual     r = X - Xbar, e = r^T Omega r
     objective    rho(e); the LM objective F (cuba_hip_optimize's chi2, cuba_hip_compute_errors, the gain ratio) is the robust edge sum plus
                  the pose factors' sums plus the landmark priors' sum
     linearised   with w = rho'(e) and the identity for a Jacobian: Hll += w Omega, bl += -w Omega r (the convention (H + lambda I) x = b
                  of the rest of the ABI: bl is minus half the gradient); no second-order term.  Both enter before the
                  damping and the 3 x 3 inverse, so the Schur complement, bsc, back-substitution, lambda_0's maximum diagonal, the gain
                  ratio's scale and the covariances see them without a term of their own (a graph without a fixed vertex that three such
                  priors hold is invertible).
   Several priors on one landmark are summed behind its edges, in the caller's order; priors on fixed landmarks are accepted and ignored
   (chi2 0).  Every solve path honours them: the device-decision loop, the host loop, both PCG forms, the exact solver, the fp32 library,
   mixed precision.  cuba_hip_set_landmark_priors replaces the whole set (n = 0 clears it): landmark[n], xyz[3 n], info[9 n], kind[n] and
   delta[n] (both NULL: no kernels).  Valid any time after cuba_hip_set_graph, which clears the set.  Setting priors never rebuilds the
   structure ("structure_builds" stays); it drops the run-to-run memories of option "heuristics" and cached covariance blocks.
   CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged: an index out of range, non-finite values, an information matrix that is not
   symmetric (beyond 1e-9 of its largest entry; within it the two triangles are averaged), a kind outside 0..3, delta <= 0 on a kind != 0,
   one of kind / delta without the other.  A prior on a FREE landmark that no reprojection edge observes is refused too (such a landmark is
   not part of the linearisation): the internal landmark order must be known to tell, so the first call that needs the set on the device
   reports CUBA_HIP_ERR_INVALID_ARGUMENT; the handle stays usable and the set is dropped.
   CUBA_HIP_ERR_STATE, the handle staying usable: a landmark-partitioned handle (and cuba_hip_set_partition on a handle with such priors,
   hence the multi-GPU driver) and a graph without edges.  A handle with such priors takes part in cuba_hip_optimize_batch through the
   path that batches the PCG iterations only (results stay bit-identical to solo runs).  A handle without them launches the kernels, with
   the arguments, of a library without this entry point.
   cuba_hip_landmark_prior_chi_squares: the plain r^T Omega r of every prior at the current estimate, in the caller's order (what a caller
   gates a doubtful control point on). */
int cuba_hip_set_landmark_priors(cuba_hip_solver* s, int n, const int32_t* landmark, const double* xyz, const double* info, const int32_t* kind,
	const double* delta);
int cuba_hip_landmark_prior_chi_squares(cuba_hip_solver* s, double* chi2_per_prior);

/* ---- position factors on the poses (GNSS-style fixes with a lever arm; the reference has no counterpart) -----------------------------
   A factor names pose `pose` (the caller's solver numbering, 0 <= pose < Pt; world -> camera T = [R | t]), a measured world position z,
   a lever arm a -- the measured point in the camera frame, zero for the camera centre --, a 3 x 3 information matrix Omega (symmetric,
   column-major) and optionally a robust kernel (kind, delta) of the pose factors' family (table above: 0 none, 1 Huber, 2 Tukey,
   3 Cauchy, the same formulas): a GNSS fix of the antenna, a total-station prism, a mocap marker, a UWB position.  An SE(3) prior cannot
   say this even with zero information on its rotation rows: the translation part of log(T Tbar^-1) depends on a prior rotation that a
   position fix does not supply.
     residual     r = R^T (a - t) - z, e = r^T Omega r
     objective    rho(e); the LM objective F (cuba_hip_optimize's chi2, cuba_hip_compute_errors, the gain ratio) gains the factors' sum
     linearised   with w = rho'(e) and dr/dd = [R^T [a]x | -R^T] (3 x 6, d = [omega; upsilon] of the update T <- exp(d) T; exact to first
                  order, r lives in a vector space): w J^T Omega J into the pose's diagonal block of the reduced matrix, -w J^T Omega r into
                  bp and bsc; no second-order term.  lambda is added afterwards as to everything else; the assemble-only pass adds the terms
                  too, so lambda_0's maximum diagonal includes them.  The terms follow the pose priors' and precede the relative-pose
                  edges' in every sum.
   Several factors on one pose are summed in the caller's order; factors on fixed poses are accepted and ignored (chi2 0).  Every solve
   path honours them: the device-decision loop (a rejected trial's restore included), the host loop, both PCG forms, the exact solver,
   the fp32 library, mixed precision, and the covariance entry points (the inverse of the weighted Hessian: three such factors give a
   graph without a fixed vertex its gauge, and a monocular one its scale).
   The fp32 library computes R^T (a - t) - z in fp32 and the library shifts nothing: callers with UTM-size coordinates subtract a local
   origin from the poses, the landmarks and z first.
   cuba_hip_set_position_factors replaces the whole set (n = 0 clears it): pose[n], position[3 n], lever_arm[3 n] (NULL: zeros), info[9 n],
   kind[n] and delta[n] (both NULL: no kernels; kinds all 0 are no kernels).  Valid any time after cuba_hip_set_graph, which clears the
   set.  Setting factors never rebuilds the structure ("structure_builds" stays); it drops the run-to-run memories of option "heuristics"
   and cached covariance blocks.
   CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged: an index out of range, non-finite values, an information matrix that is not
   symmetric (beyond 1e-9 of its largest entry; within it the two triangles are averaged), a kind outside 0..3, delta <= 0 on a kind != 0,
   one of kind / delta without the other.
   CUBA_HIP_ERR_STATE, the handle staying usable: a landmark-partitioned handle (and cuba_hip_set_partition on a handle with such factors,
   hence the multi-GPU driver) and a graph without edges.  A handle with such factors takes part in cuba_hip_optimize_batch through the
   path that batches the PCG iterations only (results stay bit-identical to solo runs).  A handle without them launches the kernels, with
   the arguments, of a library without this entry point.
   cuba_hip_position_factor_chi_squares: the plain r^T Omega r of every factor at the current estimate, in the caller's order (what a
   caller gates a doubtful fix on). */
int cuba_hip_set_position_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* position, const double* lever_arm, const double* info,
	const int32_t* kind, const double* delta);
int cuba_hip_position_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor);

/* ---- direction factors on the poses (gravity, compass, vanishing directions; the reference has no counterpart) ------------------------
   A factor names pose `pose` (the caller's solver numbering, 0 <= pose < Pt; world -> camera T = [R | t]), a world vector d, the same
   vector as measured in the camera frame, m, a 3 x 3 information matrix Omega (symmetric, column-major) and optionally a robust kernel
   (kind, delta) of the pose factors' family (table above: 0 none, 1 Huber, 2 Tukey, 3 Cauchy, the same formulas): the gravity vector of
   an accelerometer (roll and pitch, no yaw), a magnetometer or sun-sensor bearing, the vanishing direction of a Manhattan world, one star
   of a star tracker.  An SE(3) prior cannot say this: it needs a whole prior rotation Rbar, and information that nulls the rotation about
   Rbar d is exact only for a pure rotation about that axis.
     residual     r = R d - m, e = r^T Omega r.  d and m are taken as given and are NOT normalised: unit vectors are the usual case, gravity
                  in m/s^2 against a specific-force reading is another.  Omega = (I - m m^T) / sigma^2 (rank 2) is the usual information;
                  full rank and all-zero information are valid too.
     objective    rho(e); the LM objective F (cuba_hip_optimize's chi2, cuba_hip_compute_errors, the gain ratio) gains the factors' sum
     linearised   with w = rho'(e) and dr/dd = [-[R d]x | 0] (3 x 6, d = [omega; upsilon] of the update T <- exp(d) T: R' = (I + [omega]x) R,
                  so r' = r + omega x (R d); r lives in a vector space and needs no J_l; the translation columns are exactly zero).  With
                  v = R d: w [v]x^T Omega [v]x into the rotation 3 x 3 of the pose's diagonal block of the reduced matrix, -w v x (Omega r)
                  into the first three entries of the pose's bp and bsc; no second-order term.  The rest of the block and bp[3..6) are not
                  touched.  lambda is added afterwards as to everything else; the assemble-only pass adds the terms too, so lambda_0's
                  maximum diagonal includes them.  The terms follow those of every other kind in every sum.
   Several factors on one pose are summed in the caller's order; factors on fixed poses are accepted and ignored (chi2 0).  Every solve
   path honours them: the device-decision loop (a rejected trial's restore included), the host loop, both PCG forms, the exact solver,
   the fp32 library, mixed precision, and the covariance entry points (the inverse of the weighted Hessian: with position fixes on two
   poses, one direction factor off their line gives a graph without a fixed vertex its gauge).
   cuba_hip_set_direction_factors replaces the whole set (n = 0 clears it): pose[n], world_dir[3 n], measured_dir[3 n], info[9 n], kind[n]
   and delta[n] (both NULL: no kernels; kinds all 0 are no kernels).  Valid any time after cuba_hip_set_graph, which clears the set.
   Setting factors never rebuilds the structure ("structure_builds" stays); it drops the run-to-run memories of option "heuristics" and
   cached covariance blocks.
   CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged: an index out of range, non-finite values, an information matrix that is not
   symmetric (beyond 1e-9 of its largest entry; within it the two triangles are averaged), a kind outside 0..3, delta <= 0 on a kind != 0,
   one of kind / delta without the other.
   CUBA_HIP_ERR_STATE, the handle staying usable: a landmark-partitioned handle (and cuba_hip_set_partition on a handle with such factors,
   hence the multi-GPU driver) and a graph without edges.  A handle with such factors takes part in cuba_hip_optimize_batch through the
   path that batches the PCG iterations only (results stay bit-identical to solo runs).  A handle without them launches the kernels, with
   the arguments, of a library without this entry point.
   cuba_hip_direction_factor_chi_squares: the plain r^T Omega r of every factor at the current estimate, in the caller's order (what a
   caller gates a doubtful reading on). */
int cuba_hip_set_direction_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* world_dir, const double* measured_dir, const double* info,
	const int32_t* kind, const double* delta);
int cuba_hip_direction_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor);

/* ---- range factors on the poses (UWB-style distances to known anchors; the reference has no counterpart) ------------------------------
   A factor names pose `pose` (the caller's solver numbering, 0 <= pose < Pt; world -> camera T = [R | t]), an anchor b (a known world
   point), a measured range rbar >= 0, a lever arm a -- the ranging antenna in the camera frame, zero for the camera centre --, a scalar
   information Omega = 1 / sigma^2 >= 0 and optionally a robust kernel (kind, delta) of the pose factors' family (table above: 0 none,
   1 Huber, 2 Tukey, 3 Cauchy, the same formulas): a UWB anchor, an acoustic beacon, DME, a total station that reports slope distance
   only.  One range constrains the pose to a sphere: a position factor cannot say this (it needs a 3-D fix, and rank-1 information on it
   is a plane), nor can an SE(3) prior.
     residual     u = a - (R b + t) (camera frame; |u| = |R^T (a - t) - b|), rho = |u|, m = u / rho, r = rho - rbar, e = Omega r^2
     objective    rho_k(e); the LM objective F (cuba_hip_optimize's chi2, cuba_hip_compute_errors, the gain ratio) gains the factors' sum
     linearised   with w = rho_k'(e) and dr/dd = J = [(m x a)^T | -m^T] (1 x 6, d = [omega; upsilon] of the update T <- exp(d) T: b_c = R b + t
                  becomes b_c + omega x b_c + upsilon, so d rho = -m . (omega x b_c + upsilon), and b_c x m = a x m): w Omega J^T J (rank 1)
                  into the pose's diagonal block of the reduced matrix, -w Omega r J^T into bp and bsc; no second-order term.  lambda is
                  added afterwards as to everything else; the assemble-only pass adds the terms too, so lambda_0's maximum diagonal
                  includes them.  The terms follow those of every other kind in every sum.
     rho = 0      (the antenna at the anchor) m is undefined there.  The rule: when the computed rho is exactly 0, m = 0, so J = 0: the
                  factor adds nothing to the system and contributes e = Omega rbar^2.
   Several factors on one pose are summed in the caller's order; factors on fixed poses are accepted and ignored (chi2 0).  Every solve
   path honours them: the device-decision loop (a rejected trial's restore included), the host loop, both PCG forms, the exact solver,
   the fp32 library, mixed precision, and the covariance entry points (the inverse of the weighted Hessian: four non-coplanar anchors
   heard from three poses off a line give a graph without a fixed vertex its gauge, and a monocular one its scale).
   The fp32 library computes a - t - R b in fp32 and the library shifts nothing: callers with UTM-size coordinates subtract a local
   origin from the poses, the landmarks and the anchors first.
   cuba_hip_set_range_factors replaces the whole set (n = 0 clears it): pose[n], anchor[3 n], range[n], lever_arm[3 n] (NULL: zeros),
   info[n], kind[n] and delta[n] (both NULL: no kernels; kinds all 0 are no kernels).  Valid any time after cuba_hip_set_graph, which
   clears the set.  Setting factors never rebuilds the structure ("structure_builds" stays); it drops the run-to-run memories of option
   "heuristics" and cached covariance blocks.
   CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged: an index out of range, non-finite values, a negative range, a negative
   information (0 is valid and is no factor), a kind outside 0..3, delta <= 0 on a kind != 0, one of kind / delta without the other.
   CUBA_HIP_ERR_STATE, the handle staying usable: a landmark-partitioned handle (and cuba_hip_set_partition on a handle with such factors,
   hence the multi-GPU driver) and a graph without edges.  A handle with such factors takes part in cuba_hip_optimize_batch through the
   path that batches the PCG iterations only (results stay bit-identical to solo runs).  A handle without them launches the kernels, with
   the arguments, of a library without this entry point.
   cuba_hip_range_factor_chi_squares: the plain Omega r^2 of every factor at the current estimate, in the caller's order (what a caller
   gates a doubtful range -- a non-line-of-sight one -- on). */
int cuba_hip_set_range_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* anchor, const double* range, const double* lever_arm, const double* info,
	const int32_t* kind, const double* delta);
int cuba_hip_range_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor);

/* Range factors between two poses (no counterpart in the reference): the binary counterpart of the range factors
   above.  A factor names poses i != j, a measured distance rbar >= 0 between the point a_i of camera frame i and the point a_j of camera
   frame j (the lever arms: antennas, wheel centres, rig points; zero for the camera centres), a scalar information Omega = 1 / sigma^2
   >= 0 and optionally a robust kernel (kind, delta) of the pose factors' family: the travelled distance of a wheel odometer between two
   keyframes (the scale of a monocular graph, without any orientation), peer-to-peer UWB ranging, the baseline length of a rig whose
   cameras are separate poses, a taped distance between two stations.  A relative-pose edge with a rank-deficient information cannot say
   this: its residual mixes rotation into translation, and a distance is no linear function of it.
     residual     w_i = R_i^T (a_i - t_i) (world), u = a_j - (R_j w_i + t_j) (frame j), rho = |u|, m_j = u / rho, m_i = -R_i R_j^T m_j,
                  r = rho - rbar, e = Omega r^2
     objective    rho_k(e); the LM objective F gains the factors' sum
     linearised   with w = rho_k'(e), J_j = [(m_j x a_j)^T | -m_j^T] and J_i = [(m_i x a_i)^T | -m_i^T] (1 x 6 each: the range factor's
                  Jacobian with the other end's point as the anchor): w Omega J_i^T J_i and w Omega J_j^T J_j (rank 1 each) into the two
                  diagonal blocks of the reduced matrix, w Omega J_i^T J_j into the off-diagonal block of the pair, -w Omega r J^T into bp
                  and bsc; no second-order term.  The terms follow those of every other kind in every sum.
     rho = 0      when the computed rho is exactly 0, m_i = m_j = 0: the factor adds nothing to the system and contributes e = Omega rbar^2.
   Several factors on one pair or pose are summed in the caller's order.  A factor with one fixed end acts on the free end only, as a range
   factor with the fixed end's point as the anchor; one with two fixed ends is accepted and ignored (chi2 0).  The free-free pairs are part
   of the TOPOLOGY, together with the relative-pose edges' (the union of both kinds' pairs): every such pair owns a block of the reduced
   matrix, also where no landmark connects the two poses, and the structure is rebuilt ("structure_builds") exactly when a call changes
   that union; setting or clearing one kind keeps the other's blocks.  Every solve path honours the factors: the device-decision loop, the
   host loop, both PCG forms, the exact solver, the fp32 library and the covariance entry points.
   cuba_hip_set_pose_range_factors replaces the whole set (n = 0 clears it): pose_i[n], pose_j[n], range[n], lever_arm_i[3 n] and
   lever_arm_j[3 n] (either NULL: zeros), info[n], kind[n] and delta[n] (both NULL: no kernels; kinds all 0 are no kernels).  Valid any time
   after cuba_hip_set_graph, which clears the set.  It drops the run-to-run memories of option "heuristics" and cached covariance blocks.
   CUBA_HIP_ERR_INVALID_ARGUMENT, the handle unchanged: an index out of range, i = j, non-finite values, a negative range, a negative
   information (0 is valid and is no factor), a kind outside 0..3, delta <= 0 on a kind != 0, one of kind / delta without the other.
   CUBA_HIP_ERR_STATE, the handle staying usable: a landmark-partitioned handle (and cuba_hip_set_partition on a handle with such factors)
   and a graph without reprojection edges.  A handle without such factors launches the kernels, with the arguments, of a library without
   this entry point.
   cuba_hip_pose_range_factor_chi_squares: the plain Omega r^2 of every factor at the current estimate, in the caller's order. */
int cuba_hip_set_pose_range_factors(cuba_hip_solver* s, int n, const int32_t* pose_i, const int32_t* pose_j, const double* range, const double* lever_arm_i,
	const double* lever_arm_j, const double* info, const int32_t* kind, const double* delta);
int cuba_hip_pose_range_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor);

/* ---- introspection (parity tests) and multi-GPU plumbing ------------------------------------------ */

/* Structure of the reduced system: upper-triangular BSR (replaces the accessors of
   HschurSparseBlockMatrix, src/sparse_block_matrix.h:81-101). row_ptr[Pf+1], col_ind[nblk]. */
int cuba_hip_get_hsc_structure(cuba_hip_solver* s, int32_t* row_ptr, int32_t* col_ind, int* nblk);

/* Copy an internal device array to the host; out may be NULL to query *count only. */
int cuba_hip_get_array(cuba_hip_solver* s, int which, double* out, size_t* count);

/* Measurement hook for bench.py: average device milliseconds per launch, taken with HIP events on the
   handle's stream over `reps` back-to-back launches, of
     [0] residual_chi2  [1] linearize+Schur  [2] pcg_spmv  [3] pcg_update (+restrict)  [4] back_substitute
     [5] reserved (0)
     [6] coarse_setup (assemble + invert the coarse matrix, once per solve; 0 if disabled).
   Clobbers the increments and the reduced system (not the estimates). */
enum { CUBA_HIP_TIMED_KERNELS = 7 };
int cuba_hip_time_kernels(cuba_hip_solver* s, int reps, double ms_per_launch[CUBA_HIP_TIMED_KERNELS]);

/* ---- landmark-partitioned multi-GPU operation (no counterpart in the single-GPU reference) ----------------
   Every rank uploads the WHOLE graph (so all ranks share one Hsc pattern and one pose ordering) and then
   restricts itself to the landmarks [landmark_begin, landmark_end) of the solver order: residuals, Schur
   contributions, back-substitution and landmark updates are evaluated for those landmarks only.
   Per trial the driver sums cuba_hip_reduction_buffer() over the ranks between cuba_hip_schur and
   cuba_hip_solve_reduced; chi2 and the landmark parts of max-diagonal / scale are reduced as scalars. */
/* (landmark_begin, landmark_end) = (0, -1) removes the restriction again. */
int cuba_hip_set_partition(cuba_hip_solver* s, int landmark_begin, int landmark_end);
/* cuba_hip_set_graph and cuba_hip_set_partition in one call, for a rank that knows its range when it uploads: the index arrays and the
   estimates go up whole (the block pattern and the pose order are global), but meas / omega are READ ONLY for the edges whose landmark lies
   in [landmark_begin, landmark_end) -- 36 bytes per owned edge cross PCIe instead of 32 per edge of the graph, i.e. about 1 / N of the
   value arrays on each of N ranks -- and need not hold anything meaningful elsewhere.  The other edges' values read as zeros on the
   device; no stage of a partitioned handle looks at them (cuba_hip_chi_squares reports 0 for them).  Until the next upload the handle
   therefore refuses a cuba_hip_set_partition beyond this range (CUBA_HIP_ERR_STATE; lifting the restriction included) and ignores a
   "same values" promise (cuba_hip_hint_unchanged).  With the option "device_setup" = 0 the whole arrays are read. */
int cuba_hip_set_graph_partition(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf,
	const double* q, const double* t, const double* cam, const double* Xw,
	int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim,
	const double* meas, const double* omega, int landmark_begin, int landmark_end);
/* First half of cuba_hip_max_diagonal: accumulate Hpp (diagonal blocks of the reduction buffer), bp, Hll. */
int cuba_hip_assemble(cuba_hip_solver* s);
/* Second half: max diag of the (externally summed) Hpp and of this rank's Hll. */
int cuba_hip_max_diagonal_parts(cuba_hip_solver* s, double* pose_part, double* landmark_part);
/* sum x (lambda x + b) split into the replicated pose part and this rank's landmark part. */
int cuba_hip_compute_scale_parts(cuba_hip_solver* s, double lambda, double* pose_part, double* landmark_part);
/* Device address of an internal array (ids as for cuba_hip_get_array) for zero-copy collectives. */
int cuba_hip_device_pointer(cuba_hip_solver* s, int which, void** device_ptr, size_t* count);

/* {Pt, Pf, Lt, Lf, E} of the uploaded graph. */
int cuba_hip_get_sizes(cuba_hip_solver* s, int sizes[5]);

/* Test hook for the one dense kernel of the path: the blocked Gauss-Jordan inversion (matrix-core tile products) that builds the
   coarse inverse of the two-level preconditioner.  A, Ainv: n x n, column-major, SPD input.  No solver handle involved. */
int cuba_hip_debug_dense_inverse(int device, int n, const double* A, double* Ainv);

/* Test hooks for the exact reduced solve (csrc/ba_direct.hip: sparse tile Cholesky on the matrix cores + triangular solves), the
   counterpart of SparseLinearSolver::initialize / solve (/root/reference/src/cuda_linear_solver.cpp:278-348, 386-415).  A: n x n
   column-major, symmetric (n a multiple of 6: it is cut into the 6 x 6 blocks of a reduced system; off-diagonal blocks that are
   identically zero are not part of the pattern); x = A^-1 b.  *not_positive_definite != 0 reports a non-positive pivot (ref :406-410).
   slack: multiple-elimination slack of the ordering (-1 = automatic); stats (optional) = {tile columns, tiles, levels, slack used}.
   No solver handle involved.  cuba_hip_debug_dense_solve = the same with slack -1 and no statistics. */
int cuba_hip_debug_dense_solve(int device, int n, const double* A, const double* b, double* x, int* not_positive_definite);
int cuba_hip_debug_sparse_solve(int device, int n, const double* A, const double* b, double* x, int* not_positive_definite, int slack, int32_t stats[4]);
/* Test hook for the selected inversion behind cuba_hip_compute_covariance (csrc/ba_covariance.hip), on the matrix and block pattern
   cuba_hip_debug_sparse_solve takes: fill, factorisation, fail flag, selected inversion and extraction, the calls of the covariance in its
   order.  sigma: n x n column-major, A^-1 on every block of the pattern and its mirror (the diagonal blocks as the pose extraction
   delivers them, the off-diagonal ones as the block extraction does, with their transposes), zero elsewhere.  A matrix that is not
   positive definite: CUBA_HIP_OK, *not_positive_definite = 1, sigma all zero.  The fp32 library: CUBA_HIP_ERR_INVALID_ARGUMENT.
   stats (optional) as above.  No solver handle involved. */
int cuba_hip_debug_selected_inverse(int device, int n, const double* A, double* sigma, int* not_positive_definite, int slack, int32_t stats[4]);
/* The symbolic phase alone, on the host (no device needed): ordering, fill, elimination-tree levels and gather lists for the
   upper-triangular block pattern (row_ptr[n_poses + 1], col_ind; diagonal block first in every row).  which: 0 header {tile columns,
   tiles, levels, slack, gather entries, blocks}, 1 posOfSeg, 2 colPtr, 3 rowIdx, 4 gPtr, 5 gather (4 ints per entry), 6 lvlPtr,
   7 lvlTiles, 8 lvlColPtr, 9 lvlCols, 10 blkTile (see SparseCholPlan in csrc/ba_kernels.hpp); the selected inversion's plan built on
   it (cuba_hip_compute_covariance; SelInvPlan in csrc/ba_kernels.hpp): 11 header {levels, off-diagonal tiles, gather entries, tile
   products low 31 bits, high bits}, 12 stepPtr, 13 offRec (4 ints per tile), 14 colStepPtr, 15 cols, 16 gather (2 ints per entry).
   *count = length of the array; out may be NULL to ask for it.  A malformed pattern (row_ptr[0] != 0, a row without its diagonal block
   first, columns not strictly increasing or not below n_poses) is CUBA_HIP_ERR_INVALID_ARGUMENT. */
int cuba_hip_debug_sparse_plan(int n_poses, const int32_t* row_ptr, const int32_t* col_ind, int slack, int which, int32_t* out, size_t capacity, size_t* count);
/* Test hook for cuba_hip_compute_covariance_pairs' kernels on a given matrix (as cuba_hip_debug_selected_inverse): pair k is the 6 x 6
   block (block_i[k], block_j[k]) of A^-1, column-major into out[36 k], whether or not it lies on the pattern.  Fill, factorisation, fail
   flag, then the pair calls of the handle with every block index read as a free pose.  A matrix that is not positive definite:
   CUBA_HIP_OK, *not_positive_definite = 1, out all zero.  stats (optional) as above.  No solver handle involved. */
int cuba_hip_debug_inverse_blocks(int device, int n, const double* A, int n_pairs, const int32_t* block_i, const int32_t* block_j, double* out,
	int* not_positive_definite, int slack, int32_t stats[4]);
/* The pair solve's symbolic phase alone, on the host (no device needed), for the pattern of cuba_hip_debug_sparse_plan and the pose pairs
   (block_i[k], block_j[k]) as cuba_hip_debug_inverse_blocks packs them, all blocks in one chunk.  which: 0 header {blocks, slots, forward
   records, forward gather entries, backward records, backward gather entries}, 1 pairs (4 ints per pair {block, column of j, 0, 0}),
   2 fwdPtr, 3 fwdCols, 4 bwdPtr, 5 bwdCols, 6 slotPtr, 7 slotCols, 8 fLvlPtr, 9 fRec (4 ints {slot, column, first entry, entries}),
   10 fGather (2 ints {tile, slot}), 11 bLvlPtr, 12 bRec, 13 bGather (PairPlan in csrc/ba_kernels.hpp).  Malformed patterns as for
   cuba_hip_debug_sparse_plan, and block indices outside [0, n_poses), are CUBA_HIP_ERR_INVALID_ARGUMENT. */
int cuba_hip_debug_pair_plan(int n_poses, const int32_t* row_ptr, const int32_t* col_ind, int slack, int n_pairs, const int32_t* block_i,
	const int32_t* block_j, int which, int32_t* out, size_t capacity, size_t* count);

/* Test hook, read-only: the PCG configuration in force after the option rules (aggregate widening, constant coarse functions, the
   block-Jacobi fallback, the automatic upper-triangle rule, the fp64 repeat of a solve that broke down with the fp32-stored coarse inverse).
   cfg = {pcg_aggregate (0 = block-Jacobi only), coarse functions per aggregate and pose component (1 or 2), aggregates, block rows per SpMV
   workgroup (2 or 4), upper-triangle iteration (0 / 1), fixed-width row levels (20 entries each), some row wider than those (0 / 1),
   coarse inverse stored in fp32 (0 / 1), row entries per thread of the upper-triangle row update (2, 4, 8; 0 when that iteration is
   off)}.  pose_order[i] = the caller's index of the i-th free pose in the solver's internal order (aggregates are runs of consecutive
   internal indices); *count = Pf, pose_order may be NULL. */
int cuba_hip_debug_pcg_config(cuba_hip_solver* s, int32_t cfg[9], int32_t* pose_order, size_t capacity, size_t* count);

/* Test hook: the decision kernels of a device-decided run (run start, the sums' second stage with the decision, the decision of a failed
   solve, the conditional restore) on scripted partial sums, with the host's per-record logic beside them.  No solver handle involved.
   start_mode 0: the decision state as the host writes it, from F0 and lam0; 1: formed on the device from chi_slots[16] (F0 = their sum) and
   maxdiag_bits[64] (lam0 = tau * the largest bit pattern read as a double).  Trial t: ok[t] != 0 -> the partial sums a[a_off[t], a_off[t+1])
   (landmark part of the gain ratio's denominator), b (chi2), c (pose part), at most 65536 each; ok[t] == 0 -> a failed solve.  Offsets
   start at 0 and do not decrease.  At most 512 trials and iterations; scratch_count <= 2^20 numbers of scratch estimate and backup for
   the restore.  out_start[10] = the 9 state numbers {F, lambda, nu, halt, trials, accepted, rejections in a row, max rejections, tag
   base} and the damping as the kernels read it.  out[32 t + ..]: 0..8 state, 9..16 the trial's record {Fhat, denominator, rho, next
   lambda, next F, accepted, halt, tag}, 17 kernels' damping, 18..20 the sums a, b, c as their slot groups hold them, 21 the groups' other
   slots are zero (-1: no sums), 22 scratch == backup, 23 scratch untouched, 24 the host logic absorbed the record (0: it had stopped, -1:
   tag mismatch), 25 iterations done, 26 stop, 27 rejections in a row, 28 / 29 a chi2 was written / its value, 30 / 31 the host's lambda / F.
   Every trial is fed to the device whether or not the host logic has stopped. */
int cuba_hip_debug_lm_script(int device, int start_mode, double F0, double lam0, const double* chi_slots, const uint64_t* maxdiag_bits, double tau, double tag_base,
	int niter, int n_trials, const int32_t* ok, const double* a, const int32_t* a_off, const double* b, const int32_t* b_off, const double* c, const int32_t* c_off,
	size_t scratch_count, double* out_start, double* out);
/* Test hook, read-only: the 64 x 8 ring of decision records of the handle's last cuba_hip_optimize / cuba_hip_optimize_batch run (record of
   trial k in slot k % 64, layout as above; zeros before the first run).  *count = 512; out may be NULL. */
int cuba_hip_debug_lm_records(cuba_hip_solver* s, double* out, size_t capacity, size_t* count);

/* A driver that runs the Levenberg-Marquardt loop itself through the stage calls announces the start of a run (a new lambda_0):
   the coarse inverse of the two-level preconditioner and the iteration-count predictions of the previous run are dropped, as
   cuba_hip_optimize does at its start; a hand-over to the exact reduced solve that an earlier run made (option "direct_fallback")
   is forgotten as well, so the new run starts with PCG again.  Optional (they would be refreshed after one slow solve anyway). */
int cuba_hip_begin_run(cuba_hip_solver* s);

/* The HIP stream the handle enqueues on (a collective library must order its operations with the solver's kernels). */
int cuba_hip_get_stream(cuba_hip_solver* s, void** hip_stream);

/* Enqueue (no host synchronisation) the evaluation of the current estimate over this handle's landmark range and leave
   three device scalars (element size cuba_hip_scalar_size()) at *device_scalars3:
     [0] robust chi2 of the local edges, [1] landmark part of sum x (lambda x + b) from the last cuba_hip_back_substitute,
     [2] pose part (only if with_scale != 0).  A multi-GPU driver sums [0..1] over the ranks in-stream. */
int cuba_hip_evaluate_device(cuba_hip_solver* s, double lambda, int with_scale, void** device_scalars3);

/* cuba_hip_schur in parts, for a driver that overlaps the sum over the ranks with the pass that produces it.  A landmark-partitioned
   handle cuts its reduced matrix at block rows into ranges of about equal size (option "reduction_chunks": 0 = automatic, one range
   per 8 MiB of matrix values and at most 8 -- a single part below 16 MiB --, n = at most n ranges; the cuts follow from the block
   pattern alone, so all ranks make the same ones) and runs the off-diagonal block pass range by range.  cuba_hip_schur_parts reports
   the number of parts (1 without a partition).  cuba_hip_schur_part(part) enqueues part 0 = linearisation, landmark pass, pose pass
   (all diagonal blocks, bsc, bp) and the off-diagonal blocks of range 0, or part c > 0 = the off-diagonal blocks of range c; parts
   must be run in the order 0 .. n - 1, all of them.  Once the work of part c is complete in stream order, the elements
   [ranges[0], ranges[0] + ranges[1]) of cuba_hip_reduction_buffer -- the blocks of range c -- and [ranges[2], ranges[2] + ranges[3])
   -- [bsc | bp] for part 0, empty otherwise -- hold this rank's final contribution.  The results are those of cuba_hip_schur bit for
   bit (which, on such a handle, simply runs all parts). */
int cuba_hip_schur_parts(cuba_hip_solver* s, int* n_parts);
int cuba_hip_schur_part(cuba_hip_solver* s, int part, size_t ranges[4]);

/* Device address + length (in doubles) of the contiguous buffer [Hsc values | bsc | bp] that a
   landmark-partitioned multi-GPU driver must sum across ranks between cuba_hip_schur and
   cuba_hip_solve_reduced (RCCL all-reduce over xGMI; no equivalent in the single-GPU reference). */
int cuba_hip_reduction_buffer(cuba_hip_solver* s, void** device_ptr, size_t* count);

#ifdef __cplusplus
}
#endif

#endif /* CUBA_HIP_H_ */
