// ba_kernels.hpp -- launch interface of the gfx950 kernels (implemented in ba_edge.hip, ba_linearize.hip, ba_pcg.hip, ba_coarse.hip, ba_factor.hip).
//
// Device data model (all SoA, fp64 + int32):
//   poses      q[4*Pt] t[3*Pt] cam[5*Pt]          free poses [0,Pf) first, fixed after
//   landmarks  Xw[3*Lt]                           free [0,Lf) first
//   edges      sorted by (landmark, pose): e_pose (bit 31 = stereo), e_lm, e_mu/e_mv/e_mr, e_w
//              lm_ptr[Lt+1] = edge range of each landmark
//   wave list  wave_lm[2*nWaves]: each 64-lane wavefront owns whole landmarks with <= 64 edges in total,
//              one lane per edge -> Hll/bl are reduced inside the wave, no atomics on the landmark side
//   Hsc        upper-triangular BSR (row_ptr/col_ind, 6x6 col-major blocks, diagonal block first in
//              each row), prod_* = per block the edge pairs of its Schur products, adj_* = full symmetric
//              adjacency over the same storage for the PCG SpMV
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "ba_math.hpp"

namespace cubahip
{

constexpr int PCG_SETUP_POSES = 64;   // poses per workgroup of the PCG set-up (= its partial sums of r0.z0 in block-Jacobi-only mode)
constexpr int NSLOT = 16;            // partial-sum slots for global reductions (spreads same-address atomics)
constexpr int WAVE = 64;
constexpr int LIN_BLOCK = 256;       // 4 wavefronts per workgroup in the landmark-major kernels
constexpr int STEREO_BIT = 0x40000000;

struct DeviceGraph
{
	int Pt = 0, Pf = 0, Lt = 0, Lf = 0, E = 0;
	int e_begin = 0, e_end = 0;        // sorted-edge range this handle evaluates (whole graph unless landmark-partitioned)
	Scalar *q = nullptr, *t = nullptr, *cam = nullptr, *Xw = nullptr;
	int *e_pose = nullptr, *e_lm = nullptr;
	Scalar *e_mu = nullptr, *e_mv = nullptr, *e_mr = nullptr, *e_w = nullptr;
	int* lm_ptr = nullptr;
	RobustKernel rk[2] = { { 0, 0 }, { 0, 0 } };
};

constexpr int BP_HEAVY = 64;      // blocks of Hsc with more products than this get a whole wave in the block pass

struct DeviceStructure
{
	int nWaves = 0;
	int* wave_lm = nullptr;            // [2*nWaves] first / one-past-last landmark of each wave
	int nBig = 0;
	int* big_lm = nullptr;             // landmarks with more than 64 edges (own workgroup each)
	int nblk = 0;
	int *hsc_rowptr = nullptr, *hsc_colind = nullptr;
	int *adj_ptr = nullptr, *adj_blk = nullptr, *adj_col = nullptr;  // adj_blk bit 31 = use transposed
	// the first 20*ell_m entries of every adjacency row again, padded to a fixed width and interleaved so that lane
	// (slot, m) finds its (block, column) pair at ((row*ell_m + m)*20 + slot) without reading adj_ptr first;
	// column -1 = padding. ell_over != 0 when some row has more entries (those stay in adj_* only).
	int2* ell = nullptr;
	int ell_m = 0, ell_over = 0;
	// destination-major (atomic-free) Schur assembly
	int* hsc_blkrow = nullptr;         // [nblk] block row of every block
	int nOd = 0;                       // blocks that receive at least one off-diagonal (or duplicate-pose) product
	int nDiagProd = 0;                 // of these, diagonal blocks (a landmark observed twice by one pose): the block pass then updates what the pose pass stored
	int* od_blocks = nullptr;          // [nOd] their ids, largest product count first
	int inv_rows8 = 1;                 // 1 = the landmark pass also writes inv(Hll + lambda I) as 64-byte rows (lm_inv) and the block pass gathers those;
	                                   // 0 = 48-byte gathers from the 72-byte rows of lm_sys (small graphs: the extra stores cost the landmark pass more than the block pass gains)
	int nHeavy = 0;                    // the first nHeavy of them have more than BP_HEAVY products: a whole wave each in the block pass
	int *prod_ea = nullptr, *prod_eb = nullptr;   // sorted edge ids of each product (ea: row pose, eb: column pose)
	// the ranges of the product list (per block) and of the pose edge list (per free pose) that THIS handle walks: consecutive
	// entries of the [n + 1] range arrays for a whole graph, sub-ranges (the lists are in landmark order) for a landmark
	// partition built on the device
	const int *prod_beg = nullptr, *prod_end = nullptr, *pe_beg = nullptr, *pe_end = nullptr;
	int* prod_lm = nullptr;            // landmark of each product (= e_lm[prod_ea]): the block pass then fetches inv(Hll + lambda) beside the
	                                   // two edge records instead of after them (one memory round trip per product instead of two)
	int* pe_edge = nullptr;            // per free pose: its sorted edge ids (ranges: pe_beg / pe_end)
	// coarse-matrix assembly lists: for every non-empty coarse block (I,J) the fine blocks that fall into it
	int nCb = 0;                       // non-empty coarse blocks
	int *cb_I = nullptr, *cb_J = nullptr, *cb_ptr = nullptr, *cb_blk = nullptr;   // cb_blk: adjacency-style id (bit 31 = transposed)
	Scalar *cb_wi = nullptr, *cb_wj = nullptr;                                    // weights of the fine (row, column) poses of every list entry in the linear coarse functions
	Scalar* e_rec = nullptr;           // [8*E] per-edge linearisation record {Xc[3], w' (sign bit = stereo), r[3], landmark (integer bits)}
	int mixed = 0;                     // fp64 library only: 1 = records and the per-edge arithmetic of the pose / block passes in fp32
};

int spmv_rows_for(int Pf);      // block rows per SpMV workgroup (two waves each): 2, or 4 for large graphs

struct DeviceSystem
{
	Scalar* hsc = nullptr;     // [36*nblk]  } one contiguous allocation (multi-GPU reduction buffer)
	Scalar* bsc = nullptr;     // [6*Pf]     }
	Scalar* bp = nullptr;      // [6*Pf]     }
	Scalar* lm_sys = nullptr;  // [9*Lf]  6 unique of Hll or inv(Hll+lambda I), then bl
	Scalar* lm_inv = nullptr;  // [8*Lf]  copy of inv(Hll+lambda I) in 64-byte rows for the block pass (a 48-byte gather from the 72-byte rows of lm_sys
	                           // straddles two 64-byte sectors three times out of four, and the pass pays per sector: profiles/r03x_block_pass_where.txt)
	Scalar* xp = nullptr;      // [6*Pf]
	Scalar* xl = nullptr;      // [3*Lf]
	Scalar* parts = nullptr;   // per-workgroup partial sums (first stage of the deterministic global reductions)
	Scalar* slots = nullptr;   // [4*NSLOT] chi2 | landmark scale (back_substitute) | per-edge chi2 scratch | stage scale
	unsigned long long* maxdiag = nullptr;  // bit pattern of a non-negative double
	int* fail = nullptr;       // numeric failure flag
	// PCG work
	Scalar *minv = nullptr, *r = nullptr, *z = nullptr, *p0 = nullptr, *p1 = nullptr, *ap = nullptr;
	// CG scalars as per-workgroup partial sums in small rings (no atomics => fixed summation order, nothing to zero):
	//   rz: slot 0 = r0.z0 (kept for the stop test), slot 1+(k&3) = r_k.z_k (k = 0: a second copy of slot 0, so that no
	//   address depends on the absolute iteration number);  pq: slot k&3 = p_k.A p_k
	Scalar *rz = nullptr, *pq = nullptr;
	int rzStride = 0, pqStride = 0;        // entries per ring slot
	int nrz0 = 0, nrz = 0, npq = 0;        // number of partials in slot 0 / in the ring slots of rz (nrz0 <= nrz) / in pq slots
	int* done = nullptr;                   // set once the solve is over (1: the stop test fired, 2: the iteration limit): later queued launches return at once
	int* iters = nullptr;      // device iteration counter
	int* host_flags = nullptr; // device-mapped host ints: {fail, iterations done, stop flag, ticket}, refreshed by the last node of every
	                           // iteration graph and by launch_pcg_report
	int* ticket = nullptr;     // device counter of those reports
	int* kbase = nullptr;      // iteration offset added to the k / kOut kernel arguments (lets one hipGraph
	                           // of `chunk` iterations be replayed: the graph's last node advances it by `chunk`)
	// two-level preconditioner: aggregates of `agg` consecutive free poses, 6 coarse dof each
	int agg = 0;               // 0 = block-Jacobi only
	int nc = 0;                // number of aggregates
	Scalar inv_agg = 0;        // 1 / agg
	int cl = 1;                // coarse functions per aggregate and pose component: 1 = constant, 2 = constant + linear in the pose
	                           // index (coarse dimension = 6*cl*nc)
	Scalar* acinv = nullptr;   // [(6nc)^2] explicit inverse of the coarse matrix P^T A P, column-major
	float* acinv32 = nullptr;  // fp64 library, option "precond_fp32": the same inverse in fp32 (symmetrised, rows padded to a multiple of 4
	                           // numbers) -- what the iteration kernels then read instead of acinv
	Scalar* gj_pivots = nullptr;   // [2][32 x 32] scratch of the Gauss-Jordan sweep (inverse of the current / next pivot block)
	Scalar* rc = nullptr;      // [2*6nc] restricted residual P^T r_k, ping-pong by the parity of k like r / r2 (each
	                           // aggregate's owner workgroup writes its 6 entries of P^T r_{k+1})
	Scalar* hrow = nullptr;    // [36 * 20 * ell_m * Pf] row-ordered copy of Hsc for the SpMV (launch_hsc_expand), entry (row, m, slot)
	int spmv_rows = 2;         // block rows per SpMV workgroup
	Scalar* qpart = nullptr;   // [agg/spmv_rows][6*cl*nc] (weighted) sums of q = A p over the block rows of each SpMV workgroup,
	                           // indexed by the workgroup's position inside its aggregate (P^T q is summed from these:
	                           // aggregates are whole multiples of spmv_rows rows)
	Scalar* r2 = nullptr;      // second residual buffer (the fused two-level kernel ping-pongs r / r2)
	// device-resident Levenberg-Marquardt decision (cuba_hip_optimize): kernels that are handed a NEGATIVE damping read it from here
	const Scalar* lam_dev = nullptr;
	// upper-triangle iteration (large graphs; ba_pcg.hip): three launches per iteration straight from the upper-triangular BSR storage
	int upper = 0;
	Scalar* tq = nullptr;      // [6 * (nblk - Pf)] transposed products B^T p_i of the off-diagonal blocks, written by the SpMV in the order of the rows that
	                           // own them: the lower neighbours of row j are one contiguous range
	int* lowpos = nullptr;     // [nblk] position of every off-diagonal block in that order (launch_build_lowpos)
};

// robust kernel of a pose factor (cuba_hip_set_pose_factor_robust_kernels): with e = r^T Omega r the objective term is rho(e) and the
// linearisation takes w Omega, w = rho'(e), for Omega.  Kinds 1 and 2 are robust_rho / robust_weight (ba_math.hpp); Cauchy, rho =
// delta^2 log1p(e / delta^2), exists for these factors only (helpers in ba_device.hpp).
enum { POSE_FACTOR_KERNEL_NONE = 0, POSE_FACTOR_KERNEL_HUBER = 1, POSE_FACTOR_KERNEL_TUKEY = 2, POSE_FACTOR_KERNEL_CAUCHY = 3 };

// The unary kinds of factor on the poses (ba_factor.hip) -- SE(3) pose priors, position, direction and range factors -- share their device
// layout: rho(r^T Omega r) per factor, sorted by internal pose (stable: a pose's factors are contiguous and in the caller's order); factors
// on fixed poses come last and are ignored.  A kind adds its two measurement arrays.
struct DevicePoseGroups
{
	int n = 0;                     // factors
	int nPoses = 0;                // free poses with factors
	const int* pose_ptr = nullptr; // [nPoses + 1] range of every such pose in the sorted list
	const int* pose_id = nullptr;  // [nPoses] its internal pose index
	const int* pose = nullptr;     // [n] internal pose of every factor (>= Pf: a fixed pose)
	const Scalar* info = nullptr;  // [D D n] column-major, D the dimension of r
	Scalar* chi = nullptr;         // [n] r^T Omega r of the last chi2 launch (0 on fixed poses)
	const int* rk_kind = nullptr;  // [n] robust kernel of every factor, sorted as the values; null: no factor has one (the kernels' ROBUST = false)
	const Scalar* rk_delta = nullptr;   // [n]
};
// SE(3) pose priors: r = log(T Tbar^-1) in the [omega, upsilon] tangent of the pose update, D = 6
struct DevicePriors : DevicePoseGroups { const Scalar *qbar = nullptr, *tbar = nullptr; };       // [4 n] unit quaternions, [3 n]
// Position factors (GNSS-style fixes): r = R^T (a - t) - z, the world position of the point a of the camera frame (the lever arm; zero: the
// camera centre) against a measured world position z, D = 3
struct DevicePositionFactors : DevicePoseGroups { const Scalar *z = nullptr, *arm = nullptr; };  // [3 n] measured positions, [3 n] lever arms
// Direction factors (gravity, compass, vanishing directions): r = R d - m, a world vector d against the same vector as measured in the
// camera frame, m (neither is normalised), D = 3 (Omega of rank 2 as a rule)
struct DeviceDirectionFactors : DevicePoseGroups { const Scalar *d = nullptr, *m = nullptr; };   // [3 n] world vectors, [3 n] their measurements
// Range factors (UWB anchors, acoustic beacons, slope distances): r = |a - t - R b| - rbar, the distance of the point a of the camera frame
// (the lever arm of the ranging antenna; zero: the camera centre) from the world point b (the anchor) against a measured range rbar, D = 1
// (info: the scalar 1 / sigma^2).  At a computed distance of exactly 0 the direction is undefined: the factor then has J = 0 (ba_factor.hip)
struct DeviceRangeFactors : DevicePoseGroups { const Scalar *br = nullptr, *arm = nullptr; };    // [4 n] {anchor, measured range}, [3 n] lever arms

// The binary kinds of factor on the poses (ba_factor.hip) -- SE(3) relative-pose edges and range factors between two poses -- share their
// device layout and everything that works on it but the linearisation of a factor.  Sorted: the factors between two free poses first, stable
// by the block (min, max) of the internal pose pair (a block's factors contiguous, in the caller's order), then the factors with one fixed
// end (they act on the free end only), then those with two (ignored).  A kind adds its measurement arrays and the layout of its record.
// Every free-free pair owns an off-diagonal block of hsc; the kinds' gathers run one behind the other (launch_pose_factor_linearize), and a
// block without Schur products is cleared by no one, so the first gather to reach such a block STORES its sum and every later one adds:
// blk_shared says per block whether a binary kind launched earlier writes it too (all zero for the kind launched first).
struct DevicePosePairs
{
	int n = 0;                     // factors
	int nActive = 0;               // the first nActive have a free end
	int nBlocks = 0;               // off-diagonal blocks of hsc with such factors
	int nPoses = 0;                // free poses with such factors
	const int *pose_i = nullptr, *pose_j = nullptr;   // [n] internal poses of every factor (>= Pf: a fixed pose)
	const int* blk_ptr = nullptr;  // [nBlocks + 1] range of every such block in the sorted list
	const int* blk_id = nullptr;   // [nBlocks] its block of hsc
	const int* blk_shared = nullptr;    // [nBlocks] 1: the gather of a binary kind launched earlier wrote the block in this linearisation
	const int* pose_ptr = nullptr; // [nPoses + 1] range of every such pose in pose_item
	const int* pose_id = nullptr;  // [nPoses] its internal pose index
	const int* pose_item = nullptr;// the pose's factors in the caller's order: 2 * sorted factor + (0: the pose is the factor's i, 1: its j)
	const Scalar* info = nullptr;  // [D D n] column-major, D the dimension of r
	Scalar* rec = nullptr;         // [record size x n] linearisation records, number-major (number el of factor k at el n + k)
	Scalar* chi = nullptr;         // [n] r^T Omega r of the last chi2 launch (0 with both ends fixed)
	const int* rk_kind = nullptr;  // [n] robust kernel of every factor, sorted as the values; null: no factor has one (the kernels' ROBUST = false)
	const Scalar* rk_delta = nullptr;   // [n]
};
// SE(3) relative-pose edges: r = log(T_j T_i^-1 Zbar^-1), D = 6
constexpr int REL_REC = 90;        // numbers of an edge's linearisation record (layout: ba_factor.hip)
struct DeviceRelPoses : DevicePosePairs { const Scalar *q = nullptr, *t = nullptr; };       // [4 n] unit quaternions, [3 n]: the measurements Zbar
// Range factors between two poses (peer UWB, odometer distances, rig baselines): r = |u| - rbar with u = a_j - (R_j w_i + t_j),
// w_i = R_i^T (a_i - t_i): the distance of the point a_i of camera frame i from the point a_j of camera frame j against a measured range,
// D = 1 (info: the scalar 1 / sigma^2).  A low-rank term: J_i and J_j are 1 x 6 each.  At a computed distance of exactly 0 both J are 0.
constexpr int PRNG_REC = 14;       // numbers of a factor's linearisation record: J_i [6] | J_j [6] | w Omega | w Omega r
struct DevicePoseRanges : DevicePosePairs
{
	const Scalar *arm_i = nullptr, *arm_j = nullptr;  // [3 n] lever arms in the two camera frames
	const Scalar* range = nullptr; // [n] measured distances
};

// Landmark position priors (ba_factor.hip): rho(r^T Omega r), r = X - Xbar, Omega a symmetric 3 x 3 information.  Sorted by internal landmark
// (stable: a landmark's priors are contiguous and in the caller's order); priors on fixed landmarks come last and are ignored.  The landmark
// pass adds a landmark's terms w Omega / -w Omega r to its Hll / bl (ba_device.hpp: add_landmark_priors), in a kernel instantiation of its
// own that only a handle with such priors launches.
struct DeviceLandmarkPriors
{
	int n = 0;                     // priors
	const int* lm_ptr = nullptr;   // [Lf + 1] range of every free landmark in the sorted list
	const int* lm = nullptr;       // [n] internal landmark of every prior (>= Lf: a fixed landmark)
	const Scalar* xbar = nullptr;  // [3 n]
	const Scalar* info = nullptr;  // [6 n] upper triangle in the packing of sym3_idx
	const int* rk_kind = nullptr;  // [n] robust kernel of every prior (POSE_FACTOR_KERNEL_*)
	const Scalar* rk_delta = nullptr;   // [n]
	Scalar* chi = nullptr;         // [n] r^T Omega r of the last chi2 launch (0 on fixed landmarks)
};

// The factors of a handle besides the reprojection edges: what the rest of the library sees of the kinds (a kind without factors: n = 0,
// nothing of it is launched).  The landmark priors ride along for the chi2 sums only: their linearisation is the landmark pass's.
// FACTOR_*: the kinds in the order of their chi2 partials, of each() below and of the handle's table of sets (ba_solver.hpp: factorSets).
enum { FACTOR_PRIORS = 0, FACTOR_REL, FACTOR_LMP, FACTOR_POS, FACTOR_DIR, FACTOR_RNG, FACTOR_PRNG, FACTOR_KINDS };
struct DeviceFactors
{
	DevicePriors priors; DeviceRelPoses rel; DeviceLandmarkPriors lmp; DevicePositionFactors pos; DeviceDirectionFactors dir; DeviceRangeFactors rng;
	DevicePoseRanges prng;
	template <class F> void each(F&& f) const { f(priors); f(rel); f(lmp); f(pos); f(dir); f(rng); f(prng); }      // every kind's device struct, in that order
};
// The factors' linearisation behind the Schur pass, every kind in launches of its own in one stream.  THE ORDER (it exists here only):
//   1. pose priors            J = J_l(r)^-1 (6 x 6)
//   2. position factors       J = [R^T [a]x | -R^T] (3 x 6)
//   3. relative-pose edges    per-edge records, then their gather
//   4. direction factors      J = [-[R d]x | 0] (3 x 6): the rotation 3 x 3 of the diagonal block and the first three entries of bp / bsc only
//   5. range factors          J = [(m x a)^T | -m^T] (1 x 6, m the unit vector from the anchor to the antenna in the camera frame)
//   6. range factors between two poses    per-factor records {J_i, J_j, w Omega, w Omega r}, then their gather
// A unary kind adds J^T Omega J to the diagonal block of its pose in hsc (upper triangle) and -J^T Omega r to bp and (mode 1) bsc, Omega: w Omega
// of a factor with a robust kernel.  A binary kind's gather adds the same for either end and (mode 1) its cross terms to the pairs'
// off-diagonal blocks -- stored whole where a block has neither Schur products nor an earlier binary kind (DevicePosePairs: blk_shared).
// All six kinds on the poses (the seventh, the landmark priors, is the landmark pass's) add to the same diagonal blocks, bp and bsc by read-modify-write, and floating-point sums do not
// commute: the order of the launches is part of the result, a handle's bits depend on it.  THE RULE: a new kind goes BEHIND the ones a
// handle may already combine, never between two of them.  (The position factors sit between the priors and the edges because no handle
// could hold them before they came, so no existing sum changed; every kind since went last.)
void launch_pose_factor_linearize(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const DeviceFactors& pf, int mode, hipStream_t s);
// per-factor chi2 (the plain r^T Omega r) into every kind's chi, per-workgroup partial sums of rho(chi2) into
// parts[0 .. factor_chi2_parts(&pf)), kind behind kind in the order of FACTOR_*.  only >= 0: that kind alone, its partials at parts[0]
void launch_factor_chi2(const DeviceGraph& g, const DeviceFactors& pf, Scalar* parts, hipStream_t s, int only = -1);
int factor_chi2_parts(const DeviceFactors* pf);     // 0 for no factors (pf null), at most 64 per kind

// residual / robust chi2 over all edges -> sys.slots[0..NSLOT) (must be zeroed by the caller).
// per_edge (optional, sorted edge order): non-robust omega*|r|^2.
// pf (optional): the factors' chi2 partials follow the edges' and are summed with them (the objective F of the LM loop)
void launch_residual_chi2(const DeviceGraph& g, Scalar* parts, Scalar* slots, Scalar* per_edge, hipStream_t st, const DeviceFactors* pf = nullptr);

// mode 0: assemble only (Hpp -> diagonal blocks of hsc, bp, Hll/bl -> lm_sys, max diagonal of Hll)
// mode 1: full linearise + Schur reduction with damping lambda (hsc, bsc, bp, inv(Hll+lambda)/bl -> lm_sys)
// launch_linearize_dm: destination-major, atomic-free and bitwise reproducible:
//   landmark pass (Hll/bl, inverse, per-edge record) -> pose pass (diagonal blocks, bp, bsc) -> block pass (off-diagonal blocks)
// backupSrc != nullptr: the landmark pass's launch also copies backupCount numbers backupSrc -> backupDst (the LM loop's push())
// range != nullptr (landmark partitions whose reduction is cut into parts, ba_setup.hip: cutReductionParts): the block pass covers the
// entries [begin, end) of st.od_blocks only, the first `heavy` of them with a whole wave each; launch_block_pass runs a further range
struct BlockPassRange { int begin, end, heavy; };
// restoreFlag != nullptr (cuba_hip_optimize; needs st.nWaves > 0 and a backup): the LM decision state's "last trial accepted" number.  When it
// is zero the same launch undoes the rejected trial instead: the landmark workgroups read poses and landmarks from backupDst -- which holds
// the estimate the trial started from and which nobody writes in this launch -- and the copy workgroups copy backupDst -> backupSrc
void launch_linearize_dm(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, int mode, Scalar lambda, hipStream_t s,
	Scalar* backupSrc = nullptr, Scalar* backupDst = nullptr, size_t backupCount = 0, const BlockPassRange* range = nullptr, const double* restoreFlag = nullptr,
	const DeviceLandmarkPriors* lp = nullptr);
void launch_block_pass(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const BlockPassRange& range, hipStream_t s);

// max over the diagonal of the diagonal blocks of hsc (Hpp after an assemble pass) folded into sys.maxdiag
void launch_pose_maxdiag(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, hipStream_t s);

// xl = inv(Hll+lambda)(bl - Hpl^T xp); accumulates sum xl (lambda xl + bl) into slots[NSLOT..2*NSLOT)
void launch_back_substitute(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, Scalar lambda, hipStream_t s);

// pose-side part of the gain-ratio denominator: sum xp (lambda xp + bp) -> slots[0..NSLOT)
void launch_pose_scale(const DeviceGraph& g, const DeviceSystem& sys, Scalar lambda, Scalar* slots, hipStream_t s);
// back-substitution + update + evaluation of the trial + second stage of their three sums + report to the host in two launches:
// back-substitution, update and evaluation fused into one pass over the edges (`old` = copy of the state
// [q | t | Xw] made before the trial: the pass reads the pre-update estimate from it while it writes the updated one), then the sums
// + report.  trial_tail_parts(): numbers of partial-sum scratch (sys.parts) it needs.
struct LmDevice;
// pf (optional): the factors' chi2 at the updated estimate, launches between the edge pass and the sums; their partials join the edges'
// chi2 partials
// publish = 0: the decision's record goes out with plain stores, without the system-scope fence and the ticket (the caller then does not
// count a report): for decisions the host does not wait for
void launch_trial_tail_fused(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, Scalar lambda, const Scalar* old, hipStream_t s,
	const LmDevice* decide = nullptr, const DeviceFactors* pf = nullptr, int publish = 1);
size_t trial_tail_parts(const DeviceGraph& g, const DeviceStructure& st, int factorParts = 0);      // factorParts: factor_chi2_parts()
// Device-resident LM decision (control flow of CudaBundleAdjustmentImpl::optimize, /root/reference/src/cuda_bundle_adjustment.cpp:816-851):
// state = {F, lambda, nu, halt, trials, accepted (last trial), rejections in a row, max rejections} in device memory, lam = the damping as
// the kernels read it (sys.lam_dev), ring = device-mapped host records, LM_REC numbers per trial {Fhat, denominator, rho, next lambda,
// next F, accepted, halt, next nu}.  launch_trial_tail_fused(.., decide) lets the sums' second stage take the decision of the trial instead
// of only reporting them; launch_lm_decide_failed is the decision of a trial whose reduced solve failed (rho = -1);
// launch_restore_if_rejected copies the backup over the estimates when the last decision was a rejection (the reference's pop()).
constexpr int LM_REC = 8, LM_RING = 64;
struct LmDevice { double* state = nullptr; Scalar* lam = nullptr; double* ring = nullptr; };
// the start of a run on the device: state = {F0 = the sum of the NSLOT numbers at chiSlots, lambda0 = tau * the largest of the 64 numbers at maxdiag, 2, 0, 0,
// 1, 0, maxq, tagBase}, lam = lambda0
void launch_lm_run_init(const Scalar* chiSlots, const unsigned long long* maxdiag, const LmDevice& lm, double tau, double tagBase, int maxq, hipStream_t s);
void launch_lm_decide_failed(const DeviceSystem& sys, const LmDevice& lm, hipStream_t s);
// the sums' second stage of a trial on its own (what launch_trial_tail_fused ends with): partials pA[0, nA) -> oA[0..NSLOT) (total in oA[0], zeros
// behind it), likewise B and C; with `decide` the decision of the trial from them (A = landmark part of the denominator, B = chi2, C = pose
// part), with `publish` the report to the host
void launch_reduce_report(const DeviceSystem& sys, const Scalar* pA, int nA, Scalar* oA, const Scalar* pB, int nB, Scalar* oB, const Scalar* pC, int nC, Scalar* oC,
	const LmDevice* decide, int publish, hipStream_t s);
void launch_restore_if_rejected(Scalar* state, const Scalar* backup, size_t count, const LmDevice& lm, hipStream_t s);
// landmark-side part recomputed from xl and the stored bl (stage API; the fused path gets it from back_substitute)
void launch_landmark_scale(const DeviceGraph& g, const DeviceSystem& sys, Scalar lambda, Scalar* slots, hipStream_t s);

void launch_update_state(const DeviceGraph& g, const DeviceSystem& sys, hipStream_t s);   // poses + landmarks in one launch

// block-Jacobi PCG on the upper-BSR reduced system
void launch_pcg_setup(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, Scalar lambda, hipStream_t s);
void launch_pcg_spmv(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, int k, int maxIter, Scalar tol2, hipStream_t s);
void launch_pcg_update(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, int k, int maxIter, Scalar tol2, hipStream_t s);
// two-level (block-Jacobi + aggregate coarse correction) variant: 3 kernels per iteration
Scalar* launch_coarse_setup(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, Scalar* work0, Scalar* work1, hipStream_t s, hipEvent_t assembled = nullptr);
// blocked Gauss-Jordan inversion of a dense SPD n x n matrix (column-major in work0; work1 = scratch of the same size);
// returns whichever of the two buffers holds the inverse
Scalar* launch_dense_inverse(Scalar* work0, Scalar* work1, int n, Scalar* pivots, hipStream_t s);   // symmetric sweep: the result's upper triangle holds -A^-1; pivots: 2 x 32 x 32 numbers of scratch
void launch_coarse_finish(const Scalar* swept, Scalar* dst, int n, hipStream_t s);    // swept buffer -> full symmetric +A^-1 (dst may be the swept buffer)
// batched sweep of several coarse matrices (cuba_hip_optimize_batch): one launch per step for all of them
struct GjJob { Scalar* buf[2]; Scalar* piv[2]; int n, tiles; };       // buf[0]: the matrix on entry; piv: 2 x (32 x 32) scratch
void launch_coarse_assemble(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, Scalar* work0, hipStream_t s);
void launch_dense_inverse_batch(const GjJob* jobs, int m, int nMax, hipStream_t s);
void launch_pcg2_fused(const DeviceGraph& g, const DeviceSystem& sys, int k, int kOut, int maxIter, Scalar tol2, int doUpdate, hipStream_t s);
// one iteration of the upper-triangle form (sys.upper): which = 1 SpMV | 2 row updates | 4 preconditioner (7 = all three, in this order)
int spmv_upper_grid(int Pf);      // workgroups of the upper-triangle SpMV (= its p.Ap partials)
int pcg_rows_max_aggregate();     // largest aggregate (poses) the row-update launch of the upper-triangle iteration handles
int pcg_rows_entries_per_thread(const DeviceSystem& sys);   // row entries per thread of that launch for sys.agg: 2, 4 or 8
void launch_build_lowpos(const DeviceGraph& g, const DeviceStructure& st, int* lowpos, hipStream_t s);
void launch_pcg_upper_iteration(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, int k, int maxIter, Scalar tol2, hipStream_t s, int which = 7);
// what the last node of an iteration graph does, as a launch: advance the iteration offset by n, run the stop test on the residual the
// chunk left (tol2 >= 0), report to the host
void launch_pcg_advance(const DeviceSystem& sys, int n, hipStream_t s, Scalar tol2 = Scalar(-1));
void launch_coarse_to_fp32(const Scalar* swept, float* dst, int n, hipStream_t s);   // swept buffer -> +A^-1 in the sys.acinv32 layout
void launch_pcg_iteration(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, int k, int maxIter, Scalar tol2, hipStream_t s);

// ---- batched execution (cuba_hip_optimize_batch): the PCG iterations of several graphs as ONE launch chain ---------------------------
// Device table entry of one graph: what its kernels otherwise receive as kernel arguments.  The batched kernels take blockIdx.y as the
// graph number; a graph whose reduced solve has finished keeps its entry (its `done` flag makes its workgroups return at once).
struct LmDevice;
struct BatchTrial               // per-graph arguments of the batched launches around the iterations (a grid of 0: the graph sits this launch out)
{
	// landmark pass (+ state backup), pose + block pass
	unsigned lmGroups = 0, lmGrid = 0; const Scalar* backupSrc = nullptr; Scalar* backupDst = nullptr; size_t backupCount = 0;
	int poseGroups = 0; unsigned schurGrid = 0;
	// PCG set-up launch (+ row-ordered copy + copy of a fresh coarse inverse), first preconditioner application
	int nSetup = 0; size_t expandTotal = 0; unsigned nExpand = 0; const Scalar* copySrc = nullptr; Scalar* copyDst = nullptr; size_t copyPairs = 0; unsigned setupGrid = 0;
	int fusedOn = 0;
	// trial tail, sums + decision + report, conditional restore
	const Scalar* old = nullptr; Scalar *scParts = nullptr, *chiParts = nullptr, *scaleParts = nullptr; int nLm = 0, poseBlocks = 0, nScale = 0; unsigned tailGrid = 0; int nA = 0;
	double* lmState = nullptr; Scalar* lmLam = nullptr; double* lmRing = nullptr; int reportOn = 0;
	Scalar* state = nullptr; size_t stateCount = 0; unsigned restoreGrid = 0;
};
struct BatchEntry
{
	DeviceGraph g; DeviceStructure st; DeviceSystem sys;
	int maxIter = 0;
	int gridSpmv = 0;              // workgroups of this graph's SpMV launch (the batched grid is the maximum over the graphs)
	BatchTrial t;
};
// the batched launches of one trial (every graph's kernels, arguments and order as launch_linearize_dm / launch_pcg_setup_expand /
// launch_pcg2_fused(k = 0) / launch_trial_tail_fused + launch_restore_if_rejected issue them for one graph)
void batch_fill_linearize(const DeviceGraph& g, const DeviceStructure& st, const Scalar* backupSrc, Scalar* backupDst, size_t backupCount, BatchTrial& t);
void launch_batch_linearize(const BatchEntry* tab, int n, unsigned lmGridMax, unsigned schurGridMax, bool mixed, hipStream_t s);
void batch_fill_setup(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const Scalar* copySrc, Scalar* copyDst, size_t copyCount, BatchTrial& t);
void launch_batch_setup(const BatchEntry* tab, int n, unsigned gridMax, hipStream_t s);
void launch_batch_first_precond(const BatchEntry* tab, int n, const DeviceSystem& sys0, int ncMax, size_t ldsMax, Scalar tol2, hipStream_t s);
void batch_fill_tail(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const Scalar* old, const LmDevice& lm, Scalar* state, size_t stateCount, BatchTrial& t);
void launch_batch_tail(const BatchEntry* tab, int n, unsigned tailGridMax, unsigned restoreGridMax, hipStream_t s);
int batch_kernel_class(const DeviceGraph& g, const DeviceSystem& sys);       // graphs of one batch must agree on it; -1 = not batchable
size_t batch_pcg2_lds_bytes(const DeviceSystem& sys);
// one PCG iteration (chunk-local k) of all n graphs of the table: SpMV + fused two-level kernel, 2 launches
void launch_pcg_batch_iteration(const BatchEntry* tab, int n, const DeviceGraph& g0, const DeviceSystem& sys0, int gridSpmvMax, int ncMax, size_t ldsMax, int k, Scalar tol2, hipStream_t s);
// advance every graph's iteration offset by `iters`, stop test on the residual the chunk left, report to every graph's host block
void launch_pcg_batch_advance(const BatchEntry* tab, int n, int iters, hipStream_t s, Scalar tol2);

// Adds `chunk` PCG iterations (chunk-local k = 0..chunk-1) and the kbase advance to `graph` as a chain of kernel nodes.
// report != 0: the last node also copies the solver's flags and a ticket into the mapped host block (only the last graph of a
// batch needs that: the write to host memory costs several microseconds)
hipError_t graph_add_pcg_chunk(hipGraph_t graph, const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, int chunk, int maxIter, Scalar tol2, int report);

// hsc (damped, after pcg_setup) -> sys.hrow
void launch_hsc_expand(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, hipStream_t s);
// both in one launch; copySrc != nullptr: the same launch also copies copyCount (even) numbers copySrc -> copyDst (a freshly inverted
// coarse matrix into the buffer the iteration graphs read)
void launch_pcg_setup_expand(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, Scalar lambda, hipStream_t s,
	const Scalar* copySrc = nullptr, Scalar* copyDst = nullptr, size_t copyCount = 0);

// ---- exact reduced solve (ba_direct.hip): sparse tile Cholesky of the damped reduced matrix + triangular solves -------------------
// The free poses (internal order) are cut into segments of SC_TP consecutive poses = one 32 x 32 tile of the matrix (30 unknowns + 2
// identity-padded ones).  A minimum-degree elimination of the segment graph (multiple elimination: independent segments of near-minimal
// degree per round) gives the tile order, the fill and the elimination tree; columns of one tree LEVEL are independent, so the numeric
// phase is one launch per level (left-looking: every tile gathers the updates of its descendants in a fixed order -- no atomics, results
// reproducible bit for bit) and the two substitutions ride on the same levels.
constexpr int SC_T = 32;          // tile edge
constexpr int SC_TP = 5;          // poses per tile
constexpr int SC_TT = SC_T * SC_T;

struct SparseCholPlan             // host: the symbolic phase's result for one block pattern
{
	int Pf = 0, T = 0, nTiles = 0, nLevels = 0, slack = 0;
	std::vector<int> posOfSeg, segOfPos;     // segment <-> elimination position (= tile column)
	std::vector<int> colPtr;                 // [T + 1] tiles of column k: the diagonal tile first, then its rows in ascending position
	std::vector<int> rowIdx, colOfTile;      // [nTiles]
	std::vector<int> gPtr;                   // [nTiles + 1] gather list of every tile ...
	std::vector<int> gather;                 // ... 4 ints per entry {tile (i, k) or the zero tile, tile (j, k), k, 0}, k ascending, padded to a multiple of 4
	std::vector<int> wgRec;                  // [8 nTiles] per entry of lvlTiles: {tile, diagonal tile of its column, column, first gather entry, entries, 0, 0, 0}
	std::vector<int> lvlPtr, lvlTiles;       // [nLevels + 1], [nTiles]: tiles by the level of their column (work list of the factorisation)
	std::vector<int> lvlColPtr, lvlCols;     // [nLevels + 1], [T]: columns by level (work list of the backward substitution)
	std::vector<int> blkTile;                // [nblk] destination tile of every block of the upper-triangular BSR storage (bit 30: transposed)
	long long entries = 0;                   // gather entries (two tile products each at most)
	size_t tileBytes() const { return sizeof(Scalar) * (size_t)SC_TT * ((size_t)2 * nTiles + 1); }
	double secondsEstimate() const;          // what one factorisation + solve costs (a model: launches per level + tile traffic)
};
// slack < 0: automatic (the cheapest of a few multiple-elimination slacks by secondsEstimate).  false: more than maxTiles tiles of fill
bool sparse_chol_plan(int Pf, const int* rowptr, const int* colind, int slack, size_t maxTiles, SparseCholPlan& out);

struct SparseChol                 // device view
{
	Scalar* tiles = nullptr;      // [nTiles + 1][32 x 32] column-major: the matrix; the off-diagonal tiles become L; the last tile stays zero
	Scalar* tilesT = nullptr;     // [nTiles][32 x 32] the off-diagonal tiles of L once more, transposed (what the backward substitution reads); a diagonal
	                              // tile's slot: L_jj mirrored into both triangles
	Scalar* y = nullptr;          // [32 T] right-hand side -> L^-1 b -> solution, in elimination order
	Scalar* rinv = nullptr;       // [32 T] 1 / L_cc
	const int *colPtr = nullptr, *rowIdx = nullptr, *colOfTile = nullptr, *gPtr = nullptr, *gather = nullptr;
	const int *wgRec = nullptr, *lvlCols = nullptr, *blkTile = nullptr, *posOfSeg = nullptr;
	int* fail = nullptr;          // != 0 after the solve: a non-positive pivot was met (the matrix is not positive definite)
	int T = 0, Pf = 0, nTiles = 0;
};
// hsc (damped by launch_pcg_setup: full diagonal blocks) and bsc -> d.tiles / d.y; clears d.fail
void launch_sparse_chol_fill(const DeviceStructure& st, const DeviceSystem& sys, const SparseChol& d, hipStream_t s);
// factorise and solve: x[0 .. 6 Pf) = A^-1 b (internal pose order)
void launch_sparse_chol_solve(const SparseChol& d, const SparseCholPlan& plan, Scalar* x, hipStream_t s);
// the factorisation alone (the launches of launch_sparse_chol_solve's first loop)
void launch_sparse_chol_factor(const SparseChol& d, const SparseCholPlan& plan, hipStream_t s);

// ---- marginal covariances (ba_direct.hip: symbolic phase, ba_covariance.hip: numeric phase) --------------------------------------
// Selected inversion of the factorised reduced matrix S = L L^T on the factor's own pattern (Takahashi recurrence): for every column j,
// the tree's levels walked from the top down,
//     U_kj = L_kj L_jj^-1 (k in I_j, the rows of column j),   Sigma_ij = -sum_{k in I_j} Sigma_ik U_kj (i in I_j),
//     Sigma_jj = L_jj^-T L_jj^-1 - sum_{k in I_j} U_kj^T Sigma_kj.
// The rows of a column form a clique of the filled graph, so every Sigma_ik the sums read lies on the pattern, in a column of a higher
// level.  The plan is built from a SparseCholPlan and changes nothing in it.
struct SelInvPlan
{
	int nLevels = 0;
	std::vector<int> stepPtr;                // [nLevels + 1] step s = level nLevels - 1 - s: its off-diagonal tiles ...
	std::vector<int> offRec;                 // ... 4 ints each {tile (i, j), column j, first gather entry, entries}
	std::vector<int> colStepPtr, cols;       // [nLevels + 1], [T]: the columns of step s (their diagonal tiles come second in the step)
	std::vector<int> gather;                 // 2 ints per entry {Sigma tile (i, k) | bit 30 when it is stored as (k, i), tile (k, j)}, k ascending
	long long products = 0;                  // tile products of one selected inversion (diagonal tiles included)
	size_t sigmaBytes() const;               // the Sigma tile array a computation allocates (the factor's tile count)
	int nTiles = 0;
};
// false: a tile the recurrence needs is missing from the pattern (cannot happen for a factor's pattern; a bug, reported by the caller)
bool selinv_plan(const SparseCholPlan& p, SelInvPlan& out);

struct SelInv                     // device view
{
	Scalar* sigma = nullptr;      // [nTiles][32 x 32] column-major: Sigma on the factor's pattern (diagonal tiles full, both triangles)
	const int *offRec = nullptr, *gather = nullptr, *cols = nullptr;
};
// after launch_sparse_chol_factor on d: L_jj^-1 into the diagonal tiles' slots of d.tiles, U_kj into the off-diagonal slots of d.tilesT
// (row-major), then the levels top-down into v.sigma
void launch_selinv(const SparseChol& d, const SparseCholPlan& plan, const SelInvPlan& sp, const SelInv& v, hipStream_t s);
// Sigma's 6 x 6 blocks: pose_cov [36 Pf] (diagonal blocks, internal order), blk_cov [36 nblk] (the blocks of the upper-triangular BSR
// storage, through d.blkTile); either may be null
void launch_selinv_extract(const DeviceStructure& st, const SparseChol& d, const SelInv& v, Scalar* pose_cov, Scalar* blk_cov, int Pf, hipStream_t s);
// landmark marginals [9 Lf] (3 x 3 column-major, internal landmark order) at lambda = 0: Hll^-1 + Hll^-1 (sum_{p,q} W_p^T Sigma_pq W_q) Hll^-1,
// from the landmark pass's Hll^-1 (sys.lm_sys) and W recomputed per edge (w_scratch: 18 E numbers)
void launch_landmark_covariance(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const SparseChol& d, const SelInv& v,
	Scalar* w_scratch, Scalar* lm_cov, hipStream_t s);

// L_jj^-1 into the diagonal tiles' slots of d.tiles (the first launch of launch_selinv; the rest of the factor is left as it is)
void launch_diag_inverse(const SparseChol& d, hipStream_t s);
// W = the 6 x 3 Hpl block of every edge at the current estimate (18 E numbers, column-major; zero for an edge to a fixed vertex)
void launch_edge_w(const DeviceGraph& g, Scalar* W, hipStream_t s);

// ---- marginal covariances of arbitrary pairs (ba_covariance_pairs.hip) ------------------------------------------------------------
// X_b = S^-1 C_b for 32-column blocks of right-hand sides (the poses of one segment, or ten landmarks' W columns), solved only on the tree
// columns a block touches: the FORWARD set (ancestors of the segments C_b touches) and the BACKWARD set (ancestors of the segments the
// pairs' left sides read).  Both are unions of root-ward chains (parent = first off-diagonal row of a column), hence closed under the rows
// of a column.  A request is packed once; its blocks run in chunks that fit the workspace.
struct PairRequest                // host, internal numbering (pose kind 0, landmark kind 1)
{
	int nBlocks = 0;
	std::vector<int> rhsPtr, rhsPos;         // [nBlocks + 1]: tile columns (positions) the block's right-hand side touches, ascending
	std::vector<int> leftPtr, leftPos;       // [nBlocks + 1]: tile columns its pairs' extraction reads, ascending
	std::vector<int> poseRec;                // 4 ints per right pose {block, column in the block, 0, 0}, by block
	std::vector<int> lmRec;                  // 4 ints per right landmark {landmark, block, column, 0}, by block
	std::vector<int> pairRec;                // 8 ints per computed pair {kind a, a, block, column of b, kind b, b, output index, 0}
};
// pairs with a negative index (a fixed vertex) are left out; lmPtr / ePose: the landmark-major edge lists (only read for landmarks)
void pair_pack(const SparseCholPlan& p, int n, const int* kindA, const int* idxA, const int* kindB, const int* idxB,
	const std::vector<int>& lmPtr, const std::vector<int>& ePose, PairRequest& rq);
struct PairPlan                   // host: blocks [b0, b1) of a request (one chunk)
{
	int b0 = 0, b1 = 0, nLevels = 0, T = 0;
	std::vector<int> fwdPtr, fwdCols;        // per block of the chunk: the forward set, ascending
	std::vector<int> bwdPtr, bwdCols;        // per block: the backward set, ascending
	std::vector<int> slotPtr, slotCols;      // per block: its workspace tiles (the union of both sets, ascending), numbered across the chunk
	std::vector<int> slotOf;                 // [(b1 - b0) T] slot of (block, tile column), -1 outside the block's sets
	std::vector<int> fLvlPtr, fRec;          // forward work by level ascending; 4 ints per record {slot, column j, first gather entry, entries}
	std::vector<int> fGather;                // 2 ints per entry {tile (j, k), slot of k}: k in the forward set, ascending
	std::vector<int> bLvlPtr, bRec;          // backward work, step s = level nLevels - 1 - s; records as above
	std::vector<int> bGather;                // 2 ints per entry {tile (i, j), slot of i}: every row i of column j, ascending
	size_t slots() const { return slotCols.size(); }
};
size_t pair_block_slots(const SparseCholPlan& p, const PairRequest& rq, int b);
// false: a row of a column is missing from the backward set (cannot happen for a factor's pattern; a bug, reported by the caller)
bool pair_plan(const SparseCholPlan& p, const PairRequest& rq, int b0, int b1, PairPlan& out);
struct PairDev                    // device view of one chunk
{
	Scalar* X = nullptr;          // [slots][32 x 32] column-major: C -> Y -> X
	const int *fRec = nullptr, *fGather = nullptr, *bRec = nullptr, *bGather = nullptr, *slotOf = nullptr, *rhsPos = nullptr;
	int T = 0;
};

// out3 = {chi2 total, landmark scale part, pose scale part} gathered from the result slots of the kernels enqueued before
void launch_collect_eval(const DeviceSystem& sys, Scalar* out3, hipStream_t s);

// ---- edge gating (ba_gate.hip) ------------------------------------------------------------------------------------------------------
enum { GATE_RECLASSIFY = 0, GATE_ONLY_REMOVE = 1, GATE_DRY_RUN = 2 };
constexpr int GATE_COUNTS = 6;    // active mono, active stereo, gated by chi2 mono, gated by chi2 stereo, gated by depth, changed
struct EdgeGateArgs
{
	DeviceGraph g;                     // e_w: the UPLOADED information
	double chi2_mono = 0, chi2_stereo = 0;
	int require_depth = 1, mode = GATE_RECLASSIFY;
	const uint8_t* mask_in = nullptr;  // [E] sorted order; null: every edge is active
	uint8_t* mask_out = nullptr;       // [E] sorted order    } not written by a dry run
	Scalar* w_live = nullptr;          // [E] mask ? w0 : +0  }
	Scalar* chi_out = nullptr;         // [E] omega |r|^2 with the uploaded omega, sorted order (optional)
	long long* parts = nullptr;        // [GATE_COUNTS * edge_gate_grid(g)]
};
int edge_gate_grid(const DeviceGraph& g);
// an edge stays active iff chi <= chi2_max[stereo] and (no depth test or Xc[2] > 0) -- a NaN fails both --; GATE_ONLY_REMOVE: and it was
// active.  counts[GATE_COUNTS]: a depth failure counts as such whatever its chi2; `changed` compares with mask_in.
void launch_edge_gate(const EdgeGateArgs& a, long long* counts, hipStream_t s);
// the mask between the caller's edge order and the sorted one (perm[sorted position] = caller's index), with the live information
void launch_gate_apply(const uint32_t* perm, const uint8_t* maskCaller, const Scalar* w0, int E, uint8_t* maskSorted, Scalar* w_live, hipStream_t s);
void launch_gate_unsort(const uint32_t* perm, const uint8_t* maskSorted, int E, uint8_t* maskCaller, hipStream_t s);
// out[l] = active edges of landmark l in the caller's numbering (newOfOld: the internal landmark order, or null; mask null: all active);
// bigInternal[Lt]: scratch of the landmarks of big_lm (more than 64 edges: one workgroup each)
void launch_landmark_active(const int* lm_ptr, const uint8_t* mask, const int* newOfOld, int Lt, const int* big_lm, int nBig, int* bigInternal, int* out, hipStream_t s);

// ---- landmark triangulation (ba_triangulate.hip) ------------------------------------------------------------------------------------
// the statuses in the order they are decided (include/cuba_hip.h: CUBA_HIP_TRI_*)
enum { TRI_OK = 0, TRI_NOT_SELECTED, TRI_FIXED, TRI_FEW_OBSERVATIONS, TRI_LOW_PARALLAX, TRI_SINGULAR, TRI_BEHIND_CAMERA, TRI_CHI2, TRI_STATUSES };
constexpr int TRI_MAX_ITERATIONS = 16;
struct TriangulateArgs
{
	DeviceGraph g;                     // e_w: the LIVE information (a gated edge is out); rk: the handle's robust kernels
	const int* wave_lm = nullptr; int nWaves = 0;      // the landmark pass's wave list ...
	const int* big_lm = nullptr; int nBig = 0;         // ... and its landmarks of more than 64 edges
	int iterations = 0;                // Gauss-Newton steps behind the linear start
	int parallax_on = 0; double cos_half_parallax = 1; // LOW_PARALLAX: |sum of the unit rays| / n > cos(min_parallax / 2)
	double chi2_mono = 0, chi2_stereo = 0;
	int dry_run = 0;                   // 1: g.Xw is left alone
	int* status = nullptr;             // [Lt] internal landmark order (between the launches also the internal "pending" mark)
	double* xnew = nullptr;            // [3 Lt] internal order: the accepted position of an OK landmark as the state holds it (others: not written)
};
int triangulate_collect_grid(int Lt);
// status[] = NOT_SELECTED / FIXED / "pending" per landmark (select[Lt], caller's numbering, or null: all; newOfOld: the internal order
// or null), then the wave and workgroup kernels decide every pending landmark and (no dry run) store the OK ones into g.Xw
void launch_triangulate(const TriangulateArgs& a, const uint8_t* select, const int* newOfOld, hipStream_t s);
// into the caller's numbering: statusOut[Lt] (a landmark still pending -- it has no edge -- as FEW_OBSERVATIONS), xyzOut[3 Lt] (xnew of an
// OK landmark, g.Xw of every other), counts[TRI_STATUSES] through
// parts[TRI_STATUSES * triangulate_collect_grid(Lt)]
void launch_triangulate_collect(const TriangulateArgs& a, const int* newOfOld, int* statusOut, double* xyzOut, long long* parts, long long* counts, hipStream_t s);

// ---- pose refinement with the landmarks held (ba_pose_refine.hip) ---------------------------------------------------------------------
// the statuses (include/cuba_hip.h: CUBA_HIP_POSEREF_*)
enum { POSEREF_OK = 0, POSEREF_NOT_SELECTED, POSEREF_FIXED, POSEREF_FEW_OBSERVATIONS, POSEREF_SINGULAR, POSEREF_FEW_INLIERS, POSEREF_STATUSES };
constexpr int POSEREF_MAX_ROUNDS = 4, POSEREF_MAX_ITERATIONS = 32;
struct PoseRefineArgs
{
	DeviceGraph g;                     // e_w: the LIVE information (a gated edge is out); rk: the handle's robust kernels
	const int *pe_beg = nullptr, *pe_end = nullptr, *pe_edge = nullptr;      // the pose pass's edge list per free pose
	int rounds = 0, iterations = 0;    // outlier rounds, LM trials per round (a fixed count)
	int robust_rounds = 0;             // the rounds below this one use g.rk, the later ones the identity kernel
	int min_inliers = 0;
	double chi2_mono = 0, chi2_stereo = 0;
	int dry_run = 0;                   // 1: g.q / g.t are left alone
	int* status = nullptr;             // [Pt] internal pose order (between the launches also the internal "pending" mark)
	int* inliers = nullptr;            // [Pt] internal order: edges in at the pose's last classification
	double* chi2 = nullptr;            // [Pt] internal order: sum omega |r|^2 over the final inliers (0 without a final classification)
	double* qt = nullptr;              // [7 Pt] internal order: q | t of an OK pose as the state holds it (others: not written)
	uint8_t* cls = nullptr;            // [E] sorted edges: this call's classification
};
int pose_refine_collect_grid(int Pt);
// status[] = NOT_SELECTED / FIXED / "pending" per pose (select[Pt], caller's numbering, or null: all; newOfOld[Pf]: the internal order of
// the free poses or null), cls[] = "live information > 0"; then one wave per pending pose runs all its rounds and (no dry run) stores it
void launch_pose_refine(const PoseRefineArgs& a, const uint8_t* select, const int* newOfOld, hipStream_t s);
// into the caller's numbering: statusOut[Pt], inliersOut[Pt], chi2Out[Pt], qOut[4 Pt] / tOut[3 Pt] (qt of an OK pose, g.q / g.t of every
// other), counts[POSEREF_STATUSES] through parts[POSEREF_STATUSES * pose_refine_collect_grid(Pt)]
void launch_pose_refine_collect(const PoseRefineArgs& a, const int* newOfOld, int* statusOut, int* inliersOut, double* chi2Out, double* qOut, double* tOut,
	long long* parts, long long* counts, hipStream_t s);

// ---- pose localisation from scratch: P3P RANSAC per pose (ba_localize.hip) -------------------------------------------------------------
// the statuses (include/cuba_hip.h: CUBA_HIP_POSELOC_*)
enum { POSELOC_OK = 0, POSELOC_NOT_SELECTED, POSELOC_FIXED, POSELOC_FEW_OBSERVATIONS, POSELOC_NO_SOLUTION, POSELOC_FEW_INLIERS, POSELOC_STATUSES };
constexpr int POSELOC_MAX_HYPOTHESES = 4096;
struct PoseLocalizeArgs
{
	DeviceGraph g;                     // e_w: the LIVE information (a gated edge is out); g.q / g.t are written, never read
	const int *pe_beg = nullptr, *pe_end = nullptr, *pe_edge = nullptr;      // the pose pass's edge list per free pose
	const uint32_t* perm = nullptr;    // [E] the caller's index of a sorted edge
	int hypotheses = 0;                // a fixed count
	unsigned long long seed = 0;
	int min_inliers = 0;
	double chi2_mono = 0, chi2_stereo = 0;
	int dry_run = 0;                   // 1: g.q / g.t are left alone
	int* status = nullptr;             // [Pt] internal pose order (between the launches also the internal "pending" mark)
	int* inliers = nullptr;            // [Pt] internal order
	int* winner = nullptr;             // [Pt] internal order: 4 h + root of an OK pose, -1 of every other
	unsigned long long* key = nullptr; // [Pt] internal order: the pose's seed word, hashed from (seed, the CALLER's pose index)
	double* cost = nullptr;            // [Pt] internal order: the winner's MSAC score (0 without a winner)
	double* qt = nullptr;              // [7 Pt] internal order: q | t of an OK pose as the state holds it (others: not written)
	uint8_t* cls = nullptr;            // [E] sorted edges: this call's classification
};
int pose_localize_collect_grid(int Pt);
// status[] = NOT_SELECTED / FIXED / "pending" and the seed word per pose (select[Pt], caller's numbering, or null: all; newOfOld[Pf]: the
// internal order of the free poses or null), cls[] = "live information > 0"; then one workgroup per pending pose, thread = hypothesis
void launch_pose_localize(const PoseLocalizeArgs& a, const uint8_t* select, const int* newOfOld, hipStream_t s);
// into the caller's numbering: statusOut[Pt], inliersOut[Pt], winnerOut[Pt], costOut[Pt], qOut[4 Pt] / tOut[3 Pt] (qt of an OK pose,
// g.q / g.t of every other), counts[POSELOC_STATUSES] through parts[POSELOC_STATUSES * pose_localize_collect_grid(Pt)]
void launch_pose_localize_collect(const PoseLocalizeArgs& a, const int* newOfOld, int* statusOut, int* inliersOut, int* winnerOut, double* costOut,
	double* qOut, double* tOut, long long* parts, long long* counts, hipStream_t s);

// copies {fail, iters, done} into sys.host_flags (what the last node of an iteration graph does anyway)
void launch_pcg_report(const DeviceSystem& sys, hipStream_t s);

}  // namespace cubahip
