// ba_factor.hip -- the factors besides the reprojection edges: terms rho(r^T Omega r) of the objective on the vertices alone, Omega a full
// symmetric information.  Two kinds on the SE(3) poses, r in the [omega, upsilon] tangent of the solver's left-multiplicative update
// T <- exp(d) T (pose_exp_update), Omega 6 x 6, one on the landmarks, one that ties a pose to a world position, one that ties its
// rotation to a world direction, one that ties it to a measured distance from a world point and one that ties two poses to a measured
// distance between them:
//
//   pose priors (cuba_hip_set_pose_priors): unary, r = log(T Tbar^-1), linearised with the exact derivative dr/dd =
//     J_l(r)^-1.  A prior touches the diagonal 6 x 6 block of its pose in the reduced matrix and the pose's entries of bp / bsc only.
//   relative-pose edges (cuba_hip_set_relative_pose_edges; section 7d): binary, r = log(T_j T_i^-1 Zbar^-1), dr/dd_j = J_l(r)^-1 and
//     dr/dd_i = -J_l(r)^-1 Ad(T_j T_i^-1).  Such an edge owns an off-diagonal block of the reduced matrix: the set of free-free pairs seeds
//     the block pattern (ba_setup.hip), and a pair that no landmark connects gets a block without Schur products, which only the kernels
//     below write.
//   landmark position priors (cuba_hip_set_landmark_priors; section 7f): unary on the free landmarks, r = X - Xbar, Omega 3 x 3 (g2o's
//     unary XYZ prior edge; the reference has no counterpart).  The Jacobian of r is the identity, so a prior's whole linearisation is
//     Hll += w Omega, bl -= w Omega r with w = rho'(r^T Omega r) (bl: the right-hand side of the landmark's rows, minus half the gradient).
//     Hll and bl of a landmark have one writer, the head lane of the landmark pass (ba_linearize.hip), and everything downstream -- the
//     3 x 3 inverse, the pose and block passes, back-substitution, the gain ratio's scale, the covariances -- reads them from sys.lm_sys.
//     So these priors are linearised INSIDE that pass (ba_device.hpp: add_landmark_priors, in kernel instantiations that only a handle
//     with such priors launches); this file holds their chi2 kernel and their host side.
//   position factors (cuba_hip_set_position_factors; section 7g): unary on the poses, r = R^T (a - t) - z: the world position of the point a
//     of the camera frame (the lever arm of a GNSS antenna, a prism, a marker; zero: the camera centre) against a measured world position
//     z, Omega 3 x 3.  r lives in a vector space, so dr/dd = [R^T [a]x | -R^T] (3 x 6, d = [omega; upsilon]) is exact to first order without a
//     J_l.  A factor touches the diagonal block of its pose and the pose's entries of bp / bsc only, as a pose prior.
//   direction factors (cuba_hip_set_direction_factors; section 7h): unary on the poses, r = R d - m: a world vector d (gravity, magnetic
//     north, a vanishing direction, a star) against the same vector as measured in the camera frame, Omega 3 x 3, rank 2 as a rule.  Under
//     the update R' = (I + [omega]x) R, so r' = r + omega x (R d) and dr/dd = [-[R d]x | 0] (3 x 6) -- NOT the body-frame -R [d]x, which
//     equals -[R d]x R.  The translation columns are exactly zero: a factor touches the rotation 3 x 3 of its pose's diagonal block and the
//     first three entries of the pose's bp / bsc, nothing else.
//   range factors (cuba_hip_set_range_factors; section 7i): unary on the poses, the first kind with a SCALAR, non-linear residual:
//     r = rho - rbar, rho = |u|, u = a - (R b + t): the distance of the point a of the camera frame (the lever arm of the ranging antenna;
//     zero: the camera centre) from the world point b (a UWB anchor, a beacon, a total station) against a measured range rbar; Omega the
//     scalar 1 / sigma^2.  With m = u / rho (camera frame) and b_c = R b + t, the update gives b_c' = b_c + omega x b_c + upsilon, so
//     d rho = -m . (omega x b_c + upsilon), and b_c x m = a x m: dr/dd = [(m x a)^T | -m^T] (1 x 6) -- NOT with the world-frame direction
//     R^T m, and the rotation columns vanish only for a = 0.  J^T J has rank 1.  THE POINT rho = 0 (the antenna at the anchor): m is undefined
//     there; the rule is m = 0 when the computed rho is exactly 0, so J = 0: the factor adds nothing to H or g and its e = Omega rbar^2.
//   range factors between two poses (cuba_hip_set_pose_range_factors; section 7j): binary, the scalar residual of the range factors with
//     the other end's point as the anchor: w_i = R_i^T (a_i - t_i), u = (a_j - t_j) - R_j w_i, rho = |u|, m_j = u / rho, m_i = -R_i R_j^T m_j
//     (both from the ONE computed u: one rho, one rule at rho = 0 for both ends), r = rho - rbar, dr/dd_j = [(m_j x a_j)^T | -m_j^T],
//     dr/dd_i = [(m_i x a_i)^T | -m_i^T].  The first binary kind with a low-rank term: rank-1 terms on both diagonal blocks and
//     w Omega J_i^T J_j on the pair's off-diagonal block; the free-free pairs seed the block pattern together with the edges' (the union).
//
// A factor may carry a robust kernel (cuba_hip_set_pose_factor_robust_kernels; section 7e): with e = r^T Omega r its term is rho(e) and its
// linearisation takes w Omega, w = rho'(e), for Omega (no second-order term, as the reprojection edges).  The kernels that see a
// residual are templates on ROBUST; a set without kernels has null kind / delta arrays and runs the `false` instantiations, which hold
// nothing of this.  A landmark prior always carries a kind (none = 0) and comes with its kernel in one call.
//
// Order: the six kinds on the poses add to the same diagonal blocks, bp and bsc by read-modify-write, in launches of their own in one
// stream; the order of those launches is part of the result.  It is written down once, with the rule for a new kind (it goes BEHIND the
// others), at launch_pose_factor_linearize (ba_kernels.hpp).
//
// The kinds keep linearisation kernels of their own (a prior is not run as a one-ended edge: its sums would be taken in another order).
// Everything else exists once: the device helpers below (the unary kinds' accumulators and their read-modify-write: zero_pose_sums,
// add_pose_sums), one chi2 kernel over a per-kind residual, one device layout and one upload for the four unary kinds on the poses
// (ba_kernels.hpp: DevicePoseGroups), and the same for the binary kinds (DevicePosePairs): the two of them are ONE path -- one sort, one
// upload, one gather kernel over a per-kind pair of terms, one launch helper -- with a linearisation kernel and a record layout each (90
// numbers of finished sums for an edge, 14 numbers {J_i, J_j, w Omega, w Omega r} for a range: not worth forcing into one); the host-side
// validation, sorting and read-back, and one interface (ba_kernels.hpp: DeviceFactors; ba_solver.hpp: the handle's table of its sets, and
// of the binary ones in launch order).  A new kind brings a residual, a Jacobian, a setter with its widths and nouns, and its entry there;
// a new binary kind also its record, block_term and pose_term.
//
//   prior_linearize_kernel     lane = free pose with priors: its priors in the caller's order, J^T Omega J / J^T Omega r summed in
//                              registers, then added to the pose's diagonal block (upper triangle), bp and (mode 1) bsc -- one writer per
//                              block, a launch of its own behind the Schur pass (which may still update a diagonal block the pose pass stored)
//   relpose_linearize_kernel   lane = edge: r, J_i, J_j and the edge's record {J_i^T Omega J_i, J_j^T Omega J_j (upper triangles),
//                              the cross term laid out as the block (min, max) of the internal pose pair stores it, J_i^T Omega r,
//                              J_j^T Omega r}
//   position_linearize_kernel  lane = free pose with position factors: the rotation matrix once, then the pose's factors in the caller's order,
//                              J^T (Omega J) (21 numbers) and J^T Omega r (6) summed in registers, one read-modify-write of the diagonal
//                              block's upper triangle, bp and (mode 1) bsc -- one writer per number; behind the priors' launch, ahead of the
//                              edges' launches
//   direction_linearize_kernel lane = free pose with direction factors: the rotation matrix once, then the pose's factors in the caller's order,
//                              [v]x^T Omega [v]x, v = R d (6 numbers) and v x (Omega r) (3) summed in registers, one read-modify-write of the
//                              upper triangle of the block's rotation 3 x 3, of bp[0..3) and (mode 1) bsc[0..3) -- one writer per number; the
//                              launch behind the edges' gather
//   range_linearize_kernel     lane = free pose with range factors: the rotation matrix once, then the pose's factors in the caller's order,
//                              w Omega J^T J (21 numbers, rank 1 per factor) and w Omega r J^T (6) summed in registers, one read-modify-write of
//                              the diagonal block's upper triangle, bp and (mode 1) bsc -- one writer per number; the launch behind the
//                              direction factors'
//   pose_range_linearize_kernel lane = range factor between poses with a free end: the record {J_i, J_j, w Omega, w Omega r}, 14 numbers
//   pair_gather_kernel<Kind>   lane = one number of the reduced system, for either binary kind: an entry of an off-diagonal block with such
//                              factors (mode 1: the sum of block_term over the block's factors -- an edge's stored cross term, a range's
//                              J_min[r] w Omega J_max[c]; stored whole where the block has neither Schur products nor a binary kind launched
//                              earlier, added to what those stored otherwise), or an entry of a pose's diagonal block (upper triangle) / of bp
//                              and (mode 1) bsc, the sum of pose_term over the pose's factors in the caller's order -- one writer per number,
//                              fixed order, no atomics; the launch behind the kind's records
//   factor_chi2_kernel         lane = factor of one kind: r^T Omega r at the current estimate (factor_chi, an overload per kind) into the per-factor
//                              output and (rho of it) into per-workgroup partials that the caller sums together with the reprojection
//                              edges' partials (fixed order, no atomics)
//
// Host side: the caller's seven sets (validated, kept in the caller's numbering), the binary kinds' pair set (part of the topology) and the upload
// of every set in the internal pose / landmark order.
#include "ba_solver.hpp"
#include "ba_device.hpp"
#include "ba_se3.hpp"

namespace cubahip
{

constexpr int PRIOR_LIN_BLOCK = 64;
constexpr int POS_LIN_BLOCK = 64;
constexpr int DIR_LIN_BLOCK = 64;
constexpr int RNG_LIN_BLOCK = 64;
constexpr int REL_LIN_BLOCK = 64;
constexpr int PRNG_LIN_BLOCK = 64;          // (tiny, latency-bound launches: the siblings' block size)
constexpr int PAIR_GATHER_BLOCK = 256;
constexpr int CHI_BLOCK = 256;
constexpr int CHI_MAX_GROUPS = 64;     // a chi2 launch's partials (a grid-stride loop beyond): they join the reprojection edges' partials
constexpr int POSE_NUMBERS = 27;       // what a factor adds to per free end: 21 entries of the diagonal block (upper triangle) + 6 of bp / bsc
// record of an edge: [0, 21) J_i^T Omega J_i, [21, 42) J_j^T Omega J_j (upper triangles, entry c (c + 1) / 2 + r), [42, 78) the cross block
// (column-major, rows = the pose of smaller internal index), [78, 84) J_i^T Omega r, [84, 90) J_j^T Omega r
constexpr int REL_HII = 0, REL_HJJ = 21, REL_HX = 42, REL_GI = 78, REL_GJ = 84;
static_assert(REL_GJ + 6 == REL_REC, "record layout");
// record of a range factor between two poses: [0, 6) J_i, [6, 12) J_j, w Omega, w Omega r
constexpr int PRNG_JI = 0, PRNG_JJ = 6, PRNG_W = 12, PRNG_WR = 13;
static_assert(PRNG_WR + 1 == PRNG_REC, "record layout");

// ---- shared device helpers --------------------------------------------------------------------------------------------------------

// pose `ip` of a [4 n] quaternion / [3 n] translation pair of arrays (the estimates, or a set's measurements)
__device__ __forceinline__ void load_pose(const Scalar* qs, const Scalar* ts, int ip, Scalar q[4], Scalar t[3])
{
#pragma unroll
	for (int i = 0; i < 4; i++) q[i] = qs[4 * (size_t)ip + i];
#pragma unroll
	for (int i = 0; i < 3; i++) t[i] = ts[3 * (size_t)ip + i];
}

// Omega r (Omega column-major) and r^T Omega r
__device__ __forceinline__ Scalar info_times(const Scalar* O, const Scalar r[6], Scalar Or[6])
{
#pragma unroll
	for (int i = 0; i < 6; i++) Or[i] = 0;
#pragma unroll
	for (int c = 0; c < 6; c++)
#pragma unroll
		for (int i = 0; i < 6; i++) Or[i] += O[6 * c + i] * r[c];
	Scalar chi = 0;
#pragma unroll
	for (int i = 0; i < 6; i++) chi += r[i] * Or[i];
	return chi;
}

// J = [[A, 0], [B, A]], or its negative
__device__ __forceinline__ void se3_jacobian(const Scalar A[3][3], const Scalar B[3][3], Scalar J[6][6], bool negative = false)
{
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int b = 0; b < 3; b++)
		{
			const Scalar x = negative ? -A[a][b] : A[a][b], y = negative ? -B[a][b] : B[a][b];
			J[a][b] = x; J[a][3 + b] = 0; J[3 + a][b] = y; J[3 + a][3 + b] = x;
		}
}

// (rho / rho' of a factor's robust kernel: factor_rho, factor_weight in ba_device.hpp -- the landmark priors share them)

// the lanes' chi2 sums of a CHI_BLOCK workgroup -> its partial
__device__ __forceinline__ void chi2_partial(Scalar acc, Scalar* __restrict__ parts)
{
	acc = wave_sum(acc);
	__shared__ Scalar part[CHI_BLOCK / WAVE];
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) parts[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// workgroups (= partials) of a chi2 launch over n factors
static int chi2_parts(int n) { return n > 0 ? std::min((n + CHI_BLOCK - 1) / CHI_BLOCK, CHI_MAX_GROUPS) : 0; }

// ---- what the kinds' kernels share --------------------------------------------------------------------------------------------------

// the sums of a lane of a unary kind's linearisation kernel over its pose's factors, in registers: J^T Omega J over the first D rows and
// columns of the pose's diagonal block (upper triangle, H[c (c + 1) / 2 + r] as the pose pass stores it) and J^T Omega r.  D = 6, or 3 for a
// kind whose translation columns are zero
template <int D>
__device__ __forceinline__ void zero_pose_sums(Scalar (&H)[D * (D + 1) / 2], Scalar (&gv)[D])
{
#pragma unroll
	for (int k = 0; k < D * (D + 1) / 2; k++) H[k] = 0;
#pragma unroll
	for (int k = 0; k < D; k++) gv[k] = 0;
}

// one read-modify-write of the block's upper triangle, of bp and (mode 1) bsc of internal pose ip -- one writer per number; what lies beyond
// D is not touched
template <int D>
__device__ __forceinline__ void add_pose_sums(const DeviceStructure& st, const DeviceSystem& sys, int ip, int mode, const Scalar (&H)[D * (D + 1) / 2], const Scalar (&gv)[D])
{
	Scalar* blk = sys.hsc + 36 * (size_t)st.hsc_rowptr[ip];
#pragma unroll
	for (int c = 0; c < D; c++)
	{
#pragma unroll
		for (int rr = 0; rr <= c; rr++) blk[c * 6 + rr] += H[c * (c + 1) / 2 + rr];
		sys.bp[6 * (size_t)ip + c] -= gv[c];
		if (mode == 1) sys.bsc[6 * (size_t)ip + c] -= gv[c];
	}
}

// number `el` of the record of factor k of a binary kind: the records are stored number-major (all factors' number 0, then number 1, ...),
// so that the lanes of the linearisation -- consecutive factors -- store to consecutive addresses
__device__ __forceinline__ Scalar& pair_rec(const DevicePosePairs& f, int k, int el) { return f.rec[(size_t)el * f.n + k]; }

// ---- pose priors ------------------------------------------------------------------------------------------------------------------

template <bool ROBUST>
__global__ __launch_bounds__(PRIOR_LIN_BLOCK) void prior_linearize_kernel(DeviceGraph g, DeviceStructure st, DeviceSystem sys, DevicePriors pr, int mode)
{
	const int i = blockIdx.x * PRIOR_LIN_BLOCK + threadIdx.x;
	if (i >= pr.nPoses) return;
	const int ip = pr.pose_id[i];
	Scalar q[4], t[3];
	load_pose(g.q, g.t, ip, q, t);
	Scalar H[21], gv[6];
	zero_pose_sums<6>(H, gv);
	const int k1 = pr.pose_ptr[i + 1];
	for (int k = pr.pose_ptr[i]; k < k1; k++)
	{
		Scalar qb[4], tb[3], r[6], A[3][3], B[3][3], J[6][6];
		load_pose(pr.qbar, pr.tbar, k, qb, tb);
		prior_residual(q, t, qb, tb, r, A);
		prior_jacobian_b(r, A, B);
		se3_jacobian(A, B, J);
		const Scalar* O = pr.info + 36 * (size_t)k;
		Scalar Or[6];
		Scalar w = 1;
		if constexpr (ROBUST)
		{
			const Scalar e = info_times(O, r, Or);
			w = factor_weight(pr.rk_kind[k], pr.rk_delta[k], e);
		}
		// H += J^T (Omega J), column by column (upper triangle, acc[c (c + 1) / 2 + r] as the pose pass stores it)
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			Scalar oj[6];
#pragma unroll
			for (int a = 0; a < 6; a++) oj[a] = 0;
#pragma unroll
			for (int m = 0; m < 6; m++)
#pragma unroll
				for (int a = 0; a < 6; a++) oj[a] += O[6 * m + a] * J[m][c];
#pragma unroll
			for (int rr = 0; rr <= c; rr++)
			{
				Scalar s = 0;
#pragma unroll
				for (int a = 0; a < 6; a++) s += J[a][rr] * oj[a];
				if constexpr (ROBUST) H[c * (c + 1) / 2 + rr] += w * s;
				else H[c * (c + 1) / 2 + rr] += s;
			}
		}
		if constexpr (!ROBUST) (void)info_times(O, r, Or);
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			Scalar s = 0;
#pragma unroll
			for (int a = 0; a < 6; a++) s += J[a][c] * Or[a];
			if constexpr (ROBUST) gv[c] += w * s;
			else gv[c] += s;
		}
	}
	add_pose_sums<6>(st, sys, ip, mode, H, gv);
}

// r^T Omega r of prior k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DevicePriors& pr, int k)
{
	const int ip = pr.pose[k];
	if (ip >= g.Pf) return 0;
	Scalar q[4], t[3], qb[4], tb[3], r[6], A[3][3], Or[6];
	load_pose(g.q, g.t, ip, q, t);
	load_pose(pr.qbar, pr.tbar, k, qb, tb);
	prior_residual(q, t, qb, tb, r, A);
	return info_times(pr.info + 36 * (size_t)k, r, Or);
}

// ---- relative-pose edges ----------------------------------------------------------------------------------------------------------

// Hamilton product of (x, y, z, w) quaternions
__device__ __forceinline__ void quat_mul(const Scalar a[4], const Scalar b[4], Scalar o[4])
{
	o[0] = a[3] * b[0] + b[3] * a[0] + (a[1] * b[2] - a[2] * b[1]);
	o[1] = a[3] * b[1] + b[3] * a[1] + (a[2] * b[0] - a[0] * b[2]);
	o[2] = a[3] * b[2] + b[3] * a[2] + (a[0] * b[1] - a[1] * b[0]);
	o[3] = a[3] * b[3] - (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

struct RelEnds { Scalar qi[4], ti[3], qj[4], tj[3]; };

__device__ __forceinline__ void load_rel_ends(const DeviceGraph& g, const DeviceRelPoses& rp, int k, RelEnds& e)
{
	load_pose(g.q, g.t, rp.pose_i[k], e.qi, e.ti);
	load_pose(g.q, g.t, rp.pose_j[k], e.qj, e.tj);
}

// r = log(T_j T_i^-1 Zbar^-1) = log(T_j (Zbar T_i)^-1): the priors' residual of pose j against Zbar T_i; A = J_w^-1
__device__ __forceinline__ void rel_residual(const RelEnds& e, const DeviceRelPoses& rp, int k, Scalar r[6], Scalar A[3][3])
{
	Scalar qz[4], tz[3], qb[4], tb[3];
	load_pose(rp.q, rp.t, k, qz, tz);
	quat_mul(qz, e.qi, qb);
	quat_rotate(qz, e.ti, tb);
	tb[0] += tz[0]; tb[1] += tz[1]; tb[2] += tz[2];
	prior_residual(e.qj, e.tj, qb, tb, r, A);
}

template <bool ROBUST>
__global__ __launch_bounds__(REL_LIN_BLOCK) void relpose_linearize_kernel(DeviceGraph g, DeviceRelPoses rp)
{
	const int k = blockIdx.x * REL_LIN_BLOCK + threadIdx.x;
	if (k >= rp.nActive) return;
	RelEnds e;
	load_rel_ends(g, rp, k, e);
	Scalar r[6], A[3][3], B[3][3];
	rel_residual(e, rp, k, r, A);
	prior_jacobian_b(r, A, B);
	// M = T_j T_i^-1 = [R_M | t_M]
	Scalar qc[4] = { -e.qi[0], -e.qi[1], -e.qi[2], e.qi[3] }, qm[4], tM[3];
	quat_mul(e.qj, qc, qm);
	const Scalar inv = 1 / sqrt(qm[0] * qm[0] + qm[1] * qm[1] + qm[2] * qm[2] + qm[3] * qm[3]);
#pragma unroll
	for (int x = 0; x < 4; x++) qm[x] *= inv;
	const Rot3 RM = quat_to_rot(qm[0], qm[1], qm[2], qm[3]);
	quat_rotate(qm, e.ti, tM);
	tM[0] = e.tj[0] - tM[0]; tM[1] = e.tj[1] - tM[1]; tM[2] = e.tj[2] - tM[2];
	// J_j = [[A, 0], [B, A]],  J_i = -J_j Ad(M) = [[X, 0], [Y, X]],  X = -A R_M,  Y = -(B R_M + A [t_M]x R_M)
	Scalar TM[3][3], TR[3][3], X[3][3], Y[3][3], BR[3][3], ATR[3][3];
	hat3(tM, TM);
	mul3(TM, RM.m, TR);
	mul3(A, RM.m, X);
	mul3(B, RM.m, BR);
	mul3(A, TR, ATR);
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int b = 0; b < 3; b++) Y[a][b] = BR[a][b] + ATR[a][b];
	Scalar Ji[6][6], Jj[6][6];
	se3_jacobian(A, B, Jj);
	se3_jacobian(X, Y, Ji, true);
	const Scalar* O = rp.info + 36 * (size_t)k;
	Scalar Or[6];
	Scalar w = 1;
	if constexpr (ROBUST)
	{
		const Scalar e = info_times(O, r, Or);
		w = factor_weight(rp.rk_kind[k], rp.rk_delta[k], e);
	}
	// the cross term J_i^T Omega J_j is the block (i, j); the block pattern stores (min, max) of the internal indices: transposed if i > j
	const bool flip = rp.pose_i[k] > rp.pose_j[k];
#pragma unroll
	for (int c = 0; c < 6; c++)
	{
		Scalar oi[6], oj[6];
#pragma unroll
		for (int a = 0; a < 6; a++) { oi[a] = 0; oj[a] = 0; }
#pragma unroll
		for (int m = 0; m < 6; m++)
#pragma unroll
			for (int a = 0; a < 6; a++) { oi[a] += O[6 * m + a] * Ji[m][c]; oj[a] += O[6 * m + a] * Jj[m][c]; }
#pragma unroll
		for (int rr = 0; rr < 6; rr++)
		{
			Scalar sii = 0, sjj = 0, sx = 0;
#pragma unroll
			for (int a = 0; a < 6; a++) { sii += Ji[a][rr] * oi[a]; sjj += Jj[a][rr] * oj[a]; sx += Ji[a][rr] * oj[a]; }
			if constexpr (ROBUST) { sii *= w; sjj *= w; sx *= w; }
			if (rr <= c) { pair_rec(rp, k, REL_HII + c * (c + 1) / 2 + rr) = sii; pair_rec(rp, k, REL_HJJ + c * (c + 1) / 2 + rr) = sjj; }
			pair_rec(rp, k, REL_HX + (flip ? rr * 6 + c : c * 6 + rr)) = sx;
		}
	}
	if constexpr (!ROBUST) (void)info_times(O, r, Or);
#pragma unroll
	for (int c = 0; c < 6; c++)
	{
		Scalar si = 0, sj = 0;
#pragma unroll
		for (int a = 0; a < 6; a++) { si += Ji[a][c] * Or[a]; sj += Jj[a][c] * Or[a]; }
		if constexpr (ROBUST) { si *= w; sj *= w; }
		pair_rec(rp, k, REL_GI + c) = si; pair_rec(rp, k, REL_GJ + c) = sj;
	}
}

// what pair_gather_kernel sums: entry el (column-major) of the cross block of edge k as the pattern stores it, and entry el of what the
// edge adds to the pose at its end `side` (el < 21: the diagonal block's packed upper triangle, else bp / bsc) -- stored numbers both
__device__ __forceinline__ Scalar block_term(const DeviceRelPoses& rp, int k, int el) { return pair_rec(rp, k, REL_HX + el); }
__device__ __forceinline__ Scalar pose_term(const DeviceRelPoses& rp, int k, int side, int el, int, int)
{
	return pair_rec(rp, k, el < 21 ? (side ? REL_HJJ : REL_HII) + el : (side ? REL_GJ : REL_GI) + (el - 21));
}

// r^T Omega r of edge k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DeviceRelPoses& rp, int k)
{
	if (k >= rp.nActive) return 0;
	RelEnds e;
	load_rel_ends(g, rp, k, e);
	Scalar r[6], A[3][3], Or[6];
	rel_residual(e, rp, k, r, A);
	return info_times(rp.info + 36 * (size_t)k, r, Or);
}

// ---- landmark priors --------------------------------------------------------------------------------------------------------------

// r^T Omega r of prior k at the current estimate (factor_chi2_kernel; the landmark pass linearises these priors)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DeviceLandmarkPriors& lp, int k)
{
	const int il = lp.lm[k];
	if (il >= g.Lf) return 0;
	const Scalar X[3] = { g.Xw[3 * (size_t)il], g.Xw[3 * (size_t)il + 1], g.Xw[3 * (size_t)il + 2] };
	Scalar Or[3];
	return landmark_prior_residual(lp, k, X, Or);
}

// ---- position factors -------------------------------------------------------------------------------------------------------------

// r = R^T (a - t) - z of factor k at the pose [R | t] (R row-major in Rm), Or = Omega r; returns r^T Omega r
__device__ __forceinline__ Scalar position_residual(const DevicePositionFactors& pp, int k, const Scalar Rm[3][3], const Scalar t[3], Scalar r[3], Scalar Or[3])
{
	const Scalar* a = pp.arm + 3 * (size_t)k;
	const Scalar* z = pp.z + 3 * (size_t)k;
	const Scalar* O = pp.info + 9 * (size_t)k;
	const Scalar d[3] = { a[0] - t[0], a[1] - t[1], a[2] - t[2] };
#pragma unroll
	for (int i = 0; i < 3; i++) r[i] = (Rm[0][i] * d[0] + Rm[1][i] * d[1] + Rm[2][i] * d[2]) - z[i];
#pragma unroll
	for (int i = 0; i < 3; i++) Or[i] = O[i] * r[0] + O[3 + i] * r[1] + O[6 + i] * r[2];
	return r[0] * Or[0] + r[1] * Or[1] + r[2] * Or[2];
}

template <bool ROBUST>
__global__ __launch_bounds__(POS_LIN_BLOCK) void position_linearize_kernel(DeviceGraph g, DeviceStructure st, DeviceSystem sys, DevicePositionFactors pp, int mode)
{
	const int i = blockIdx.x * POS_LIN_BLOCK + threadIdx.x;
	if (i >= pp.nPoses) return;
	const int ip = pp.pose_id[i];
	Scalar q[4], t[3];
	load_pose(g.q, g.t, ip, q, t);
	const Rot3 R = quat_to_rot(q[0], q[1], q[2], q[3]);
	Scalar H[21], gv[6];
	zero_pose_sums<6>(H, gv);
	const int k1 = pp.pose_ptr[i + 1];
	for (int k = pp.pose_ptr[i]; k < k1; k++)
	{
		Scalar r[3], Or[3];
		const Scalar e = position_residual(pp, k, R.m, t, r, Or);
		Scalar w = 1;
		if constexpr (ROBUST) w = factor_weight(pp.rk_kind[k], pp.rk_delta[k], e);
		// J = [R^T [a]x | -R^T] (3 x 6)
		const Scalar* a = pp.arm + 3 * (size_t)k;
		Scalar Ax[3][3], J[3][6];
		hat3(a, Ax);
#pragma unroll
		for (int m = 0; m < 3; m++)
#pragma unroll
			for (int c = 0; c < 3; c++)
			{
				J[m][c] = R.m[0][m] * Ax[0][c] + R.m[1][m] * Ax[1][c] + R.m[2][m] * Ax[2][c];
				J[m][3 + c] = -R.m[c][m];
			}
		const Scalar* O = pp.info + 9 * (size_t)k;
		// H += J^T (Omega J), column by column (upper triangle, H[c (c + 1) / 2 + r] as the pose pass stores it); gv += J^T (Omega r)
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			Scalar oj[3];
#pragma unroll
			for (int x = 0; x < 3; x++) oj[x] = O[x] * J[0][c] + O[3 + x] * J[1][c] + O[6 + x] * J[2][c];
#pragma unroll
			for (int rr = 0; rr <= c; rr++)
			{
				const Scalar s = J[0][rr] * oj[0] + J[1][rr] * oj[1] + J[2][rr] * oj[2];
				if constexpr (ROBUST) H[c * (c + 1) / 2 + rr] += w * s;
				else H[c * (c + 1) / 2 + rr] += s;
			}
			const Scalar s = J[0][c] * Or[0] + J[1][c] * Or[1] + J[2][c] * Or[2];
			if constexpr (ROBUST) gv[c] += w * s;
			else gv[c] += s;
		}
	}
	add_pose_sums<6>(st, sys, ip, mode, H, gv);
}

// r^T Omega r of factor k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DevicePositionFactors& pp, int k)
{
	const int ip = pp.pose[k];
	if (ip >= g.Pf) return 0;
	Scalar q[4], t[3], r[3], Or[3];
	load_pose(g.q, g.t, ip, q, t);
	const Rot3 R = quat_to_rot(q[0], q[1], q[2], q[3]);
	return position_residual(pp, k, R.m, t, r, Or);
}

// ---- direction factors ------------------------------------------------------------------------------------------------------------

// v = R d and r = v - m of factor k at the rotation R (row-major in Rm), Or = Omega r; returns r^T Omega r
__device__ __forceinline__ Scalar direction_residual(const DeviceDirectionFactors& df, int k, const Scalar Rm[3][3], Scalar v[3], Scalar Or[3])
{
	const Scalar* d = df.d + 3 * (size_t)k;
	const Scalar* m = df.m + 3 * (size_t)k;
	const Scalar* O = df.info + 9 * (size_t)k;
	Scalar r[3];
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
		v[i] = Rm[i][0] * d[0] + Rm[i][1] * d[1] + Rm[i][2] * d[2];
		r[i] = v[i] - m[i];
	}
#pragma unroll
	for (int i = 0; i < 3; i++) Or[i] = O[i] * r[0] + O[3 + i] * r[1] + O[6 + i] * r[2];
	return r[0] * Or[0] + r[1] * Or[1] + r[2] * Or[2];
}

template <bool ROBUST>
__global__ __launch_bounds__(DIR_LIN_BLOCK) void direction_linearize_kernel(DeviceGraph g, DeviceStructure st, DeviceSystem sys, DeviceDirectionFactors df, int mode)
{
	const int i = blockIdx.x * DIR_LIN_BLOCK + threadIdx.x;
	if (i >= df.nPoses) return;
	const int ip = df.pose_id[i];
	const Scalar* q = g.q + 4 * (size_t)ip;
	const Rot3 R = quat_to_rot(q[0], q[1], q[2], q[3]);
	Scalar H[6], gv[3];
	zero_pose_sums<3>(H, gv);
	const int k1 = df.pose_ptr[i + 1];
	for (int k = df.pose_ptr[i]; k < k1; k++)
	{
		Scalar v[3], Or[3];
		const Scalar e = direction_residual(df, k, R.m, v, Or);
		Scalar w = 1;
		if constexpr (ROBUST) w = factor_weight(df.rk_kind[k], df.rk_delta[k], e);
		// J = [-[v]x | 0]: J^T Omega J = [v]x^T (Omega [v]x), column by column (upper triangle, H[c (c + 1) / 2 + r]); J^T Omega r = v x (Omega r)
		Scalar V[3][3];
		hat3(v, V);
		const Scalar* O = df.info + 9 * (size_t)k;
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			Scalar ov[3];
#pragma unroll
			for (int x = 0; x < 3; x++) ov[x] = O[x] * V[0][c] + O[3 + x] * V[1][c] + O[6 + x] * V[2][c];
#pragma unroll
			for (int rr = 0; rr <= c; rr++)
			{
				const Scalar s = V[0][rr] * ov[0] + V[1][rr] * ov[1] + V[2][rr] * ov[2];
				if constexpr (ROBUST) H[c * (c + 1) / 2 + rr] += w * s;
				else H[c * (c + 1) / 2 + rr] += s;
			}
		}
		const Scalar x[3] = { v[1] * Or[2] - v[2] * Or[1], v[2] * Or[0] - v[0] * Or[2], v[0] * Or[1] - v[1] * Or[0] };
#pragma unroll
		for (int c = 0; c < 3; c++)
		{
			if constexpr (ROBUST) gv[c] += w * x[c];
			else gv[c] += x[c];
		}
	}
	// (the translation rows and columns of the block, bp[3..6) and bsc[3..6) are not this kind's: add_pose_sums<3> does not touch them)
	add_pose_sums<3>(st, sys, ip, mode, H, gv);
}

// r^T Omega r of factor k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DeviceDirectionFactors& df, int k)
{
	const int ip = df.pose[k];
	if (ip >= g.Pf) return 0;
	const Scalar* q = g.q + 4 * (size_t)ip;
	const Rot3 R = quat_to_rot(q[0], q[1], q[2], q[3]);
	Scalar v[3], Or[3];
	return direction_residual(df, k, R.m, v, Or);
}

// ---- range factors ----------------------------------------------------------------------------------------------------------------

// u = (a - t) - R b, rho = |u| and r = rho - rbar of factor k at the pose [R | t] (R row-major in Rm); m = u / rho, the unit vector from the
// anchor to the antenna in the camera frame.  THE POINT rho = 0 (the antenna at the anchor): there m is undefined, and 0 / 0 would put NaN
// into the system.  The rule: when the computed rho is exactly 0, m = 0 -- so J = 0, the factor adds nothing to H or g, and its
// e = info rbar^2.  Returns e = info r^2
__device__ __forceinline__ Scalar range_residual(const DeviceRangeFactors& rf, int k, const Scalar Rm[3][3], const Scalar t[3], Scalar m[3], Scalar& r)
{
	const Scalar* a = rf.arm + 3 * (size_t)k;
	const Scalar* b = rf.br + 4 * (size_t)k;
	Scalar u[3];
#pragma unroll
	for (int i = 0; i < 3; i++) u[i] = (a[i] - t[i]) - (Rm[i][0] * b[0] + Rm[i][1] * b[1] + Rm[i][2] * b[2]);
	const Scalar rho = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
	const Scalar inv = rho > 0 ? 1 / rho : 0;
#pragma unroll
	for (int i = 0; i < 3; i++) m[i] = u[i] * inv;
	r = rho - b[3];
	return rf.info[k] * r * r;
}

template <bool ROBUST>
__global__ __launch_bounds__(RNG_LIN_BLOCK) void range_linearize_kernel(DeviceGraph g, DeviceStructure st, DeviceSystem sys, DeviceRangeFactors rf, int mode)
{
	const int i = blockIdx.x * RNG_LIN_BLOCK + threadIdx.x;
	if (i >= rf.nPoses) return;
	const int ip = rf.pose_id[i];
	Scalar q[4], t[3];
	load_pose(g.q, g.t, ip, q, t);
	const Rot3 R = quat_to_rot(q[0], q[1], q[2], q[3]);
	Scalar H[21], gv[6];
	zero_pose_sums<6>(H, gv);
	const int k1 = rf.pose_ptr[i + 1];
	for (int k = rf.pose_ptr[i]; k < k1; k++)
	{
		Scalar m[3], r;
		const Scalar e = range_residual(rf, k, R.m, t, m, r);
		Scalar w = rf.info[k];
		if constexpr (ROBUST) w *= factor_weight(rf.rk_kind[k], rf.rk_delta[k], e);
		// J = [(m x a)^T | -m^T] (1 x 6; all zero at rho = 0): H += w info J^T J (upper triangle, H[c (c + 1) / 2 + r]), gv += w info r J^T
		const Scalar* a = rf.arm + 3 * (size_t)k;
		const Scalar J[6] = { m[1] * a[2] - m[2] * a[1], m[2] * a[0] - m[0] * a[2], m[0] * a[1] - m[1] * a[0], -m[0], -m[1], -m[2] };
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			const Scalar wj = w * J[c];
#pragma unroll
			for (int rr = 0; rr <= c; rr++) H[c * (c + 1) / 2 + rr] += J[rr] * wj;
			gv[c] += wj * r;
		}
	}
	add_pose_sums<6>(st, sys, ip, mode, H, gv);
}

// info r^2 of factor k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DeviceRangeFactors& rf, int k)
{
	const int ip = rf.pose[k];
	if (ip >= g.Pf) return 0;
	Scalar q[4], t[3], m[3], r;
	load_pose(g.q, g.t, ip, q, t);
	const Rot3 R = quat_to_rot(q[0], q[1], q[2], q[3]);
	return range_residual(rf, k, R.m, t, m, r);
}

// ---- range factors between two poses ----------------------------------------------------------------------------------------------

// w_i = R_i^T (a_i - t_i), the world position of the point on pose i; u = (a_j - t_j) - R_j w_i: the unary range factor on pose j with the
// anchor w_i; rho = |u|, r = rho - rbar, mj = u / rho (frame j) and mi = -R_i R_j^T mj (frame i) -- from the ONE computed u, so that rho
// and the rule at rho = 0 (range_residual: mi = mj = 0, e = info rbar^2) are the same for both ends.  Returns e = info r^2
__device__ __forceinline__ Scalar pose_range_residual(const DeviceGraph& g, const DevicePoseRanges& pr, int k, Scalar mi[3], Scalar mj[3], Scalar& r)
{
	Scalar qi[4], ti[3], qj[4], tj[3];
	load_pose(g.q, g.t, pr.pose_i[k], qi, ti);
	load_pose(g.q, g.t, pr.pose_j[k], qj, tj);
	const Rot3 Ri = quat_to_rot(qi[0], qi[1], qi[2], qi[3]);
	const Rot3 Rj = quat_to_rot(qj[0], qj[1], qj[2], qj[3]);
	const Scalar* ai = pr.arm_i + 3 * (size_t)k;
	const Scalar* aj = pr.arm_j + 3 * (size_t)k;
	const Scalar d[3] = { ai[0] - ti[0], ai[1] - ti[1], ai[2] - ti[2] };
	Scalar w[3], u[3], v[3];
#pragma unroll
	for (int i = 0; i < 3; i++) w[i] = Ri.m[0][i] * d[0] + Ri.m[1][i] * d[1] + Ri.m[2][i] * d[2];
#pragma unroll
	for (int i = 0; i < 3; i++) u[i] = (aj[i] - tj[i]) - (Rj.m[i][0] * w[0] + Rj.m[i][1] * w[1] + Rj.m[i][2] * w[2]);
	const Scalar rho = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
	const Scalar inv = rho > 0 ? 1 / rho : 0;
#pragma unroll
	for (int i = 0; i < 3; i++) mj[i] = u[i] * inv;
#pragma unroll
	for (int i = 0; i < 3; i++) v[i] = Rj.m[0][i] * mj[0] + Rj.m[1][i] * mj[1] + Rj.m[2][i] * mj[2];
#pragma unroll
	for (int i = 0; i < 3; i++) mi[i] = -(Ri.m[i][0] * v[0] + Ri.m[i][1] * v[1] + Ri.m[i][2] * v[2]);
	r = rho - pr.range[k];
	return pr.info[k] * r * r;
}

template <bool ROBUST>
__global__ __launch_bounds__(PRNG_LIN_BLOCK) void pose_range_linearize_kernel(DeviceGraph g, DevicePoseRanges pr)
{
	const int k = blockIdx.x * PRNG_LIN_BLOCK + threadIdx.x;
	if (k >= pr.nActive) return;
	Scalar mi[3], mj[3], r;
	const Scalar e = pose_range_residual(g, pr, k, mi, mj, r);
	Scalar w = pr.info[k];
	if constexpr (ROBUST) w *= factor_weight(pr.rk_kind[k], pr.rk_delta[k], e);
	// J_i = [(m_i x a_i)^T | -m_i^T], J_j = [(m_j x a_j)^T | -m_j^T] (1 x 6 each; all zero at rho = 0)
	const Scalar* ai = pr.arm_i + 3 * (size_t)k;
	const Scalar* aj = pr.arm_j + 3 * (size_t)k;
	const Scalar J[12] = { mi[1] * ai[2] - mi[2] * ai[1], mi[2] * ai[0] - mi[0] * ai[2], mi[0] * ai[1] - mi[1] * ai[0], -mi[0], -mi[1], -mi[2],
		mj[1] * aj[2] - mj[2] * aj[1], mj[2] * aj[0] - mj[0] * aj[2], mj[0] * aj[1] - mj[1] * aj[0], -mj[0], -mj[1], -mj[2] };
#pragma unroll
	for (int c = 0; c < 12; c++) pair_rec(pr, k, PRNG_JI + c) = J[c];
	pair_rec(pr, k, PRNG_W) = w;
	pair_rec(pr, k, PRNG_WR) = w * r;
}

// what pair_gather_kernel sums: entry el = (rr, c), column-major, of the block (min, max) of the internal pair, J_min[rr] w Omega J_max[c],
// and entry el of what the factor adds to the pose at its end `side`: J[rr] w Omega J[c] (el < 21: (rr, c) of the upper triangle), else
// J[c] w Omega r -- products of the record's numbers
__device__ __forceinline__ Scalar block_term(const DevicePoseRanges& pr, int k, int el)
{
	const int c = el / 6, rr = el - 6 * c;
	const bool flip = pr.pose_i[k] > pr.pose_j[k];
	return pair_rec(pr, k, (flip ? PRNG_JJ : PRNG_JI) + rr) * (pair_rec(pr, k, PRNG_W) * pair_rec(pr, k, (flip ? PRNG_JI : PRNG_JJ) + c));
}
__device__ __forceinline__ Scalar pose_term(const DevicePoseRanges& pr, int k, int side, int el, int rr, int c)
{
	const int J = side ? PRNG_JJ : PRNG_JI;
	if (el < 21) return pair_rec(pr, k, J + rr) * (pair_rec(pr, k, PRNG_W) * pair_rec(pr, k, J + c));
	return pair_rec(pr, k, J + c) * pair_rec(pr, k, PRNG_WR);
}

// info r^2 of factor k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DevicePoseRanges& pr, int k)
{
	if (k >= pr.nActive) return 0;
	Scalar mi[3], mj[3], r;
	return pose_range_residual(g, pr, k, mi, mj, r);
}

// ---- the binary kinds' gather -----------------------------------------------------------------------------------------------------

// The sums of a binary kind's records into the reduced system: lane = one number of it -- in mode 1 first the 36 entries of every
// off-diagonal block with such factors (block_term over the block's factors), then POSE_NUMBERS per free pose with such factors: the upper
// triangle of its diagonal block, bp and (mode 1) bsc (pose_term over the pose's items, in the caller's order).  One writer per number,
// fixed order, no atomics.  block_term / pose_term: an overload per kind next to its record layout
template <class Kind>
__global__ __launch_bounds__(PAIR_GATHER_BLOCK) void pair_gather_kernel(DeviceStructure st, DeviceSystem sys, Kind f, int mode)
{
	const int x = blockIdx.x * PAIR_GATHER_BLOCK + threadIdx.x;
	const int nBlkNumbers = mode == 1 ? 36 * f.nBlocks : 0;
	if (x < nBlkNumbers)
	{
		const int b = x / 36, el = x - 36 * b;
		const int blk = f.blk_id[b];
		Scalar s = 0;
		const int k1 = f.blk_ptr[b + 1];
		for (int k = f.blk_ptr[b]; k < k1; k++) s += block_term(f, k, el);
		Scalar* dst = sys.hsc + 36 * (size_t)blk + el;
		// (a block with products was stored by the Schur pass of this linearisation, a shared one by an earlier binary kind's gather; a block
		// with neither has no other writer and is cleared by no one: store)
		*dst = st.prod_end[blk] > st.prod_beg[blk] || f.blk_shared[b] ? *dst + s : s;
		return;
	}
	const int y = x - nBlkNumbers;
	const int p = y / POSE_NUMBERS, el = y - POSE_NUMBERS * p;
	if (p >= f.nPoses) return;
	const int ip = f.pose_id[p];
	// packed upper-triangle index -> (rr, c); el >= 21: entry c of bp / bsc
	int c = el - 21, rr = 0;
	if (el < 21)
	{
		c = 0;
		while ((c + 1) * (c + 2) / 2 <= el) c++;
		rr = el - c * (c + 1) / 2;
	}
	Scalar s = 0;
	const int k1 = f.pose_ptr[p + 1];
	for (int k = f.pose_ptr[p]; k < k1; k++)
	{
		const int item = f.pose_item[k];
		s += pose_term(f, item >> 1, item & 1, el, rr, c);
	}
	if (el < 21) sys.hsc[36 * (size_t)st.hsc_rowptr[ip] + c * 6 + rr] += s;
	else
	{
		sys.bp[6 * (size_t)ip + c] -= s;
		if (mode == 1) sys.bsc[6 * (size_t)ip + c] -= s;
	}
}

// ---- chi2 -------------------------------------------------------------------------------------------------------------------------

// The chi2 of a kind: lane = factor, r^T Omega r at the current estimate -- factor_chi(g, kind, k), one overload per kind above, 0 for a factor
// on a fixed vertex -- into the per-factor output and (rho of it) into per-workgroup partials that the caller sums together with the
// reprojection edges' partials (fixed order, no atomics)
template <class Kind, bool ROBUST>
__global__ __launch_bounds__(CHI_BLOCK) void factor_chi2_kernel(DeviceGraph g, Kind f, Scalar* __restrict__ parts)
{
	Scalar acc = 0;
	for (int k = blockIdx.x * CHI_BLOCK + threadIdx.x; k < f.n; k += gridDim.x * CHI_BLOCK)
	{
		const Scalar chi = factor_chi(g, f, k);
		f.chi[k] = chi;
		if constexpr (ROBUST) acc += factor_rho(f.rk_kind[k], f.rk_delta[k], chi);
		else acc += chi;
	}
	chi2_partial(acc, parts);
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------

// (a landmark prior always carries a kind: that kind has no ROBUST = false instantiation)
template <class Kind> constexpr bool ALWAYS_ROBUST = std::is_same<Kind, DeviceLandmarkPriors>::value;

// the chi2 launch of one kind; returns its workgroups (= partials)
template <class Kind>
static int launch_chi2(const DeviceGraph& g, const Kind& f, Scalar* parts, hipStream_t s)
{
	const int grid = chi2_parts(f.n);
	if (grid <= 0) return 0;
	if (ALWAYS_ROBUST<Kind> || f.rk_kind) hipLaunchKernelGGL((factor_chi2_kernel<Kind, true>), dim3(grid), dim3(CHI_BLOCK), 0, s, g, f, parts);
	else if constexpr (!ALWAYS_ROBUST<Kind>) hipLaunchKernelGGL((factor_chi2_kernel<Kind, false>), dim3(grid), dim3(CHI_BLOCK), 0, s, g, f, parts);
	return grid;
}

int factor_chi2_parts(const DeviceFactors* pf)
{
	int parts = 0;
	if (pf) pf->each([&](const auto& f) { parts += chi2_parts(f.n); });
	return parts;
}

void launch_factor_chi2(const DeviceGraph& g, const DeviceFactors& pf, Scalar* parts, hipStream_t s, int only)
{
	int kind = 0, offset = 0;
	pf.each([&](const auto& f) {
		if (only < 0) offset += launch_chi2(g, f, parts + offset, s);
		else if (only == kind) launch_chi2(g, f, parts, s);
		kind++;
	});
}

// a unary kind's launch: lane = free pose with such factors; `plain` / `robust`: the kind's kernel without / with robust kernels
template <class Kind>
using UnaryKernel = void (*)(DeviceGraph, DeviceStructure, DeviceSystem, Kind, int);
template <class Kind>
static void launch_unary(UnaryKernel<Kind> plain, UnaryKernel<Kind> robust, int block, const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const Kind& f,
	int mode, hipStream_t s)
{
	if (f.nPoses <= 0) return;
	const UnaryKernel<Kind> kernel = f.rk_kind ? robust : plain;
	hipLaunchKernelGGL(kernel, dim3((f.nPoses + block - 1) / block), dim3(block), 0, s, g, st, sys, f, mode);
}

// a binary kind's two launches: the records (lane = factor with a free end), then their gather
template <class Kind>
using BinaryKernel = void (*)(DeviceGraph, Kind);
template <class Kind>
static void launch_binary(BinaryKernel<Kind> plain, BinaryKernel<Kind> robust, int block, const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const Kind& f,
	int mode, hipStream_t s)
{
	if (f.nActive <= 0) return;
	const BinaryKernel<Kind> kernel = f.rk_kind ? robust : plain;
	hipLaunchKernelGGL(kernel, dim3((f.nActive + block - 1) / block), dim3(block), 0, s, g, f);
	const size_t numbers = (mode == 1 ? (size_t)36 * f.nBlocks : 0) + (size_t)POSE_NUMBERS * f.nPoses;
	hipLaunchKernelGGL(pair_gather_kernel<Kind>, dim3((unsigned)((numbers + PAIR_GATHER_BLOCK - 1) / PAIR_GATHER_BLOCK)), dim3(PAIR_GATHER_BLOCK), 0, s, st, sys, f, mode);
}

// (the order and the rule for a new kind: ba_kernels.hpp, at this function's declaration)
void launch_pose_factor_linearize(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const DeviceFactors& pf, int mode, hipStream_t s)
{
	launch_unary(prior_linearize_kernel<false>, prior_linearize_kernel<true>, PRIOR_LIN_BLOCK, g, st, sys, pf.priors, mode, s);
	launch_unary(position_linearize_kernel<false>, position_linearize_kernel<true>, POS_LIN_BLOCK, g, st, sys, pf.pos, mode, s);
	launch_binary(relpose_linearize_kernel<false>, relpose_linearize_kernel<true>, REL_LIN_BLOCK, g, st, sys, pf.rel, mode, s);
	launch_unary(direction_linearize_kernel<false>, direction_linearize_kernel<true>, DIR_LIN_BLOCK, g, st, sys, pf.dir, mode, s);
	launch_unary(range_linearize_kernel<false>, range_linearize_kernel<true>, RNG_LIN_BLOCK, g, st, sys, pf.rng, mode, s);
	launch_binary(pose_range_linearize_kernel<false>, pose_range_linearize_kernel<true>, PRNG_LIN_BLOCK, g, st, sys, pf.prng, mode, s);
}

}  // namespace cubahip

// ---- host side --------------------------------------------------------------------------------------------------------------------

// a factor's D x D information O as the caller gave it -> `sym`: finite, symmetric within 1e-9 of its largest entry, symmetrised (within
// that tolerance the two triangles may differ by rounding; the pose factors' kernels read both).  `noun`: how the messages name the factor
template <int D>
static void take_information(const double* O, double* sym, const std::string& noun)
{
	double m = 0;
	for (int i = 0; i < D * D; i++) { if (!std::isfinite(O[i])) throw ArgError{ "non-finite " + noun + " information" }; m = std::max(m, std::fabs(O[i])); }
	for (int c = 0; c < D; c++)
		for (int r = 0; r < c; r++)
			if (std::fabs(O[D * c + r] - O[D * r + c]) > 1e-9 * m) throw ArgError{ noun + " information is not symmetric" };
	for (int c = 0; c < D; c++)
		for (int r = 0; r < D; r++) sym[D * c + r] = r == c ? O[D * c + r] : 0.5 * (O[D * c + r] + O[D * r + c]);
}

// a factor's robust kernel as the caller gave it: a known kind, a finite delta, a positive one for a real kernel
static void check_factor_kernel(int kind, double delta, const char* noun)
{
	if (kind < cubahip::POSE_FACTOR_KERNEL_NONE || kind > cubahip::POSE_FACTOR_KERNEL_CAUCHY) throw ArgError{ std::string("bad ") + noun + " robust kernel" };
	if (!std::isfinite(delta)) throw ArgError{ "non-finite robust-kernel delta" };
	if (kind != cubahip::POSE_FACTOR_KERNEL_NONE && !(delta > 0)) throw ArgError{ "robust-kernel delta must be positive" };
}

// what every setter checks before it reads its arrays: the state of the handle, the count, and for a non-empty set that the arrays are
// there (`arrays`) and that kind and delta come together.  The messages name the kind by the set's nouns; `edges`: what the graph must have
static void check_factor_call(const cuba_hip_solver& s, const FactorSet& set, int n, bool arrays, const int32_t* kind, const double* delta, const char* edges = "edges")
{
	const std::string noun = set.noun, plural = set.plural;
	if (!s.haveGraph) throw StateError{ "set_graph must be called first" };
	if (n < 0) throw ArgError{ "negative " + noun + " count" };
	if (n == 0) return;
	if (s.partHi >= 0 || s.valuesPartial) throw StateError{ plural + " are not available on a landmark-partitioned handle" };
	if (s.E == 0) throw StateError{ plural + " need a graph with " + edges };
	if (!arrays) throw ArgError{ "null " + noun + " array" };
	if ((kind == nullptr) != (delta == nullptr)) throw ArgError{ noun + " kernels: kind and delta come together" };
}

// a caller's set, validated: the vertex of every factor, its two measurement arrays, the symmetrised information and the kernels
struct TakenFactors { std::vector<int> idx; std::vector<double> a, b, info; std::vector<int> kind; std::vector<double> delta; };

// a caller's set of factors with a 3-vector residual, factor by factor: the index of its vertex (`vertex`: "pose" / "landmark") within
// [0, limit), the vectors a and -- where given; zero otherwise, none at all without a whatB -- b finite, the information symmetric, the
// kernel a known one.  kind / delta come back as given, or empty when no factor has a real kernel (kinds all 0: no kernels, the set runs
// the kernels' ROBUST = false instantiations)
static TakenFactors take_factors3(const FactorSet& set, int n, const int32_t* idx, int limit, const char* vertex, const double* a, const char* whatA, const double* b,
	const char* whatB, const double* info, const int32_t* kind, const double* delta)
{
	const std::string noun = set.noun;
	TakenFactors v;
	v.idx.resize((size_t)n); v.a.resize((size_t)3 * n); v.b.assign(whatB ? (size_t)3 * n : 0, 0.0); v.info.resize((size_t)9 * n);
	bool any = false;
	for (int k = 0; k < n; k++)
	{
		if (idx[k] < 0 || idx[k] >= limit) throw ArgError{ noun + ": " + vertex + " index out of range" };
		v.idx[k] = idx[k];
		for (size_t x = 3 * (size_t)k; x < 3 * (size_t)k + 3; x++)
		{
			if (!std::isfinite(a[x])) throw ArgError{ "non-finite " + noun + " " + whatA };
			v.a[x] = a[x];
			if (!b) continue;
			if (!std::isfinite(b[x])) throw ArgError{ "non-finite " + noun + " " + whatB };
			v.b[x] = b[x];
		}
		take_information<3>(info + 9 * (size_t)k, v.info.data() + 9 * (size_t)k, noun);
		if (kind)
		{
			check_factor_kernel(kind[k], delta[k], set.noun);
			any = any || kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE;
		}
	}
	if (any) { v.kind.assign(kind, kind + n); v.delta.assign(delta, delta + n); }
	return v;
}

// the q | t | information of factor k of a caller's set into vq | vt | vinfo (sized by the caller): finite, the quaternion normalised, the
// information symmetric and symmetrised.  `what`, `kind`: how the messages name the factor's measurement ("prior" / "relative") and its kind
static void take_factor_values(double* vq, double* vt, double* vinfo, int k, const double* q, const double* t, const double* info, const std::string& what, const std::string& kind)
{
	double nq = 0;
	for (int i = 0; i < 4; i++) { if (!std::isfinite(q[4 * (size_t)k + i])) throw ArgError{ "non-finite " + what + " rotation" }; nq += q[4 * (size_t)k + i] * q[4 * (size_t)k + i]; }
	nq = std::sqrt(nq);
	if (!(nq > 0) || !std::isfinite(nq)) throw ArgError{ kind + " quaternion of zero norm" };
	for (int i = 0; i < 4; i++) vq[4 * (size_t)k + i] = q[4 * (size_t)k + i] / nq;
	for (int i = 0; i < 3; i++) { if (!std::isfinite(t[3 * (size_t)k + i])) throw ArgError{ "non-finite " + what + " translation" }; vt[3 * (size_t)k + i] = t[3 * (size_t)k + i]; }
	take_information<6>(info + 36 * (size_t)k, vinfo + 36 * (size_t)k, kind);
}

// a validated set replaces the handle's: its device copy is due, and the run-to-run memories that the values of the system feed go, as a
// new graph drops them (a run after a change of the factors depends on the state and the factors only)
static void forget_factor_memories(cuba_hip_solver& s, FactorSet& set)
{
	set.uploaded = false;
	s.forgetRunMemories();
}

// (the replaced set is a new set: the robust kernels of the previous one go with it)
static void adopt_unary_pose_factors(cuba_hip_solver& s, UnaryPoseFactorSet& set, TakenFactors& v)
{
	set.pose.swap(v.idx); set.a.swap(v.a); set.b.swap(v.b); set.info.swap(v.info); set.kind.swap(v.kind); set.delta.swap(v.delta);
	forget_factor_memories(s, set);
	set.dev = cubahip::DevicePoseGroups();
}

void cuba_hip_solver::setPosePriors(int n, const int32_t* pose, const double* q, const double* t, const double* info)
{
	check_factor_call(*this, priorSet, n, pose && q && t && info, nullptr, nullptr);
	TakenFactors v;
	v.idx.resize((size_t)n); v.a.resize((size_t)4 * n); v.b.resize((size_t)3 * n); v.info.resize((size_t)36 * n);
	for (int k = 0; k < n; k++)
	{
		if (pose[k] < 0 || pose[k] >= Pt) throw ArgError{ "prior pose index out of range" };
		v.idx[k] = pose[k];
		take_factor_values(v.a.data(), v.b.data(), v.info.data(), k, q, t, info, "prior", "prior");
	}
	adopt_unary_pose_factors(*this, priorSet, v);
}

// the two ends of a binary factor: distinct pose indices within [0, limit)
static void check_pose_pair(int i, int j, int limit, const std::string& noun)
{
	if (i < 0 || i >= limit || j < 0 || j >= limit) throw ArgError{ noun + ": pose index out of range" };
	if (i == j) throw ArgError{ noun + " between a pose and itself" };
}

// a validated binary set replaces the handle's (adopt_unary_pose_factors' counterpart; vals: the kind's value arrays in the set's order).
// The pairs are part of the topology; a binary kind launched later stores or adds into a block by whether this one writes it, so the
// later sets' device copies are due again; the covariance blocks describe the factors -- and the block pattern -- they were computed on
static void adopt_binary_pose_factors(cuba_hip_solver& s, BinaryPoseFactorSet& set, std::vector<int>& vi, std::vector<int>& vj, std::initializer_list<std::vector<double>*> vals,
	std::vector<int>& kind, std::vector<double>& delta)
{
	set.pi.swap(vi); set.pj.swap(vj); set.kind.swap(kind); set.delta.swap(delta);
	size_t a = 0;
	for (std::vector<double>* v : vals) set.vals[a++].host.swap(*v);
	s.collectBinaryPairs();
	forget_factor_memories(s, set);
	set.dev = DevicePosePairs();
	bool later = false;
	for (BinaryPoseFactorSet* other : s.binarySets)
	{
		if (later) other->uploaded = false;
		later = later || other == &set;
	}
	s.covBlocksValid = false;
}

void cuba_hip_solver::setRelativePoseEdges(int n, const int32_t* pi, const int32_t* pj, const double* q, const double* t, const double* info)
{
	check_factor_call(*this, relSet, n, pi && pj && q && t && info, nullptr, nullptr, "reprojection edges");
	std::vector<int> vi((size_t)n), vj((size_t)n), vk;
	std::vector<double> vq((size_t)4 * n), vt((size_t)3 * n), vinfo((size_t)36 * n), vd;
	for (int k = 0; k < n; k++)
	{
		check_pose_pair(pi[k], pj[k], Pt, relSet.noun);
		vi[k] = pi[k]; vj[k] = pj[k];
		take_factor_values(vq.data(), vt.data(), vinfo.data(), k, q, t, info, "relative", "relative-pose");
	}
	// (the replaced set is a new set: the robust kernels of the previous one go with it)
	adopt_binary_pose_factors(*this, relSet, vi, vj, { &vq, &vt, &vinfo }, vk, vd);
}

// the distinct free-free pairs of the binary kinds (caller's numbering, smaller index first): part of the topology -- need() rebuilds the
// structure when they differ from the pairs the current one was seeded with.  Every binary setter recomputes the union, so that setting or
// clearing one kind keeps the others' pairs
void cuba_hip_solver::collectBinaryPairs()
{
	std::vector<uint64_t> pairs;
	for (const BinaryPoseFactorSet* set : binarySets)
		for (size_t k = 0; k < set->pi.size(); k++)
		{
			const int i = set->pi[k], j = set->pj[k];
			if (i < Pf && j < Pf) pairs.push_back(((uint64_t)(uint32_t)std::min(i, j) << 32) | (uint32_t)std::max(i, j));
		}
	std::sort(pairs.begin(), pairs.end());
	pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
	h_relPairs.swap(pairs);
}

// kernels of the current set of one type, in the caller's order; n = 0 (or kinds all 0) clears them.  The values of the system change, its
// structure does not: the device copy of the set is due again, nothing else
void cuba_hip_solver::setPoseFactorRobustKernels(int factorType, int n, const int32_t* kind, const double* delta)
{
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (factorType < 0 || factorType > 1) throw ArgError{ "bad pose-factor type" };
	FactorSet& set = factorType == 0 ? static_cast<FactorSet&>(priorSet) : relSet;
	if (n != 0 && n != set.n()) throw ArgError{ "robust kernels: the count differs from the set's" };
	if (n > 0 && (!kind || !delta)) throw ArgError{ "null robust-kernel array" };
	bool any = false;
	for (int k = 0; k < n; k++)
	{
		check_factor_kernel(kind[k], delta[k], "pose-factor");
		any = any || kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE;
	}
	if (any) { set.kind.assign(kind, kind + n); set.delta.assign(delta, delta + n); }
	else { set.kind.clear(); set.delta.clear(); }
	forget_factor_memories(*this, set);
	(factorType == 0 ? pf.priors.rk_kind : pf.rel.rk_kind) = nullptr;
	(factorType == 0 ? pf.priors.rk_delta : pf.rel.rk_delta) = nullptr;
	covBlocksValid = false;
}

void cuba_hip_solver::setLandmarkPriors(int n, const int32_t* landmark, const double* xyz, const double* info, const int32_t* kind, const double* delta)
{
	check_factor_call(*this, lmPriorSet, n, landmark && xyz && info, kind, delta);
	TakenFactors v = take_factors3(lmPriorSet, n, landmark, Lt, "landmark", xyz, "position", nullptr, nullptr, info, kind, delta);
	// the symmetrised information's upper triangle, in the packing of sym3_idx; every prior with a kernel (none: kind 0, delta 1)
	std::vector<double> U((size_t)6 * n), dl((size_t)n, 1.0);
	std::vector<int> kd((size_t)n, cubahip::POSE_FACTOR_KERNEL_NONE);
	for (int k = 0; k < n; k++)
	{
		const double* S = v.info.data() + 9 * (size_t)k;
		double* u = U.data() + 6 * (size_t)k;
		u[0] = S[0]; u[1] = S[3]; u[2] = S[6]; u[3] = S[4]; u[4] = S[7]; u[5] = S[8];
		if (!v.kind.empty() && v.kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE) { kd[k] = v.kind[k]; dl[k] = v.delta[k]; }
	}
	lmPriorSet.lm.swap(v.idx); lmPriorSet.xyz.swap(v.a); lmPriorSet.info.swap(U); lmPriorSet.kind.swap(kd); lmPriorSet.delta.swap(dl);
	forget_factor_memories(*this, lmPriorSet);
	pf.lmp = DeviceLandmarkPriors();
	covBlocksValid = false;
}

void cuba_hip_solver::setPositionFactors(int n, const int32_t* pose, const double* position, const double* leverArm, const double* info, const int32_t* kind,
	const double* delta)
{
	check_factor_call(*this, posSet, n, pose && position && info, kind, delta);
	TakenFactors v = take_factors3(posSet, n, pose, Pt, "pose", position, "position", leverArm, "lever arm", info, kind, delta);
	adopt_unary_pose_factors(*this, posSet, v);
	covBlocksValid = false;
}

// (the vectors are taken as given: neither is normalised)
void cuba_hip_solver::setDirectionFactors(int n, const int32_t* pose, const double* worldDir, const double* measuredDir, const double* info, const int32_t* kind,
	const double* delta)
{
	check_factor_call(*this, dirSet, n, pose && worldDir && measuredDir && info, kind, delta);
	TakenFactors v = take_factors3(dirSet, n, pose, Pt, "pose", worldDir, "world direction", measuredDir, "measurement", info, kind, delta);
	adopt_unary_pose_factors(*this, dirSet, v);
	covBlocksValid = false;
}

// what the two scalar kinds check of factor k: the 3-vectors of `vecs` finite (component by component, each vector where given), the range
// and the information finite and not negative (0: no factor), the kernel a known one.  Returns whether the factor has a real kernel
struct Vec3Arg { const double* v; const char* what; };
static bool check_range_factor(const FactorSet& set, int k, std::initializer_list<Vec3Arg> vecs, const double* range, const double* info, const int32_t* kind, const double* delta)
{
	const std::string noun = set.noun;
	for (int i = 0; i < 3; i++)
		for (const Vec3Arg& a : vecs)
			if (a.v && !std::isfinite(a.v[3 * (size_t)k + i])) throw ArgError{ "non-finite " + noun + " " + a.what };
	if (!std::isfinite(range[k])) throw ArgError{ "non-finite " + noun + " range" };
	if (range[k] < 0) throw ArgError{ "negative " + noun + " range" };
	if (!std::isfinite(info[k])) throw ArgError{ "non-finite " + noun + " information" };
	if (info[k] < 0) throw ArgError{ "negative " + noun + " information" };
	if (!kind) return false;
	check_factor_kernel(kind[k], delta[k], set.noun);
	return kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE;
}

// a caller's set of range factors, factor by factor (the scalar kind's counterpart of take_factors3): the pose index within [0, limit), the
// rest by check_range_factor.  a: {anchor, range} (width 4), b: the arm (zero where none is given).  kind / delta as take_factors3
static TakenFactors take_range_factors(const FactorSet& set, int n, const int32_t* pose, int limit, const double* anchor, const double* range, const double* arm,
	const double* info, const int32_t* kind, const double* delta)
{
	const std::string noun = set.noun;
	TakenFactors v;
	v.idx.resize((size_t)n); v.a.resize((size_t)4 * n); v.b.assign((size_t)3 * n, 0.0); v.info.resize((size_t)n);
	bool any = false;
	for (int k = 0; k < n; k++)
	{
		if (pose[k] < 0 || pose[k] >= limit) throw ArgError{ noun + ": pose index out of range" };
		v.idx[k] = pose[k];
		any = check_range_factor(set, k, { { anchor, "anchor" }, { arm, "lever arm" } }, range, info, kind, delta) || any;
		for (int i = 0; i < 3; i++)
		{
			v.a[4 * (size_t)k + i] = anchor[3 * (size_t)k + i];
			if (arm) v.b[3 * (size_t)k + i] = arm[3 * (size_t)k + i];
		}
		v.a[4 * (size_t)k + 3] = range[k];
		v.info[k] = info[k];
	}
	if (any) { v.kind.assign(kind, kind + n); v.delta.assign(delta, delta + n); }
	return v;
}

void cuba_hip_solver::setRangeFactors(int n, const int32_t* pose, const double* anchor, const double* range, const double* leverArm, const double* info,
	const int32_t* kind, const double* delta)
{
	check_factor_call(*this, rngSet, n, pose && anchor && range && info, kind, delta);
	TakenFactors v = take_range_factors(rngSet, n, pose, Pt, anchor, range, leverArm, info, kind, delta);
	adopt_unary_pose_factors(*this, rngSet, v);
	covBlocksValid = false;
}

void cuba_hip_solver::setPoseRangeFactors(int n, const int32_t* pi, const int32_t* pj, const double* range, const double* armI, const double* armJ, const double* info,
	const int32_t* kind, const double* delta)
{
	check_factor_call(*this, prngSet, n, pi && pj && range && info, kind, delta, "reprojection edges");
	std::vector<int> vi((size_t)n), vj((size_t)n), vk;
	std::vector<double> vai((size_t)3 * n, 0.0), vaj((size_t)3 * n, 0.0), vr((size_t)n), vinfo((size_t)n), vd;
	bool any = false;
	for (int k = 0; k < n; k++)
	{
		check_pose_pair(pi[k], pj[k], Pt, prngSet.noun);
		vi[k] = pi[k]; vj[k] = pj[k];
		any = check_range_factor(prngSet, k, { { armI, "lever arm" }, { armJ, "lever arm" } }, range, info, kind, delta) || any;
		for (size_t x = 3 * (size_t)k; x < 3 * (size_t)k + 3; x++)
		{
			if (armI) vai[x] = armI[x];
			if (armJ) vaj[x] = armJ[x];
		}
		vr[k] = range[k]; vinfo[k] = info[k];
	}
	if (any) { vk.assign(kind, kind + n); vd.assign(delta, delta + n); }
	adopt_binary_pose_factors(*this, prngSet, vi, vj, { &vai, &vaj, &vr, &vinfo }, vk, vd);
}

std::vector<uint64_t> cuba_hip_solver::relSeedKeys() const
{
	std::vector<uint64_t> keys(h_relPairs.size());
	for (size_t x = 0; x < keys.size(); x++)
	{
		int a = (int)(h_relPairs[x] >> 32), b = (int)(uint32_t)h_relPairs[x];
		if (reorderActive) { a = poseNewOfOld[a]; b = poseNewOfOld[b]; }
		keys[x] = ((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b);
	}
	std::sort(keys.begin(), keys.end());
	return keys;
}

// set.order: the caller's factors stable by `key` (factors of equal key stay in the caller's order)
static void sort_factors(FactorSet& set, const std::vector<uint64_t>& key)
{
	set.order.resize(key.size());
	std::iota(set.order.begin(), set.order.end(), 0);
	std::stable_sort(set.order.begin(), set.order.end(), [&](int a, int b) { return key[a] < key[b]; });
}

static std::vector<int> concat(std::initializer_list<const std::vector<int>*> parts)
{
	std::vector<int> out;
	for (const std::vector<int>* p : parts) out.insert(out.end(), p->begin(), p->end());
	return out;
}

// a unary kind's factors on the poses -> device, in the internal pose order (stable by internal pose: every pose's factors contiguous, in
// the caller's order; the factors on fixed poses last).  The same layout for the four kinds:
// ints: pose_ptr [np + 1] | pose_id [np] | pose [n] | kind [n, robust];  values: a [wa n] | b [wb n] | info [wi n] | delta [n, robust]
void UnaryPoseFactorSet::upload(cuba_hip_solver& s)
{
	const int Pf = s.Pf;
	const size_t N = (size_t)n();
	const bool robust = !kind.empty();
	std::vector<uint64_t> internal(N);
	for (size_t k = 0; k < N; k++) internal[k] = (uint64_t)s.internalPose(pose[k]);
	sort_factors(*this, internal);
	std::vector<int> ptr, ids, poses(N);
	for (size_t p = 0; p < N; p++)
	{
		poses[p] = (int)internal[order[p]];
		if (poses[p] < Pf && (ids.empty() || ids.back() != poses[p])) { ids.push_back(poses[p]); ptr.push_back((int)p); }
	}
	size_t nFree = 0;
	while (nFree < N && poses[nFree] < Pf) nFree++;
	ptr.push_back((int)nFree);
	const int np = (int)ids.size();
	std::vector<int> ints = concat({ &ptr, &ids, &poses });
	const size_t nInts = ints.size();
	std::vector<Scalar> vals((size_t)(wa + wb + wi + (robust ? 1 : 0)) * N);
	Scalar* va = vals.data(); Scalar* vb = va + wa * N; Scalar* vi = vb + wb * N;
	for (size_t p = 0; p < N; p++)
	{
		const size_t k = (size_t)order[p];
		for (int i = 0; i < wa; i++) va[wa * p + i] = (Scalar)a[wa * k + i];
		for (int i = 0; i < wb; i++) vb[wb * p + i] = (Scalar)b[wb * k + i];
		for (int i = 0; i < wi; i++) vi[wi * p + i] = (Scalar)info[wi * k + i];
		if (robust) { ints.push_back(kind[k]); vi[wi * N + p] = (Scalar)delta[k]; }
	}
	d_ints.upload(ints, s.stream);
	d_vals.upload(vals, s.stream);
	d_chi.resize(std::max(N, (size_t)1));
	s.sync();          // (the staging vectors go out of scope)
	dev.n = (int)N; dev.nPoses = np;
	dev.pose_ptr = d_ints.data(); dev.pose_id = dev.pose_ptr + (np + 1); dev.pose = dev.pose_id + np;
	da = d_vals.data(); db = da + wa * N; dev.info = db + wb * N;
	dev.chi = d_chi.data();
	dev.rk_kind = robust ? d_ints.data() + nInts : nullptr; dev.rk_delta = robust ? dev.info + wi * N : nullptr;
	uploaded = true;
}

// a binary kind's factors in the internal pose order: free-free factors first, stable by the block (min, max) of the internal pair -- a
// block's factors contiguous and in the caller's order --, then the factors with one fixed end, then (inactive) those with two
// (sets set.order; blkKey: the (min << 32 | max) key of every block of blkId, ascending)
struct BinaryLayout { std::vector<int> si, sj, blkPtr, blkId, posePtr, poseId, poseItem; std::vector<uint64_t> blkKey; int nActive = 0; };
static BinaryLayout sort_binary_factors(cuba_hip_solver& s, FactorSet& set, const std::vector<int>& pi, const std::vector<int>& pj)
{
	const int n = (int)pi.size(), Pf = s.Pf;
	std::vector<int> a((size_t)n), b((size_t)n);
	std::vector<uint64_t> key((size_t)n);
	for (int k = 0; k < n; k++)
	{
		a[k] = s.internalPose(pi[k]); b[k] = s.internalPose(pj[k]);
		const int nFixed = (a[k] >= Pf) + (b[k] >= Pf);
		key[k] = nFixed == 0 ? (((uint64_t)(uint32_t)std::min(a[k], b[k]) << 32) | (uint32_t)std::max(a[k], b[k])) : (~0ull - (uint64_t)(2 - nFixed));
	}
	sort_factors(set, key);
	std::vector<int> posOf((size_t)n);
	for (int p = 0; p < n; p++) posOf[set.order[p]] = p;
	s.ensureHostPattern();
	BinaryLayout lay;
	std::vector<int>&si = lay.si, &sj = lay.sj, &blkPtr = lay.blkPtr, &blkId = lay.blkId, &posePtr = lay.posePtr, &poseId = lay.poseId, &poseItem = lay.poseItem;
	si.resize((size_t)n); sj.resize((size_t)n);
	int& nActive = lay.nActive;
	for (int p = 0; p < n; p++)
	{
		const int k = set.order[p];
		si[p] = a[k]; sj[p] = b[k];
		if (a[k] < Pf || b[k] < Pf) nActive = p + 1;
		if (a[k] < Pf && b[k] < Pf && (p == 0 || key[k] != key[set.order[p - 1]]))
		{
			const int row = std::min(a[k], b[k]), col = std::max(a[k], b[k]);
			const int* c0 = s.h_colind.data() + s.h_rowptr[row]; const int* c1 = s.h_colind.data() + s.h_rowptr[row + 1];
			const int* it = std::lower_bound(c0, c1, col);
			if (it == c1 || *it != col) throw StateError{ std::string(set.noun) + " without its block in the pattern" };
			blkPtr.push_back(p); blkId.push_back((int)(it - s.h_colind.data())); lay.blkKey.push_back(key[k]);
		}
	}
	int nFreeFree = 0;
	while (nFreeFree < n && si[nFreeFree] < Pf && sj[nFreeFree] < Pf) nFreeFree++;
	blkPtr.push_back(nFreeFree);
	// per free pose: its edges in the caller's order (item = 2 * sorted position + end: 0 = the pose is i, 1 = j)
	std::vector<std::pair<int, int>> items;
	for (int k = 0; k < n; k++)
	{
		if (a[k] < Pf) items.emplace_back(a[k], 2 * posOf[k]);
		if (b[k] < Pf) items.emplace_back(b[k], 2 * posOf[k] + 1);
	}
	std::stable_sort(items.begin(), items.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first < y.first; });
	for (size_t x = 0; x < items.size(); x++)
	{
		if (x == 0 || items[x].first != items[x - 1].first) { posePtr.push_back((int)x); poseId.push_back(items[x].first); }
		poseItem.push_back(items[x].second);
	}
	posePtr.push_back((int)items.size());
	return lay;
}

// a binary kind's factors -> device, sorted by sort_binary_factors.  blk_shared: the blocks that the gather of a binary kind launched
// EARLIER writes too (binarySets is in launch order; that gather stores a block without Schur products, so this kind's adds there) -- the
// device copy depends on the structure AND on the earlier binary sets: their setters mark it due again.  The same layout for the kinds:
// ints: pose_i [n] | pose_j [n] | blk_ptr [nb + 1] | blk_id [nb] | blk_shared [nb] | pose_ptr [np + 1] | pose_id [np] | pose_item | kind [n, robust]
// values: the kind's arrays in the order of vals, [width n] each, the information last | delta [n, robust]
void BinaryPoseFactorSet::upload(cuba_hip_solver& s)
{
	const size_t N = (size_t)n();
	const bool robust = !kind.empty();
	const BinaryLayout lay = sort_binary_factors(s, *this, pi, pj);
	std::vector<uint64_t> earlier;
	for (const BinaryPoseFactorSet* set : s.binarySets)
	{
		if (set == this) break;
		for (int k = 0; k < set->n(); k++)
		{
			const int a = s.internalPose(set->pi[k]), b = s.internalPose(set->pj[k]);
			if (a < s.Pf && b < s.Pf) earlier.push_back(((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b));
		}
	}
	std::sort(earlier.begin(), earlier.end());
	const int nb = (int)lay.blkId.size(), np = (int)lay.poseId.size();
	std::vector<int> blkShared((size_t)nb);
	for (int b = 0; b < nb; b++) blkShared[b] = std::binary_search(earlier.begin(), earlier.end(), lay.blkKey[b]) ? 1 : 0;
	std::vector<int> ints = concat({ &lay.si, &lay.sj, &lay.blkPtr, &lay.blkId, &blkShared, &lay.posePtr, &lay.poseId, &lay.poseItem });
	const size_t nInts = ints.size();
	size_t width = 0;
	for (const Values& v : vals) width += (size_t)v.width;
	std::vector<Scalar> staged((width + (robust ? 1 : 0)) * N);
	Scalar* out = staged.data();
	for (const Values& v : vals)
		for (size_t p = 0; p < N; p++)
			for (int i = 0; i < v.width; i++) *out++ = (Scalar)v.host[(size_t)v.width * order[p] + i];
	for (size_t p = 0; robust && p < N; p++) { ints.push_back(kind[order[p]]); *out++ = (Scalar)delta[order[p]]; }
	d_ints.upload(ints, s.stream);
	d_vals.upload(staged, s.stream);
	d_chi.resize(std::max(N, (size_t)1));
	d_rec.resize((size_t)recSize * std::max(N, (size_t)1));
	s.sync();          // (the staging vectors go out of scope)
	dev.n = (int)N; dev.nActive = lay.nActive; dev.nBlocks = nb; dev.nPoses = np;
	dev.pose_i = d_ints.data(); dev.pose_j = dev.pose_i + N;
	dev.blk_ptr = dev.pose_j + N; dev.blk_id = dev.blk_ptr + (nb + 1); dev.blk_shared = dev.blk_id + nb;
	dev.pose_ptr = dev.blk_shared + nb; dev.pose_id = dev.pose_ptr + (np + 1); dev.pose_item = dev.pose_id + np;
	const Scalar* d = d_vals.data();
	for (const Values& v : vals) { v.dev = d; d += (size_t)v.width * N; }
	dev.rec = d_rec.data(); dev.chi = d_chi.data();
	dev.rk_kind = robust ? d_ints.data() + nInts : nullptr; dev.rk_delta = robust ? d : nullptr;
	uploaded = true; structure = s.cntStructureBuilds;
}

// the caller's priors -> device, in the internal landmark order (stable by internal landmark: every landmark's priors contiguous, in the
// caller's order; the priors on fixed landmarks last).  A prior on a free landmark without an edge cannot be honoured -- the landmark pass
// walks the landmarks of the edge list --: the set is dropped and the call that got here reports it.
void LandmarkPriorSet::upload(cuba_hip_solver& s)
{
	LandmarkPriorSet& set = *this;
	const int n = set.n(), Lf = s.Lf;
	std::vector<int> lmMap, lmPtr((size_t)Lf + 1, 0);
	if (s.lmOrderActive && Lf > 0)
	{
		lmMap.resize(Lf);
		HIP_TRY(hipMemcpyAsync(lmMap.data(), s.d_lmMap.data(), sizeof(int) * (size_t)Lf, hipMemcpyDeviceToHost, s.stream));
	}
	HIP_TRY(hipMemcpyAsync(lmPtr.data(), s.g.lm_ptr, sizeof(int) * ((size_t)Lf + 1), hipMemcpyDeviceToHost, s.stream));
	s.sync();
	std::vector<uint64_t> internal((size_t)n);
	for (int k = 0; k < n; k++)
	{
		const int l = set.lm[k];
		internal[k] = (uint64_t)(l < Lf && !lmMap.empty() ? lmMap[l] : l);
		if (l < Lf && lmPtr[internal[k]] == lmPtr[internal[k] + 1])
		{
			set.clear(); s.pf.lmp = DeviceLandmarkPriors();
			throw ArgError{ "landmark prior on free landmark " + std::to_string(l) + ", which no edge observes: the set is dropped" };
		}
	}
	sort_factors(set, internal);
	// ints: lm_ptr [Lf + 1] | lm [n] | kind [n];  values: xbar [3 n] | info [6 n] | delta [n]
	std::vector<int> ints((size_t)Lf + 1 + 2 * (size_t)n, 0);
	std::vector<Scalar> vals((size_t)10 * n);
	int* ptr = ints.data(); int* lm = ptr + Lf + 1; int* kd = lm + n;
	Scalar* vx = vals.data(); Scalar* vi = vx + 3 * (size_t)n; Scalar* vd = vi + 6 * (size_t)n;
	for (int p = 0; p < n; p++)
	{
		const size_t k = (size_t)set.order[p];
		lm[p] = (int)internal[k]; kd[p] = set.kind[k]; vd[p] = (Scalar)set.delta[k];
		if (lm[p] < Lf) ptr[lm[p] + 1]++;
		for (int i = 0; i < 3; i++) vx[3 * (size_t)p + i] = (Scalar)set.xyz[3 * k + i];
		for (int i = 0; i < 6; i++) vi[6 * (size_t)p + i] = (Scalar)set.info[6 * k + i];
	}
	for (int l = 0; l < Lf; l++) ptr[l + 1] += ptr[l];
	set.d_ints.upload(ints, s.stream);
	set.d_vals.upload(vals, s.stream);
	set.d_chi.resize((size_t)n);
	s.sync();          // (the staging vectors go out of scope)
	DeviceLandmarkPriors lp;
	lp.n = n;
	lp.lm_ptr = set.d_ints.data(); lp.lm = lp.lm_ptr + Lf + 1; lp.rk_kind = lp.lm + n;
	lp.xbar = set.d_vals.data(); lp.info = lp.xbar + 3 * (size_t)n; lp.rk_delta = lp.info + 6 * (size_t)n;
	lp.chi = set.d_chi.data();
	s.pf.lmp = lp;
	set.uploaded = true; set.structure = s.cntStructureBuilds;
}

// (the unary kinds on the poses depend on the pose order only -- a change of it marks them: poseOrderChanged() --, the edges' blocks and the
// landmark priors' order on the structure)
void cuba_hip_solver::uploadFactors()
{
	for (FactorSet* set : factorSets)
		if (set->n() > 0 && (!set->uploaded || (set->onStructure && set->structure != cntStructureBuilds))) set->upload(*this);
}

void cuba_hip_solver::factorChiSquares(int kind, double* out)
{
	need();
	const FactorSet& set = *factorSets[kind];
	if (set.n() == 0) return;
	launch_factor_chi2(g, pf, d_parts.data(), stream, kind);
	// the per-factor chi2 of the launch just issued (sorted order on the device) -> the caller's order
	const size_t n = set.order.size();
	std::vector<double> sorted(n);
	downloadAsDouble(set.d_chi.data(), sorted.data(), n);
	for (size_t p = 0; p < n; p++) out[set.order[p]] = sorted[p];
}
