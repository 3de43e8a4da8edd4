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
// Order: the pose priors, the position factors, the relative-pose edges, the direction factors and the range factors all add to the diagonal
// blocks, bp and bsc that the pose and Schur passes stored, by read-modify-write.  launch_pose_factor_linearize issues them in one stream in
// this order -- priors, position factors, the edges' records, the edges' gather, direction factors, range factors, the records and the
// gather of the range factors between poses -- and that order is part of the result
// (floating-point sums do not commute): a handle's bits depend on it, and a new kind goes BEHIND the ones a handle may already combine,
// never between two of them.  (The position factors sit between the priors and the edges: no handle could hold them before they came, so
// no existing sum changed.  The direction factors came when handles could combine all of the others, so they went last; the range factors came after them and go
// behind them, the range factors between poses after those.)
//
// The kinds keep linearisation kernels of their own (a prior is not run as a one-ended edge: its sums would be taken in another order).
// Everything else exists once: the device helpers below (the unary kinds' accumulators and their read-modify-write: zero_pose_sums,
// add_pose_sums), one chi2 kernel over a per-kind residual, one device layout and one upload for the four unary kinds on the poses
// (ba_kernels.hpp: DevicePoseGroups), the host-side validation, sorting and read-back, and one interface (ba_kernels.hpp: DeviceFactors;
// ba_solver.hpp: the handle's table of its sets).  A new kind brings a residual, a Jacobian, a setter with its widths and nouns, and its
// entry there.
//
//   prior_linearize_kernel     lane = free pose with priors: its priors in the caller's order, J^T Omega J / J^T Omega r summed in
//                              registers, then added to the pose's diagonal block (upper triangle), bp and (mode 1) bsc -- one writer per
//                              block, a launch of its own behind the Schur pass (which may still update a diagonal block the pose pass stored)
//   relpose_linearize_kernel   lane = edge: r, J_i, J_j and the edge's record {J_i^T Omega J_i, J_j^T Omega J_j (upper triangles),
//                              the cross term laid out as the block (min, max) of the internal pose pair stores it, J_i^T Omega r,
//                              J_j^T Omega r}
//   relpose_gather_kernel      lane = one number of the reduced system: an entry of an off-diagonal block with relative edges (the sum of
//                              its edges' cross terms, added to what the Schur pass stored, or stored whole when the block has no products),
//                              or an entry of a pose's diagonal block (upper triangle) / of bp and (mode 1) bsc, summed over the pose's
//                              edges in the caller's order -- one writer per number, fixed order, no atomics; behind the Schur pass and the
//                              priors' launch
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
//                              the diagonal block's upper triangle, bp and (mode 1) bsc -- one writer per number; the last launch, behind the
//                              direction factors'
//   pose_range_linearize_kernel lane = range factor between poses with a free end: the record {J_i, J_j, w Omega, w Omega r}, 14 numbers
//   pose_range_gather_kernel   lane = one number of the reduced system, as relpose_gather_kernel: an entry of an off-diagonal block with such
//                              factors (mode 1: J_min[r] w Omega J_max[c] summed over the block's factors; stored whole where the block has
//                              neither Schur products nor a relative-pose edge, added to what those stored otherwise), or an entry of a
//                              pose's diagonal block (upper triangle) / of bp and (mode 1) bsc, summed over the pose's factors in the
//                              caller's order -- one writer per number, fixed order, no atomics; the last two launches
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
constexpr int REL_GATHER_BLOCK = 256;
constexpr int CHI_BLOCK = 256;
constexpr int CHI_MAX_GROUPS = 64;     // a chi2 launch's partials (a grid-stride loop beyond): they join the reprojection edges' partials
// record of an edge: [0, 21) J_i^T Omega J_i, [21, 42) J_j^T Omega J_j (upper triangles, entry c (c + 1) / 2 + r), [42, 78) the cross block
// (column-major, rows = the pose of smaller internal index), [78, 84) J_i^T Omega r, [84, 90) J_j^T Omega r
constexpr int REL_HII = 0, REL_HJJ = 21, REL_HX = 42, REL_GI = 78, REL_GJ = 84;
static_assert(REL_GJ + 6 == REL_REC, "record layout");
constexpr int REL_POSE_NUMBERS = 27;        // 21 entries of a diagonal block + 6 of bp / bsc
// the range factors between two poses run as the edges do (tiny, latency-bound launches: the siblings' block sizes)
constexpr int PRNG_LIN_BLOCK = 64;
constexpr int PRNG_GATHER_BLOCK = 256;
// record of such a factor: [0, 6) J_i, [6, 12) J_j, w Omega, w Omega r
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

// number `el` of the record of edge k: the records are stored number-major (all edges' number 0, then number 1, ...), so that the lanes of
// the linearisation -- consecutive edges -- store to consecutive addresses
__device__ __forceinline__ Scalar& rel_rec(const DeviceRelPoses& rp, int k, int el) { return rp.rec[(size_t)el * rp.n + k]; }

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
			if (rr <= c) { rel_rec(rp, k, REL_HII + c * (c + 1) / 2 + rr) = sii; rel_rec(rp, k, REL_HJJ + c * (c + 1) / 2 + rr) = sjj; }
			rel_rec(rp, k, REL_HX + (flip ? rr * 6 + c : c * 6 + rr)) = sx;
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
		rel_rec(rp, k, REL_GI + c) = si; rel_rec(rp, k, REL_GJ + c) = sj;
	}
}

__global__ __launch_bounds__(REL_GATHER_BLOCK) void relpose_gather_kernel(DeviceStructure st, DeviceSystem sys, DeviceRelPoses rp, int mode)
{
	const int x = blockIdx.x * REL_GATHER_BLOCK + threadIdx.x;
	const int nBlkNumbers = mode == 1 ? 36 * rp.nBlocks : 0;
	if (x < nBlkNumbers)
	{
		const int b = x / 36, el = x - 36 * b;
		const int blk = rp.blk_id[b];
		Scalar s = 0;
		const int k1 = rp.blk_ptr[b + 1];
		for (int k = rp.blk_ptr[b]; k < k1; k++) s += rel_rec(rp, k, REL_HX + el);
		Scalar* dst = sys.hsc + 36 * (size_t)blk + el;
		// (a block with products was stored by the Schur pass of this linearisation; one without has no other writer)
		*dst = st.prod_end[blk] > st.prod_beg[blk] ? *dst + s : s;
		return;
	}
	const int y = x - nBlkNumbers;
	const int p = y / REL_POSE_NUMBERS, el = y - REL_POSE_NUMBERS * p;
	if (p >= rp.nPoses) return;
	const int ip = rp.pose_id[p];
	Scalar s = 0;
	const int k1 = rp.pose_ptr[p + 1];
	for (int k = rp.pose_ptr[p]; k < k1; k++)
	{
		const int item = rp.pose_item[k], side = item & 1;
		s += rel_rec(rp, item >> 1, el < 21 ? (side ? REL_HJJ : REL_HII) + el : (side ? REL_GJ : REL_GI) + (el - 21));
	}
	if (el < 21)
	{
		// packed upper-triangle index -> (r, c)
		int c = 0;
		while ((c + 1) * (c + 2) / 2 <= el) c++;
		const int rr = el - c * (c + 1) / 2;
		sys.hsc[36 * (size_t)st.hsc_rowptr[ip] + c * 6 + rr] += s;
	}
	else
	{
		sys.bp[6 * (size_t)ip + (el - 21)] -= s;
		if (mode == 1) sys.bsc[6 * (size_t)ip + (el - 21)] -= s;
	}
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

// number `el` of the record of factor k: number-major as rel_rec, so that the lanes of the linearisation store to consecutive addresses
__device__ __forceinline__ Scalar& prng_rec(const DevicePoseRanges& pr, int k, int el) { return pr.rec[(size_t)el * pr.n + k]; }

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
	for (int c = 0; c < 12; c++) prng_rec(pr, k, PRNG_JI + c) = J[c];
	prng_rec(pr, k, PRNG_W) = w;
	prng_rec(pr, k, PRNG_WR) = w * r;
}

__global__ __launch_bounds__(PRNG_GATHER_BLOCK) void pose_range_gather_kernel(DeviceStructure st, DeviceSystem sys, DevicePoseRanges pr, int mode)
{
	const int x = blockIdx.x * PRNG_GATHER_BLOCK + threadIdx.x;
	const int nBlkNumbers = mode == 1 ? 36 * pr.nBlocks : 0;
	if (x < nBlkNumbers)
	{
		// entry (rr, c) of the block (min, max) of the internal pair, column-major: J_min[rr] w Omega J_max[c]
		const int b = x / 36, el = x - 36 * b;
		const int c = el / 6, rr = el - 6 * c;
		const int blk = pr.blk_id[b];
		Scalar s = 0;
		const int k1 = pr.blk_ptr[b + 1];
		for (int k = pr.blk_ptr[b]; k < k1; k++)
		{
			const bool flip = pr.pose_i[k] > pr.pose_j[k];
			s += prng_rec(pr, k, (flip ? PRNG_JJ : PRNG_JI) + rr) * (prng_rec(pr, k, PRNG_W) * prng_rec(pr, k, (flip ? PRNG_JI : PRNG_JJ) + c));
		}
		Scalar* dst = sys.hsc + 36 * (size_t)blk + el;
		// (a block with products was stored by the Schur pass of this linearisation, one with a relative-pose edge by relpose_gather_kernel;
		// a block with neither has no other writer)
		*dst = st.prod_end[blk] > st.prod_beg[blk] || pr.blk_rel[b] ? *dst + s : s;
		return;
	}
	const int y = x - nBlkNumbers;
	const int p = y / REL_POSE_NUMBERS, el = y - REL_POSE_NUMBERS * p;
	if (p >= pr.nPoses) return;
	const int ip = pr.pose_id[p];
	// packed upper-triangle index -> (rr, c); el >= 21: entry c of bp / bsc
	int c = el - 21, rr = 0;
	if (el < 21)
	{
		c = 0;
		while ((c + 1) * (c + 2) / 2 <= el) c++;
		rr = el - c * (c + 1) / 2;
	}
	Scalar s = 0;
	const int k1 = pr.pose_ptr[p + 1];
	for (int k = pr.pose_ptr[p]; k < k1; k++)
	{
		const int item = pr.pose_item[k], f = item >> 1, J = item & 1 ? PRNG_JJ : PRNG_JI;
		if (el < 21) s += prng_rec(pr, f, J + rr) * (prng_rec(pr, f, PRNG_W) * prng_rec(pr, f, J + c));
		else s += prng_rec(pr, f, J + c) * prng_rec(pr, f, PRNG_WR);
	}
	if (el < 21) sys.hsc[36 * (size_t)st.hsc_rowptr[ip] + c * 6 + rr] += s;
	else
	{
		sys.bp[6 * (size_t)ip + c] -= s;
		if (mode == 1) sys.bsc[6 * (size_t)ip + c] -= s;
	}
}

// info r^2 of factor k at the current estimate (factor_chi2_kernel)
__device__ __forceinline__ Scalar factor_chi(const DeviceGraph& g, const DevicePoseRanges& pr, int k)
{
	if (k >= pr.nActive) return 0;
	Scalar mi[3], mj[3], r;
	return pose_range_residual(g, pr, k, mi, mj, r);
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

void launch_pose_factor_linearize(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const DeviceFactors& pf, int mode, hipStream_t s)
{
	const DevicePriors& pr = pf.priors;
	if (pr.nPoses > 0)
	{
		const dim3 grid((pr.nPoses + PRIOR_LIN_BLOCK - 1) / PRIOR_LIN_BLOCK);
		if (pr.rk_kind) hipLaunchKernelGGL(prior_linearize_kernel<true>, grid, dim3(PRIOR_LIN_BLOCK), 0, s, g, st, sys, pr, mode);
		else hipLaunchKernelGGL(prior_linearize_kernel<false>, grid, dim3(PRIOR_LIN_BLOCK), 0, s, g, st, sys, pr, mode);
	}
	const DevicePositionFactors& pp = pf.pos;
	if (pp.nPoses > 0)
	{
		const dim3 grid((pp.nPoses + POS_LIN_BLOCK - 1) / POS_LIN_BLOCK);
		if (pp.rk_kind) hipLaunchKernelGGL(position_linearize_kernel<true>, grid, dim3(POS_LIN_BLOCK), 0, s, g, st, sys, pp, mode);
		else hipLaunchKernelGGL(position_linearize_kernel<false>, grid, dim3(POS_LIN_BLOCK), 0, s, g, st, sys, pp, mode);
	}
	const DeviceRelPoses& rp = pf.rel;
	if (rp.nActive > 0)
	{
		const dim3 linGrid((rp.nActive + REL_LIN_BLOCK - 1) / REL_LIN_BLOCK);
		if (rp.rk_kind) hipLaunchKernelGGL(relpose_linearize_kernel<true>, linGrid, dim3(REL_LIN_BLOCK), 0, s, g, rp);
		else hipLaunchKernelGGL(relpose_linearize_kernel<false>, linGrid, dim3(REL_LIN_BLOCK), 0, s, g, rp);
		const size_t numbers = (mode == 1 ? (size_t)36 * rp.nBlocks : 0) + (size_t)REL_POSE_NUMBERS * rp.nPoses;
		hipLaunchKernelGGL(relpose_gather_kernel, dim3((unsigned)((numbers + REL_GATHER_BLOCK - 1) / REL_GATHER_BLOCK)), dim3(REL_GATHER_BLOCK), 0, s, st, sys, rp, mode);
	}
	const DeviceDirectionFactors& df = pf.dir;
	if (df.nPoses > 0)
	{
		const dim3 grid((df.nPoses + DIR_LIN_BLOCK - 1) / DIR_LIN_BLOCK);
		if (df.rk_kind) hipLaunchKernelGGL(direction_linearize_kernel<true>, grid, dim3(DIR_LIN_BLOCK), 0, s, g, st, sys, df, mode);
		else hipLaunchKernelGGL(direction_linearize_kernel<false>, grid, dim3(DIR_LIN_BLOCK), 0, s, g, st, sys, df, mode);
	}
	const DeviceRangeFactors& rf = pf.rng;
	if (rf.nPoses > 0)
	{
		const dim3 grid((rf.nPoses + RNG_LIN_BLOCK - 1) / RNG_LIN_BLOCK);
		if (rf.rk_kind) hipLaunchKernelGGL(range_linearize_kernel<true>, grid, dim3(RNG_LIN_BLOCK), 0, s, g, st, sys, rf, mode);
		else hipLaunchKernelGGL(range_linearize_kernel<false>, grid, dim3(RNG_LIN_BLOCK), 0, s, g, st, sys, rf, mode);
	}
	const DevicePoseRanges& pg = pf.prng;
	if (pg.nActive > 0)
	{
		const dim3 linGrid((pg.nActive + PRNG_LIN_BLOCK - 1) / PRNG_LIN_BLOCK);
		if (pg.rk_kind) hipLaunchKernelGGL(pose_range_linearize_kernel<true>, linGrid, dim3(PRNG_LIN_BLOCK), 0, s, g, pg);
		else hipLaunchKernelGGL(pose_range_linearize_kernel<false>, linGrid, dim3(PRNG_LIN_BLOCK), 0, s, g, pg);
		const size_t numbers = (mode == 1 ? (size_t)36 * pg.nBlocks : 0) + (size_t)REL_POSE_NUMBERS * pg.nPoses;
		hipLaunchKernelGGL(pose_range_gather_kernel, dim3((unsigned)((numbers + PRNG_GATHER_BLOCK - 1) / PRNG_GATHER_BLOCK)), dim3(PRNG_GATHER_BLOCK), 0, s, st, sys, pg, mode);
	}
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

void cuba_hip_solver::setRelativePoseEdges(int n, const int32_t* pi, const int32_t* pj, const double* q, const double* t, const double* info)
{
	check_factor_call(*this, relSet, n, pi && pj && q && t && info, nullptr, nullptr, "reprojection edges");
	std::vector<int> vi((size_t)n), vj((size_t)n);
	std::vector<double> vq((size_t)4 * n), vt((size_t)3 * n), vinfo((size_t)36 * n);
	for (int k = 0; k < n; k++)
	{
		if (pi[k] < 0 || pi[k] >= Pt || pj[k] < 0 || pj[k] >= Pt) throw ArgError{ "relative-pose edge: pose index out of range" };
		if (pi[k] == pj[k]) throw ArgError{ "relative-pose edge between a pose and itself" };
		vi[k] = pi[k]; vj[k] = pj[k];
		take_factor_values(vq.data(), vt.data(), vinfo.data(), k, q, t, info, "relative", "relative-pose");
	}
	// (the replaced set is a new set: the robust kernels of the previous one go with it)
	relSet.pi.swap(vi); relSet.pj.swap(vj); relSet.q.swap(vq); relSet.t.swap(vt); relSet.info.swap(vinfo);
	relSet.kind.clear(); relSet.delta.clear();
	collectBinaryPairs();
	forget_factor_memories(*this, relSet);
	pf.rel = DeviceRelPoses();
	// (the range factors between poses store or add into a block by whether these edges write it: their device copy is due again)
	prngSet.uploaded = false;
	covBlocksValid = false;          // (the covariance blocks describe the edge set -- and the block pattern -- they were computed on)
}

// the distinct free-free pairs of both binary kinds (caller's numbering, smaller index first): part of the topology -- need() rebuilds the
// structure when they differ from the pairs the current one was seeded with.  Either kind's setter recomputes the union, so that setting or
// clearing one kind keeps the other's pairs
void cuba_hip_solver::collectBinaryPairs()
{
	std::vector<uint64_t> pairs;
	const auto take = [&](const std::vector<int>& vi, const std::vector<int>& vj) {
		for (size_t k = 0; k < vi.size(); k++)
			if (vi[k] < Pf && vj[k] < Pf) pairs.push_back(((uint64_t)(uint32_t)std::min(vi[k], vj[k]) << 32) | (uint32_t)std::max(vi[k], vj[k]));
	};
	take(relSet.pi, relSet.pj);
	take(prngSet.pi, prngSet.pj);
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

// a caller's set of range factors, factor by factor (the scalar kind's counterpart of take_factors3): the pose index within [0, limit), the
// anchor, the lever arm (where given; zero otherwise) and the range finite, the range and the information not negative (0: no factor), the
// kernel a known one.  a: {anchor, range} (width 4), b: the arm.  kind / delta as take_factors3
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
		for (int i = 0; i < 3; i++)
		{
			if (!std::isfinite(anchor[3 * (size_t)k + i])) throw ArgError{ "non-finite " + noun + " anchor" };
			v.a[4 * (size_t)k + i] = anchor[3 * (size_t)k + i];
			if (!arm) continue;
			if (!std::isfinite(arm[3 * (size_t)k + i])) throw ArgError{ "non-finite " + noun + " lever arm" };
			v.b[3 * (size_t)k + i] = arm[3 * (size_t)k + i];
		}
		if (!std::isfinite(range[k])) throw ArgError{ "non-finite " + noun + " range" };
		if (range[k] < 0) throw ArgError{ "negative " + noun + " range" };
		v.a[4 * (size_t)k + 3] = range[k];
		if (!std::isfinite(info[k])) throw ArgError{ "non-finite " + noun + " information" };
		if (info[k] < 0) throw ArgError{ "negative " + noun + " information" };
		v.info[k] = info[k];
		if (kind)
		{
			check_factor_kernel(kind[k], delta[k], set.noun);
			any = any || kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE;
		}
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
	const std::string noun = prngSet.noun;
	std::vector<int> vi((size_t)n), vj((size_t)n), vk;
	std::vector<double> vai((size_t)3 * n, 0.0), vaj((size_t)3 * n, 0.0), vr((size_t)n), vinfo((size_t)n), vd;
	bool any = false;
	for (int k = 0; k < n; k++)
	{
		if (pi[k] < 0 || pi[k] >= Pt || pj[k] < 0 || pj[k] >= Pt) throw ArgError{ noun + ": pose index out of range" };
		if (pi[k] == pj[k]) throw ArgError{ noun + " between a pose and itself" };
		vi[k] = pi[k]; vj[k] = pj[k];
		for (size_t x = 3 * (size_t)k; x < 3 * (size_t)k + 3; x++)
		{
			if ((armI && !std::isfinite(armI[x])) || (armJ && !std::isfinite(armJ[x]))) throw ArgError{ "non-finite " + noun + " lever arm" };
			if (armI) vai[x] = armI[x];
			if (armJ) vaj[x] = armJ[x];
		}
		if (!std::isfinite(range[k])) throw ArgError{ "non-finite " + noun + " range" };
		if (range[k] < 0) throw ArgError{ "negative " + noun + " range" };
		vr[k] = range[k];
		if (!std::isfinite(info[k])) throw ArgError{ "non-finite " + noun + " information" };
		if (info[k] < 0) throw ArgError{ "negative " + noun + " information" };
		vinfo[k] = info[k];
		if (kind)
		{
			check_factor_kernel(kind[k], delta[k], prngSet.noun);
			any = any || kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE;
		}
	}
	if (any) { vk.assign(kind, kind + n); vd.assign(delta, delta + n); }
	prngSet.pi.swap(vi); prngSet.pj.swap(vj); prngSet.ai.swap(vai); prngSet.aj.swap(vaj); prngSet.range.swap(vr); prngSet.info.swap(vinfo);
	prngSet.kind.swap(vk); prngSet.delta.swap(vd);
	collectBinaryPairs();
	forget_factor_memories(*this, prngSet);
	pf.prng = DevicePoseRanges();
	covBlocksValid = false;          // (the covariance blocks describe the factors -- and the block pattern -- they were computed on)
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

// the edges' index arrays (`ints`, laid out by the caller) and their values q | t | information in the sorted order -> device; the device
// pointers of the values and of the per-factor chi2 come back through q, t, info, chi.  A set with robust kernels: their kinds follow the
// index arrays, their deltas the values, by the same permutation (rk_kind, rk_delta; null without)
static void upload_factor_arrays(cuba_hip_solver& s, RelPoseSet& set, std::vector<int> ints, const Scalar*& q, const Scalar*& t, const Scalar*& info, Scalar*& chi,
	const int*& rk_kind, const Scalar*& rk_delta)
{
	const size_t n = set.order.size();
	const bool robust = !set.kind.empty();
	const size_t nInts = ints.size();
	std::vector<Scalar> vals((robust ? 44 : 43) * n);
	Scalar* vq = vals.data(); Scalar* vt = vq + 4 * n; Scalar* vi = vt + 3 * n;
	for (size_t p = 0; p < n; p++)
	{
		const size_t k = (size_t)set.order[p];
		for (int i = 0; i < 4; i++) vq[4 * p + i] = (Scalar)set.q[4 * k + i];
		for (int i = 0; i < 3; i++) vt[3 * p + i] = (Scalar)set.t[3 * k + i];
		for (int i = 0; i < 36; i++) vi[36 * p + i] = (Scalar)set.info[36 * k + i];
		if (robust) { ints.push_back(set.kind[k]); vi[36 * n + p] = (Scalar)set.delta[k]; }
	}
	set.d_ints.upload(ints, s.stream);
	set.d_vals.upload(vals, s.stream);
	set.d_chi.resize(std::max(n, (size_t)1));
	q = set.d_vals.data(); t = q + 4 * n; info = t + 3 * n;
	chi = set.d_chi.data();
	rk_kind = robust ? set.d_ints.data() + nInts : nullptr; rk_delta = robust ? info + 36 * n : nullptr;
	s.sync();          // (the staging vectors go out of scope)
	set.uploaded = true;
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

// the caller's edges -> device, in the internal pose order: free-free edges first, stable by the block (min, max) of the internal pair -- a
// block's edges contiguous and in the caller's order --, then the edges with one fixed end, then (inactive) those with two
// (shared by the two binary kinds: sets set.order; blkKey: the (min << 32 | max) key of every block of blkId, ascending)
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

void RelPoseSet::upload(cuba_hip_solver& s)
{
	RelPoseSet& set = *this;
	const int n = set.n();
	const BinaryLayout lay = sort_binary_factors(s, set, set.pi, set.pj);
	const int nActive = lay.nActive, nb = (int)lay.blkId.size(), np = (int)lay.poseId.size();
	DeviceRelPoses rp;
	upload_factor_arrays(s, set, concat({ &lay.si, &lay.sj, &lay.blkPtr, &lay.blkId, &lay.posePtr, &lay.poseId, &lay.poseItem }), rp.q, rp.t, rp.info, rp.chi, rp.rk_kind,
		rp.rk_delta);
	s.d_relRec.resize((size_t)cubahip::REL_REC * std::max(n, 1));
	rp.n = n; rp.nActive = nActive; rp.nBlocks = nb; rp.nPoses = np;
	rp.pose_i = set.d_ints.data(); rp.pose_j = rp.pose_i + n;
	rp.blk_ptr = rp.pose_j + n; rp.blk_id = rp.blk_ptr + (nb + 1);
	rp.pose_ptr = rp.blk_id + nb; rp.pose_id = rp.pose_ptr + (np + 1); rp.pose_item = rp.pose_id + np;
	rp.rec = s.d_relRec.data();
	s.pf.rel = rp;
	set.structure = s.cntStructureBuilds;
}

// the caller's range factors between two poses -> device, sorted as the relative-pose edges.  blk_rel: the blocks that the relative-pose
// edges' gather writes too (it stores a block without Schur products, so this kind's gather, which runs behind it, adds there) -- this
// device copy depends on the structure AND on the relative-pose set: setRelativePoseEdges marks it due again.
// ints: pose_i [n] | pose_j [n] | blk_ptr [nb + 1] | blk_id [nb] | blk_rel [nb] | pose_ptr [np + 1] | pose_id [np] | pose_item | kind [n, robust]
// values: arm_i [3 n] | arm_j [3 n] | range [n] | info [n] | delta [n, robust]
void PoseRangeSet::upload(cuba_hip_solver& s)
{
	const size_t N = (size_t)n();
	const bool robust = !kind.empty();
	const BinaryLayout lay = sort_binary_factors(s, *this, pi, pj);
	std::vector<uint64_t> relKeys;
	for (int k = 0; k < s.relSet.n(); k++)
	{
		const int a = s.internalPose(s.relSet.pi[k]), b = s.internalPose(s.relSet.pj[k]);
		if (a < s.Pf && b < s.Pf) relKeys.push_back(((uint64_t)(uint32_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b));
	}
	std::sort(relKeys.begin(), relKeys.end());
	const int nb = (int)lay.blkId.size(), np = (int)lay.poseId.size();
	std::vector<int> blkRel((size_t)nb);
	for (int b = 0; b < nb; b++) blkRel[b] = std::binary_search(relKeys.begin(), relKeys.end(), lay.blkKey[b]) ? 1 : 0;
	std::vector<int> ints = concat({ &lay.si, &lay.sj, &lay.blkPtr, &lay.blkId, &blkRel, &lay.posePtr, &lay.poseId, &lay.poseItem });
	const size_t nInts = ints.size();
	std::vector<Scalar> vals((robust ? 9 : 8) * N);
	Scalar* vai = vals.data(); Scalar* vaj = vai + 3 * N; Scalar* vr = vaj + 3 * N; Scalar* vi = vr + N;
	for (size_t p = 0; p < N; p++)
	{
		const size_t k = (size_t)order[p];
		for (int i = 0; i < 3; i++) { vai[3 * p + i] = (Scalar)ai[3 * k + i]; vaj[3 * p + i] = (Scalar)aj[3 * k + i]; }
		vr[p] = (Scalar)range[k]; vi[p] = (Scalar)info[k];
		if (robust) { ints.push_back(kind[k]); vi[N + p] = (Scalar)delta[k]; }
	}
	d_ints.upload(ints, s.stream);
	d_vals.upload(vals, s.stream);
	d_chi.resize(std::max(N, (size_t)1));
	d_rec.resize((size_t)cubahip::PRNG_REC * std::max(N, (size_t)1));
	s.sync();          // (the staging vectors go out of scope)
	DevicePoseRanges pr;
	pr.n = (int)N; pr.nActive = lay.nActive; pr.nBlocks = nb; pr.nPoses = np;
	pr.pose_i = d_ints.data(); pr.pose_j = pr.pose_i + N;
	pr.blk_ptr = pr.pose_j + N; pr.blk_id = pr.blk_ptr + (nb + 1); pr.blk_rel = pr.blk_id + nb;
	pr.pose_ptr = pr.blk_rel + nb; pr.pose_id = pr.pose_ptr + (np + 1); pr.pose_item = pr.pose_id + np;
	pr.arm_i = d_vals.data(); pr.arm_j = pr.arm_i + 3 * N; pr.range = pr.arm_j + 3 * N; pr.info = pr.range + N;
	pr.rec = d_rec.data(); pr.chi = d_chi.data();
	pr.rk_kind = robust ? d_ints.data() + nInts : nullptr; pr.rk_delta = robust ? pr.info + N : nullptr;
	s.pf.prng = pr;
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
