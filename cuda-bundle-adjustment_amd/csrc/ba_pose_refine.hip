// ba_pose_refine.hip -- pose refinement on the device with the landmarks held: the value a pose gets from the current landmarks (g2o's
// motion-only bundle adjustment with EdgeSE3ProjectXYZOnlyPose, ORB-SLAM's Optimizer::PoseOptimization, the PnP refinement of a
// relocalisation candidate, which the reference lacks).  The mirror image of ba_triangulate.hip.  With every landmark held each free pose is
// a 6-parameter problem of its own: all its Levenberg-Marquardt trials and all its outlier rounds run inside ONE launch, every pose with a
// damping of its own.  The definition in full: include/cuba_hip.h (cuba_hip_refine_poses) and tests/pose_refinement_reference.py.  The only
// terms are the pose's reprojection edges of live information omega > 0; pose priors, relative-pose edges, position, direction and range
// factors take no part.
//
// ALL ARITHMETIC IS DOUBLE in both libraries (H mixes fx^2-scaled rotation and translation entries: the argument of DESIGN 7l); the state
// is read as Scalar and written as Scalar once, behind the last round.  The file carries its own double rotation / residual / Jacobian /
// exponential (the formulas of ba_math.hpp): nothing of ba_math.hpp or ba_device.hpp is routed through here, so no existing kernel's
// instructions move.
//
// Mapping: that of the pose pass.  Wave = one free pose, its lanes stride over the pose's entries of pe_edge (which include the edges to
// fixed landmarks).  An edge is evaluated from the raw state (q, t, camera, Xw, measurement, live omega), never from e_rec.  One PASS over the
// edges at a pose value gives H (21), b (6), F, the non-robust chi2, the edge count and a "depth <= 0" count: 31 sums, reduced by a
// butterfly in a fixed order so that every lane holds them; the 6 x 6 LDL^T solve and every decision are then done redundantly per lane:
// no LDS, no workgroup barrier, no atomics, and the control flow is wave-uniform.  A trial's pass at the candidate T' gives F' AND the
// linearisation there, so an accepted trial needs no second pass: 1 + iterations passes per round, one more for the final classification.
// A wave writes only its own pose and its own edges' scratch bytes.  Below the kernels: the handle's side.

#include "ba_solver.hpp"
#include "ba_device.hpp"

#include <cmath>

namespace cubahip
{

namespace
{
constexpr int PR_T = 256;
constexpr int PR_SUMS = 31;       // H[21] (upper triangle, entry (r, c) at c (c + 1) / 2 + r) | b[6] | F | sum omega |r|^2 | edges in | edges in with depth <= 0
constexpr int PR_B = 21, PR_F = 27, PR_CHI = 28, PR_N = 29, PR_BAD = 30;
constexpr int PR_PENDING = POSEREF_STATUSES;      // internal to a call, never reported: selected and free, for the wave kernel to decide

// rho(e) and rho'(e) (robust_rho / robust_weight of ba_math.hpp)
__device__ __forceinline__ void pr_robust(int kind, double delta, double e, double& rho, double& weight)
{
	const double d2 = delta * delta;
	rho = e; weight = 1;
	if (kind == ROBUST_HUBER && !(e <= d2))
	{
		const double s = sqrt(e);
		rho = 2 * s * delta - d2; weight = delta / s;
	}
	if (kind == ROBUST_TUKEY)
	{
		const double u = 1 - e / d2, top = (1.0 / 3) * d2;
		rho = e <= d2 ? top * (1 - u * u * u) : top;
		weight = e <= d2 ? u * u : 0.0;
	}
}

// (quat_to_rot of ba_math.hpp)
__device__ __forceinline__ void pr_rotation(const double q[4], double R[3][3])
{
	const double x = q[0], y = q[1], z = q[2], w = q[3];
	const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
	const double twx = tx * w, twy = ty * w, twz = tz * w;
	const double txx = tx * x, txy = ty * x, txz = tz * x;
	const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
	R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz;       R[0][2] = txz + twy;
	R[1][0] = txy + twz;       R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
	R[2][0] = txz - twy;       R[2][1] = tyz + twx;       R[2][2] = 1 - (txx + tyy);
}

// q (x) v (x) q^-1 (quat_rotate of ba_math.hpp)
__device__ __forceinline__ void pr_quat_rotate(const double q[4], const double v[3], double out[3])
{
	double a0 = q[1] * v[2] - q[2] * v[1];
	double a1 = q[2] * v[0] - q[0] * v[2];
	double a2 = q[0] * v[1] - q[1] * v[0];
	a0 += a0; a1 += a1; a2 += a2;
	out[0] = v[0] + q[3] * a0 + (q[1] * a2 - q[2] * a1);
	out[1] = v[1] + q[3] * a1 + (q[2] * a0 - q[0] * a2);
	out[2] = v[2] + q[3] * a2 + (q[0] * a1 - q[1] * a0);
}

template <int I, int J, int K>
__device__ __forceinline__ void pr_shepperd_branch(const double (&R)[3][3], double (&qe)[4])
{
	double tr = sqrt(R[I][I] - R[J][J] - R[K][K] + 1);
	qe[I] = 0.5 * tr;
	tr = 0.5 / tr;
	qe[3] = (R[K][J] - R[J][K]) * tr;
	qe[J] = (R[J][I] + R[I][J]) * tr;
	qe[K] = (R[K][I] + R[I][K]) * tr;
}

// T <- exp([omega; upsilon]) T (pose_exp_update of ba_math.hpp, in double)
__device__ __forceinline__ void pr_exp_update(const double upd[6], double q[4], double t[3])
{
	const double wx = upd[0], wy = upd[1], wz = upd[2];
	const double theta = sqrt(wx * wx + wy * wy + wz * wz);
	double a1, a2, a3;
	if (theta < 0.00001) { a1 = 1; a2 = 0.5; a3 = 1.0 / 6; }
	else
	{
		const double sn = sin(theta), cs = cos(theta);
		a1 = sn / theta;
		a2 = (1 - cs) / (theta * theta);
		a3 = (theta - sn) / (theta * theta * theta);
	}
	const double xx = wx * wx, yy = wy * wy, zz = wz * wz, xy = wx * wy, yz = wy * wz, zx = wz * wx;
	const double K[3][3] = { { 0, -wz, wy }, { wz, 0, -wx }, { -wy, wx, 0 } };
	const double K2[3][3] = { { -yy - zz, xy, zx }, { xy, -zz - xx, yz }, { zx, yz, -xx - yy } };
	double R[3][3], te[3];
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
		double acc = 0;
#pragma unroll
		for (int j = 0; j < 3; j++)
		{
			const double I = (i == j) ? 1.0 : 0.0;
			R[i][j] = I + a1 * K[i][j] + a2 * K2[i][j];
			acc += (I + a2 * K[i][j] + a3 * K2[i][j]) * upd[3 + j];
		}
		te[i] = acc;
	}
	double qe[4];
	double tr = R[0][0] + R[1][1] + R[2][2];
	if (tr > 0)
	{
		tr = sqrt(tr + 1);
		qe[3] = 0.5 * tr;
		tr = 0.5 / tr;
		qe[0] = (R[2][1] - R[1][2]) * tr;
		qe[1] = (R[0][2] - R[2][0]) * tr;
		qe[2] = (R[1][0] - R[0][1]) * tr;
	}
	else
	{
		const bool c1 = R[1][1] > R[0][0];
		const bool c2 = R[2][2] > (c1 ? R[1][1] : R[0][0]);
		if (c2) pr_shepperd_branch<2, 0, 1>(R, qe);
		else if (c1) pr_shepperd_branch<1, 2, 0>(R, qe);
		else pr_shepperd_branch<0, 1, 2>(R, qe);
	}
	double u[3];
	pr_quat_rotate(qe, t, u);
	t[0] = te[0] + u[0]; t[1] = te[1] + u[1]; t[2] = te[2] + u[2];
	double c[4];
	c[3] = qe[3] * q[3] - qe[0] * q[0] - qe[1] * q[1] - qe[2] * q[2];
	c[0] = qe[3] * q[0] + qe[0] * q[3] + qe[1] * q[2] - qe[2] * q[1];
	c[1] = qe[3] * q[1] + qe[1] * q[3] + qe[2] * q[0] - qe[0] * q[2];
	c[2] = qe[3] * q[2] + qe[2] * q[3] + qe[0] * q[1] - qe[1] * q[0];
	double invn = 1 / sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
	if (c[3] < 0) invn = -invn;
	q[0] = invn * c[0]; q[1] = invn * c[1]; q[2] = invn * c[2]; q[3] = invn * c[3];
}

// One pass over the pose's edges [p0, p1) of pe_edge at the pose value (q, t): the 31 sums, in every lane.
//   CLASSIFY  the edge's scratch byte is decided here -- omega > 0, depth > 0 and (chi_test) omega |r|^2 <= chi2_max[stereo], a NaN fails --
//             and written; otherwise it is read (this lane wrote it: the same lane meets the same entry in every pass).
//   robust    the handle's robust kernels (rounds below robust_rounds) or the identity kernel
template <bool CLASSIFY>
__device__ __forceinline__ void pr_pass(const PoseRefineArgs& a, int p0, int p1, int lane, const double q[4], const double t[3], const double cam[5],
	bool chi_test, bool robust, double (&s)[PR_SUMS])
{
	const DeviceGraph& g = a.g;
	double R[3][3];
	pr_rotation(q, R);
#pragma unroll
	for (int k = 0; k < PR_SUMS; k++) s[k] = 0;
	for (int p = p0 + lane; p < p1; p += WAVE)
	{
		const int e = a.pe_edge[p];
		const double w = (double)g.e_w[e];
		if (!(w > 0))
		{
			if (CLASSIFY) a.cls[e] = 0;
			continue;
		}
		if (!CLASSIFY && !a.cls[e]) continue;
		const bool stereo = (g.e_pose[e] & STEREO_BIT) != 0;
		const size_t il = (size_t)g.e_lm[e];
		const double X[3] = { (double)g.Xw[3 * il], (double)g.Xw[3 * il + 1], (double)g.Xw[3 * il + 2] };
		const double m[3] = { (double)g.e_mu[e], (double)g.e_mv[e], stereo ? (double)g.e_mr[e] : 0.0 };
		double Xc[3], r[3];
#pragma unroll
		for (int i = 0; i < 3; i++) Xc[i] = R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i];
		// (edge_residual of ba_math.hpp)
		const double invZ = 1 / Xc[2], invZZ = invZ * invZ;
		const double u = cam[0] * invZ * Xc[0] + cam[2];
		const double v = cam[1] * invZ * Xc[1] + cam[3];
		r[0] = u - m[0];
		r[1] = v - m[1];
		r[2] = stereo ? (u - cam[4] * invZ) - m[2] : 0.0;
		const double chi = w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
		if (CLASSIFY)
		{
			const bool in = Xc[2] > 0 && (!chi_test || chi <= (stereo ? a.chi2_stereo : a.chi2_mono));
			a.cls[e] = in ? 1 : 0;
			if (!in) continue;
		}
		s[PR_N] += 1;
		if (!(Xc[2] > 0)) s[PR_BAD] += 1;
		double rho, wr;
		pr_robust(robust ? (stereo ? g.rk[1].kind : g.rk[0].kind) : ROBUST_NONE, (double)(stereo ? g.rk[1].delta : g.rk[0].delta), chi, rho, wr);
		wr *= w;
		s[PR_F] += rho;
		s[PR_CHI] += chi;
		// (the pose half of edge_jacobians: J = -d proj / d [omega; upsilon] for T <- exp([omega; upsilon]) T)
		const double Xx = Xc[0], Yy = Xc[1];
		const double fu = cam[0], fv = cam[1], bf = stereo ? cam[4] : 0.0, sf = stereo ? 1.0 : 0.0;
		double J[3][6];
		J[0][0] = Xx * Yy * invZZ * fu;
		J[0][1] = -(1 + (Xx * Xx * invZZ)) * fu;
		J[0][2] = Yy * invZ * fu;
		J[0][3] = -invZ * fu;
		J[0][4] = 0;
		J[0][5] = Xx * invZZ * fu;
		J[1][0] = (1 + Yy * Yy * invZZ) * fv;
		J[1][1] = -Xx * Yy * invZZ * fv;
		J[1][2] = -Xx * invZ * fv;
		J[1][3] = 0;
		J[1][4] = -invZ * fv;
		J[1][5] = Yy * invZZ * fv;
		J[2][0] = sf * (J[0][0] - bf * Yy * invZZ);
		J[2][1] = sf * (J[0][1] + bf * Xx * invZZ);
		J[2][2] = sf * J[0][2];
		J[2][3] = sf * J[0][3];
		J[2][4] = 0;
		J[2][5] = sf * (J[0][5] - bf * invZZ);
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
#pragma unroll
			for (int rr = 0; rr <= c; rr++) s[c * (c + 1) / 2 + rr] += wr * (J[0][rr] * J[0][c] + J[1][rr] * J[1][c] + J[2][rr] * J[2][c]);
			s[PR_B + c] += wr * (J[0][c] * r[0] + J[1][c] * r[1] + J[2][c] * r[2]);
		}
	}
#pragma unroll
	for (int k = 0; k < PR_SUMS; k++)
	{
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
	}
}

// (H + lambda I) d = b by a 6 x 6 LDL^T; false: a non-positive pivot or a non-finite number
__device__ __forceinline__ bool pr_solve(const double (&s)[PR_SUMS], double lambda, double d[6])
{
	double L[6][6], D[6];
	bool ok = true;
#pragma unroll
	for (int j = 0; j < 6; j++)
	{
		double p = s[j * (j + 1) / 2 + j] + lambda;
#pragma unroll
		for (int k = 0; k < j; k++) p -= L[j][k] * L[j][k] * D[k];
		if (!(p > 0)) ok = false;
		D[j] = p;
		const double ip = 1 / p;
#pragma unroll
		for (int i = j + 1; i < 6; i++)
		{
			double v = s[i * (i + 1) / 2 + j];
#pragma unroll
			for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
			L[i][j] = v * ip;
		}
	}
	double y[6];
#pragma unroll
	for (int i = 0; i < 6; i++)
	{
		double v = s[PR_B + i];
#pragma unroll
		for (int k = 0; k < i; k++) v -= L[i][k] * y[k];
		y[i] = v;
	}
#pragma unroll
	for (int i = 5; i >= 0; i--)
	{
		double v = y[i] / D[i];
#pragma unroll
		for (int k = i + 1; k < 6; k++) v -= L[k][i] * d[k];
		d[i] = v;
		if (!isfinite(v)) ok = false;
	}
	return ok;
}

// Entry i of max(Pt, E): what is decided without looking at an edge.  Pose i of the caller's numbering: NOT_SELECTED / FIXED / the
// internal "pending" mark, no inliers, chi2 0.  Sorted edge i: its scratch byte = its live information is positive (what edge_inlier
// reports for an edge of a pose that does not reach the final classification).
__global__ __launch_bounds__(PR_T) void pose_refine_init_kernel(PoseRefineArgs a, const uint8_t* __restrict__ select, const int* __restrict__ newOfOld)
{
	const int i = blockIdx.x * PR_T + threadIdx.x;
	if (i < a.g.Pt)
	{
		const int m = newOfOld && i < a.g.Pf ? newOfOld[i] : i;
		a.status[m] = select && !select[i] ? POSEREF_NOT_SELECTED : i >= a.g.Pf ? POSEREF_FIXED : PR_PENDING;
		a.inliers[m] = 0;
		a.chi2[m] = 0;
	}
	if (i < a.g.E) a.cls[i] = (double)a.g.e_w[i] > 0 ? 1 : 0;
}

// wave = one free pose (internal order), lane-strided over its entries of pe_edge; every lane holds every sum and takes every decision
__global__ __launch_bounds__(PR_T) void pose_refine_kernel(PoseRefineArgs a)
{
	const DeviceGraph& g = a.g;
	const int lane = threadIdx.x & (WAVE - 1);
	const int ip = blockIdx.x * (PR_T / WAVE) + threadIdx.x / WAVE;
	if (ip >= g.Pf) return;
	if (a.status[ip] != PR_PENDING) return;
	const int p0 = a.pe_beg[ip], p1 = a.pe_end[ip];
	double q[4], t[3], cam[5];
#pragma unroll
	for (int k = 0; k < 4; k++) q[k] = (double)g.q[4 * (size_t)ip + k];
#pragma unroll
	for (int k = 0; k < 3; k++) t[k] = (double)g.t[3 * (size_t)ip + k];
#pragma unroll
	for (int k = 0; k < 5; k++) cam[k] = (double)g.cam[5 * (size_t)ip + k];
	const double need_in = (double)max(3, a.min_inliers);
	int status = POSEREF_OK;
	double s[PR_SUMS];
	bool final_reached = false;
	for (int round = 0; round < a.rounds && status == POSEREF_OK; round++)
	{
		const bool robust = round < a.robust_rounds;
		pr_pass<true>(a, p0, p1, lane, q, t, cam, round > 0, robust, s);
		if (round == 0 ? s[PR_N] < 3 : s[PR_N] < need_in) { status = round == 0 ? POSEREF_FEW_OBSERVATIONS : POSEREF_FEW_INLIERS; break; }
		double hmax = s[0];
#pragma unroll
		for (int k = 1; k < 6; k++) hmax = fmax(hmax, s[k * (k + 1) / 2 + k]);
		double lambda = 1e-5 * hmax, nu = 2;
		for (int it = 0; it < a.iterations; it++)
		{
			double d[6];
			if (!pr_solve(s, lambda, d)) { status = POSEREF_SINGULAR; break; }
			double q2[4] = { q[0], q[1], q[2], q[3] }, t2[3] = { t[0], t[1], t[2] };
			pr_exp_update(d, q2, t2);
			double s2[PR_SUMS];
			pr_pass<false>(a, p0, p1, lane, q2, t2, cam, false, robust, s2);
			double den = 0;
#pragma unroll
			for (int k = 0; k < 6; k++) den += d[k] * (lambda * d[k] + s[PR_B + k]);
			const double gain = (s[PR_F] - s2[PR_F]) / den;
			if (s2[PR_BAD] == 0 && isfinite(s2[PR_F]) && den != 0 && gain > 0)      // (den == 0: d = 0, nothing to gain -- rejected, as in the reference)
			{
#pragma unroll
				for (int k = 0; k < 4; k++) q[k] = q2[k];
#pragma unroll
				for (int k = 0; k < 3; k++) t[k] = t2[k];
#pragma unroll
				for (int k = 0; k < PR_SUMS; k++) s[k] = s2[k];
				const double c = 2 * gain - 1;
				lambda *= fmax(1.0 / 3, 1 - c * c * c);
				nu = 2;
			}
			else { lambda *= nu; nu *= 2; }
		}
	}
	if (status == POSEREF_OK)
	{
		pr_pass<true>(a, p0, p1, lane, q, t, cam, true, false, s);
		final_reached = true;
		if (s[PR_N] < need_in) status = POSEREF_FEW_INLIERS;
	}
	else
	{
		// (no final classification: the pose's edges report whether their live information is positive)
		for (int p = p0 + lane; p < p1; p += WAVE) { const int e = a.pe_edge[p]; a.cls[e] = (double)g.e_w[e] > 0 ? 1 : 0; }
	}
	if (lane == 0)
	{
		a.status[ip] = status;
		a.inliers[ip] = (int)s[PR_N];
		a.chi2[ip] = final_reached ? s[PR_CHI] : 0.0;
		if (status == POSEREF_OK)
		{
#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const Scalar x = (Scalar)q[k];
				a.qt[7 * (size_t)ip + k] = (double)x;
				if (!a.dry_run) g.q[4 * (size_t)ip + k] = x;
			}
#pragma unroll
			for (int k = 0; k < 3; k++)
			{
				const Scalar x = (Scalar)t[k];
				a.qt[7 * (size_t)ip + 4 + k] = (double)x;
				if (!a.dry_run) g.t[3 * (size_t)ip + k] = x;
			}
		}
	}
}

// Pose p of the caller's numbering: status, inliers, chi2 and pose out of the internal order, the statuses counted per workgroup.
__global__ __launch_bounds__(PR_T) void pose_refine_collect_kernel(PoseRefineArgs a, const int* __restrict__ newOfOld, int* __restrict__ statusOut,
	int* __restrict__ inliersOut, double* __restrict__ chi2Out, double* __restrict__ qOut, double* __restrict__ tOut, long long* __restrict__ parts)
{
	__shared__ int red[PR_T / WAVE][POSEREF_STATUSES];
	const int Pt = a.g.Pt;
	int cnt[POSEREF_STATUSES] = { 0, 0, 0, 0, 0, 0 };     // wave-uniform
	// (whole waves walk the loop together: the ballots need every lane of the wave)
	for (int base = blockIdx.x * PR_T; base < Pt; base += gridDim.x * PR_T)
	{
		const int p = base + threadIdx.x;
		int s = -1;
		if (p < Pt)
		{
			const size_t m = (size_t)(newOfOld && p < a.g.Pf ? newOfOld[p] : p);
			s = a.status[m];
			statusOut[p] = s;
			inliersOut[p] = a.inliers[m];
			chi2Out[p] = a.chi2[m];
#pragma unroll
			for (int k = 0; k < 4; k++) qOut[4 * (size_t)p + k] = s == POSEREF_OK ? a.qt[7 * m + k] : (double)a.g.q[4 * m + k];
#pragma unroll
			for (int k = 0; k < 3; k++) tOut[3 * (size_t)p + k] = s == POSEREF_OK ? a.qt[7 * m + 4 + k] : (double)a.g.t[3 * m + k];
		}
#pragma unroll
		for (int k = 0; k < POSEREF_STATUSES; k++) cnt[k] += __popcll(__ballot(s == k));
	}
	if ((threadIdx.x & (WAVE - 1)) == 0)
#pragma unroll
		for (int k = 0; k < POSEREF_STATUSES; k++) red[threadIdx.x / WAVE][k] = cnt[k];
	__syncthreads();
	if (threadIdx.x < POSEREF_STATUSES)
	{
		long long s = 0;
#pragma unroll
		for (int w = 0; w < PR_T / WAVE; w++) s += red[w][threadIdx.x];
		parts[(size_t)POSEREF_STATUSES * blockIdx.x + threadIdx.x] = s;
	}
}

// second stage: one wave adds the n workgroups' partials, lane-strided, then across the lanes
__global__ __launch_bounds__(WAVE) void pose_refine_counts_kernel(const long long* __restrict__ parts, int n, long long* __restrict__ out)
{
	long long s[POSEREF_STATUSES] = { 0, 0, 0, 0, 0, 0 };
	for (int i = threadIdx.x; i < n; i += WAVE)
#pragma unroll
		for (int k = 0; k < POSEREF_STATUSES; k++) s[k] += parts[(size_t)POSEREF_STATUSES * i + k];
#pragma unroll
	for (int k = 0; k < POSEREF_STATUSES; k++)
	{
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
		if (threadIdx.x == 0) out[k] = s[k];
	}
}
}  // namespace

int pose_refine_collect_grid(int Pt) { return Pt > 0 ? min((Pt + PR_T - 1) / PR_T, 1024) : 0; }

void launch_pose_refine(const PoseRefineArgs& a, const uint8_t* select, const int* newOfOld, hipStream_t s)
{
	const int n = max(a.g.Pt, a.g.E);
	if (n > 0) hipLaunchKernelGGL(pose_refine_init_kernel, dim3((n + PR_T - 1) / PR_T), dim3(PR_T), 0, s, a, select, newOfOld);
	if (a.g.Pf > 0) hipLaunchKernelGGL(pose_refine_kernel, dim3((a.g.Pf + PR_T / WAVE - 1) / (PR_T / WAVE)), dim3(PR_T), 0, s, a);
}

void launch_pose_refine_collect(const PoseRefineArgs& a, const int* newOfOld, int* statusOut, int* inliersOut, double* chi2Out, double* qOut, double* tOut,
	long long* parts, long long* counts, hipStream_t s)
{
	const int grid = pose_refine_collect_grid(a.g.Pt);
	if (grid > 0) hipLaunchKernelGGL(pose_refine_collect_kernel, dim3(grid), dim3(PR_T), 0, s, a, newOfOld, statusOut, inliersOut, chi2Out, qOut, tOut, parts);
	hipLaunchKernelGGL(pose_refine_counts_kernel, dim3(1), dim3(WAVE), 0, s, parts, grid, counts);
}

}  // namespace cubahip

// ---------------------------------------------------------------------------------------------------------------------------------------
// The handle's side.  Nothing is kept between calls but the buffers: every call decides every pose afresh.  The handle's gate is read
// only through the live information and never written; the classification of a call lives in d_prCls.
// ---------------------------------------------------------------------------------------------------------------------------------------
void cuba_hip_solver::refinePoses(const uint8_t* select, int rounds, int iterations, int robustRounds, const double chi2Max[2], int minInliers, bool dryRun,
	int32_t* status, int64_t* counts, int32_t* inliers, double* chi2, double* q, double* t, uint8_t* edgeInlier)
{
	if (rounds < 1 || rounds > POSEREF_MAX_ROUNDS) throw ArgError{ "rounds must lie in 1 ... 4" };
	if (iterations < 1 || iterations > POSEREF_MAX_ITERATIONS) throw ArgError{ "iterations must lie in 1 ... 32" };
	if (robustRounds < 0 || robustRounds > rounds) throw ArgError{ "robust_rounds must lie in 0 ... rounds" };
	if (minInliers < 0) throw ArgError{ "min_inliers must not be negative" };
	if (!chi2Max || std::isnan(chi2Max[0]) || std::isnan(chi2Max[1])) throw ArgError{ "chi2_max must be two numbers (+inf: no chi2 test)" };
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (partHi >= 0) throw StateError{ "pose refinement is not available on a landmark-partitioned handle" };
	need();
	PoseRefineArgs a;
	a.g = g;
	a.pe_beg = st.pe_beg; a.pe_end = st.pe_end; a.pe_edge = st.pe_edge;
	a.rounds = rounds; a.iterations = iterations; a.robust_rounds = robustRounds; a.min_inliers = minInliers;
	a.chi2_mono = chi2Max[0]; a.chi2_stereo = chi2Max[1];
	a.dry_run = dryRun ? 1 : 0;
	const int grid = pose_refine_collect_grid(Pt);
	// [status | inliers] in the internal order, then in the caller's; [chi2 | q t] in the internal order, then [chi2 | q | t] in the caller's
	d_prInt.resize((size_t)4 * Pt); d_prReal.resize((size_t)16 * Pt);
	d_prCls.resize((size_t)2 * E);
	d_prCounts.resize((size_t)POSEREF_STATUSES * (1 + grid));
	a.status = d_prInt.data(); a.inliers = d_prInt.data() + Pt;
	a.chi2 = d_prReal.data(); a.qt = d_prReal.data() + Pt;
	a.cls = d_prCls.data();
	if (select && Pt) d_prSelect.uploadRaw(select, (size_t)Pt, stream);
	const int* newOfOld = reorderActive ? d_poseMap.data() : nullptr;
	int* statusOut = d_prInt.data() + 2 * (size_t)Pt;
	int* inliersOut = statusOut + Pt;
	double* chi2Out = d_prReal.data() + 8 * (size_t)Pt;
	double* qOut = chi2Out + Pt;
	double* tOut = qOut + 4 * (size_t)Pt;
	launch_pose_refine(a, select && Pt ? d_prSelect.data() : nullptr, newOfOld, stream);
	launch_pose_refine_collect(a, newOfOld, statusOut, inliersOut, chi2Out, qOut, tOut, d_prCounts.data() + POSEREF_STATUSES, d_prCounts.data(), stream);
	long long h[POSEREF_STATUSES];
	HIP_TRY(hipMemcpyAsync(h, d_prCounts.data(), sizeof h, hipMemcpyDeviceToHost, stream));
	if (status && Pt) HIP_TRY(hipMemcpyAsync(status, statusOut, sizeof(int32_t) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (inliers && Pt) HIP_TRY(hipMemcpyAsync(inliers, inliersOut, sizeof(int32_t) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (chi2 && Pt) HIP_TRY(hipMemcpyAsync(chi2, chi2Out, sizeof(double) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (q && Pt) HIP_TRY(hipMemcpyAsync(q, qOut, sizeof(double) * 4 * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (t && Pt) HIP_TRY(hipMemcpyAsync(t, tOut, sizeof(double) * 3 * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (edgeInlier && E)
	{
		launch_gate_unsort(permDevice(), d_prCls.data(), E, d_prCls.data() + E, stream);
		HIP_TRY(hipMemcpyAsync(edgeInlier, d_prCls.data() + E, (size_t)E, hipMemcpyDeviceToHost, stream));
	}
	sync();
	if (!dryRun && h[POSEREF_OK] > 0) covBlocksValid = false;
	if (counts) for (int k = 0; k < POSEREF_STATUSES; k++) counts[k] = h[k];
}
