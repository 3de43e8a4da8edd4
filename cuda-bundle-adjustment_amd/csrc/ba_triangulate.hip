// ba_triangulate.hip -- landmark triangulation on the device: the position a free landmark has BEFORE it is optimised (g2o's
// StructureOnlySolver<3>, ORB-SLAM's CreateNewMapPoints, which the reference lacks), from its active reprojection edges -- live information
// omega > 0, so a gated edge is out -- and the current pose estimates.  Per landmark: a linear start (the DLT rows of every edge, weighted
// by omega, through the 3 x 3 normal equations), `iterations` Gauss-Newton steps on the robustified reprojection cost with the poses held
// (the terms of the landmark pass: H = sum w' JL^T JL, h = sum w' JL^T r, X += H^-1 h), then the acceptance tests.  The definition in full:
// include/cuba_hip.h (cuba_hip_triangulate_landmarks) and tests/triangulation_reference.py.  Landmark priors take no part.
//
// ALL ARITHMETIC IS DOUBLE in both libraries: the rows have entries of order fx^2 n and the normal equations condition numbers of
// 1e4 - 1e5, which leaves an fp32 solve two or three digits.  The state is read as Scalar and written as Scalar.  The file carries its own
// double residual / Jacobian / inverse (the formulas of ba_math.hpp): nothing of ba_math.hpp or ba_device.hpp is routed through here, so no
// existing kernel's instructions move.
//
// Mapping: that of the landmark pass.  Wave = one entry of wave_lm, lane = sorted edge; every lane keeps its edge (rotation, translation,
// camera, measurement, omega) in registers over all steps, puts its terms into the wave's LDS rows, the landmark's head lane adds its
// segment front to back, solves, and publishes the new position through LDS for the lanes of its segment -- wave_lds_sync between, no
// workgroup barrier.  A landmark of the big_lm class (more than 64 edges) has a 256-thread workgroup: a strided loop over its edges, a wave
// sum, the four waves' sums added by thread 0.  No atomics, every sum in a fixed order.  The status counts are wave ballots into
// per-workgroup partials added by a second stage (as in ba_gate.hip).  Below the kernels: the handle's side.

#include "ba_solver.hpp"
#include "ba_device.hpp"

#include <cmath>

namespace cubahip
{

namespace
{
constexpr int TRI_T = 256;
constexpr int TRI_START = 14;     // a lane's numbers in the linear start's sum: A[6] | g[3] | unit ray [3] | active | stereo with positive disparity
constexpr int TRI_GN = 9;         // ... in a Gauss-Newton step's: H[6] | h[3]
constexpr int TRI_FLAGS = 2;      // ... in the acceptance's: behind the camera | over the chi2 threshold
constexpr int TRI_PUB = 4;        // what a head publishes: X[3] | 1 = the landmark is still in the running
constexpr int TRI_PENDING = TRI_STATUSES;      // internal to a call, never reported: selected and free, for the edge kernels to decide

// one reprojection edge as a lane keeps it.  on = false (no edge, an edge of a landmark that is not triangulated, omega <= 0 or NaN):
// nothing else is set and every term of the lane is an exact zero
struct TriEdge
{
	bool on, stereo;
	double R[3][3], t[3], cam[5], m[3], w;
};

__device__ __forceinline__ void tri_load(const DeviceGraph& g, int e, TriEdge& ed)
{
	ed.w = (double)g.e_w[e];
	ed.on = ed.w > 0;
	if (!ed.on) return;
	const int pe = g.e_pose[e];
	ed.stereo = (pe & STEREO_BIT) != 0;
	const size_t ip = (size_t)(pe & ~STEREO_BIT);
	const double x = (double)g.q[4 * ip], y = (double)g.q[4 * ip + 1], z = (double)g.q[4 * ip + 2], w = (double)g.q[4 * ip + 3];
	// (quat_to_rot of ba_math.hpp)
	const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
	const double twx = tx * w, twy = ty * w, twz = tz * w;
	const double txx = tx * x, txy = ty * x, txz = tz * x;
	const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
	ed.R[0][0] = 1 - (tyy + tzz); ed.R[0][1] = txy - twz;       ed.R[0][2] = txz + twy;
	ed.R[1][0] = txy + twz;       ed.R[1][1] = 1 - (txx + tzz); ed.R[1][2] = tyz - twx;
	ed.R[2][0] = txz - twy;       ed.R[2][1] = tyz + twx;       ed.R[2][2] = 1 - (txx + tyy);
#pragma unroll
	for (int i = 0; i < 3; i++) ed.t[i] = (double)g.t[3 * ip + i];
#pragma unroll
	for (int i = 0; i < 5; i++) ed.cam[i] = (double)g.cam[5 * ip + i];
	ed.m[0] = (double)g.e_mu[e]; ed.m[1] = (double)g.e_mv[e]; ed.m[2] = ed.stereo ? (double)g.e_mr[e] : 0.0;
}

// the edge's part of A = sum omega a a^T, g = sum omega a b over its two or three rows a X = b, its unit ray in the world frame, 1, and
// 1 for a stereo edge of positive disparity
__device__ __forceinline__ void tri_start_terms(const TriEdge& ed, double v[TRI_START])
{
#pragma unroll
	for (int k = 0; k < TRI_START; k++) v[k] = 0;
	if (!ed.on) return;
	const double fx = ed.cam[0], fy = ed.cam[1], cx = ed.cam[2], cy = ed.cam[3], bf = ed.cam[4];
	const double du = cx - ed.m[0], dv = cy - ed.m[1], dr = cx - ed.m[2];
	const double s = ed.stereo ? 1.0 : 0.0;
	double a[3][3], b[3];
#pragma unroll
	for (int j = 0; j < 3; j++)
	{
		a[0][j] = fx * ed.R[0][j] + du * ed.R[2][j];
		a[1][j] = fy * ed.R[1][j] + dv * ed.R[2][j];
		a[2][j] = s * (fx * ed.R[0][j] + dr * ed.R[2][j]);
	}
	b[0] = -(fx * ed.t[0] + du * ed.t[2]);
	b[1] = -(fy * ed.t[1] + dv * ed.t[2]);
	b[2] = s * (bf - (fx * ed.t[0] + dr * ed.t[2]));
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
#pragma unroll
		for (int j = i; j < 3; j++) v[sym3_idx(i, j)] = ed.w * (a[0][i] * a[0][j] + a[1][i] * a[1][j] + a[2][i] * a[2][j]);
		v[6 + i] = ed.w * (a[0][i] * b[0] + a[1][i] * b[1] + a[2][i] * b[2]);
	}
	const double nx = -du / fx, ny = -dv / fy;
	const double inv = 1 / sqrt(nx * nx + ny * ny + 1);
	const double d[3] = { nx * inv, ny * inv, inv };
#pragma unroll
	for (int j = 0; j < 3; j++) v[9 + j] = ed.R[0][j] * d[0] + ed.R[1][j] * d[1] + ed.R[2][j] * d[2];
	v[12] = 1;
	v[13] = ed.stereo && ed.m[0] - ed.m[2] > 0 ? 1.0 : 0.0;
}

// X in the camera frame and the residual proj - meas (edge_residual of ba_math.hpp, the rotation as a matrix); returns |r|^2
__device__ __forceinline__ double tri_residual(const TriEdge& ed, const double X[3], double Xc[3], double r[3])
{
#pragma unroll
	for (int i = 0; i < 3; i++) Xc[i] = ed.R[i][0] * X[0] + ed.R[i][1] * X[1] + ed.R[i][2] * X[2] + ed.t[i];
	const double invZ = 1 / Xc[2];
	const double u = ed.cam[0] * invZ * Xc[0] + ed.cam[2];
	const double v = ed.cam[1] * invZ * Xc[1] + ed.cam[3];
	r[0] = u - ed.m[0];
	r[1] = v - ed.m[1];
	r[2] = ed.stereo ? (u - ed.cam[4] * invZ) - ed.m[2] : 0.0;
	return r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
}

// rho'(e) (robust_weight of ba_math.hpp)
__device__ __forceinline__ double tri_robust_weight(int kind, double delta, double e)
{
	const double d2 = delta * delta;
	if (kind == ROBUST_HUBER) return e <= d2 ? 1.0 : delta / sqrt(e);
	if (kind == ROBUST_TUKEY)
	{
		const double u = 1 - e / d2;
		return e <= d2 ? u * u : 0.0;
	}
	return 1;
}

// the edge's part of H = sum w' JL^T JL and h = sum w' JL^T r at X, w' = omega rho'(omega |r|^2), JL = -d proj / d X (edge_jacobians)
__device__ __forceinline__ void tri_gn_terms(const TriEdge& ed, const double X[3], const RobustKernel (&rk)[2], double v[TRI_GN])
{
#pragma unroll
	for (int k = 0; k < TRI_GN; k++) v[k] = 0;
	if (!ed.on) return;
	double Xc[3], r[3];
	const double chi = ed.w * tri_residual(ed, X, Xc, r);
	const int kind = ed.stereo ? rk[1].kind : rk[0].kind;
	const double delta = (double)(ed.stereo ? rk[1].delta : rk[0].delta);
	const double wr = ed.w * tri_robust_weight(kind, delta, chi);
	const double invZ = 1 / Xc[2], invZZ = invZ * invZ;
	const double fu = ed.cam[0], fv = ed.cam[1], bf = ed.stereo ? ed.cam[4] : 0.0, s = ed.stereo ? 1.0 : 0.0;
	double JL[3][3];
#pragma unroll
	for (int j = 0; j < 3; j++)
	{
		JL[0][j] = -fu * ed.R[0][j] * invZ + fu * Xc[0] * ed.R[2][j] * invZZ;
		JL[1][j] = -fv * ed.R[1][j] * invZ + fv * Xc[1] * ed.R[2][j] * invZZ;
		JL[2][j] = s * (JL[0][j] - bf * ed.R[2][j] * invZZ);
	}
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
#pragma unroll
		for (int j = i; j < 3; j++) v[sym3_idx(i, j)] = wr * (JL[0][i] * JL[0][j] + JL[1][i] * JL[1][j] + JL[2][i] * JL[2][j]);
		v[6 + i] = wr * (JL[0][i] * r[0] + JL[1][i] * r[1] + JL[2][i] * r[2]);
	}
}

__device__ __forceinline__ void tri_accept_terms(const TriEdge& ed, const double X[3], const TriangulateArgs& a, double v[TRI_FLAGS])
{
	v[0] = 0; v[1] = 0;
	if (!ed.on) return;
	double Xc[3], r[3];
	const double chi = ed.w * tri_residual(ed, X, Xc, r);
	v[0] = Xc[2] <= 0 ? 1.0 : 0.0;
	v[1] = chi > (ed.stereo ? a.chi2_stereo : a.chi2_mono) ? 1.0 : 0.0;
}

// x = A^-1 b through the adjugate (sym3_inverse of ba_math.hpp); false: det <= 0 or a non-finite number
__device__ __forceinline__ bool tri_solve(const double A[6], const double b[3], double x[3])
{
	const double A00 = A[0], A01 = A[1], A02 = A[2], A11 = A[3], A12 = A[4], A22 = A[5];
	const double det = A00 * A11 * A22 + A01 * A12 * A02 + A02 * A01 * A12 - A00 * A12 * A12 - A02 * A11 * A02 - A01 * A01 * A22;
	const double id = 1 / det;
	double B[6];
	B[0] = id * (A11 * A22 - A12 * A12);
	B[1] = id * (A02 * A12 - A01 * A22);
	B[2] = id * (A01 * A12 - A02 * A11);
	B[3] = id * (A00 * A22 - A02 * A02);
	B[4] = id * (A02 * A01 - A00 * A12);
	B[5] = id * (A00 * A11 - A01 * A01);
	x[0] = B[0] * b[0] + B[1] * b[1] + B[2] * b[2];
	x[1] = B[1] * b[0] + B[3] * b[1] + B[4] * b[2];
	x[2] = B[2] * b[0] + B[4] * b[1] + B[5] * b[2];
	return det > 0 && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// the head's three decisions.  Each returns the landmark's status so far (TRI_OK: still in the running)
__device__ __forceinline__ int tri_start_solve(const double s[TRI_START], const TriangulateArgs& a, double X[3])
{
	const double n = s[12];
	const bool depth = s[13] > 0;
	if (n < 2 && !depth) return TRI_FEW_OBSERVATIONS;
	if (!depth && a.parallax_on)
	{
		const double c = sqrt(s[9] * s[9] + s[10] * s[10] + s[11] * s[11]) / n;
		if (c > a.cos_half_parallax) return TRI_LOW_PARALLAX;
	}
	return tri_solve(s, s + 6, X) ? TRI_OK : TRI_SINGULAR;
}

__device__ __forceinline__ int tri_gn_solve(const double s[TRI_GN], double X[3])
{
	double d[3];
	const bool ok = tri_solve(s, s + 6, d);
	X[0] += d[0]; X[1] += d[1]; X[2] += d[2];
	return ok && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) ? TRI_OK : TRI_SINGULAR;
}

__device__ __forceinline__ int tri_accept(const double s[TRI_FLAGS]) { return s[0] > 0 ? TRI_BEHIND_CAMERA : s[1] > 0 ? TRI_CHI2 : TRI_OK; }

// the landmark's result: its status, and the position of an OK landmark as the state holds it
__device__ __forceinline__ void tri_store(const TriangulateArgs& a, int il, int status, const double X[3])
{
	a.status[il] = status;
	if (status != TRI_OK) return;
#pragma unroll
	for (int k = 0; k < 3; k++)
	{
		const Scalar x = (Scalar)X[k];
		a.xnew[3 * (size_t)il + k] = (double)x;
		if (!a.dry_run) a.g.Xw[3 * (size_t)il + k] = x;
	}
}

template <int N>
__device__ __forceinline__ void tri_lanes_to_lds(double* lds, int lane, const double v[N])
{
#pragma unroll
	for (int k = 0; k < N; k++) lds[lane * N + k] = v[k];
	wave_lds_sync();
}

template <int N>
__device__ __forceinline__ void tri_segment_sum(const double* lds, int seg0, int seg1, double s[N])
{
#pragma unroll
	for (int k = 0; k < N; k++) s[k] = 0;
	for (int j = seg0; j < seg1; j++)
#pragma unroll
		for (int k = 0; k < N; k++) s[k] += lds[j * N + k];
}

// Lane l of the caller's numbering: what is decided without looking at an edge.  TRI_PENDING marks the landmarks the edge kernels take
// up; one that no edge kernel reaches -- a landmark without an edge in the wave list -- leaves the collect kernel as FEW_OBSERVATIONS.
__global__ __launch_bounds__(TRI_T) void triangulate_init_kernel(const uint8_t* __restrict__ select, const int* __restrict__ newOfOld, int Lt, int Lf, int* __restrict__ status)
{
	const int l = blockIdx.x * TRI_T + threadIdx.x;
	if (l >= Lt) return;
	const int m = newOfOld ? newOfOld[l] : l;
	status[m] = select && !select[l] ? TRI_NOT_SELECTED : m >= Lf ? TRI_FIXED : TRI_PENDING;
}

// wave = one entry of wave_lm, lane = sorted edge
__global__ __launch_bounds__(TRI_T) void triangulate_wave_kernel(TriangulateArgs a)
{
	__shared__ double sums_all[TRI_T / WAVE][WAVE * TRI_START];
	__shared__ double pub_all[TRI_T / WAVE][WAVE * TRI_PUB];
	const DeviceGraph& g = a.g;
	const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
	const int wave = blockIdx.x * (TRI_T / WAVE) + wv;
	if (wave >= a.nWaves) return;
	double* sums = sums_all[wv];
	double* pub = pub_all[wv];
	const int lm0 = a.wave_lm[2 * wave], lm1 = a.wave_lm[2 * wave + 1];
	const int e0 = g.lm_ptr[lm0], e1 = g.lm_ptr[lm1];
	const int e = e0 + lane;
	TriEdge ed;
	ed.on = false;
	int il = lm0, seg0 = lane, seg1 = lane;
	bool work = false;
	if (e < e1)
	{
		il = g.e_lm[e];
		work = a.status[il] == TRI_PENDING;     // (selected and free; its head stores the status behind the last step)
		if (work)
		{
			tri_load(g, e, ed);
			seg0 = g.lm_ptr[il] - e0;
			seg1 = g.lm_ptr[il + 1] - e0;
		}
	}
	const bool head = work && lane == seg0;
	int status = TRI_OK;
	double X[3] = { 0, 0, 0 };
	// linear start
	{
		double v[TRI_START];
		tri_start_terms(ed, v);
		tri_lanes_to_lds<TRI_START>(sums, lane, v);
		if (head)
		{
			double s[TRI_START];
			tri_segment_sum<TRI_START>(sums, seg0, seg1, s);
			status = tri_start_solve(s, a, X);
			pub[seg0 * TRI_PUB] = X[0]; pub[seg0 * TRI_PUB + 1] = X[1]; pub[seg0 * TRI_PUB + 2] = X[2];
			pub[seg0 * TRI_PUB + 3] = status == TRI_OK ? 1.0 : 0.0;
		}
		wave_lds_sync();
	}
	// Gauss-Newton steps: every lane of a segment reads the head's position
	for (int it = 0; it < a.iterations; it++)
	{
		const bool alive = work && pub[seg0 * TRI_PUB + 3] != 0;
		double v[TRI_GN] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
		if (alive)
		{
			const double Xl[3] = { pub[seg0 * TRI_PUB], pub[seg0 * TRI_PUB + 1], pub[seg0 * TRI_PUB + 2] };
			tri_gn_terms(ed, Xl, g.rk, v);
		}
		tri_lanes_to_lds<TRI_GN>(sums, lane, v);
		if (head && status == TRI_OK)
		{
			double s[TRI_GN];
			tri_segment_sum<TRI_GN>(sums, seg0, seg1, s);
			status = tri_gn_solve(s, X);
			pub[seg0 * TRI_PUB] = X[0]; pub[seg0 * TRI_PUB + 1] = X[1]; pub[seg0 * TRI_PUB + 2] = X[2];
			pub[seg0 * TRI_PUB + 3] = status == TRI_OK ? 1.0 : 0.0;
		}
		wave_lds_sync();
	}
	// acceptance at the final position
	{
		const bool alive = work && pub[seg0 * TRI_PUB + 3] != 0;
		double v[TRI_FLAGS] = { 0, 0 };
		if (alive)
		{
			const double Xl[3] = { pub[seg0 * TRI_PUB], pub[seg0 * TRI_PUB + 1], pub[seg0 * TRI_PUB + 2] };
			tri_accept_terms(ed, Xl, a, v);
		}
		tri_lanes_to_lds<TRI_FLAGS>(sums, lane, v);
		if (head)
		{
			if (status == TRI_OK)
			{
				double s[TRI_FLAGS];
				tri_segment_sum<TRI_FLAGS>(sums, seg0, seg1, s);
				status = tri_accept(s);
			}
			tri_store(a, il, status, X);
		}
	}
}

// every wave's sum of v[0..N) (a butterfly: the order is fixed) into red[wave], a barrier
template <int N>
__device__ __forceinline__ void tri_four_waves_to_lds(double (&red)[TRI_T / WAVE][TRI_START], double (&v)[N])
{
#pragma unroll
	for (int k = 0; k < N; k++)
	{
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
	}
	if ((threadIdx.x & (WAVE - 1)) == 0)
#pragma unroll
		for (int k = 0; k < N; k++) red[threadIdx.x / WAVE][k] = v[k];
	__syncthreads();
}

template <int N>
__device__ __forceinline__ void tri_four_wave_sum(const double (&red)[TRI_T / WAVE][TRI_START], double s[N])
{
#pragma unroll
	for (int k = 0; k < N; k++) s[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
}

// workgroup = one landmark of the big_lm class: the edges are loaded again in every step (a thread has several)
__global__ __launch_bounds__(TRI_T) void triangulate_big_kernel(TriangulateArgs a)
{
	__shared__ double red[TRI_T / WAVE][TRI_START];
	__shared__ double pub[TRI_PUB];
	const DeviceGraph& g = a.g;
	const int il = a.big_lm[blockIdx.x];
	if (a.status[il] != TRI_PENDING) return;     // (the whole workgroup: thread 0 stores the status behind the last barrier)
	const int e0 = g.lm_ptr[il], e1 = g.lm_ptr[il + 1];
	int status = TRI_OK;
	double X[3] = { 0, 0, 0 };
	{
		double acc[TRI_START] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
		for (int e = e0 + (int)threadIdx.x; e < e1; e += TRI_T)
		{
			TriEdge ed;
			double v[TRI_START];
			tri_load(g, e, ed);
			tri_start_terms(ed, v);
#pragma unroll
			for (int k = 0; k < TRI_START; k++) acc[k] += v[k];
		}
		tri_four_waves_to_lds<TRI_START>(red, acc);
		if (threadIdx.x == 0)
		{
			double s[TRI_START];
			tri_four_wave_sum<TRI_START>(red, s);
			status = tri_start_solve(s, a, X);
			pub[0] = X[0]; pub[1] = X[1]; pub[2] = X[2]; pub[3] = status == TRI_OK ? 1.0 : 0.0;
		}
		__syncthreads();
	}
	for (int it = 0; it < a.iterations; it++)
	{
		if (pub[3] == 0) break;                            // (the same number in every thread)
		const double Xl[3] = { pub[0], pub[1], pub[2] };
		double acc[TRI_GN] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
		for (int e = e0 + (int)threadIdx.x; e < e1; e += TRI_T)
		{
			TriEdge ed;
			double v[TRI_GN];
			tri_load(g, e, ed);
			tri_gn_terms(ed, Xl, g.rk, v);
#pragma unroll
			for (int k = 0; k < TRI_GN; k++) acc[k] += v[k];
		}
		tri_four_waves_to_lds<TRI_GN>(red, acc);           // (behind this barrier nobody reads the old pub any more)
		if (threadIdx.x == 0)
		{
			double s[TRI_GN];
			tri_four_wave_sum<TRI_GN>(red, s);
			status = tri_gn_solve(s, X);
			pub[0] = X[0]; pub[1] = X[1]; pub[2] = X[2]; pub[3] = status == TRI_OK ? 1.0 : 0.0;
		}
		__syncthreads();
	}
	if (pub[3] != 0)
	{
		const double Xl[3] = { pub[0], pub[1], pub[2] };
		double acc[TRI_FLAGS] = { 0, 0 };
		for (int e = e0 + (int)threadIdx.x; e < e1; e += TRI_T)
		{
			TriEdge ed;
			double v[TRI_FLAGS];
			tri_load(g, e, ed);
			tri_accept_terms(ed, Xl, a, v);
			acc[0] += v[0]; acc[1] += v[1];
		}
		tri_four_waves_to_lds<TRI_FLAGS>(red, acc);
		if (threadIdx.x == 0)
		{
			double s[TRI_FLAGS];
			tri_four_wave_sum<TRI_FLAGS>(red, s);
			status = tri_accept(s);
		}
	}
	if (threadIdx.x == 0) tri_store(a, il, status, X);
}

// Lane l of the caller's numbering: status and position out of the internal order, the statuses counted per workgroup.
__global__ __launch_bounds__(TRI_T) void triangulate_collect_kernel(TriangulateArgs a, const int* __restrict__ newOfOld, int* __restrict__ statusOut,
	double* __restrict__ xyzOut, long long* __restrict__ parts)
{
	__shared__ int red[TRI_T / WAVE][TRI_STATUSES];
	const int Lt = a.g.Lt;
	int cnt[TRI_STATUSES] = { 0, 0, 0, 0, 0, 0, 0, 0 };     // wave-uniform
	// (whole waves walk the loop together: the ballots need every lane of the wave)
	for (int base = blockIdx.x * TRI_T; base < Lt; base += gridDim.x * TRI_T)
	{
		const int l = base + threadIdx.x;
		int s = -1;
		if (l < Lt)
		{
			const size_t m = (size_t)(newOfOld ? newOfOld[l] : l);
			s = a.status[m];
			if (s == TRI_PENDING) s = TRI_FEW_OBSERVATIONS;      // (no edge kernel reached it: it has no edge)
			statusOut[l] = s;
#pragma unroll
			for (int k = 0; k < 3; k++) xyzOut[3 * (size_t)l + k] = s == TRI_OK ? a.xnew[3 * m + k] : (double)a.g.Xw[3 * m + k];
		}
#pragma unroll
		for (int k = 0; k < TRI_STATUSES; k++) cnt[k] += __popcll(__ballot(s == k));
	}
	if ((threadIdx.x & (WAVE - 1)) == 0)
#pragma unroll
		for (int k = 0; k < TRI_STATUSES; k++) red[threadIdx.x / WAVE][k] = cnt[k];
	__syncthreads();
	if (threadIdx.x < TRI_STATUSES)
	{
		long long s = 0;
#pragma unroll
		for (int w = 0; w < TRI_T / WAVE; w++) s += red[w][threadIdx.x];
		parts[(size_t)TRI_STATUSES * blockIdx.x + threadIdx.x] = s;
	}
}

// second stage: one wave adds the n workgroups' partials, lane-strided, then across the lanes
__global__ __launch_bounds__(WAVE) void triangulate_counts_kernel(const long long* __restrict__ parts, int n, long long* __restrict__ out)
{
	long long s[TRI_STATUSES] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (int i = threadIdx.x; i < n; i += WAVE)
#pragma unroll
		for (int k = 0; k < TRI_STATUSES; k++) s[k] += parts[(size_t)TRI_STATUSES * i + k];
#pragma unroll
	for (int k = 0; k < TRI_STATUSES; k++)
	{
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
		if (threadIdx.x == 0) out[k] = s[k];
	}
}
}  // namespace

int triangulate_collect_grid(int Lt) { return Lt > 0 ? min((Lt + TRI_T - 1) / TRI_T, 1024) : 0; }

void launch_triangulate(const TriangulateArgs& a, const uint8_t* select, const int* newOfOld, hipStream_t s)
{
	const int Lt = a.g.Lt;
	if (Lt <= 0) return;
	hipLaunchKernelGGL(triangulate_init_kernel, dim3((Lt + TRI_T - 1) / TRI_T), dim3(TRI_T), 0, s, select, newOfOld, Lt, a.g.Lf, a.status);
	if (a.nWaves > 0) hipLaunchKernelGGL(triangulate_wave_kernel, dim3((a.nWaves + TRI_T / WAVE - 1) / (TRI_T / WAVE)), dim3(TRI_T), 0, s, a);
	if (a.nBig > 0) hipLaunchKernelGGL(triangulate_big_kernel, dim3(a.nBig), dim3(TRI_T), 0, s, a);
}

void launch_triangulate_collect(const TriangulateArgs& a, const int* newOfOld, int* statusOut, double* xyzOut, long long* parts, long long* counts, hipStream_t s)
{
	const int grid = triangulate_collect_grid(a.g.Lt);
	if (grid > 0) hipLaunchKernelGGL(triangulate_collect_kernel, dim3(grid), dim3(TRI_T), 0, s, a, newOfOld, statusOut, xyzOut, parts);
	hipLaunchKernelGGL(triangulate_counts_kernel, dim3(1), dim3(WAVE), 0, s, parts, grid, counts);
}

}  // namespace cubahip

// ---------------------------------------------------------------------------------------------------------------------------------------
// The handle's side.  Nothing is kept between calls but the buffers: every call decides every landmark afresh.
// ---------------------------------------------------------------------------------------------------------------------------------------
void cuba_hip_solver::triangulateLandmarks(const uint8_t* select, int refineIterations, double minParallaxDeg, const double chi2Max[2], bool dryRun,
	int32_t* status, int64_t* counts, double* xyz)
{
	if (refineIterations < 0 || refineIterations > TRI_MAX_ITERATIONS) throw ArgError{ "refine_iterations must lie in 0 ... 16" };
	if (std::isnan(minParallaxDeg)) throw ArgError{ "min_parallax_deg is NaN (<= 0: no parallax test)" };
	if (!chi2Max || std::isnan(chi2Max[0]) || std::isnan(chi2Max[1])) throw ArgError{ "chi2_max must be two numbers (+inf: no chi2 test)" };
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (partHi >= 0) throw StateError{ "landmark triangulation is not available on a landmark-partitioned handle" };
	need();
	TriangulateArgs a;
	a.g = g;
	a.wave_lm = st.wave_lm; a.nWaves = st.nWaves; a.big_lm = st.big_lm; a.nBig = st.nBig;
	a.iterations = refineIterations;
	a.parallax_on = minParallaxDeg > 0 ? 1 : 0;
	a.cos_half_parallax = std::cos(0.5 * minParallaxDeg * (3.14159265358979323846 / 180.0));
	a.chi2_mono = chi2Max[0]; a.chi2_stereo = chi2Max[1];
	a.dry_run = dryRun ? 1 : 0;
	const int grid = triangulate_collect_grid(Lt);
	d_triStatus.resize((size_t)2 * Lt); d_triX.resize((size_t)6 * Lt);
	d_triCounts.resize((size_t)TRI_STATUSES * (1 + grid));
	a.status = d_triStatus.data(); a.xnew = d_triX.data();
	if (select && Lt) d_triSelect.uploadRaw(select, (size_t)Lt, stream);
	const int* newOfOld = lmOrderActive ? d_lmMap.data() : nullptr;
	launch_triangulate(a, select && Lt ? d_triSelect.data() : nullptr, newOfOld, stream);
	launch_triangulate_collect(a, newOfOld, d_triStatus.data() + Lt, d_triX.data() + 3 * (size_t)Lt, d_triCounts.data() + TRI_STATUSES, d_triCounts.data(), stream);
	long long h[TRI_STATUSES];
	HIP_TRY(hipMemcpyAsync(h, d_triCounts.data(), sizeof h, hipMemcpyDeviceToHost, stream));
	if (status && Lt) HIP_TRY(hipMemcpyAsync(status, d_triStatus.data() + Lt, sizeof(int32_t) * (size_t)Lt, hipMemcpyDeviceToHost, stream));
	if (xyz && Lt) HIP_TRY(hipMemcpyAsync(xyz, d_triX.data() + 3 * (size_t)Lt, sizeof(double) * 3 * (size_t)Lt, hipMemcpyDeviceToHost, stream));
	sync();
	if (!dryRun && h[TRI_OK] > 0) covBlocksValid = false;
	if (counts) for (int k = 0; k < TRI_STATUSES; k++) counts[k] = h[k];
}
