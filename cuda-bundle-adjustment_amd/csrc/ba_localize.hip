// ba_localize.hip -- pose localisation from scratch on the device: an absolute pose per selected free pose from its active reprojection
// edges and the current landmarks only, by a deterministic RANSAC over a minimal three-point solver (the first half of ORB-SLAM's
// Tracking::Relocalization; ba_pose_refine.hip is the second half).  The counterpart of the triangulation's linear start: THE POSE'S CURRENT
// VALUE IS NEVER READ.  The definition in full: include/cuba_hip.h (cuba_hip_localize_poses) and tests/pose_localization_reference.py.
//
// ALL ARITHMETIC IS DOUBLE in both libraries; the state is read as Scalar and the winner written as Scalar once.  The file carries its own
// double residual and quaternion helpers (the formulas of ba_math.hpp): nothing of ba_math.hpp or ba_device.hpp is routed through here, so
// no existing kernel's instructions move.
//
// Mapping: workgroup = one free pose, THREAD = HYPOTHESIS (batches of 256 in a loop): the hypotheses are independent and the edges shared,
// so one relocalised keyframe still fills four waves and the P3P is solved once per hypothesis.  Every thread walks the pose's entries of
// pe_edge itself -- the loop bounds and the addresses are the same in every lane --: once to find its three smallest keys, once per
// surviving root to score it (roots one at a time: a single candidate [R | t] is live beside the thread's best).  One block arg-min on
// (C, 4 h + root) in a fixed order through LDS, then the whole workgroup walks the edges once more, thread-strided, to write the
// classification at the winner.  No atomics; a workgroup writes only its own pose and its own edges' scratch bytes.  Below the kernels:
// the handle's side.

#include "ba_solver.hpp"
#include "ba_device.hpp"

#include <climits>
#include <cmath>

// No contraction of a * b + c into a fused multiply-add in this file: the P3P's conditioning multiplies every rounding difference, and
// the device is held to the reference (tests/pose_localization_reference.py, separate multiplications and additions) pose by pose.
#pragma clang fp contract(off)

namespace cubahip
{

namespace
{
constexpr int PL_T = 256;
constexpr int PL_WAVES = PL_T / WAVE;
constexpr int PL_PENDING = POSELOC_STATUSES;      // internal to a call, never reported: selected and free, for the workgroup to decide
using u64 = unsigned long long;

// the finaliser of splitmix64
__host__ __device__ __forceinline__ u64 pl_mix(u64 x)
{
	x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
	x ^= x >> 27; x *= 0x94d049bb133111ebULL;
	x ^= x >> 31;
	return x;
}

__device__ __forceinline__ bool pl_before(u64 ka, unsigned ea, u64 kb, unsigned eb) { return ka < kb || (ka == kb && ea < eb); }

// omega |r|^2 of an edge at [R | t] (edge_residual of ba_math.hpp) and its point's depth
__device__ __forceinline__ double pl_chi(const double (&R)[3][3], const double (&t)[3], const double (&cam)[5], const double (&X)[3], const double (&m)[3],
	bool stereo, double w, double& depth)
{
	double Xc[3];
#pragma unroll
	for (int i = 0; i < 3; i++) Xc[i] = R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i];
	const double invZ = 1 / Xc[2];
	const double u = cam[0] * invZ * Xc[0] + cam[2];
	const double v = cam[1] * invZ * Xc[1] + cam[3];
	const double r0 = u - m[0], r1 = v - m[1];
	const double r2 = stereo ? (u - cam[4] * invZ) - m[2] : 0.0;
	depth = Xc[2];
	return w * (r0 * r0 + r1 * r1 + r2 * r2);
}

// sorted edge e: landmark, measurement, information, kind
__device__ __forceinline__ void pl_load(const DeviceGraph& g, int e, double (&X)[3], double (&m)[3], double& w, bool& stereo)
{
	stereo = (g.e_pose[e] & STEREO_BIT) != 0;
	const size_t il = (size_t)g.e_lm[e];
	X[0] = (double)g.Xw[3 * il]; X[1] = (double)g.Xw[3 * il + 1]; X[2] = (double)g.Xw[3 * il + 2];
	m[0] = (double)g.e_mu[e]; m[1] = (double)g.e_mv[e]; m[2] = stereo ? (double)g.e_mr[e] : 0.0;
	w = (double)g.e_w[e];
}

__device__ __forceinline__ void pl_unit(const double (&v)[3], double (&o)[3])
{
	const double inv = 1 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	o[0] = inv * v[0]; o[1] = inv * v[1]; o[2] = inv * v[2];
}

__device__ __forceinline__ void pl_cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
	o[0] = a[1] * b[2] - a[2] * b[1];
	o[1] = a[2] * b[0] - a[0] * b[2];
	o[2] = a[0] * b[1] - a[1] * b[0];
}

// the orthonormal triad of three points: e1 = unit(B - A), e3 = unit(e1 x (C - A)), e2 = e3 x e1; false: the points are collinear (or
// coincide) to rounding, |e1 x (C - A)|^2 <= 1e-24 |C - A|^2 -- the normal would be rounding noise
__device__ __forceinline__ bool pl_triad(const double (&A)[3], const double (&B)[3], const double (&C)[3], double (&e)[3][3])
{
	const double d1[3] = { B[0] - A[0], B[1] - A[1], B[2] - A[2] }, d2[3] = { C[0] - A[0], C[1] - A[1], C[2] - A[2] };
	double n[3];
	pl_unit(d1, e[0]);
	pl_cross(e[0], d2, n);
	pl_unit(n, e[2]);
	pl_cross(e[2], e[0], e[1]);
	return n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 1e-24 * (d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]);
}

template <int I, int J, int K>
__device__ __forceinline__ void pl_shepperd_branch(const double (&R)[3][3], double (&qe)[4])
{
	double tr = sqrt(R[I][I] - R[J][J] - R[K][K] + 1);
	qe[I] = 0.5 * tr;
	tr = 0.5 / tr;
	qe[3] = (R[K][J] - R[J][K]) * tr;
	qe[J] = (R[J][I] + R[I][J]) * tr;
	qe[K] = (R[K][I] + R[I][K]) * tr;
}

// the unit quaternion (x, y, z, w), w >= 0, of a rotation matrix (Shepperd, the branches of pose_exp_update in ba_math.hpp)
__device__ __forceinline__ void pl_quaternion(const double (&R)[3][3], double (&q)[4])
{
	double c[4];
	double tr = R[0][0] + R[1][1] + R[2][2];
	if (tr > 0)
	{
		tr = sqrt(tr + 1);
		c[3] = 0.5 * tr;
		tr = 0.5 / tr;
		c[0] = (R[2][1] - R[1][2]) * tr;
		c[1] = (R[0][2] - R[2][0]) * tr;
		c[2] = (R[1][0] - R[0][1]) * tr;
	}
	else
	{
		const bool c1 = R[1][1] > R[0][0];
		const bool c2 = R[2][2] > (c1 ? R[1][1] : R[0][0]);
		if (c2) pl_shepperd_branch<2, 0, 1>(R, c);
		else if (c1) pl_shepperd_branch<1, 2, 0>(R, c);
		else pl_shepperd_branch<0, 1, 2>(R, c);
	}
	double invn = 1 / sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
	if (c[3] < 0) invn = -invn;
	q[0] = invn * c[0]; q[1] = invn * c[1]; q[2] = invn * c[2]; q[3] = invn * c[3];
}

// Grunert's system for the sample (bearings f, landmarks X, in key order) reduced to the normalised quartic v^4 + B v^3 + C v^2 + D v + E in
// v = s_3 / s_1 and split by Ferrari into two quadratics: the roots are (sh +- sqrt(disc)) / 2 - B / 4, (sh, disc) = (s, disc[0]) for the root
// indices 0, 1 and (-s, disc[1]) for 2, 3.  Kept for the roots' second halves: the coefficients of N, the cosines, the squared sides.
struct PlQuartic
{
	double B, C, D, E;       // normalised quartic
	double s, disc[2];
	double n2, n1, n0;       // N(v)
	double ca, cb, cg, a2, b2, c2;
};

__device__ __forceinline__ void pl_quartic(const double (&f)[3][3], const double (&X)[3][3], PlQuartic& k)
{
	double a2 = 0, b2 = 0, c2 = 0, ca = 0, cb = 0, cg = 0;
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
		const double d23 = X[1][i] - X[2][i], d13 = X[0][i] - X[2][i], d12 = X[0][i] - X[1][i];
		a2 += d23 * d23; b2 += d13 * d13; c2 += d12 * d12;
		ca += f[1][i] * f[2][i]; cb += f[0][i] * f[2][i]; cg += f[0][i] * f[1][i];
	}
	const double K = (a2 - c2) / b2, Cc = c2 / b2;
	const double n2 = K - 1, n1 = -2 * K * cb, n0 = 1 + K;
	const double d1 = -2 * ca, d0 = 2 * cg;
	const double w2 = -Cc, w1 = 2 * Cc * cb, w0 = 1 - Cc;
	const double g2 = 2 * cg;
	const double A4 = n2 * n2 + d1 * d1 * w2;
	const double A3 = 2 * n2 * n1 - g2 * (n2 * d1) + d1 * d1 * w1 + 2 * d1 * d0 * w2;
	const double A2 = n1 * n1 + 2 * n2 * n0 - g2 * (n2 * d0 + n1 * d1) + d1 * d1 * w0 + 2 * d1 * d0 * w1 + d0 * d0 * w2;
	const double A1 = 2 * n1 * n0 - g2 * (n1 * d0 + n0 * d1) + 2 * d1 * d0 * w0 + d0 * d0 * w1;
	const double A0 = n0 * n0 - g2 * (n0 * d0) + d0 * d0 * w0;
	const double B = A3 / A4, C = A2 / A4, D = A1 / A4, E = A0 / A4;
	// depressed quartic y^4 + p y^2 + q y + r, v = y - B / 4
	const double BB = B * B;
	const double p = C - 3 * BB / 8;
	const double q = D - B * C / 2 + BB * B / 8;
	const double r = E - B * D / 4 + BB * C / 16 - 3 * BB * BB / 256;
	// the largest real root m of the resolvent m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8, m = z - p / 3, z^3 + P z + Q = 0
	const double c1 = p * p / 4 - r, c0 = -q * q / 8;
	const double P = -p * p / 12 - r;
	const double Q = -p * p * p / 108 + p * r / 3 - q * q / 8;
	const double disc = Q * Q / 4 + P * P * P / 27;
	double z = 0;
	if (disc > 0)
	{
		double A = cbrt(fabs(Q) / 2 + sqrt(disc));
		if (Q > 0) A = -A;
		z = A - P / (3 * A);
	}
	else if (P < 0)
	{
		const double sp = sqrt(-P / 3);
		double arg = (3 * Q / (2 * P)) / sp;
		arg = arg > 1 ? 1 : arg < -1 ? -1 : arg;
		z = 2 * sp * cos(acos(arg) / 3);
	}
	double m = z - p / 3;
#pragma unroll
	for (int it = 0; it < 2; it++)
	{
		const double gm = ((m + p) * m + c1) * m + c0;
		const double gp = (3 * m + 2 * p) * m + c1;
		if (gp != 0) m -= gm / gp;
	}
	const double s = sqrt(2 * m);
	const double hq = q / (2 * s);
	k.B = B; k.C = C; k.D = D; k.E = E;
	k.s = s;
	k.disc[0] = s * s - 4 * (p / 2 + m + hq);
	k.disc[1] = s * s - 4 * (p / 2 + m - hq);
	k.n2 = n2; k.n1 = n1; k.n0 = n0;
	k.ca = ca; k.cb = cb; k.cg = cg; k.a2 = a2; k.b2 = b2; k.c2 = c2;
}

// root `slot` of the quartic -> the candidate [R | t]; false: no such root, or a discarded candidate (a distance <= 0, a number that is
// not finite, collinear points).  The test on the sample's own three edges is the caller's.
__device__ __forceinline__ bool pl_candidate(const PlQuartic& k, int slot, const double (&f)[3][3], const double (&X)[3][3], double (&R)[3][3], double (&t)[3])
{
	const double disc = slot < 2 ? k.disc[0] : k.disc[1];
	if (!(disc >= 0)) return false;
	const double sq = sqrt(disc);
	double v = ((slot < 2 ? k.s : -k.s) + ((slot & 1) ? -sq : sq)) / 2 - k.B / 4;
#pragma unroll
	for (int it = 0; it < 2; it++)
	{
		const double fv = (((v + k.B) * v + k.C) * v + k.D) * v + k.E;
		const double fp = ((4 * v + 3 * k.B) * v + 2 * k.C) * v + k.D;
		if (fp != 0) v -= fv / fp;
	}
	const double u = ((k.n2 * v + k.n1) * v + k.n0) / (2 * (k.cg - k.ca * v));
	double s1 = sqrt(k.b2 / (1 + v * v - 2 * v * k.cb));
	double s2 = u * s1, s3 = v * s1;
	// two Newton steps on the law-of-cosines system itself, in the three distances (Cramer's rule): near a double root of the quartic the
	// ratio N / D and the quartic's own polish lose digits that the system still holds
#pragma unroll
	for (int it = 0; it < 2; it++)
	{
		const double F1 = s2 * s2 + s3 * s3 - 2 * s2 * s3 * k.ca - k.a2;
		const double F2 = s1 * s1 + s3 * s3 - 2 * s1 * s3 * k.cb - k.b2;
		const double F3 = s1 * s1 + s2 * s2 - 2 * s1 * s2 * k.cg - k.c2;
		const double ja = 2 * (s2 - s3 * k.ca), jb = 2 * (s3 - s2 * k.ca);
		const double jc = 2 * (s1 - s3 * k.cb), jd = 2 * (s3 - s1 * k.cb);
		const double je = 2 * (s1 - s2 * k.cg), jg = 2 * (s2 - s1 * k.cg);
		const double det = ja * jd * je + jb * jc * jg;
		if (det != 0)
		{
			s1 -= (-F1 * jd * jg + ja * jd * F3 + jb * jg * F2) / det;
			s2 -= (F1 * jd * je + jb * jc * F3 - jb * je * F2) / det;
			s3 -= (-ja * jc * F3 + ja * je * F2 + F1 * jc * jg) / det;
		}
	}
	if (!(s1 > 0 && s2 > 0 && s3 > 0)) return false;
	double Y[3][3];
#pragma unroll
	for (int i = 0; i < 3; i++) { Y[0][i] = s1 * f[0][i]; Y[1][i] = s2 * f[1][i]; Y[2][i] = s3 * f[2][i]; }
	double ec[3][3], ew[3][3];
	bool ok = pl_triad(Y[0], Y[1], Y[2], ec);
	ok = pl_triad(X[0], X[1], X[2], ew) && ok;
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
#pragma unroll
		for (int j = 0; j < 3; j++)
		{
			R[i][j] = ec[0][i] * ew[0][j] + ec[1][i] * ew[1][j] + ec[2][i] * ew[2][j];
			ok = ok && isfinite(R[i][j]);
		}
	}
#pragma unroll
	for (int i = 0; i < 3; i++)
	{
		t[i] = Y[0][i] - (R[i][0] * X[0][0] + R[i][1] * X[0][1] + R[i][2] * X[0][2]);
		ok = ok && isfinite(t[i]);
	}
	return ok;
}

// Entry i of max(Pt, E): what is decided without looking at an edge.  Pose i of the caller's numbering: NOT_SELECTED / FIXED / the
// internal "pending" mark, its seed word mix(mix(seed + golden) + i), no inliers, no winner, cost 0.  Sorted edge i: its scratch byte =
// its live information is positive (what edge_inlier reports for an edge of a pose without a winner).
__global__ __launch_bounds__(PL_T) void pose_localize_init_kernel(PoseLocalizeArgs a, const uint8_t* __restrict__ select, const int* __restrict__ newOfOld)
{
	const int i = blockIdx.x * PL_T + threadIdx.x;
	if (i < a.g.Pt)
	{
		const int m = newOfOld && i < a.g.Pf ? newOfOld[i] : i;
		a.status[m] = select && !select[i] ? POSELOC_NOT_SELECTED : i >= a.g.Pf ? POSELOC_FIXED : PL_PENDING;
		a.inliers[m] = 0;
		a.winner[m] = -1;
		a.cost[m] = 0;
		a.key[m] = pl_mix(pl_mix(a.seed + 0x9e3779b97f4a7c15ULL) + (u64)i);
	}
	if (i < a.g.E) a.cls[i] = (double)a.g.e_w[i] > 0 ? 1 : 0;
}

// workgroup = one free pose (internal order), thread = hypothesis
__global__ __launch_bounds__(PL_T) void pose_localize_kernel(PoseLocalizeArgs a)
{
	__shared__ double redC[PL_WAVES];
	__shared__ int redI[PL_WAVES];
	__shared__ int redN[PL_WAVES];
	__shared__ double win[13];       // the winner's R | t | C
	__shared__ int winI;
	const DeviceGraph& g = a.g;
	const int ip = blockIdx.x;
	const int tid = threadIdx.x;
	if (a.status[ip] != PL_PENDING) return;       // (the same in every thread of the workgroup)
	const int p0 = a.pe_beg[ip], p1 = a.pe_end[ip];
	const u64 poseKey = a.key[ip];
	double cam[5];
#pragma unroll
	for (int k = 0; k < 5; k++) cam[k] = (double)g.cam[5 * (size_t)ip + k];
	const double thr[2] = { a.chi2_mono, a.chi2_stereo };

	double bestC = INFINITY, bestR[3][3], bestT[3];
	int bestI = INT_MAX, usable = 0;
#pragma unroll
	for (int i = 0; i < 3; i++) { bestT[i] = 0; bestR[i][0] = bestR[i][1] = bestR[i][2] = 0; }

	for (int h0 = 0; h0 < a.hypotheses; h0 += PL_T)
	{
		const int h = h0 + tid;
		const bool live = h < a.hypotheses;
		const u64 kh = pl_mix(poseKey + (u64)h);
		// the three usable edges of smallest key, ordered by key
		u64 sk[3] = { 0, 0, 0 };
		unsigned sc[3] = { 0, 0, 0 };
		int se[3] = { -1, -1, -1 };
		usable = 0;
		for (int p = p0; p < p1; p++)
		{
			const int e = a.pe_edge[p];
			if (!((double)g.e_w[e] > 0)) continue;
			usable++;
			const unsigned ce = a.perm[e];
			const u64 key = pl_mix(kh + (u64)ce);
			if (se[2] < 0 || pl_before(key, ce, sk[2], sc[2]))
			{
				sk[2] = key; sc[2] = ce; se[2] = e;
#pragma unroll
				for (int j = 2; j > 0; j--)
				{
					if (se[j - 1] < 0 || pl_before(sk[j], sc[j], sk[j - 1], sc[j - 1]))
					{
						const u64 tk = sk[j]; sk[j] = sk[j - 1]; sk[j - 1] = tk;
						const unsigned tc = sc[j]; sc[j] = sc[j - 1]; sc[j - 1] = tc;
						const int te = se[j]; se[j] = se[j - 1]; se[j - 1] = te;
					}
				}
			}
		}
		if (usable < 4) break;       // (the same in every thread)

		double X[3][3], f[3][3], ms[3][3], ws[3];
		bool st[3];
#pragma unroll
		for (int i = 0; i < 3; i++)
		{
			pl_load(g, se[i], X[i], ms[i], ws[i], st[i]);
			const double b[3] = { (ms[i][0] - cam[2]) / cam[0], (ms[i][1] - cam[3]) / cam[1], 1.0 };
			pl_unit(b, f[i]);
		}
		PlQuartic k;
		pl_quartic(f, X, k);
		for (int slot = 0; slot < 4; slot++)
		{
			double R[3][3], t[3];
			bool valid = live && pl_candidate(k, slot, f, X, R, t);
			if (valid)
			{
#pragma unroll
				for (int i = 0; i < 3; i++)
				{
					double depth;
					const double chi = pl_chi(R, t, cam, X[i], ms[i], st[i], ws[i], depth);
					valid = valid && depth > 0 && chi <= thr[st[i] ? 1 : 0];
				}
			}
			if (__ballot(valid) == 0) continue;       // (per wave: no candidate of this root index to score)
			if (!valid)
			{
#pragma unroll
				for (int i = 0; i < 3; i++) { t[i] = 0; R[i][0] = R[i][1] = R[i][2] = 0; }
			}
			// the MSAC score: every lane of the wave walks the same entries
			double C = 0;
			for (int p = p0; p < p1; p++)
			{
				const int e = a.pe_edge[p];
				double Xe[3], me[3], we;
				bool ste;
				pl_load(g, e, Xe, me, we, ste);
				if (!(we > 0)) continue;
				double depth;
				const double chi = pl_chi(R, t, cam, Xe, me, ste, we, depth);
				const double cap = thr[ste ? 1 : 0];
				C += (depth > 0 && chi <= cap) ? chi : cap;
			}
			const int idx = 4 * h + slot;
			if (valid && (C < bestC || (C == bestC && idx < bestI)))
			{
				bestC = C; bestI = idx;
#pragma unroll
				for (int i = 0; i < 3; i++) { bestT[i] = t[i]; bestR[i][0] = R[i][0]; bestR[i][1] = R[i][1]; bestR[i][2] = R[i][2]; }
			}
		}
	}
	if (usable < 4)
	{
		if (tid == 0) { a.status[ip] = POSELOC_FEW_OBSERVATIONS; a.inliers[ip] = usable; }
		return;
	}

	// block arg-min on (C, 4 h + root): a butterfly per wave, then the waves' results in turn
	double rc = bestC;
	int ri = bestI;
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1)
	{
		const double oc = __shfl_xor(rc, o);
		const int oi = __shfl_xor(ri, o);
		if (oc < rc || (oc == rc && oi < ri)) { rc = oc; ri = oi; }
	}
	if ((tid & (WAVE - 1)) == 0) { redC[tid / WAVE] = rc; redI[tid / WAVE] = ri; }
	__syncthreads();
	if (tid == 0)
	{
#pragma unroll
		for (int w = 1; w < PL_WAVES; w++)
			if (redC[w] < rc || (redC[w] == rc && redI[w] < ri)) { rc = redC[w]; ri = redI[w]; }
		winI = ri;
	}
	__syncthreads();
	const int wi = winI;
	if (wi == INT_MAX)
	{
		if (tid == 0) { a.status[ip] = POSELOC_NO_SOLUTION; a.inliers[ip] = usable; }
		return;
	}
	if (bestI == wi)
	{
#pragma unroll
		for (int i = 0; i < 3; i++) { win[3 * i] = bestR[i][0]; win[3 * i + 1] = bestR[i][1]; win[3 * i + 2] = bestR[i][2]; win[9 + i] = bestT[i]; }
		win[12] = bestC;
	}
	__syncthreads();
	double R[3][3], t[3];
#pragma unroll
	for (int i = 0; i < 3; i++) { R[i][0] = win[3 * i]; R[i][1] = win[3 * i + 1]; R[i][2] = win[3 * i + 2]; t[i] = win[9 + i]; }

	// the classification at the winner, thread-strided
	int n = 0;
	for (int p = p0 + tid; p < p1; p += PL_T)
	{
		const int e = a.pe_edge[p];
		double Xe[3], me[3], we, depth;
		bool ste;
		pl_load(g, e, Xe, me, we, ste);
		const double chi = pl_chi(R, t, cam, Xe, me, ste, we, depth);
		const bool in = we > 0 && depth > 0 && chi <= thr[ste ? 1 : 0];
		a.cls[e] = in ? 1 : 0;
		n += in ? 1 : 0;
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) n += __shfl_xor(n, o);
	if ((tid & (WAVE - 1)) == 0) redN[tid / WAVE] = n;
	__syncthreads();
	if (tid == 0)
	{
		n = 0;
#pragma unroll
		for (int w = 0; w < PL_WAVES; w++) n += redN[w];
		const int status = n < max(4, a.min_inliers) ? POSELOC_FEW_INLIERS : POSELOC_OK;
		a.status[ip] = status;
		a.inliers[ip] = n;
		a.cost[ip] = win[12];
		if (status == POSELOC_OK)
		{
			a.winner[ip] = wi;
			double q[4];
			pl_quaternion(R, q);
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

// Pose p of the caller's numbering: status, inliers, winner, cost and pose out of the internal order, the statuses counted per workgroup.
__global__ __launch_bounds__(PL_T) void pose_localize_collect_kernel(PoseLocalizeArgs a, const int* __restrict__ newOfOld, int* __restrict__ statusOut,
	int* __restrict__ inliersOut, int* __restrict__ winnerOut, double* __restrict__ costOut, double* __restrict__ qOut, double* __restrict__ tOut,
	long long* __restrict__ parts)
{
	__shared__ int red[PL_WAVES][POSELOC_STATUSES];
	const int Pt = a.g.Pt;
	int cnt[POSELOC_STATUSES] = { 0, 0, 0, 0, 0, 0 };     // wave-uniform
	// (whole waves walk the loop together: the ballots need every lane of the wave)
	for (int base = blockIdx.x * PL_T; base < Pt; base += gridDim.x * PL_T)
	{
		const int p = base + threadIdx.x;
		int s = -1;
		if (p < Pt)
		{
			const size_t m = (size_t)(newOfOld && p < a.g.Pf ? newOfOld[p] : p);
			s = a.status[m];
			statusOut[p] = s;
			inliersOut[p] = a.inliers[m];
			winnerOut[p] = a.winner[m];
			costOut[p] = a.cost[m];
#pragma unroll
			for (int k = 0; k < 4; k++) qOut[4 * (size_t)p + k] = s == POSELOC_OK ? a.qt[7 * m + k] : (double)a.g.q[4 * m + k];
#pragma unroll
			for (int k = 0; k < 3; k++) tOut[3 * (size_t)p + k] = s == POSELOC_OK ? a.qt[7 * m + 4 + k] : (double)a.g.t[3 * m + k];
		}
#pragma unroll
		for (int k = 0; k < POSELOC_STATUSES; k++) cnt[k] += __popcll(__ballot(s == k));
	}
	if ((threadIdx.x & (WAVE - 1)) == 0)
#pragma unroll
		for (int k = 0; k < POSELOC_STATUSES; k++) red[threadIdx.x / WAVE][k] = cnt[k];
	__syncthreads();
	if (threadIdx.x < POSELOC_STATUSES)
	{
		long long s = 0;
#pragma unroll
		for (int w = 0; w < PL_WAVES; w++) s += red[w][threadIdx.x];
		parts[(size_t)POSELOC_STATUSES * blockIdx.x + threadIdx.x] = s;
	}
}

// second stage: one wave adds the n workgroups' partials, lane-strided, then across the lanes
__global__ __launch_bounds__(WAVE) void pose_localize_counts_kernel(const long long* __restrict__ parts, int n, long long* __restrict__ out)
{
	long long s[POSELOC_STATUSES] = { 0, 0, 0, 0, 0, 0 };
	for (int i = threadIdx.x; i < n; i += WAVE)
#pragma unroll
		for (int k = 0; k < POSELOC_STATUSES; k++) s[k] += parts[(size_t)POSELOC_STATUSES * i + k];
#pragma unroll
	for (int k = 0; k < POSELOC_STATUSES; k++)
	{
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
		if (threadIdx.x == 0) out[k] = s[k];
	}
}
}  // namespace

int pose_localize_collect_grid(int Pt) { return Pt > 0 ? min((Pt + PL_T - 1) / PL_T, 1024) : 0; }

void launch_pose_localize(const PoseLocalizeArgs& a, const uint8_t* select, const int* newOfOld, hipStream_t s)
{
	const int n = max(a.g.Pt, a.g.E);
	if (n > 0) hipLaunchKernelGGL(pose_localize_init_kernel, dim3((n + PL_T - 1) / PL_T), dim3(PL_T), 0, s, a, select, newOfOld);
	if (a.g.Pf > 0) hipLaunchKernelGGL(pose_localize_kernel, dim3(a.g.Pf), dim3(PL_T), 0, s, a);
}

void launch_pose_localize_collect(const PoseLocalizeArgs& a, const int* newOfOld, int* statusOut, int* inliersOut, int* winnerOut, double* costOut,
	double* qOut, double* tOut, long long* parts, long long* counts, hipStream_t s)
{
	const int grid = pose_localize_collect_grid(a.g.Pt);
	if (grid > 0)
		hipLaunchKernelGGL(pose_localize_collect_kernel, dim3(grid), dim3(PL_T), 0, s, a, newOfOld, statusOut, inliersOut, winnerOut, costOut, qOut, tOut, parts);
	hipLaunchKernelGGL(pose_localize_counts_kernel, dim3(1), dim3(WAVE), 0, s, parts, grid, counts);
}

}  // namespace cubahip

// ---------------------------------------------------------------------------------------------------------------------------------------
// The handle's side.  Nothing is kept between calls but the buffers: every call decides every pose afresh.  The handle's gate is read
// only through the live information and never written; the classification of a call lives in d_plCls.
// ---------------------------------------------------------------------------------------------------------------------------------------
void cuba_hip_solver::localizePoses(const uint8_t* select, int hypotheses, uint64_t seed, const double chi2Max[2], int minInliers, bool dryRun,
	int32_t* status, int64_t* counts, int32_t* inliers, double* cost, int32_t* winner, double* q, double* t, uint8_t* edgeInlier)
{
	if (hypotheses < 1 || hypotheses > POSELOC_MAX_HYPOTHESES) throw ArgError{ "hypotheses must lie in 1 ... 4096" };
	if (minInliers < 0) throw ArgError{ "min_inliers must not be negative" };
	if (!chi2Max || !std::isfinite(chi2Max[0]) || !std::isfinite(chi2Max[1]) || !(chi2Max[0] > 0) || !(chi2Max[1] > 0))
		throw ArgError{ "chi2_max must be two finite positive numbers" };
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (partHi >= 0) throw StateError{ "pose localisation is not available on a landmark-partitioned handle" };
	need();
	PoseLocalizeArgs a;
	a.g = g;
	a.pe_beg = st.pe_beg; a.pe_end = st.pe_end; a.pe_edge = st.pe_edge;
	a.hypotheses = hypotheses; a.seed = (unsigned long long)seed; a.min_inliers = minInliers;
	a.chi2_mono = chi2Max[0]; a.chi2_stereo = chi2Max[1];
	a.dry_run = dryRun ? 1 : 0;
	const int grid = pose_localize_collect_grid(Pt);
	// [status | inliers | winner] in the internal order, then in the caller's; [cost | q t] in the internal order, then [cost | q | t] in the caller's
	d_plInt.resize((size_t)6 * Pt); d_plReal.resize((size_t)16 * Pt); d_plKey.resize((size_t)Pt);
	d_plCls.resize((size_t)2 * E);
	d_plCounts.resize((size_t)POSELOC_STATUSES * (1 + grid));
	a.status = d_plInt.data(); a.inliers = d_plInt.data() + Pt; a.winner = d_plInt.data() + 2 * (size_t)Pt;
	a.cost = d_plReal.data(); a.qt = d_plReal.data() + Pt;
	a.key = d_plKey.data();
	a.cls = d_plCls.data();
	a.perm = permDevice();
	if (select && Pt) d_plSelect.uploadRaw(select, (size_t)Pt, stream);
	const int* newOfOld = reorderActive ? d_poseMap.data() : nullptr;
	int* statusOut = d_plInt.data() + 3 * (size_t)Pt;
	int* inliersOut = statusOut + Pt;
	int* winnerOut = inliersOut + Pt;
	double* costOut = d_plReal.data() + 8 * (size_t)Pt;
	double* qOut = costOut + Pt;
	double* tOut = qOut + 4 * (size_t)Pt;
	launch_pose_localize(a, select && Pt ? d_plSelect.data() : nullptr, newOfOld, stream);
	launch_pose_localize_collect(a, newOfOld, statusOut, inliersOut, winnerOut, costOut, qOut, tOut, d_plCounts.data() + POSELOC_STATUSES, d_plCounts.data(), stream);
	long long h[POSELOC_STATUSES];
	HIP_TRY(hipMemcpyAsync(h, d_plCounts.data(), sizeof h, hipMemcpyDeviceToHost, stream));
	if (status && Pt) HIP_TRY(hipMemcpyAsync(status, statusOut, sizeof(int32_t) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (inliers && Pt) HIP_TRY(hipMemcpyAsync(inliers, inliersOut, sizeof(int32_t) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (winner && Pt) HIP_TRY(hipMemcpyAsync(winner, winnerOut, sizeof(int32_t) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (cost && Pt) HIP_TRY(hipMemcpyAsync(cost, costOut, sizeof(double) * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (q && Pt) HIP_TRY(hipMemcpyAsync(q, qOut, sizeof(double) * 4 * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (t && Pt) HIP_TRY(hipMemcpyAsync(t, tOut, sizeof(double) * 3 * (size_t)Pt, hipMemcpyDeviceToHost, stream));
	if (edgeInlier && E)
	{
		launch_gate_unsort(a.perm, d_plCls.data(), E, d_plCls.data() + E, stream);
		HIP_TRY(hipMemcpyAsync(edgeInlier, d_plCls.data() + E, (size_t)E, hipMemcpyDeviceToHost, stream));
	}
	sync();
	if (!dryRun && h[POSELOC_OK] > 0) covBlocksValid = false;
	if (counts) for (int k = 0; k < POSELOC_STATUSES; k++) counts[k] = h[k];
}
