// ba_prior.hip -- SE(3) pose priors (cuba_hip_set_pose_priors): unary factors r^T Omega r on single poses, r = log(T Tbar^-1) in the
// [omega, upsilon] tangent of the solver's left-multiplicative update T <- exp(d) T (pose_exp_update), linearised with the exact
// derivative dr/dd = J_l(r)^-1.  A prior touches the diagonal 6 x 6 block of its pose in the reduced matrix and the
// pose's entries of bp / bsc only: the block pattern, the product lists and every other part of the launch sequence stay as they are.
//
//   prior_linearize_kernel   lane = free pose with priors: its priors in the caller's order, J^T Omega J / J^T Omega r summed in
//                            registers, then added to the pose's diagonal block (upper triangle), bp and (mode 1) bsc -- one writer per
//                            block, a launch of its own behind the Schur pass (which may still update a diagonal block the pose pass stored)
//   prior_chi2_kernel        lane = prior: r^T Omega r at the current estimate into the per-prior output and into per-workgroup partials
//                            that the caller sums together with the edges' partials (fixed order, no atomics)
//
// Host side: the caller's prior set (validated, kept in the caller's numbering) and its upload in the internal pose order.
#include "ba_solver.hpp"
#include "ba_device.hpp"

namespace cubahip
{

constexpr int PRIOR_LIN_BLOCK = 64;
constexpr int PRIOR_CHI_BLOCK = 256;
constexpr int PRIOR_CHI_MAX_GROUPS = 64;     // the chi2 launch's partials (a grid-stride loop beyond): they join the edges' partials

__device__ __forceinline__ void hat3(const Scalar v[3], Scalar M[3][3])
{
	M[0][0] = 0;     M[0][1] = -v[2]; M[0][2] = v[1];
	M[1][0] = v[2];  M[1][1] = 0;     M[1][2] = -v[0];
	M[2][0] = -v[1]; M[2][1] = v[0];  M[2][2] = 0;
}

__device__ __forceinline__ void mul3(const Scalar A[3][3], const Scalar B[3][3], Scalar C[3][3])
{
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) C[i][j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j];
}

// Residual r = [w ; V(w)^-1 (t - R Rbar^T tbar)], w = log(R Rbar^T), of pose (q, t) against (qb, tb) (both unit quaternions), and A = J_w^-1
// = I - W / 2 + d W^2.  The rotation part comes from the relative quaternion (atan2: well defined up to theta = pi).
__device__ __forceinline__ void prior_residual(const Scalar q[4], const Scalar t[3], const Scalar qb[4], const Scalar tb[3], Scalar r[6], Scalar A[3][3])
{
	// qr = q (x) conj(qb)
	Scalar qr[4];
	qr[3] = q[3] * qb[3] + q[0] * qb[0] + q[1] * qb[1] + q[2] * qb[2];
	qr[0] = qb[3] * q[0] - q[3] * qb[0] - (q[1] * qb[2] - q[2] * qb[1]);
	qr[1] = qb[3] * q[1] - q[3] * qb[1] - (q[2] * qb[0] - q[0] * qb[2]);
	qr[2] = qb[3] * q[2] - q[3] * qb[2] - (q[0] * qb[1] - q[1] * qb[0]);
	Scalar inv = 1 / sqrt(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2] + qr[3] * qr[3]);
	if (qr[3] < 0) inv = -inv;
#pragma unroll
	for (int k = 0; k < 4; k++) qr[k] *= inv;
	const Scalar n = sqrt(qr[0] * qr[0] + qr[1] * qr[1] + qr[2] * qr[2]);
	const Scalar s = n < Scalar(1e-4) ? 2 / qr[3] * (1 - (n / qr[3]) * (n / qr[3]) / 3) : 2 * atan2(n, qr[3]) / n;
	const Scalar w[3] = { s * qr[0], s * qr[1], s * qr[2] };
	Scalar u[3];
	quat_rotate(qr, tb, u);
	u[0] = t[0] - u[0]; u[1] = t[1] - u[1]; u[2] = t[2] - u[2];
	const Scalar th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
	Scalar d;
	if (th < Scalar(0.25)) d = Scalar(1) / 12 + th2 * (Scalar(1) / 720 + th2 * (Scalar(1) / 30240 + th2 * (Scalar(1) / 1209600)));
	else d = (1 - Scalar(0.5) * th * cos(Scalar(0.5) * th) / sin(Scalar(0.5) * th)) / th2;
	Scalar W[3][3], W2[3][3];
	hat3(w, W);
	mul3(W, W, W2);
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) A[i][j] = (i == j ? Scalar(1) : Scalar(0)) - Scalar(0.5) * W[i][j] + d * W2[i][j];
#pragma unroll
	for (int i = 0; i < 3; i++) { r[i] = w[i]; r[3 + i] = A[i][0] * u[0] + A[i][1] * u[1] + A[i][2] * u[2]; }
}

// B = -A Q A, Q = Q(w, v) the lower-left block of the SE(3) left Jacobian in [omega, upsilon] order:
//   Q = P/2 + c1 (WP + PW + WPW) + c2 (WWP + PWW - 3 WPW) + c3 (WPWW + WWPW),  P = [v]x,
//   c1 = (th - sin th) / th^3, c2 = (th^2/2 + cos th - 1) / th^4, c3 = (c2 + 3 (th - sin th - th^3/6) / th^5) / 2 (series below th = 0.25)
__device__ __forceinline__ void prior_jacobian_b(const Scalar r[6], const Scalar A[3][3], Scalar B[3][3])
{
	const Scalar th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = sqrt(th2);
	Scalar c1, c2, c3;
	if (th < Scalar(0.25))
	{
		c1 = Scalar(1) / 6 - th2 * (Scalar(1) / 120 - th2 * (Scalar(1) / 5040 - th2 * (Scalar(1) / 362880)));
		c2 = Scalar(1) / 24 - th2 * (Scalar(1) / 720 - th2 * (Scalar(1) / 40320 - th2 * (Scalar(1) / 3628800)));
		c3 = Scalar(1) / 120 - th2 * (Scalar(1) / 2520 - th2 * (Scalar(1) / 120960 - th2 * (Scalar(1) / 9979200)));
	}
	else
	{
		const Scalar sn = sin(th), cs = cos(th), th3 = th2 * th;
		c1 = (th - sn) / th3;
		c2 = (th2 / 2 + cs - 1) / (th2 * th2);
		c3 = Scalar(0.5) * (c2 + 3 * (th - sn - th3 / 6) / (th3 * th2));
	}
	Scalar W[3][3], P[3][3], WP[3][3], PW[3][3], WPW[3][3], Q[3][3];
	hat3(r, W);
	hat3(r + 3, P);
	mul3(W, P, WP);
	mul3(P, W, PW);
	mul3(WP, W, WPW);
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++)
		{
			const Scalar wwp = W[i][0] * WP[0][j] + W[i][1] * WP[1][j] + W[i][2] * WP[2][j];
			const Scalar pww = PW[i][0] * W[0][j] + PW[i][1] * W[1][j] + PW[i][2] * W[2][j];
			const Scalar wpww = WPW[i][0] * W[0][j] + WPW[i][1] * W[1][j] + WPW[i][2] * W[2][j];
			const Scalar wwpw = W[i][0] * WPW[0][j] + W[i][1] * WPW[1][j] + W[i][2] * WPW[2][j];
			Q[i][j] = Scalar(0.5) * P[i][j] + c1 * (WP[i][j] + PW[i][j] + WPW[i][j]) + c2 * (wwp + pww - 3 * WPW[i][j]) + c3 * (wpww + wwpw);
		}
	Scalar QA[3][3];
	mul3(Q, A, QA);
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int j = 0; j < 3; j++) B[i][j] = -(A[i][0] * QA[0][j] + A[i][1] * QA[1][j] + A[i][2] * QA[2][j]);
}

__device__ __forceinline__ void load_prior(const DevicePriors& pr, int k, Scalar qb[4], Scalar tb[3])
{
#pragma unroll
	for (int i = 0; i < 4; i++) qb[i] = pr.qbar[4 * (size_t)k + i];
#pragma unroll
	for (int i = 0; i < 3; i++) tb[i] = pr.tbar[3 * (size_t)k + i];
}

// Omega r (Omega column-major) and r^T Omega r
__device__ __forceinline__ Scalar prior_info_times(const DevicePriors& pr, int k, const Scalar r[6], Scalar Or[6])
{
	const Scalar* O = pr.info + 36 * (size_t)k;
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

__global__ __launch_bounds__(PRIOR_LIN_BLOCK) void prior_linearize_kernel(DeviceGraph g, DeviceStructure st, DeviceSystem sys, DevicePriors pr, int mode)
{
	const int i = blockIdx.x * PRIOR_LIN_BLOCK + threadIdx.x;
	if (i >= pr.nPoses) return;
	const int ip = pr.pose_id[i];
	Scalar q[4], t[3];
#pragma unroll
	for (int k = 0; k < 4; k++) q[k] = g.q[4 * (size_t)ip + k];
#pragma unroll
	for (int k = 0; k < 3; k++) t[k] = g.t[3 * (size_t)ip + k];
	Scalar H[21], gv[6];
#pragma unroll
	for (int k = 0; k < 21; k++) H[k] = 0;
#pragma unroll
	for (int k = 0; k < 6; k++) gv[k] = 0;
	const int k1 = pr.pose_ptr[i + 1];
	for (int k = pr.pose_ptr[i]; k < k1; k++)
	{
		Scalar qb[4], tb[3], r[6], A[3][3], B[3][3];
		load_prior(pr, k, qb, tb);
		prior_residual(q, t, qb, tb, r, A);
		prior_jacobian_b(r, A, B);
		// J = [[A, 0], [B, A]]
		Scalar J[6][6];
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int b = 0; b < 3; b++) { J[a][b] = A[a][b]; J[a][3 + b] = 0; J[3 + a][b] = B[a][b]; J[3 + a][3 + b] = A[a][b]; }
		const Scalar* O = pr.info + 36 * (size_t)k;
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
				H[c * (c + 1) / 2 + rr] += s;
			}
		}
		Scalar Or[6];
		(void)prior_info_times(pr, k, r, Or);
#pragma unroll
		for (int c = 0; c < 6; c++)
		{
			Scalar s = 0;
#pragma unroll
			for (int a = 0; a < 6; a++) s += J[a][c] * Or[a];
			gv[c] += s;
		}
	}
	Scalar* blk = sys.hsc + 36 * (size_t)st.hsc_rowptr[ip];
#pragma unroll
	for (int c = 0; c < 6; c++)
	{
#pragma unroll
		for (int rr = 0; rr <= c; rr++) blk[c * 6 + rr] += H[c * (c + 1) / 2 + rr];
		sys.bp[6 * (size_t)ip + c] -= gv[c];
		if (mode == 1) sys.bsc[6 * (size_t)ip + c] -= gv[c];
	}
}

__global__ __launch_bounds__(PRIOR_CHI_BLOCK) void prior_chi2_kernel(DeviceGraph g, DevicePriors pr, Scalar* __restrict__ parts)
{
	Scalar acc = 0;
	for (int k = blockIdx.x * PRIOR_CHI_BLOCK + threadIdx.x; k < pr.n; k += gridDim.x * PRIOR_CHI_BLOCK)
	{
		const int ip = pr.pose[k];
		Scalar chi = 0;
		if (ip < g.Pf)
		{
			Scalar q[4], t[3], qb[4], tb[3], r[6], A[3][3], Or[6];
#pragma unroll
			for (int i = 0; i < 4; i++) q[i] = g.q[4 * (size_t)ip + i];
#pragma unroll
			for (int i = 0; i < 3; i++) t[i] = g.t[3 * (size_t)ip + i];
			load_prior(pr, k, qb, tb);
			prior_residual(q, t, qb, tb, r, A);
			chi = prior_info_times(pr, k, r, Or);
		}
		pr.chi[k] = chi;
		acc += chi;
	}
	acc = wave_sum(acc);
	__shared__ Scalar part[PRIOR_CHI_BLOCK / WAVE];
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) parts[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

int prior_chi2_parts(const DevicePriors* pr)
{
	return pr && pr->n > 0 ? std::min((pr->n + PRIOR_CHI_BLOCK - 1) / PRIOR_CHI_BLOCK, PRIOR_CHI_MAX_GROUPS) : 0;
}

void launch_prior_linearize(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const DevicePriors& pr, int mode, hipStream_t s)
{
	if (pr.nPoses <= 0) return;
	hipLaunchKernelGGL(prior_linearize_kernel, dim3((pr.nPoses + PRIOR_LIN_BLOCK - 1) / PRIOR_LIN_BLOCK), dim3(PRIOR_LIN_BLOCK), 0, s, g, st, sys, pr, mode);
}

void launch_prior_chi2(const DeviceGraph& g, const DevicePriors& pr, Scalar* parts, hipStream_t s)
{
	const int grid = prior_chi2_parts(&pr);
	if (grid > 0) hipLaunchKernelGGL(prior_chi2_kernel, dim3(grid), dim3(PRIOR_CHI_BLOCK), 0, s, g, pr, parts);
}

}  // namespace cubahip

// ---- host side --------------------------------------------------------------------------------------------------------------------

void cuba_hip_solver::setPosePriors(int n, const int32_t* pose, const double* q, const double* t, const double* info)
{
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (n < 0) throw ArgError{ "negative prior count" };
	if (n > 0 && (partHi >= 0 || valuesPartial)) throw StateError{ "pose priors are not available on a landmark-partitioned handle" };
	if (n > 0 && E == 0) throw StateError{ "pose priors need a graph with edges" };
	if (n > 0 && (!pose || !q || !t || !info)) throw ArgError{ "null prior array" };
	std::vector<int> hp((size_t)n);
	std::vector<double> hq((size_t)4 * n), ht((size_t)3 * n), hi((size_t)36 * n);
	for (int k = 0; k < n; k++)
	{
		if (pose[k] < 0 || pose[k] >= Pt) throw ArgError{ "prior pose index out of range" };
		hp[k] = pose[k];
		double nq = 0;
		for (int i = 0; i < 4; i++) { if (!std::isfinite(q[4 * (size_t)k + i])) throw ArgError{ "non-finite prior rotation" }; nq += q[4 * (size_t)k + i] * q[4 * (size_t)k + i]; }
		nq = std::sqrt(nq);
		if (!(nq > 0) || !std::isfinite(nq)) throw ArgError{ "prior quaternion of zero norm" };
		for (int i = 0; i < 4; i++) hq[4 * (size_t)k + i] = q[4 * (size_t)k + i] / nq;
		for (int i = 0; i < 3; i++) { if (!std::isfinite(t[3 * (size_t)k + i])) throw ArgError{ "non-finite prior translation" }; ht[3 * (size_t)k + i] = t[3 * (size_t)k + i]; }
		const double* O = info + 36 * (size_t)k;
		double m = 0;
		for (int i = 0; i < 36; i++) { if (!std::isfinite(O[i])) throw ArgError{ "non-finite prior information" }; m = std::max(m, std::fabs(O[i])); }
		for (int c = 0; c < 6; c++)
			for (int r = 0; r < c; r++)
				if (std::fabs(O[6 * c + r] - O[6 * r + c]) > 1e-9 * m) throw ArgError{ "prior information is not symmetric" };
		// (symmetrised: within the tolerance above the two triangles may differ by rounding; the kernels read both)
		for (int c = 0; c < 6; c++)
			for (int r = 0; r < 6; r++) hi[36 * (size_t)k + 6 * c + r] = r == c ? O[6 * c + r] : 0.5 * (O[6 * c + r] + O[6 * r + c]);
	}
	h_priorPose.swap(hp); h_priorQ.swap(hq); h_priorT.swap(ht); h_priorInfo.swap(hi);
	priorsUploaded = false;
	pri = DevicePriors();
	// (the run-to-run memories the values of the system feed, as a new graph drops them: a run after a prior change depends on the state
	// and the priors only)
	firstInvValid = false; firstInvPending = false; prevRunIters.clear(); runIters.clear(); firstSolveIters = 0;
}

// the caller's set -> device, in the internal pose order (stable by internal pose: every pose's priors contiguous, in the caller's order)
void cuba_hip_solver::uploadPriors()
{
	const int n = (int)h_priorPose.size();
	std::vector<int> internal((size_t)n);
	for (int k = 0; k < n; k++) internal[k] = h_priorPose[k] < Pf && reorderActive ? poseNewOfOld[h_priorPose[k]] : h_priorPose[k];
	h_priorOrder.resize((size_t)n);
	std::iota(h_priorOrder.begin(), h_priorOrder.end(), 0);
	std::stable_sort(h_priorOrder.begin(), h_priorOrder.end(), [&](int a, int b) { return internal[a] < internal[b]; });
	std::vector<int> ptr, ids, poses((size_t)n);
	std::vector<Scalar> vals((size_t)43 * n);
	Scalar* vq = vals.data(); Scalar* vt = vq + (size_t)4 * n; Scalar* vi = vt + (size_t)3 * n;
	for (int s = 0; s < n; s++)
	{
		const int k = h_priorOrder[s], p = internal[k];
		poses[s] = p;
		if (p < Pf && (ids.empty() || ids.back() != p)) { ids.push_back(p); ptr.push_back(s); }
		for (int i = 0; i < 4; i++) vq[4 * (size_t)s + i] = (Scalar)h_priorQ[4 * (size_t)k + i];
		for (int i = 0; i < 3; i++) vt[3 * (size_t)s + i] = (Scalar)h_priorT[3 * (size_t)k + i];
		for (int i = 0; i < 36; i++) vi[36 * (size_t)s + i] = (Scalar)h_priorInfo[36 * (size_t)k + i];
	}
	int nFree = 0;
	while (nFree < n && poses[nFree] < Pf) nFree++;
	ptr.push_back(nFree);
	const int np = (int)ids.size();
	std::vector<int> ints;
	ints.reserve(ptr.size() + ids.size() + poses.size());
	ints.insert(ints.end(), ptr.begin(), ptr.end());
	ints.insert(ints.end(), ids.begin(), ids.end());
	ints.insert(ints.end(), poses.begin(), poses.end());
	d_priorInts.upload(ints, stream);
	d_priorVals.upload(vals, stream);
	d_priorChi.resize((size_t)std::max(n, 1));
	pri = DevicePriors();
	pri.n = n; pri.nPoses = np;
	pri.pose_ptr = d_priorInts.data(); pri.pose_id = pri.pose_ptr + (np + 1); pri.pose = pri.pose_id + np;
	pri.qbar = d_priorVals.data(); pri.tbar = pri.qbar + (size_t)4 * n; pri.info = pri.tbar + (size_t)3 * n;
	pri.chi = d_priorChi.data();
	sync();          // (the staging vectors go out of scope)
	priorsUploaded = true;
}

void cuba_hip_solver::priorChiSquares(double* out)
{
	need();
	const int n = (int)h_priorPose.size();
	if (n == 0) return;
	launch_prior_chi2(g, pri, d_parts.data(), stream);
	std::vector<double> sorted((size_t)n);
	downloadAsDouble(pri.chi, sorted.data(), (size_t)n);
	for (int s = 0; s < n; s++) out[h_priorOrder[s]] = sorted[s];
}
