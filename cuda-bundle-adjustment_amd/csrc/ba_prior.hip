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
#include "ba_se3.hpp"

namespace cubahip
{

constexpr int PRIOR_LIN_BLOCK = 64;
constexpr int PRIOR_CHI_BLOCK = 256;
constexpr int PRIOR_CHI_MAX_GROUPS = 64;     // the chi2 launch's partials (a grid-stride loop beyond): they join the edges' partials

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
