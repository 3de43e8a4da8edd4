// ba_lmfactor.hip -- landmark position priors (cuba_hip_set_landmark_priors): unary terms rho(r^T Omega r) of the
// objective on the free landmarks, r = X - Xbar, Omega a symmetric 3 x 3 information, rho one of the pose factors' kernels (none, Huber,
// Tukey, Cauchy).  g2o's unary XYZ prior edge; the reference has no counterpart.
//
// The Jacobian of r is the identity, so a prior's whole linearisation is Hll += w Omega, bl -= w Omega r with w = rho'(r^T Omega r) (bl:
// the right-hand side of the landmark's rows, minus half the gradient; no second-order term, as every other kernel of the library).  Hll and bl of a landmark have one writer, the head lane of the landmark pass
// (ba_linearize.hip), and everything downstream -- the 3 x 3 inverse, the pose and block passes, back-substitution, the gain ratio's
// scale, the covariances -- reads them from sys.lm_sys.  So the priors are linearised INSIDE that pass (ba_device.hpp:
// add_landmark_priors, in kernel instantiations that only a handle with priors launches) and this file holds the rest:
//
//   landmark_prior_chi2_kernel   lane = prior: r^T Omega r at the current estimate into the per-prior output and rho of it into
//                                per-workgroup partials that join the pose factors' behind the reprojection edges' (fixed order, no atomics)
//
// and the host side: the caller's set (validated, kept in the caller's numbering) and its upload in the internal landmark order.
#include "ba_solver.hpp"
#include "ba_device.hpp"

namespace cubahip
{

constexpr int LMP_CHI_BLOCK = 256;
constexpr int LMP_CHI_MAX_GROUPS = 64;     // a chi2 launch's partials (a grid-stride loop beyond)

__global__ __launch_bounds__(LMP_CHI_BLOCK) void landmark_prior_chi2_kernel(DeviceGraph g, DeviceLandmarkPriors lp, Scalar* __restrict__ parts)
{
	Scalar acc = 0;
	for (int k = blockIdx.x * LMP_CHI_BLOCK + threadIdx.x; k < lp.n; k += gridDim.x * LMP_CHI_BLOCK)
	{
		const int il = lp.lm[k];
		Scalar chi = 0;
		if (il < g.Lf)
		{
			const Scalar X[3] = { g.Xw[3 * (size_t)il], g.Xw[3 * (size_t)il + 1], g.Xw[3 * (size_t)il + 2] };
			Scalar Or[3];
			chi = landmark_prior_residual(lp, k, X, Or);
		}
		lp.chi[k] = chi;
		acc += factor_rho(lp.rk_kind[k], lp.rk_delta[k], chi);
	}
	acc = wave_sum(acc);
	__shared__ Scalar part[LMP_CHI_BLOCK / WAVE];
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) parts[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

int landmark_prior_chi2_parts(const DeviceLandmarkPriors& lp) { return lp.n > 0 ? std::min((lp.n + LMP_CHI_BLOCK - 1) / LMP_CHI_BLOCK, LMP_CHI_MAX_GROUPS) : 0; }

void launch_landmark_prior_chi2(const DeviceGraph& g, const DeviceLandmarkPriors& lp, Scalar* parts, hipStream_t s)
{
	const int grid = landmark_prior_chi2_parts(lp);
	if (grid <= 0) return;
	hipLaunchKernelGGL(landmark_prior_chi2_kernel, dim3(grid), dim3(LMP_CHI_BLOCK), 0, s, g, lp, parts);
}

}  // namespace cubahip

// ---- host side --------------------------------------------------------------------------------------------------------------------

void cuba_hip_solver::setLandmarkPriors(int n, const int32_t* landmark, const double* xyz, const double* info, const int32_t* kind, const double* delta)
{
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (n < 0) throw ArgError{ "negative landmark prior count" };
	if (n > 0 && (partHi >= 0 || valuesPartial)) throw StateError{ "landmark priors are not available on a landmark-partitioned handle" };
	if (n > 0 && E == 0) throw StateError{ "landmark priors need a graph with edges" };
	if (n > 0 && (!landmark || !xyz || !info)) throw ArgError{ "null landmark prior array" };
	if (n > 0 && (kind == nullptr) != (delta == nullptr)) throw ArgError{ "landmark prior kernels: kind and delta come together" };
	LandmarkPriorSet v;
	v.lm.resize((size_t)n); v.xyz.resize((size_t)3 * n); v.info.resize((size_t)6 * n); v.kind.assign((size_t)n, cubahip::POSE_FACTOR_KERNEL_NONE); v.delta.assign((size_t)n, 1.0);
	for (int k = 0; k < n; k++)
	{
		if (landmark[k] < 0 || landmark[k] >= Lt) throw ArgError{ "landmark prior: landmark index out of range" };
		v.lm[k] = landmark[k];
		for (int i = 0; i < 3; i++)
		{
			if (!std::isfinite(xyz[3 * (size_t)k + i])) throw ArgError{ "non-finite landmark prior position" };
			v.xyz[3 * (size_t)k + i] = xyz[3 * (size_t)k + i];
		}
		const double* O = info + 9 * (size_t)k;
		double m = 0;
		for (int i = 0; i < 9; i++) { if (!std::isfinite(O[i])) throw ArgError{ "non-finite landmark prior information" }; m = std::max(m, std::fabs(O[i])); }
		for (int c = 0; c < 3; c++)
			for (int r = 0; r < c; r++)
				if (std::fabs(O[3 * c + r] - O[3 * r + c]) > 1e-9 * m) throw ArgError{ "landmark prior information is not symmetric" };
		// (symmetrised: within the tolerance above the two triangles may differ by rounding) -> upper triangle, the packing of sym3_idx
		double* U = v.info.data() + 6 * (size_t)k;
		U[0] = O[0]; U[1] = 0.5 * (O[3] + O[1]); U[2] = 0.5 * (O[6] + O[2]); U[3] = O[4]; U[4] = 0.5 * (O[7] + O[5]); U[5] = O[8];
		if (kind)
		{
			if (kind[k] < cubahip::POSE_FACTOR_KERNEL_NONE || kind[k] > cubahip::POSE_FACTOR_KERNEL_CAUCHY) throw ArgError{ "bad landmark prior robust kernel" };
			if (!std::isfinite(delta[k])) throw ArgError{ "non-finite robust-kernel delta" };
			if (kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE && !(delta[k] > 0)) throw ArgError{ "robust-kernel delta must be positive" };
			if (kind[k] != cubahip::POSE_FACTOR_KERNEL_NONE) { v.kind[k] = kind[k]; v.delta[k] = delta[k]; }
		}
	}
	// a validated set replaces the handle's: its device copy is due, and the memories that the values of the system feed go
	lmPriorSet.lm.swap(v.lm); lmPriorSet.xyz.swap(v.xyz); lmPriorSet.info.swap(v.info); lmPriorSet.kind.swap(v.kind); lmPriorSet.delta.swap(v.delta);
	lmPriorSet.order.clear(); lmPriorSet.uploaded = false;
	pf.lmp = DeviceLandmarkPriors();
	forgetRunMemories();
	covBlocksValid = false;
}

// the caller's priors -> device, in the internal landmark order (stable by internal landmark: every landmark's priors contiguous, in the
// caller's order; the priors on fixed landmarks last).  A prior on a free landmark without an edge cannot be honoured -- the landmark pass
// walks the landmarks of the edge list --: the set is dropped and the call that got here reports it.
void cuba_hip_solver::uploadLandmarkPriors()
{
	LandmarkPriorSet& set = lmPriorSet;
	const int n = set.n();
	if (n == 0 || (set.uploaded && set.structure == cntStructureBuilds)) return;
	std::vector<int> lmMap, lmPtr((size_t)Lf + 1, 0);
	if (lmOrderActive && Lf > 0)
	{
		lmMap.resize(Lf);
		HIP_TRY(hipMemcpyAsync(lmMap.data(), d_lmMap.data(), sizeof(int) * (size_t)Lf, hipMemcpyDeviceToHost, stream));
	}
	HIP_TRY(hipMemcpyAsync(lmPtr.data(), g.lm_ptr, sizeof(int) * ((size_t)Lf + 1), hipMemcpyDeviceToHost, stream));
	sync();
	std::vector<int> internal((size_t)n);
	for (int k = 0; k < n; k++)
	{
		const int l = set.lm[k];
		internal[k] = l < Lf && !lmMap.empty() ? lmMap[l] : l;
		if (l < Lf && lmPtr[internal[k]] == lmPtr[internal[k] + 1])
		{
			set.clear(); pf.lmp = DeviceLandmarkPriors();
			throw ArgError{ "landmark prior on free landmark " + std::to_string(l) + ", which no edge observes: the set is dropped" };
		}
	}
	set.order.resize((size_t)n);
	std::iota(set.order.begin(), set.order.end(), 0);
	std::stable_sort(set.order.begin(), set.order.end(), [&](int a, int b) { return internal[a] < internal[b]; });
	// ints: lm_ptr [Lf + 1] | lm [n] | kind [n];  values: xbar [3 n] | info [6 n] | delta [n]
	std::vector<int> ints((size_t)Lf + 1 + 2 * (size_t)n, 0);
	std::vector<Scalar> vals((size_t)10 * n);
	int* ptr = ints.data(); int* lm = ptr + Lf + 1; int* kd = lm + n;
	Scalar* vx = vals.data(); Scalar* vi = vx + 3 * (size_t)n; Scalar* vd = vi + 6 * (size_t)n;
	for (int p = 0; p < n; p++)
	{
		const size_t k = (size_t)set.order[p];
		lm[p] = internal[k]; kd[p] = set.kind[k]; vd[p] = (Scalar)set.delta[k];
		if (lm[p] < Lf) ptr[lm[p] + 1]++;
		for (int i = 0; i < 3; i++) vx[3 * (size_t)p + i] = (Scalar)set.xyz[3 * k + i];
		for (int i = 0; i < 6; i++) vi[6 * (size_t)p + i] = (Scalar)set.info[6 * k + i];
	}
	for (int l = 0; l < Lf; l++) ptr[l + 1] += ptr[l];
	set.d_ints.upload(ints, stream);
	set.d_vals.upload(vals, stream);
	set.d_chi.resize((size_t)n);
	sync();          // (the staging vectors go out of scope)
	DeviceLandmarkPriors lp;
	lp.n = n;
	lp.lm_ptr = set.d_ints.data(); lp.lm = lp.lm_ptr + Lf + 1; lp.rk_kind = lp.lm + n;
	lp.xbar = set.d_vals.data(); lp.info = lp.xbar + 3 * (size_t)n; lp.rk_delta = lp.info + 6 * (size_t)n;
	lp.chi = set.d_chi.data();
	pf.lmp = lp;
	set.uploaded = true; set.structure = cntStructureBuilds;
}

// the plain r^T Omega r of every prior at the current estimate, in the caller's order
void cuba_hip_solver::landmarkPriorChiSquares(double* out)
{
	need();
	const size_t n = (size_t)lmPriorSet.n();
	if (n == 0) return;
	launch_landmark_prior_chi2(g, pf.lmp, d_parts.data(), stream);
	std::vector<double> sorted(n);
	downloadAsDouble(pf.lmp.chi, sorted.data(), n);
	for (size_t p = 0; p < n; p++) out[lmPriorSet.order[p]] = sorted[p];
}
