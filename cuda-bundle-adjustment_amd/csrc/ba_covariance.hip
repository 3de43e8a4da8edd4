// ba_covariance.hip -- marginal covariances at the current estimate: the inverse of the UNDAMPED Gauss-Newton Hessian, selected on the
// blocks a user asks for (g2o's SparseOptimizer::computeMarginals / Ceres' Covariance; the reference has no counterpart).
//
//   1. landmark pass + Schur pass at lambda = 0 (the LM path's own kernels)            -> S = Hpp - Hpl Hll^-1 Hlp, Hll^-1
//   2. fill + factorisation of S with the exact solver's plan (ba_direct.hip)          -> L
//   3. selected inversion on L's pattern (Takahashi recurrence, levels top-down)       -> Sigma = S^-1 on the pattern
//        selinv_diag_inverse_kernel   L_jj^-1, one wave per tile column
//        selinv_u_kernel              U_kj = L_kj L_jj^-1 for every off-diagonal tile (one launch: no dependencies)
//        per step (= level, top-down): selinv_off_level_kernel   Sigma_ij = -sum_k Sigma_ik U_kj
//                                      selinv_diag_level_kernel  Sigma_jj = L_jj^-T L_jj^-1 - sum_k U_kj^T Sigma_kj
//   4. extraction: pose blocks / blocks of the reduced matrix from Sigma's tiles; landmark marginals by a landmark-major pass over the
//      edges, Sigma_l = Hll^-1 + Hll^-1 (sum_{p,q in obs(l)} W_p^T Sigma_pq W_q) Hll^-1.
// Tile products on v_mfma_f64_16x16x4_f64; one writer per tile, gather lists in a fixed order, no atomics: bit-reproducible.
#include "ba_solver.hpp"
#include "ba_mfma.hpp"

using namespace cubahip;

namespace cubahip
{

// A operand slab of a tile stored TRANSPOSED (the logical matrix is X^T, X column-major): element (row0 + (lane & 15), 4 s + (lane >> 4))
// of X^T = X[(row0 + (lane & 15)) * 32 + 4 s + (lane >> 4)].  (The plain layout is ba_direct.hip's load_slab: tile[128 s + rowOff].)
__device__ __forceinline__ void slab_plain(const Scalar* __restrict__ X, int rowOff, Scalar out[8])
{
#pragma unroll
	for (int s = 0; s < 8; s++) out[s] = X[128 * s + rowOff];
}
__device__ __forceinline__ void slab_trans(const Scalar* __restrict__ X, int row0, int lane, Scalar out[8])
{
	const Scalar* p = X + (row0 + (lane & 15)) * SC_T + (lane >> 4);
#pragma unroll
	for (int s = 0; s < 8; s++) out[s] = p[4 * s];
}

// L_jj^-1 (lower triangular) into the diagonal tile's slot of d.tiles, column-major.  One wave per tile column, lane c < 32 = column c of
// the inverse: forward substitution L x = e_c with the rows of L broadcast from LDS (the padded unknowns' identity carries over).
__global__ __launch_bounds__(64) void selinv_diag_inverse_kernel(SparseChol d)
{
	__shared__ Scalar Ls[SC_T][SC_T + 1];
	const int j = blockIdx.x, lane = threadIdx.x;
	const int t0 = d.colPtr[j];
	const Scalar* L0 = d.tilesT + (size_t)SC_TT * t0;           // L_jj mirrored into both triangles
	for (int e = lane; e < SC_TT; e += 64) Ls[e & 31][e >> 5] = L0[e];
	__syncthreads();
	if (lane >= SC_T) return;
	const int c = lane;
	Scalar x[SC_T];
#pragma unroll
	for (int r = 0; r < SC_T; r++)
	{
		Scalar v = r == c ? Scalar(1) : Scalar(0);
#pragma unroll
		for (int m = 0; m < r; m++) v -= Ls[r][m] * x[m];
		x[r] = v * d.rinv[SC_T * (size_t)j + r];
	}
	Scalar* out = d.tiles + (size_t)SC_TT * t0 + c * SC_T;
#pragma unroll
	for (int r = 0; r < SC_T; r++) out[r] = x[r];
}

// U_kj = L_kj L_jj^-1 for every off-diagonal tile, stored ROW-major into its slot of d.tilesT (the transposed copy of L is not needed
// any more): the B operand of the off-diagonal step and the A operand (as U^T) of the diagonal step then load like plain slabs.
__global__ __launch_bounds__(256) void selinv_u_kernel(SparseChol d, const int* __restrict__ offRec)
{
	const int4 rec = reinterpret_cast<const int4*>(offRec)[blockIdx.x];
	const int t = rec.x, j = rec.y;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wi = wv >> 1, wj = wv & 1;
	const int off = (lane >> 4) * SC_T + (lane & 15);
	const Scalar* Lkj = d.tiles + (size_t)SC_TT * t;
	const Scalar* Li = d.tiles + (size_t)SC_TT * d.colPtr[j];
	Scalar a[8], b[8];
	slab_plain(Lkj, 16 * wi + off, a);
	slab_trans(Li, 16 * wj, lane, b);            // B(k, c) = Linv(k, c) = Li[c * 32 + k]
	MfmaAcc acc = mfma_zero();
#pragma unroll
	for (int s = 0; s < 8; s++) acc = mfma_16x16x4(a[s], b[s], acc);
	Scalar* U = d.tilesT + (size_t)SC_TT * t;
	const int col = 16 * wj + (lane & 15);
#pragma unroll
	for (int q = 0; q < 4; q++) U[(16 * wi + mfma_row(lane, q)) * SC_T + col] = mfma_get(acc, q);
}

// One step's off-diagonal tiles: workgroup = tile (i, j), Sigma_ij = -sum_{k in I_j} Sigma~_ik U_kj over its gather list (Sigma~_ik read
// transposed from the stored (k, i) when i < k).  Four waves, one 16 x 16 quadrant each; the next entry's operands are loaded under the
// current entry's products.
__global__ __launch_bounds__(256) void selinv_off_level_kernel(SparseChol d, SelInv v, int first)
{
	const int4 rec = reinterpret_cast<const int4*>(v.offRec)[first + blockIdx.x];
	const int t = rec.x, g0 = rec.z, n = rec.w;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wi = wv >> 1, wj = wv & 1;
	const int off = (lane >> 4) * SC_T + (lane & 15);
	const int2* __restrict__ G = reinterpret_cast<const int2*>(v.gather) + g0;
	MfmaAcc acc = mfma_zero();
	Scalar a[8], b[8];
	auto load = [&](int e) {
		const int2 g = G[e];
		const Scalar* S = v.sigma + (size_t)SC_TT * (g.x & 0x3fffffff);
		if (g.x >> 30) slab_trans(S, 16 * wi, lane, a);
		else slab_plain(S, 16 * wi + off, a);
		slab_plain(d.tilesT + (size_t)SC_TT * g.y, 16 * wj + off, b);      // B(k, c) = U(k, c), row-major
	};
	if (n > 0) load(0);
	for (int e = 0; e < n; e++)
	{
		Scalar ca[8], cb[8];
#pragma unroll
		for (int s = 0; s < 8; s++) { ca[s] = a[s]; cb[s] = b[s]; }
		if (e + 1 < n) load(e + 1);
#pragma unroll
		for (int s = 0; s < 8; s++) acc = mfma_16x16x4(ca[s], cb[s], acc);
	}
	Scalar* out = v.sigma + (size_t)SC_TT * t;
	const int col = 16 * wj + (lane & 15);
#pragma unroll
	for (int q = 0; q < 4; q++) out[col * SC_T + 16 * wi + mfma_row(lane, q)] = -mfma_get(acc, q);
}

// One step's diagonal tiles: workgroup = column j, Sigma_jj = L_jj^-T L_jj^-1 - sum_{k in I_j} U_kj^T Sigma_kj (the column's own
// off-diagonal tiles, written by the step's first launch), stored full: the lower triangle mirrored into the upper one.
__global__ __launch_bounds__(256) void selinv_diag_level_kernel(SparseChol d, SelInv v, int first)
{
	__shared__ Scalar Ds[SC_T][SC_T + 1];
	const int j = v.cols[first + blockIdx.x];
	const int t0 = d.colPtr[j], t1 = d.colPtr[j + 1];
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wi = wv >> 1, wj = wv & 1;
	const int off = (lane >> 4) * SC_T + (lane & 15);
	Scalar a[8], b[8];
	MfmaAcc acc0 = mfma_zero(), acc = mfma_zero();
	{
		const Scalar* Li = d.tiles + (size_t)SC_TT * t0;
		slab_trans(Li, 16 * wi, lane, a);           // A(r, k) = Linv(k, r)
		slab_trans(Li, 16 * wj, lane, b);           // B(k, c) = Linv(k, c)
#pragma unroll
		for (int s = 0; s < 8; s++) acc0 = mfma_16x16x4(a[s], b[s], acc0);
	}
	for (int t = t0 + 1; t < t1; t++)
	{
		slab_plain(d.tilesT + (size_t)SC_TT * t, 16 * wi + off, a);       // A(r, k) = U^T(r, k) = U(k, r): U row-major
		slab_trans(v.sigma + (size_t)SC_TT * t, 16 * wj, lane, b);        // B(k, c) = Sigma_kj(k, c), column-major
#pragma unroll
		for (int s = 0; s < 8; s++) acc = mfma_16x16x4(a[s], b[s], acc);
	}
	{
		const int col = 16 * wj + (lane & 15);
#pragma unroll
		for (int q = 0; q < 4; q++) Ds[16 * wi + mfma_row(lane, q)][col] = mfma_get(acc0, q) - mfma_get(acc, q);
	}
	__syncthreads();
	Scalar* out = v.sigma + (size_t)SC_TT * t0;
	for (int e = tid; e < SC_TT; e += 256)
	{
		const int r = e & 31, c = e >> 5;
		out[e] = r >= c ? Ds[r][c] : Ds[c][r];         // element (r, c), column-major
	}
}

void launch_selinv(const SparseChol& d, const SparseCholPlan& plan, const SelInvPlan& sp, const SelInv& v, hipStream_t s)
{
	if (d.T <= 0) return;
	hipLaunchKernelGGL(selinv_diag_inverse_kernel, dim3(d.T), dim3(64), 0, s, d);
	const int nOff = (int)(sp.offRec.size() / 4);
	if (nOff > 0) hipLaunchKernelGGL(selinv_u_kernel, dim3(nOff), dim3(256), 0, s, d, v.offRec);
	for (int st = 0; st < sp.nLevels; st++)
	{
		const int n = sp.stepPtr[st + 1] - sp.stepPtr[st];
		if (n > 0) hipLaunchKernelGGL(selinv_off_level_kernel, dim3(n), dim3(256), 0, s, d, v, sp.stepPtr[st]);
		const int m = sp.colStepPtr[st + 1] - sp.colStepPtr[st];
		if (m > 0) hipLaunchKernelGGL(selinv_diag_level_kernel, dim3(m), dim3(256), 0, s, d, v, sp.colStepPtr[st]);
	}
	(void)plan;
}

void launch_diag_inverse(const SparseChol& d, hipStream_t s)
{
	if (d.T > 0) hipLaunchKernelGGL(selinv_diag_inverse_kernel, dim3(d.T), dim3(64), 0, s, d);
}

// element (r, c) of Sigma's 6 x 6 block (pa, pb) of free poses (internal order) whose tile is known: the addressing of
// schol_fill_blocks_kernel (tile (row position, column position), column-major)
__device__ __forceinline__ Scalar sigma_elem(const Scalar* __restrict__ tile, int tr, int li, int lj)
{
	const int row = tr ? li : lj, col = tr ? lj : li;
	return tile[col * SC_T + row];
}

__global__ __launch_bounds__(256) void selinv_extract_kernel(DeviceStructure st, SparseChol d, SelInv v, Scalar* __restrict__ poseCov,
	Scalar* __restrict__ blkCov, int Pf)
{
	const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
	const int e = (int)(idx % 36), r = e % 6, c = e / 6;
	const size_t item = idx / 36;
	if (item < (size_t)Pf)
	{
		if (!poseCov) return;
		const int p = (int)item;
		const int li = 6 * (p % SC_TP);
		const Scalar* T0 = v.sigma + (size_t)SC_TT * d.colPtr[d.posOfSeg[p / SC_TP]];
		poseCov[idx] = T0[(li + c) * SC_T + li + r];
		return;
	}
	const size_t b = item - Pf;
	if (!blkCov || b >= (size_t)st.nblk) return;
	const int bi = st.hsc_blkrow[b], bj = st.hsc_colind[b];
	const int tt = d.blkTile[b];
	blkCov[36 * b + e] = sigma_elem(v.sigma + (size_t)SC_TT * (tt & 0x3fffffff), tt >> 30, 6 * (bi % SC_TP) + r, 6 * (bj % SC_TP) + c);
}

void launch_selinv_extract(const DeviceStructure& st, const SparseChol& d, const SelInv& v, Scalar* pose_cov, Scalar* blk_cov, int Pf, hipStream_t s)
{
	const size_t total = (size_t)36 * ((size_t)Pf + (blk_cov ? (size_t)st.nblk : 0));
	if (Pf > 0 && total) hipLaunchKernelGGL(selinv_extract_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st, d, v, pose_cov, blk_cov, Pf);
}

// W = Hpl block of every edge (6 x 3, column-major: J_p^T w rho' J_l) at the current estimate; zero for an edge to a fixed pose or landmark
__global__ __launch_bounds__(256) void edge_w_kernel(DeviceGraph g, Scalar* __restrict__ W)
{
	const int e = blockIdx.x * 256 + threadIdx.x;
	if (e >= g.E) return;
	LaneEdge le;
	linearize_edge(g, e, le);
	const bool on = le.ip < g.Pf && le.il < g.Lf;
	Scalar* w = W + 18 * (size_t)e;
#pragma unroll
	for (int c = 0; c < 3; c++)
#pragma unroll
		for (int r = 0; r < 6; r++)
		{
			const Scalar v = le.lin.JP[0][r] * le.lin.JL[0][c] + le.lin.JP[1][r] * le.lin.JL[1][c] + le.lin.JP[2][r] * le.lin.JL[2][c];
			w[c * 6 + r] = on ? le.wr * v : Scalar(0);
		}
}

void launch_edge_w(const DeviceGraph& g, Scalar* W, hipStream_t s)
{
	if (g.E > 0) hipLaunchKernelGGL(edge_w_kernel, dim3((g.E + 255) / 256), dim3(256), 0, s, g, W);
}

// the tile of Sigma that holds block (ka, kb) of tile positions (ka != kb): (max, min) in column min's sorted row list
__device__ __forceinline__ const Scalar* sigma_tile(const SparseChol& d, const SelInv& v, int ka, int kb)
{
	const int c = ka < kb ? ka : kb, r = ka < kb ? kb : ka;
	int lo = d.colPtr[c] + 1, hi = d.colPtr[c + 1] - 1;
	if (lo > hi) return v.sigma + (size_t)SC_TT * d.colPtr[c];     // (cannot happen: a co-visible pair's tile is on the pattern)
	while (lo < hi)
	{
		const int mid = (lo + hi) >> 1;
		if (d.rowIdx[mid] < r) lo = mid + 1; else hi = mid;
	}
	return v.sigma + (size_t)SC_TT * lo;
}

// Landmark-major pass, one wave per free landmark: lane a (strided over the landmark's edges) forms V_a = sum_b Sigma_{p_a p_b} W_b and
// its share W_a^T V_a; the wave sums the shares in a fixed order; Sigma_l = Hll^-1 + Hll^-1 M Hll^-1 with Hll^-1 from the landmark pass
// at lambda = 0 (sys.lm_sys).
__global__ __launch_bounds__(256) void landmark_cov_kernel(DeviceGraph g, DeviceSystem sys, SparseChol d, SelInv v, const Scalar* __restrict__ W,
	Scalar* __restrict__ out)
{
	const int il = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (il >= g.Lf) return;
	const int e0 = g.lm_ptr[il], e1 = g.lm_ptr[il + 1];
	Scalar m[6] = { 0, 0, 0, 0, 0, 0 };          // (00, 01, 02, 11, 12, 22)
	for (int ea = e0 + lane; ea < e1; ea += 64)
	{
		const int pa = g.e_pose[ea] & ~STEREO_BIT;
		if (pa >= g.Pf) continue;
		const int ka = d.posOfSeg[pa / SC_TP], la = 6 * (pa % SC_TP);
		Scalar V[18];
#pragma unroll
		for (int k = 0; k < 18; k++) V[k] = 0;
		for (int eb = e0; eb < e1; eb++)
		{
			const int pb = g.e_pose[eb] & ~STEREO_BIT;
			if (pb >= g.Pf) continue;
			const int kb = d.posOfSeg[pb / SC_TP], lb = 6 * (pb % SC_TP);
			// S(r, c) = Sigma(pa unknown r, pb unknown c): the stored tile holds Sigma_{ka kb} (ka > kb or ka == kb, column-major) or Sigma_{kb ka}
			const Scalar* S;
			int sr, sc;
			if (ka == kb) { S = v.sigma + (size_t)SC_TT * d.colPtr[ka]; sr = 1; sc = SC_T; }
			else if (ka > kb) { S = sigma_tile(d, v, ka, kb); sr = 1; sc = SC_T; }
			else { S = sigma_tile(d, v, ka, kb); sr = SC_T; sc = 1; }
			S += la * sr + lb * sc;
			const Scalar* wb = W + 18 * (size_t)eb;
			Scalar Wb[18];
#pragma unroll
			for (int k = 0; k < 18; k++) Wb[k] = wb[k];
#pragma unroll
			for (int c6 = 0; c6 < 6; c6++)
			{
				Scalar sv[6];
#pragma unroll
				for (int r = 0; r < 6; r++) sv[r] = S[r * sr + c6 * sc];
#pragma unroll
				for (int c = 0; c < 3; c++)
#pragma unroll
					for (int r = 0; r < 6; r++) V[c * 6 + r] += sv[r] * Wb[c * 6 + c6];
			}
		}
		const Scalar* wa = W + 18 * (size_t)ea;
		Scalar Wa[18];
#pragma unroll
		for (int k = 0; k < 18; k++) Wa[k] = wa[k];
#pragma unroll
		for (int i = 0; i < 3; i++)
#pragma unroll
			for (int jj = i; jj < 3; jj++)
			{
				Scalar s = 0;
#pragma unroll
				for (int r = 0; r < 6; r++) s += Wa[i * 6 + r] * V[jj * 6 + r];
				m[sym3_idx(i, jj)] += s;
			}
	}
#pragma unroll
	for (int k = 0; k < 6; k++) m[k] = wave_sum(m[k]);
	if (lane >= 9) return;
	const Scalar* h = sys.lm_sys + 9 * (size_t)il;          // Hll^-1 (6 unique entries) at lambda = 0
	Scalar H[3][3], M[3][3];
#pragma unroll
	for (int i = 0; i < 3; i++)
#pragma unroll
		for (int jj = 0; jj < 3; jj++) { H[i][jj] = h[sym3_idx(i, jj)]; M[i][jj] = m[sym3_idx(i, jj)]; }
	const int r = lane % 3, c = lane / 3;
	Scalar s = H[r][c];
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int b = 0; b < 3; b++) s += H[r][a] * M[a][b] * H[b][c];
	out[9 * (size_t)il + c * 3 + r] = s;
}

void launch_landmark_covariance(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const SparseChol& d, const SelInv& v,
	Scalar* w_scratch, Scalar* lm_cov, hipStream_t s)
{
	(void)st;
	if (g.Lf <= 0) return;
	if (g.E > 0) hipLaunchKernelGGL(edge_w_kernel, dim3((g.E + 255) / 256), dim3(256), 0, s, g, w_scratch);
	hipLaunchKernelGGL(landmark_cov_kernel, dim3((g.Lf + 3) / 4), dim3(256), 0, s, g, sys, d, v, w_scratch, lm_cov);
}

}  // namespace cubahip

// ---------------------------------------------------------------------------------------------------------------------------------------
// handle orchestration
// ---------------------------------------------------------------------------------------------------------------------------------------
void cubahip_host::upload_selinv_plan(const SelInvPlan& p, DevBuf<int>& d_ints, SelInv& view, hipStream_t s)
{
	std::vector<int> ints;
	auto put = [&](const std::vector<int>& v) { const size_t o = ints.size(); ints.insert(ints.end(), v.begin(), v.end()); while (ints.size() % 4) ints.push_back(0); return o; };
	const size_t oRec = put(p.offRec), oG = put(p.gather), oCols = put(p.cols);
	if (ints.empty()) ints.push_back(0);
	d_ints.upload(ints, s);
	HIP_TRY(hipStreamSynchronize(s));
	view.offRec = d_ints.data() + oRec; view.gather = d_ints.data() + oG; view.cols = d_ints.data() + oCols;
}

bool cuba_hip_solver::computeCovariance(double* poseCov, double* lmCov)
{
	if (sizeof(Scalar) != 8) throw ArgError{ "marginal covariances need the fp64 library: an fp32 inverse of a bundle-adjustment Hessian is not meaningful" };
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (partHi >= 0) throw StateError{ "marginal covariances are not available on a landmark-partitioned handle" };
	need();
	const auto t0 = Clock::now();
	if (Pf > 0)
	{
		// the exact solver's plan and buffers; a refusal here is the covariance's alone -- the LM path decides for itself at its first exact solve
		const bool validBefore = directPlanValid, refusedBefore = directRefused;
		if (!ensureDirectPlan())
		{
			const std::string why = lastError;
			directPlanValid = validBefore; directRefused = refusedBefore;
			throw std::runtime_error("marginal covariances: " + why);
		}
		if (selPlanFor != directPlanBuilds)
		{
			if (!selinv_plan(directPlan, selPlan)) throw std::logic_error("marginal covariances: a tile of the selected inversion is missing from the factor's pattern");
			upload_selinv_plan(selPlan, d_selInts, selDev, stream);
			selPlanFor = directPlanBuilds;
		}
		const size_t sigmaCount = (size_t)SC_TT * std::max(1, directPlan.nTiles);
		if (d_sigma.size() < sigmaCount)
		{
			size_t freeB = 0, totalB = 0;
			const size_t bytes = selPlan.sigmaBytes() + sizeof(Scalar) * 36 * ((size_t)Pf + st.nblk) + sizeof(Scalar) * 18 * (size_t)E;
			if (hipMemGetInfo(&freeB, &totalB) != hipSuccess || bytes > freeB)
			{
				(void)hipGetLastError();
				char buf[200];
				std::snprintf(buf, sizeof buf, "marginal covariances: the inverse on the factor's pattern needs %.1f MB, %.1f MB of device memory are free", bytes / 1e6, freeB / 1e6);
				throw std::runtime_error(buf);
			}
			d_sigma.resize(sigmaCount);
		}
	}
	covBlocksValid = false;
	// 1-2: linearisation and Schur complement at lambda = 0 (the damping the kernels see is this argument, not the handle's `lambda`),
	// in fp64 throughout even under "mixed_precision": its fp32 records perturb the reduced matrix by ~1e-7 relative, which the inverse
	// amplifies to ~1e-2 on a 40-pose graph (the LM step tolerates that, a covariance does not).  need() restores the mode.
	zeroReduced();
	st.mixed = 0;
	linearize(1, 0.0, false);
	st.mixed = mixedPrecision ? 1 : 0;
	int* hflag = (int*)hostStage();
	if (Pf > 0)
	{
		// 3: fill (the diagonal blocks' upper triangles are all the fill reads: no damping step needed) and factorisation
		launch_sparse_chol_fill(st, sys, directDev, stream);
		launch_sparse_chol_factor(directDev, directPlan, stream);
		HIP_TRY(hipMemcpyAsync(hflag, directDev.fail, sizeof(int), hipMemcpyDeviceToHost, stream));
		sync();
		if (*hflag) return false;
		selDev.sigma = d_sigma.data();
		launch_selinv(directDev, directPlan, selPlan, selDev, stream);
		// 4: extraction
		d_covPose.resize((size_t)36 * Pf); d_covBlk.resize((size_t)36 * std::max(1, st.nblk));
		launch_selinv_extract(st, directDev, selDev, d_covPose.data(), d_covBlk.data(), Pf, stream);
	}
	if (lmCov && Lf > 0)
	{
		d_covW.resize((size_t)18 * std::max(1, E)); d_covLm.resize((size_t)9 * Lf);
		launch_landmark_covariance(g, st, sys, directDev, selDev, d_covW.data(), d_covLm.data(), stream);
	}
	HIP_TRY(hipStreamSynchronize(stream));
	covSeconds = std::chrono::duration<double>(Clock::now() - t0).count();
	covBlocksValid = Pf > 0;
	if (poseCov)
	{
		std::fill(poseCov, poseCov + (size_t)36 * Pt, 0.0);
		std::vector<double> v((size_t)36 * Pf);
		downloadAsDouble(d_covPose.data(), v.data(), v.size());
		for (int i = 0; i < Pf; i++) std::copy(v.begin() + 36 * (size_t)i, v.begin() + 36 * (size_t)(i + 1), poseCov + 36 * (size_t)poseOldOfNew[i]);
	}
	if (lmCov)
	{
		std::fill(lmCov, lmCov + (size_t)9 * Lt, 0.0);
		if (Lf > 0) downloadAsDouble(landmarkRowsForCaller(d_covLm.data(), Lf, 9), lmCov, (size_t)9 * Lf);
	}
	if (std::getenv("CUBA_HIP_DEBUG"))
		std::fprintf(stderr, "[cuba_hip] marginal covariances: %d poses, %d tiles, %d levels, %lld tile products, landmarks %s, %.3f ms\n",
			Pf, directPlan.nTiles, directPlan.nLevels, selPlan.products, lmCov ? "yes" : "no", 1e3 * covSeconds);
	return true;
}

void cuba_hip_solver::covarianceBlocks(double* out)
{
	if (!haveGraph || !covBlocksValid) throw StateError{ "no covariance computed on the current graph (cuba_hip_compute_covariance first)" };
	const size_t n = (size_t)36 * st.nblk;
	if (!out || !n) return;
	downloadAsDouble(d_covBlk.data(), out, n);
	if (reorderActive)
	{
		const std::vector<double> v(out, out + n);
		const auto blocks = callerBlocks();
		for (size_t k = 0; k < blocks.size(); k++)
		{
			const double* src36 = v.data() + 36 * (size_t)blocks[k].src;
			double* dst = out + 36 * k;
			for (int c = 0; c < 6; c++)
				for (int r = 0; r < 6; r++) dst[c * 6 + r] = blocks[k].transposed ? src36[r * 6 + c] : src36[c * 6 + r];
		}
	}
}
