// ba_relpose.hip -- SE(3) relative-pose edges (cuba_hip_set_relative_pose_edges): binary factors r^T Omega r between two poses i, j,
// r = log(T_j T_i^-1 Zbar^-1) in the [omega, upsilon] tangent of the solver's left-multiplicative update T <- exp(d) T, linearised with the
// exact derivatives dr/dd_j = J_l(r)^-1 and dr/dd_i = -J_l(r)^-1 Ad(T_j T_i^-1).  Unlike a prior, such an edge owns an
// off-diagonal block of the reduced matrix: the set of free-free pairs seeds the block pattern (ba_setup.hip), and a pair that no
// landmark connects gets a block without Schur products, which only the kernels below write.
//
//   relpose_linearize_kernel   lane = edge: r, J_i, J_j and the edge's record {J_i^T Omega J_i, J_j^T Omega J_j (upper triangles),
//                              the cross term laid out as the block (min, max) of the internal pose pair stores it, J_i^T Omega r,
//                              J_j^T Omega r}
//   relpose_gather_kernel      lane = one number of the reduced system: an entry of an off-diagonal block with relative edges (the sum of
//                              its edges' cross terms, added to what the Schur pass stored, or stored whole when the block has no products),
//                              or an entry of a pose's diagonal block (upper triangle) / of bp and (mode 1) bsc, summed over the pose's
//                              edges in the caller's order -- one writer per number, fixed order, no atomics; behind the Schur pass and the
//                              priors' launch
//   relpose_chi2_kernel        lane = edge: r^T Omega r at the current estimate into the per-edge output and into per-workgroup partials that
//                              join the reprojection edges' and the priors' in one fixed-order sum
//
// Host side: the caller's edge set (validated, kept in the caller's numbering), its pair set (part of the topology) and its upload in the
// internal pose order.
#include "ba_solver.hpp"
#include "ba_device.hpp"
#include "ba_se3.hpp"

namespace cubahip
{

constexpr int REL_LIN_BLOCK = 64;
constexpr int REL_GATHER_BLOCK = 256;
constexpr int REL_CHI_BLOCK = 256;
constexpr int REL_CHI_MAX_GROUPS = 64;
// record of an edge: [0, 21) J_i^T Omega J_i, [21, 42) J_j^T Omega J_j (upper triangles, entry c (c + 1) / 2 + r), [42, 78) the cross block
// (column-major, rows = the pose of smaller internal index), [78, 84) J_i^T Omega r, [84, 90) J_j^T Omega r
constexpr int REL_HII = 0, REL_HJJ = 21, REL_HX = 42, REL_GI = 78, REL_GJ = 84;
static_assert(REL_GJ + 6 == REL_REC, "record layout");
constexpr int REL_POSE_NUMBERS = 27;        // 21 entries of a diagonal block + 6 of bp / bsc

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
	const int a = rp.pose_i[k], b = rp.pose_j[k];
#pragma unroll
	for (int x = 0; x < 4; x++) { e.qi[x] = g.q[4 * (size_t)a + x]; e.qj[x] = g.q[4 * (size_t)b + x]; }
#pragma unroll
	for (int x = 0; x < 3; x++) { e.ti[x] = g.t[3 * (size_t)a + x]; e.tj[x] = g.t[3 * (size_t)b + x]; }
}

// r = log(T_j T_i^-1 Zbar^-1) = log(T_j (Zbar T_i)^-1): the priors' residual of pose j against Zbar T_i; A = J_w^-1
__device__ __forceinline__ void rel_residual(const RelEnds& e, const DeviceRelPoses& rp, int k, Scalar r[6], Scalar A[3][3])
{
	Scalar qz[4], tz[3], qb[4], tb[3];
#pragma unroll
	for (int x = 0; x < 4; x++) qz[x] = rp.q[4 * (size_t)k + x];
#pragma unroll
	for (int x = 0; x < 3; x++) tz[x] = rp.t[3 * (size_t)k + x];
	quat_mul(qz, e.qi, qb);
	quat_rotate(qz, e.ti, tb);
	tb[0] += tz[0]; tb[1] += tz[1]; tb[2] += tz[2];
	prior_residual(e.qj, e.tj, qb, tb, r, A);
}

// Omega r (Omega column-major) and r^T Omega r
__device__ __forceinline__ Scalar rel_info_times(const Scalar* O, const Scalar r[6], Scalar Or[6])
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
	Scalar TM[3][3], TR[3][3], X[3][3], BR[3][3], ATR[3][3];
	hat3(tM, TM);
	mul3(TM, RM.m, TR);
	mul3(A, RM.m, X);
	mul3(B, RM.m, BR);
	mul3(A, TR, ATR);
	Scalar Ji[6][6], Jj[6][6];
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int b = 0; b < 3; b++)
		{
			Jj[a][b] = A[a][b]; Jj[a][3 + b] = 0; Jj[3 + a][b] = B[a][b]; Jj[3 + a][3 + b] = A[a][b];
			Ji[a][b] = -X[a][b]; Ji[a][3 + b] = 0; Ji[3 + a][b] = -(BR[a][b] + ATR[a][b]); Ji[3 + a][3 + b] = -X[a][b];
		}
	const Scalar* O = rp.info + 36 * (size_t)k;
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
			if (rr <= c) { rel_rec(rp, k, REL_HII + c * (c + 1) / 2 + rr) = sii; rel_rec(rp, k, REL_HJJ + c * (c + 1) / 2 + rr) = sjj; }
			rel_rec(rp, k, REL_HX + (flip ? rr * 6 + c : c * 6 + rr)) = sx;
		}
	}
	Scalar Or[6];
	(void)rel_info_times(O, r, Or);
#pragma unroll
	for (int c = 0; c < 6; c++)
	{
		Scalar si = 0, sj = 0;
#pragma unroll
		for (int a = 0; a < 6; a++) { si += Ji[a][c] * Or[a]; sj += Jj[a][c] * Or[a]; }
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

__global__ __launch_bounds__(REL_CHI_BLOCK) void relpose_chi2_kernel(DeviceGraph g, DeviceRelPoses rp, Scalar* __restrict__ parts)
{
	Scalar acc = 0;
	for (int k = blockIdx.x * REL_CHI_BLOCK + threadIdx.x; k < rp.n; k += gridDim.x * REL_CHI_BLOCK)
	{
		Scalar chi = 0;
		if (k < rp.nActive)
		{
			RelEnds e;
			load_rel_ends(g, rp, k, e);
			Scalar r[6], A[3][3], Or[6];
			rel_residual(e, rp, k, r, A);
			chi = rel_info_times(rp.info + 36 * (size_t)k, r, Or);
		}
		rp.chi[k] = chi;
		acc += chi;
	}
	acc = wave_sum(acc);
	__shared__ Scalar part[REL_CHI_BLOCK / WAVE];
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
	__syncthreads();
	if (threadIdx.x == 0) parts[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

int relpose_chi2_parts(const DeviceRelPoses* rp)
{
	return rp && rp->n > 0 ? std::min((rp->n + REL_CHI_BLOCK - 1) / REL_CHI_BLOCK, REL_CHI_MAX_GROUPS) : 0;
}

void launch_relpose_linearize(const DeviceGraph& g, const DeviceStructure& st, const DeviceSystem& sys, const DeviceRelPoses& rp, int mode, hipStream_t s)
{
	if (rp.nActive <= 0) return;
	hipLaunchKernelGGL(relpose_linearize_kernel, dim3((rp.nActive + REL_LIN_BLOCK - 1) / REL_LIN_BLOCK), dim3(REL_LIN_BLOCK), 0, s, g, rp);
	const size_t numbers = (mode == 1 ? (size_t)36 * rp.nBlocks : 0) + (size_t)REL_POSE_NUMBERS * rp.nPoses;
	hipLaunchKernelGGL(relpose_gather_kernel, dim3((unsigned)((numbers + REL_GATHER_BLOCK - 1) / REL_GATHER_BLOCK)), dim3(REL_GATHER_BLOCK), 0, s, st, sys, rp, mode);
}

void launch_relpose_chi2(const DeviceGraph& g, const DeviceRelPoses& rp, Scalar* parts, hipStream_t s)
{
	const int grid = relpose_chi2_parts(&rp);
	if (grid > 0) hipLaunchKernelGGL(relpose_chi2_kernel, dim3(grid), dim3(REL_CHI_BLOCK), 0, s, g, rp, parts);
}

}  // namespace cubahip

// ---- host side --------------------------------------------------------------------------------------------------------------------

void cuba_hip_solver::setRelativePoseEdges(int n, const int32_t* pi, const int32_t* pj, const double* q, const double* t, const double* info)
{
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (n < 0) throw ArgError{ "negative relative-pose edge count" };
	if (n > 0 && (partHi >= 0 || valuesPartial)) throw StateError{ "relative-pose edges are not available on a landmark-partitioned handle" };
	if (n > 0 && E == 0) throw StateError{ "relative-pose edges need a graph with reprojection edges" };
	if (n > 0 && (!pi || !pj || !q || !t || !info)) throw ArgError{ "null relative-pose edge array" };
	std::vector<int> hi_((size_t)n), hj((size_t)n);
	std::vector<double> hq((size_t)4 * n), ht((size_t)3 * n), hinf((size_t)36 * n);
	for (int k = 0; k < n; k++)
	{
		if (pi[k] < 0 || pi[k] >= Pt || pj[k] < 0 || pj[k] >= Pt) throw ArgError{ "relative-pose edge: pose index out of range" };
		if (pi[k] == pj[k]) throw ArgError{ "relative-pose edge between a pose and itself" };
		hi_[k] = pi[k]; hj[k] = pj[k];
		double nq = 0;
		for (int i = 0; i < 4; i++) { if (!std::isfinite(q[4 * (size_t)k + i])) throw ArgError{ "non-finite relative rotation" }; nq += q[4 * (size_t)k + i] * q[4 * (size_t)k + i]; }
		nq = std::sqrt(nq);
		if (!(nq > 0) || !std::isfinite(nq)) throw ArgError{ "relative-pose quaternion of zero norm" };
		for (int i = 0; i < 4; i++) hq[4 * (size_t)k + i] = q[4 * (size_t)k + i] / nq;
		for (int i = 0; i < 3; i++) { if (!std::isfinite(t[3 * (size_t)k + i])) throw ArgError{ "non-finite relative translation" }; ht[3 * (size_t)k + i] = t[3 * (size_t)k + i]; }
		const double* O = info + 36 * (size_t)k;
		double m = 0;
		for (int i = 0; i < 36; i++) { if (!std::isfinite(O[i])) throw ArgError{ "non-finite relative-pose information" }; m = std::max(m, std::fabs(O[i])); }
		for (int c = 0; c < 6; c++)
			for (int r = 0; r < c; r++)
				if (std::fabs(O[6 * c + r] - O[6 * r + c]) > 1e-9 * m) throw ArgError{ "relative-pose information is not symmetric" };
		for (int c = 0; c < 6; c++)
			for (int r = 0; r < 6; r++) hinf[36 * (size_t)k + 6 * c + r] = r == c ? O[6 * c + r] : 0.5 * (O[6 * c + r] + O[6 * r + c]);
	}
	// the distinct free-free pairs (caller's numbering, smaller index first): part of the topology -- need() rebuilds the structure when
	// they differ from the pairs the current one was seeded with
	std::vector<uint64_t> pairs;
	for (int k = 0; k < n; k++)
		if (hi_[k] < Pf && hj[k] < Pf) pairs.push_back(((uint64_t)(uint32_t)std::min(hi_[k], hj[k]) << 32) | (uint32_t)std::max(hi_[k], hj[k]));
	std::sort(pairs.begin(), pairs.end());
	pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
	h_relI.swap(hi_); h_relJ.swap(hj); h_relQ.swap(hq); h_relT.swap(ht); h_relInfo.swap(hinf); h_relPairs.swap(pairs);
	relUploaded = false;
	rel = DeviceRelPoses();
	covBlocksValid = false;          // (the covariance blocks describe the edge set -- and the block pattern -- they were computed on)
	// (the run-to-run memories the values of the system feed, as a new graph drops them)
	firstInvValid = false; firstInvPending = false; prevRunIters.clear(); runIters.clear(); firstSolveIters = 0;
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

// the caller's set -> device, in the internal pose order: free-free edges first, stable by the block (min, max) of the internal pair -- a
// block's edges contiguous and in the caller's order --, then the edges with one fixed end, then (inactive) those with two
void cuba_hip_solver::uploadRelativePoseEdges()
{
	const int n = (int)h_relI.size();
	auto internal = [&](int p) { return p < Pf && reorderActive ? poseNewOfOld[p] : p; };
	std::vector<int> a((size_t)n), b((size_t)n);
	std::vector<uint64_t> key((size_t)n);
	for (int k = 0; k < n; k++)
	{
		a[k] = internal(h_relI[k]); b[k] = internal(h_relJ[k]);
		const int nFixed = (a[k] >= Pf) + (b[k] >= Pf);
		key[k] = nFixed == 0 ? (((uint64_t)(uint32_t)std::min(a[k], b[k]) << 32) | (uint32_t)std::max(a[k], b[k])) : (~0ull - (uint64_t)(2 - nFixed));
	}
	h_relOrder.resize((size_t)n);
	std::iota(h_relOrder.begin(), h_relOrder.end(), 0);
	std::stable_sort(h_relOrder.begin(), h_relOrder.end(), [&](int x, int y) { return key[x] < key[y]; });
	std::vector<int> posOf((size_t)n);
	for (int s = 0; s < n; s++) posOf[h_relOrder[s]] = s;
	ensureHostPattern();
	std::vector<int> si((size_t)n), sj((size_t)n), blkPtr, blkId;
	std::vector<Scalar> vals((size_t)43 * n);
	Scalar* vq = vals.data(); Scalar* vt = vq + (size_t)4 * n; Scalar* vi = vt + (size_t)3 * n;
	int nActive = 0;
	for (int s = 0; s < n; s++)
	{
		const int k = h_relOrder[s];
		si[s] = a[k]; sj[s] = b[k];
		if (a[k] < Pf || b[k] < Pf) nActive = s + 1;
		if (a[k] < Pf && b[k] < Pf && (s == 0 || key[k] != key[h_relOrder[s - 1]]))
		{
			const int row = std::min(a[k], b[k]), col = std::max(a[k], b[k]);
			const int* c0 = h_colind.data() + h_rowptr[row]; const int* c1 = h_colind.data() + h_rowptr[row + 1];
			const int* it = std::lower_bound(c0, c1, col);
			if (it == c1 || *it != col) throw StateError{ "relative-pose edge without its block in the pattern" };
			blkPtr.push_back(s); blkId.push_back((int)(it - h_colind.data()));
		}
		for (int i = 0; i < 4; i++) vq[4 * (size_t)s + i] = (Scalar)h_relQ[4 * (size_t)k + i];
		for (int i = 0; i < 3; i++) vt[3 * (size_t)s + i] = (Scalar)h_relT[3 * (size_t)k + i];
		for (int i = 0; i < 36; i++) vi[36 * (size_t)s + i] = (Scalar)h_relInfo[36 * (size_t)k + i];
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
	std::vector<int> posePtr, poseId, poseItem;
	for (size_t x = 0; x < items.size(); x++)
	{
		if (x == 0 || items[x].first != items[x - 1].first) { posePtr.push_back((int)x); poseId.push_back(items[x].first); }
		poseItem.push_back(items[x].second);
	}
	posePtr.push_back((int)items.size());
	const int nb = (int)blkId.size(), np = (int)poseId.size();
	std::vector<int> ints;
	ints.reserve(2 * (size_t)n + blkPtr.size() + blkId.size() + posePtr.size() + poseId.size() + poseItem.size());
	ints.insert(ints.end(), si.begin(), si.end());
	ints.insert(ints.end(), sj.begin(), sj.end());
	ints.insert(ints.end(), blkPtr.begin(), blkPtr.end());
	ints.insert(ints.end(), blkId.begin(), blkId.end());
	ints.insert(ints.end(), posePtr.begin(), posePtr.end());
	ints.insert(ints.end(), poseId.begin(), poseId.end());
	ints.insert(ints.end(), poseItem.begin(), poseItem.end());
	d_relInts.upload(ints, stream);
	d_relVals.upload(vals, stream);
	d_relRec.resize((size_t)REL_REC * std::max(n, 1));
	d_relChi.resize((size_t)std::max(n, 1));
	rel = DeviceRelPoses();
	rel.n = n; rel.nActive = nActive; rel.nBlocks = nb; rel.nPoses = np;
	rel.pose_i = d_relInts.data(); rel.pose_j = rel.pose_i + n;
	rel.blk_ptr = rel.pose_j + n; rel.blk_id = rel.blk_ptr + (nb + 1);
	rel.pose_ptr = rel.blk_id + nb; rel.pose_id = rel.pose_ptr + (np + 1); rel.pose_item = rel.pose_id + np;
	rel.q = d_relVals.data(); rel.t = rel.q + (size_t)4 * n; rel.info = rel.t + (size_t)3 * n;
	rel.rec = d_relRec.data(); rel.chi = d_relChi.data();
	sync();          // (the staging vectors go out of scope)
	relUploaded = true; relStructure = cntStructureBuilds;
}

void cuba_hip_solver::relativePoseChiSquares(double* out)
{
	need();
	const int n = (int)h_relI.size();
	if (n == 0) return;
	launch_relpose_chi2(g, rel, d_parts.data(), stream);
	std::vector<double> sorted((size_t)n);
	downloadAsDouble(rel.chi, sorted.data(), (size_t)n);
	for (int s = 0; s < n; s++) out[h_relOrder[s]] = sorted[s];
}
