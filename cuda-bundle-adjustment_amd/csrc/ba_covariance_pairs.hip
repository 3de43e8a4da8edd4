// ba_covariance_pairs.hip -- marginal covariances of ARBITRARY pose / landmark pairs (g2o's computeMarginals with a free block list): blocks of
// the inverse of the undamped Gauss-Newton Hessian off the factor's pattern, by triangular solves with many right-hand sides that walk only
// the parts of the elimination tree a request touches.
//
//   S = L L^T the undamped reduced matrix, factorised with the exact solver's plan (ba_direct.hip), W_ql the 6 x 3 block of Hpl.
//   Every RIGHT vertex b of a request gets a right-hand side C_b -- pose b: its 6 identity columns, landmark m: sum_r E_r W_rm (3 columns) --
//   packed into blocks of 32 columns (the poses of one segment, or ten landmarks), and X_b = L^-T L^-1 C_b is solved:
//     forward   Y_j = L_jj^-1 (C_j - sum_k L_jk Y_k)        levels ascending, j in the block's FORWARD set  (the tree ancestors of C's segments)
//     backward  X_j = L_jj^-T (Y_j - sum_i L_ij^T X_i)      levels descending, j in the BACKWARD set (the ancestors of the segments the left side reads)
//   then the pair's block follows from X (pose rows) or from a landmark-major pass over the left landmark's edges with Hll^-1 (sys.lm_sys).
// Tile products on v_mfma_f64_16x16x4_f64; one writer per tile, gather lists in ascending order, no atomics: bit-reproducible.
#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "ba_solver.hpp"
#include "ba_mfma.hpp"

using namespace cubahip;

namespace cubahip
{

// =====================================================================================================================================
// symbolic phase (host)
// =====================================================================================================================================

// A request in internal numbering: right vertices packed into 32-column blocks, pairs pointing at them.
void pair_pack(const SparseCholPlan& p, int n, const int* kindA, const int* idxA, const int* kindB, const int* idxB,
	const std::vector<int>& lmPtr, const std::vector<int>& ePose, PairRequest& rq)
{
	rq = PairRequest();
	const int T = p.T;
	auto posOfPose = [&](int q) { return p.posOfSeg[q / SC_TP]; };
	auto freeObservers = [&](int l, std::vector<int>& out) {
		out.clear();
		for (int e = lmPtr[l]; e < lmPtr[l + 1]; e++) { const int q = ePose[e] & ~STEREO_BIT; if (q < p.Pf) out.push_back(q); }
	};
	// right vertices: poses grouped by segment (one block per segment, column 6 (q mod 5)), landmarks by the first elimination position
	// of their observers' segments, ten per block
	std::vector<int> poseSegs, lms;
	for (int k = 0; k < n; k++)
	{
		if (idxA[k] < 0 || idxB[k] < 0) continue;
		if (kindB[k] == 0) poseSegs.push_back(idxB[k] / SC_TP);
		else lms.push_back(idxB[k]);
	}
	std::sort(poseSegs.begin(), poseSegs.end(), [&](int a, int b) { return p.posOfSeg[a] < p.posOfSeg[b]; });
	poseSegs.erase(std::unique(poseSegs.begin(), poseSegs.end()), poseSegs.end());
	std::sort(lms.begin(), lms.end());
	lms.erase(std::unique(lms.begin(), lms.end()), lms.end());
	std::vector<int> obs;
	std::vector<std::pair<int, int>> lmKey(lms.size());
	for (size_t a = 0; a < lms.size(); a++)
	{
		freeObservers(lms[a], obs);
		int key = T;
		for (int q : obs) key = std::min(key, posOfPose(q));
		lmKey[a] = { key, lms[a] };
	}
	std::sort(lmKey.begin(), lmKey.end());
	const int nPoseBlocks = (int)poseSegs.size(), nb = nPoseBlocks + (int)((lmKey.size() + 9) / 10);
	std::vector<int> blockOfSeg(std::max(T, 1), -1);
	for (int b = 0; b < nPoseBlocks; b++) blockOfSeg[poseSegs[b]] = b;
	std::vector<std::vector<int>> rhs((size_t)nb), left((size_t)nb);
	for (int b = 0; b < nPoseBlocks; b++) rhs[b].push_back(p.posOfSeg[poseSegs[b]]);
	for (size_t a = 0; a < lmKey.size(); a++)
	{
		const int b = nPoseBlocks + (int)(a / 10), l = lmKey[a].second;
		rq.lmRec.insert(rq.lmRec.end(), { l, b, 3 * (int)(a % 10), 0 });
		freeObservers(l, obs);
		for (int q : obs) rhs[b].push_back(posOfPose(q));
	}
	std::vector<std::pair<int, int>> lmSlot;             // (landmark, record): the right landmarks by id
	for (size_t r = 0; r < rq.lmRec.size(); r += 4) lmSlot.push_back({ rq.lmRec[r], (int)(r / 4) });
	std::sort(lmSlot.begin(), lmSlot.end());
	for (int k = 0; k < n; k++)
	{
		if (idxA[k] < 0 || idxB[k] < 0) continue;
		int blk, col;
		if (kindB[k] == 0) { blk = blockOfSeg[idxB[k] / SC_TP]; col = 6 * (idxB[k] % SC_TP); }
		else
		{
			const auto it = std::lower_bound(lmSlot.begin(), lmSlot.end(), std::make_pair(idxB[k], -1));
			blk = rq.lmRec[4 * (size_t)it->second + 1]; col = rq.lmRec[4 * (size_t)it->second + 2];
		}
		rq.pairRec.insert(rq.pairRec.end(), { kindA[k], idxA[k], blk, col, kindB[k], idxB[k], k, 0 });
		if (kindA[k] == 0) left[blk].push_back(posOfPose(idxA[k]));
		else { freeObservers(idxA[k], obs); for (int q : obs) left[blk].push_back(posOfPose(q)); }
	}
	// identity columns for the poses a request names (the other columns of a segment's block stay zero, their X too)
	{
		std::vector<int> qs;
		for (int k = 0; k < n; k++) if (idxA[k] >= 0 && idxB[k] >= 0 && kindB[k] == 0) qs.push_back(idxB[k]);
		std::sort(qs.begin(), qs.end());
		qs.erase(std::unique(qs.begin(), qs.end()), qs.end());
		// (by block, as the chunks take them: blocks follow the elimination order, pose ids need not)
		std::stable_sort(qs.begin(), qs.end(), [&](int a, int b) { return blockOfSeg[a / SC_TP] < blockOfSeg[b / SC_TP]; });
		for (int q : qs) rq.poseRec.insert(rq.poseRec.end(), { blockOfSeg[q / SC_TP], 6 * (q % SC_TP), 0, 0 });
	}
	rq.nBlocks = nb;
	rq.rhsPtr.assign(1, 0); rq.leftPtr.assign(1, 0);
	for (int b = 0; b < nb; b++)
	{
		auto& r = rhs[b]; auto& l = left[b];
		std::sort(r.begin(), r.end()); r.erase(std::unique(r.begin(), r.end()), r.end());
		std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end());
		rq.rhsPos.insert(rq.rhsPos.end(), r.begin(), r.end()); rq.rhsPtr.push_back((int)rq.rhsPos.size());
		rq.leftPos.insert(rq.leftPos.end(), l.begin(), l.end()); rq.leftPtr.push_back((int)rq.leftPos.size());
	}
}

namespace
{
inline int parent_of(const SparseCholPlan& p, int j) { return p.colPtr[j + 1] - p.colPtr[j] > 1 ? p.rowIdx[p.colPtr[j] + 1] : -1; }

// the union of the ancestor chains of pos[0 .. n) (parent = first off-diagonal row of a column), ascending; stamp = a value not yet in mark
void chain_union(const SparseCholPlan& p, const int* pos, int n, std::vector<int>& mark, int stamp, std::vector<int>& out)
{
	out.clear();
	for (int a = 0; a < n; a++)
		for (int j = pos[a]; j >= 0 && mark[j] != stamp; j = parent_of(p, j)) { mark[j] = stamp; out.push_back(j); }
	std::sort(out.begin(), out.end());
}
}  // namespace

size_t pair_block_slots(const SparseCholPlan& p, const PairRequest& rq, int b)
{
	std::vector<int> mark(std::max(p.T, 1), -1), f, bw;
	chain_union(p, rq.rhsPos.data() + rq.rhsPtr[b], rq.rhsPtr[b + 1] - rq.rhsPtr[b], mark, 0, f);
	chain_union(p, rq.leftPos.data() + rq.leftPtr[b], rq.leftPtr[b + 1] - rq.leftPtr[b], mark, 1, bw);
	std::vector<int> u;
	std::set_union(f.begin(), f.end(), bw.begin(), bw.end(), std::back_inserter(u));
	return u.size();
}

bool pair_plan(const SparseCholPlan& p, const PairRequest& rq, int b0, int b1, PairPlan& out)
{
	out = PairPlan();
	const int T = p.T, L = p.nLevels, nb = b1 - b0;
	out.b0 = b0; out.b1 = b1; out.nLevels = L; out.T = T;
	std::vector<int> level((size_t)std::max(T, 1), 0);
	for (int l = 0; l < L; l++)
		for (int c = p.lvlColPtr[l]; c < p.lvlColPtr[l + 1]; c++) level[p.lvlCols[c]] = l;
	// the finished columns k < j with a tile (j, k), ascending (the row lists of the factorisation)
	std::vector<int> rowPtr((size_t)T + 1, 0);
	for (int t = 0; t < p.nTiles; t++) if (p.rowIdx[t] != p.colOfTile[t]) rowPtr[p.rowIdx[t] + 1]++;
	for (int j = 0; j < T; j++) rowPtr[j + 1] += rowPtr[j];
	std::vector<int> rowK((size_t)rowPtr[T]), rowT((size_t)rowPtr[T]), fill(rowPtr.begin(), rowPtr.end() - 1);
	for (int k = 0; k < T; k++)
		for (int t = p.colPtr[k] + 1; t < p.colPtr[k + 1]; t++) { const int e = fill[p.rowIdx[t]]++; rowK[e] = k; rowT[e] = t; }
	out.fwdPtr.assign(1, 0); out.bwdPtr.assign(1, 0); out.slotPtr.assign(1, 0);
	out.slotOf.assign((size_t)nb * T, -1);
	std::vector<int> markF((size_t)std::max(T, 1), -1), markB((size_t)std::max(T, 1), -1), f, bw, u;
	std::vector<std::vector<int>> fRecL((size_t)L), fGL((size_t)L), bRecL((size_t)L), bGL((size_t)L);
	for (int b = b0; b < b1; b++)
	{
		const int lb = b - b0;
		chain_union(p, rq.rhsPos.data() + rq.rhsPtr[b], rq.rhsPtr[b + 1] - rq.rhsPtr[b], markF, b, f);
		chain_union(p, rq.leftPos.data() + rq.leftPtr[b], rq.leftPtr[b + 1] - rq.leftPtr[b], markB, b, bw);
		u.clear();
		std::set_union(f.begin(), f.end(), bw.begin(), bw.end(), std::back_inserter(u));
		int* so = out.slotOf.data() + (size_t)lb * T;
		for (int j : u) { so[j] = (int)out.slotCols.size(); out.slotCols.push_back(j); }
		out.slotPtr.push_back((int)out.slotCols.size());
		out.fwdCols.insert(out.fwdCols.end(), f.begin(), f.end()); out.fwdPtr.push_back((int)out.fwdCols.size());
		out.bwdCols.insert(out.bwdCols.end(), bw.begin(), bw.end()); out.bwdPtr.push_back((int)out.bwdCols.size());
		for (int j : f)
		{
			auto& G = fGL[level[j]];
			const int g0 = (int)(G.size() / 2);
			for (int e = rowPtr[j]; e < rowPtr[j + 1]; e++)
				if (markF[rowK[e]] == b) { G.push_back(rowT[e]); G.push_back(so[rowK[e]]); }
			fRecL[level[j]].insert(fRecL[level[j]].end(), { so[j], j, g0, (int)(G.size() / 2) - g0 });
		}
		for (int j : bw)
		{
			auto& G = bGL[level[j]];
			const int g0 = (int)(G.size() / 2);
			for (int t = p.colPtr[j] + 1; t < p.colPtr[j + 1]; t++)
			{
				const int i = p.rowIdx[t];
				if (markB[i] != b) return false;          // (cannot happen: the rows of a column are among its ancestors)
				G.push_back(t); G.push_back(so[i]);
			}
			bRecL[level[j]].insert(bRecL[level[j]].end(), { so[j], j, g0, (int)(G.size() / 2) - g0 });
		}
	}
	// work lists: forward by level ascending, backward by level descending (step s = level L - 1 - s); record order inside a level =
	// (block, column) ascending
	out.fLvlPtr.assign((size_t)L + 1, 0); out.bLvlPtr.assign((size_t)L + 1, 0);
	for (int s = 0; s < L; s++)
	{
		const int gF = (int)(out.fGather.size() / 2);
		for (size_t r = 0; r < fRecL[s].size(); r += 4) fRecL[s][r + 2] += gF;
		out.fRec.insert(out.fRec.end(), fRecL[s].begin(), fRecL[s].end());
		out.fGather.insert(out.fGather.end(), fGL[s].begin(), fGL[s].end());
		out.fLvlPtr[s + 1] = (int)(out.fRec.size() / 4);
		const int l = L - 1 - s, gB = (int)(out.bGather.size() / 2);
		for (size_t r = 0; r < bRecL[l].size(); r += 4) bRecL[l][r + 2] += gB;
		out.bRec.insert(out.bRec.end(), bRecL[l].begin(), bRecL[l].end());
		out.bGather.insert(out.bGather.end(), bGL[l].begin(), bGL[l].end());
		out.bLvlPtr[s + 1] = (int)(out.bRec.size() / 4);
	}
	return true;
}

// =====================================================================================================================================
// numeric phase (device)
// =====================================================================================================================================
namespace
{
// A operand slab of a column-major tile: element (row0 + (lane & 15), 4 s + (lane >> 4)); B operand slab of a column-major tile:
// element (4 s + (lane >> 4), col0 + (lane & 15)) = X[(col0 + (lane & 15)) * 32 + 4 s + (lane >> 4)]
__device__ __forceinline__ void slab_a(const Scalar* __restrict__ X, int rowOff, Scalar out[8])
{
#pragma unroll
	for (int s = 0; s < 8; s++) out[s] = X[128 * s + rowOff];
}
__device__ __forceinline__ void slab_b(const Scalar* __restrict__ X, int col0, int lane, Scalar out[8])
{
	const Scalar* q = X + (col0 + (lane & 15)) * SC_T + (lane >> 4);
#pragma unroll
	for (int s = 0; s < 8; s++) out[s] = q[4 * s];
}
}  // namespace

// identity columns of the right-hand side: rec {block, row = column of the pose in its block}
__global__ __launch_bounds__(256) void pairs_rhs_pose_kernel(PairDev v, const int* __restrict__ rec, int n)
{
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= 6 * n) return;
	const int r = idx / 6, k = idx % 6;
	const int blk = rec[4 * r], c = rec[4 * r + 1];
	const int slot = v.slotOf[(size_t)blk * v.T + v.rhsPos[blk]];
	v.X[(size_t)SC_TT * slot + (c + k) * SC_T + c + k] = Scalar(1);
}

// C_m = sum_{r in obs_free(m)} E_r W_rm: thread = (landmark, element (k, c) of W), the landmark's edges in their stored order
__global__ __launch_bounds__(256) void pairs_rhs_landmark_kernel(DeviceGraph g, PairDev v, const int* __restrict__ rec, int n,
	const int* __restrict__ posOfSeg, const Scalar* __restrict__ W)
{
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= 18 * n) return;
	const int r = idx / 18, e18 = idx % 18, k = e18 % 6, c = e18 / 6;
	const int il = rec[4 * r], blk = rec[4 * r + 1], col = rec[4 * r + 2];
	const int* so = v.slotOf + (size_t)blk * v.T;
	for (int e = g.lm_ptr[il]; e < g.lm_ptr[il + 1]; e++)
	{
		const int q = g.e_pose[e] & ~STEREO_BIT;
		if (q >= g.Pf) continue;
		Scalar* x = v.X + (size_t)SC_TT * so[posOfSeg[q / SC_TP]] + (col + c) * SC_T + 6 * (q % SC_TP) + k;
		*x += W[18 * (size_t)e + c * 6 + k];
	}
}

// Forward step: workgroup = (block, column j) of one level, Y_j = L_jj^-1 (C_j - sum_k L_jk Y_k) over the restricted gather list.  Four
// waves, one 16 x 16 quadrant each; the next entry's operands are loaded under the current entry's products.  L_jj^-1 sits in the diagonal
// tile's slot of d.tiles (selinv_diag_inverse_kernel).
__global__ __launch_bounds__(256) void pairs_forward_level_kernel(SparseChol d, PairDev v, int first)
{
	__shared__ Scalar Ws[SC_T][SC_T + 1];
	const int4 rec = reinterpret_cast<const int4*>(v.fRec)[first + blockIdx.x];
	const int slot = rec.x, j = rec.y, g0 = rec.z, n = rec.w;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wi = wv >> 1, wj = wv & 1;
	const int off = (lane >> 4) * SC_T + (lane & 15);
	const int2* __restrict__ G = reinterpret_cast<const int2*>(v.fGather) + g0;
	MfmaAcc acc = mfma_zero();
	Scalar a[8], b[8];
	auto load = [&](int e) {
		const int2 gg = G[e];
		slab_a(d.tiles + (size_t)SC_TT * gg.x, 16 * wi + off, a);           // L_jk, column-major
		slab_b(v.X + (size_t)SC_TT * gg.y, 16 * wj, lane, b);              // Y_k, column-major
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
	Scalar* Y = v.X + (size_t)SC_TT * slot;
	const int col = 16 * wj + (lane & 15);
#pragma unroll
	for (int q = 0; q < 4; q++) { const int row = 16 * wi + mfma_row(lane, q); Ws[row][col] = Y[col * SC_T + row] - mfma_get(acc, q); }
	__syncthreads();
	slab_a(d.tiles + (size_t)SC_TT * d.colPtr[j], 16 * wi + off, a);        // L_jj^-1, column-major
#pragma unroll
	for (int s = 0; s < 8; s++) b[s] = Ws[4 * s + (lane >> 4)][col];
	MfmaAcc y = mfma_zero();
#pragma unroll
	for (int s = 0; s < 8; s++) y = mfma_16x16x4(a[s], b[s], y);
#pragma unroll
	for (int q = 0; q < 4; q++) Y[col * SC_T + 16 * wi + mfma_row(lane, q)] = mfma_get(y, q);
}

// Backward step: workgroup = (block, column j), X_j = L_jj^-T (Y_j - sum_{i in rows(j)} L_ij^T X_i); L_ij^T is the transposed copy of the
// factor (d.tilesT, L_ij row-major = L_ij^T column-major), Y_j is what the forward steps left in the slot (zero outside the forward set).
__global__ __launch_bounds__(256) void pairs_backward_level_kernel(SparseChol d, PairDev v, int first)
{
	__shared__ Scalar Ws[SC_T][SC_T + 1];
	const int4 rec = reinterpret_cast<const int4*>(v.bRec)[first + blockIdx.x];
	const int slot = rec.x, j = rec.y, g0 = rec.z, n = rec.w;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wi = wv >> 1, wj = wv & 1;
	const int off = (lane >> 4) * SC_T + (lane & 15);
	const int2* __restrict__ G = reinterpret_cast<const int2*>(v.bGather) + g0;
	MfmaAcc acc = mfma_zero();
	Scalar a[8], b[8];
	auto load = [&](int e) {
		const int2 gg = G[e];
		slab_a(d.tilesT + (size_t)SC_TT * gg.x, 16 * wi + off, a);          // L_ij^T, column-major
		slab_b(v.X + (size_t)SC_TT * gg.y, 16 * wj, lane, b);              // X_i
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
	Scalar* X = v.X + (size_t)SC_TT * slot;
	const int col = 16 * wj + (lane & 15);
#pragma unroll
	for (int q = 0; q < 4; q++) { const int row = 16 * wi + mfma_row(lane, q); Ws[row][col] = X[col * SC_T + row] - mfma_get(acc, q); }
	__syncthreads();
	// A(r, k) = L_jj^-T (r, k) = Linv(k, r) = Linv[r * 32 + k]
	{
		const Scalar* Li = d.tiles + (size_t)SC_TT * d.colPtr[j] + (16 * wi + (lane & 15)) * SC_T + (lane >> 4);
#pragma unroll
		for (int s = 0; s < 8; s++) a[s] = Li[4 * s];
	}
#pragma unroll
	for (int s = 0; s < 8; s++) b[s] = Ws[4 * s + (lane >> 4)][col];
	MfmaAcc x = mfma_zero();
#pragma unroll
	for (int s = 0; s < 8; s++) x = mfma_16x16x4(a[s], b[s], x);
#pragma unroll
	for (int q = 0; q < 4; q++) X[col * SC_T + 16 * wi + mfma_row(lane, q)] = mfma_get(x, q);
}

// One wave per pair, rec {kind a, a, block, column of b, kind b, b, output index, 0} (internal numbering); lane e < dim(a) dim(b) = element
// (e mod dim(a), e / dim(a)) of the block, column-major.  Pose a: 6 rows of X_b; landmark l: M = sum_{q in obs(l)} W_ql^T X_b[q] over its
// edges in their stored order, then the Hll^-1 factors and signs of DESIGN.md section 7b.
__global__ __launch_bounds__(64) void pairs_extract_kernel(DeviceGraph g, DeviceSystem sys, PairDev v, const int* __restrict__ posOfSeg,
	const Scalar* __restrict__ W, const int* __restrict__ recs, Scalar* __restrict__ out)
{
	__shared__ Scalar Ms[3][6];
	const int* rec = recs + 8 * (size_t)blockIdx.x;
	const int ka = rec[0], ia = rec[1], blk = rec[2], colB = rec[3], kb = rec[4], ib = rec[5], o = rec[6];
	const int lane = threadIdx.x;
	const int da = ka ? 3 : 6, db = kb ? 3 : 6;
	const int r = lane % da, c = lane / da;
	const int* so = v.slotOf + (size_t)blk * v.T;
	Scalar Hm[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, Hl[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
	if (kb)
	{
		const Scalar* h = sys.lm_sys + 9 * (size_t)ib;
#pragma unroll
		for (int i = 0; i < 3; i++)
#pragma unroll
			for (int k = 0; k < 3; k++) Hm[i][k] = h[sym3_idx(i, k)];
	}
	Scalar val = 0;
	if (ka == 0)
	{
		if (lane < da * db)
		{
			const Scalar* x = v.X + (size_t)SC_TT * so[posOfSeg[ia / SC_TP]] + 6 * (ia % SC_TP) + r;
			if (!kb) val = x[(colB + c) * SC_T];
			else
			{
				Scalar s = 0;
#pragma unroll
				for (int k = 0; k < 3; k++) s += x[(colB + k) * SC_T] * Hm[k][c];
				val = -s;
			}
		}
	}
	else
	{
		const Scalar* h = sys.lm_sys + 9 * (size_t)ia;
#pragma unroll
		for (int i = 0; i < 3; i++)
#pragma unroll
			for (int k = 0; k < 3; k++) Hl[i][k] = h[sym3_idx(i, k)];
		if (lane < 3 * db)
		{
			Scalar m = 0;
			for (int e = g.lm_ptr[ia]; e < g.lm_ptr[ia + 1]; e++)
			{
				const int q = g.e_pose[e] & ~STEREO_BIT;
				if (q >= g.Pf) continue;
				const Scalar* x = v.X + (size_t)SC_TT * so[posOfSeg[q / SC_TP]] + (colB + c) * SC_T + 6 * (q % SC_TP);
				const Scalar* w = W + 18 * (size_t)e + r * 6;
#pragma unroll
				for (int k = 0; k < 6; k++) m += w[k] * x[k];
			}
			Ms[r][c] = m;
		}
		__syncthreads();
		if (lane < da * db)
		{
			if (!kb)
			{
				Scalar s = 0;
#pragma unroll
				for (int k = 0; k < 3; k++) s += Hl[r][k] * Ms[k][c];
				val = -s;
			}
			else
			{
				Scalar s = ia == ib ? Hl[r][c] : Scalar(0);
#pragma unroll
				for (int k = 0; k < 3; k++)
#pragma unroll
					for (int k2 = 0; k2 < 3; k2++) s += Hl[r][k] * Ms[k][k2] * Hm[k2][c];
				val = s;
			}
		}
	}
	if (lane < 36) out[36 * (size_t)o + lane] = lane < da * db ? val : Scalar(0);
}

}  // namespace cubahip

// ---------------------------------------------------------------------------------------------------------------------------------------
// host driver: chunks of RHS blocks against the workspace budget
// ---------------------------------------------------------------------------------------------------------------------------------------
int cubahip_host::run_covariance_pairs(const SparseChol& d, const SparseCholPlan& plan, const DeviceGraph& g, const DeviceSystem& sys, const Scalar* W,
	const PairRequest& rq, size_t budgetBytes, PairWork& w, Scalar* out, hipStream_t s)
{
	const size_t tileBytes = sizeof(Scalar) * SC_TT;
	// (the factor's tiles stay as the factorisation left them, except the diagonal slots of d.tiles: A_jj -> L_jj^-1)
	if (d.T > 0) launch_diag_inverse(d, s);
	std::vector<size_t> slots((size_t)rq.nBlocks);
	for (int b = 0; b < rq.nBlocks; b++)
	{
		slots[b] = pair_block_slots(plan, rq, b);
		if (slots[b] * tileBytes > budgetBytes)
		{
			char buf[200];
			std::snprintf(buf, sizeof buf, "covariance pairs: one block of right-hand sides needs %.1f MB of workspace, %.1f MB are available", slots[b] * tileBytes / 1e6, budgetBytes / 1e6);
			throw std::runtime_error(buf);
		}
	}
	// pairs, pose and landmark records of every chunk: by block (the records are grouped by block already except the pairs)
	std::vector<int> pairOrder((size_t)(rq.pairRec.size() / 8));
	for (size_t k = 0; k < pairOrder.size(); k++) pairOrder[k] = (int)k;
	std::stable_sort(pairOrder.begin(), pairOrder.end(), [&](int a, int b) { return rq.pairRec[8 * (size_t)a + 2] < rq.pairRec[8 * (size_t)b + 2]; });
	int chunks = 0;
	size_t pp = 0, pr = 0, lr = 0;
	for (int b0 = 0; b0 < rq.nBlocks;)
	{
		int b1 = b0;
		size_t used = 0;
		while (b1 < rq.nBlocks && (b1 == b0 || (used + slots[b1]) * tileBytes <= budgetBytes)) used += slots[b1++];
		PairPlan pl;
		if (!pair_plan(plan, rq, b0, b1, pl)) throw std::logic_error("covariance pairs: a row of a column is not among its ancestors");
		std::vector<int> poseRec, lmRec, pairRec, rhsPos;
		for (; pr < rq.poseRec.size() && rq.poseRec[pr] < b1; pr += 4) poseRec.insert(poseRec.end(), { rq.poseRec[pr] - b0, rq.poseRec[pr + 1], 0, 0 });
		for (; lr < rq.lmRec.size() && rq.lmRec[lr + 1] < b1; lr += 4) lmRec.insert(lmRec.end(), { rq.lmRec[lr], rq.lmRec[lr + 1] - b0, rq.lmRec[lr + 2], 0 });
		for (; pp < pairOrder.size() && rq.pairRec[8 * (size_t)pairOrder[pp] + 2] < b1; pp++)
		{
			const int* r = rq.pairRec.data() + 8 * (size_t)pairOrder[pp];
			pairRec.insert(pairRec.end(), { r[0], r[1], r[2] - b0, r[3], r[4], r[5], r[6], 0 });
		}
		for (int b = b0; b < b1; b++) rhsPos.push_back(rq.rhsPtr[b + 1] > rq.rhsPtr[b] ? rq.rhsPos[rq.rhsPtr[b]] : 0);
		std::vector<int> ints;
		auto put = [&](const std::vector<int>& v) { const size_t o = ints.size(); ints.insert(ints.end(), v.begin(), v.end()); while (ints.size() % 4) ints.push_back(0); return o; };
		const size_t oF = put(pl.fRec), oFG = put(pl.fGather), oB = put(pl.bRec), oBG = put(pl.bGather), oS = put(pl.slotOf), oR = put(rhsPos),
			oP = put(poseRec), oL = put(lmRec), oX = put(pairRec);
		if (ints.empty()) ints.push_back(0);
		w.ints.upload(ints, s);
		w.X.resize(std::max<size_t>(1, pl.slots()) * SC_TT);
		if (pl.slots()) HIP_TRY(hipMemsetAsync(w.X.data(), 0, tileBytes * pl.slots(), s));
		HIP_TRY(hipStreamSynchronize(s));            // (`ints` is a local)
		const int* base = w.ints.data();
		PairDev v;
		v.X = w.X.data(); v.fRec = base + oF; v.fGather = base + oFG; v.bRec = base + oB; v.bGather = base + oBG; v.slotOf = base + oS; v.rhsPos = base + oR;
		v.T = plan.T;
		const int nPose = (int)(poseRec.size() / 4), nLm = (int)(lmRec.size() / 4), nPair = (int)(pairRec.size() / 8);
		if (nPose) hipLaunchKernelGGL(pairs_rhs_pose_kernel, dim3((6 * nPose + 255) / 256), dim3(256), 0, s, v, base + oP, nPose);
		if (nLm) hipLaunchKernelGGL(pairs_rhs_landmark_kernel, dim3((18 * nLm + 255) / 256), dim3(256), 0, s, g, v, base + oL, nLm, d.posOfSeg, W);
		for (int st = 0; st < pl.nLevels; st++)
		{
			const int n = pl.fLvlPtr[st + 1] - pl.fLvlPtr[st];
			if (n > 0) hipLaunchKernelGGL(pairs_forward_level_kernel, dim3(n), dim3(256), 0, s, d, v, pl.fLvlPtr[st]);
		}
		for (int st = 0; st < pl.nLevels; st++)
		{
			const int n = pl.bLvlPtr[st + 1] - pl.bLvlPtr[st];
			if (n > 0) hipLaunchKernelGGL(pairs_backward_level_kernel, dim3(n), dim3(256), 0, s, d, v, pl.bLvlPtr[st]);
		}
		if (nPair) hipLaunchKernelGGL(pairs_extract_kernel, dim3(nPair), dim3(64), 0, s, g, sys, v, d.posOfSeg, W, base + oX, out);
		HIP_TRY(hipGetLastError());
		chunks++;
		b0 = b1;
	}
	return chunks;
}

bool cuba_hip_solver::computeCovariancePairs(int n, const int32_t* kindA, const int32_t* indexA, const int32_t* kindB, const int32_t* indexB, double* out)
{
	if (sizeof(Scalar) != 8) throw ArgError{ "marginal covariances need the fp64 library: an fp32 inverse of a bundle-adjustment Hessian is not meaningful" };
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (partHi >= 0) throw StateError{ "marginal covariances are not available on a landmark-partitioned handle" };
	if (n < 0 || (n > 0 && (!kindA || !indexA || !kindB || !indexB || !out))) throw ArgError{ "covariance pairs: null argument or negative count" };
	for (int k = 0; k < n; k++)
		for (int side = 0; side < 2; side++)
		{
			const int kind = side ? kindB[k] : kindA[k], idx = side ? indexB[k] : indexA[k];
			if (kind != CUBA_HIP_VERTEX_POSE && kind != CUBA_HIP_VERTEX_LANDMARK) throw ArgError{ "covariance pairs: pair " + std::to_string(k) + " has an unknown vertex kind" };
			if (idx < 0 || idx >= (kind == CUBA_HIP_VERTEX_POSE ? Pt : Lt)) throw ArgError{ "covariance pairs: pair " + std::to_string(k) + " names a vertex out of range" };
		}
	need();
	const auto t0 = Clock::now();
	SparseCholPlan none;
	const SparseCholPlan* plan = &none;
	if (Pf > 0)
	{
		const bool validBefore = directPlanValid, refusedBefore = directRefused;
		if (!ensureDirectPlan())
		{
			const std::string why = lastError;
			directPlanValid = validBefore; directRefused = refusedBefore;
			throw std::runtime_error("covariance pairs: " + why);
		}
		plan = &directPlan;
	}
	// caller -> internal numbering; a fixed vertex is -1 (a zero block)
	bool anyLm = false;
	for (int k = 0; k < n; k++) anyLm = anyLm || kindA[k] == CUBA_HIP_VERTEX_LANDMARK || kindB[k] == CUBA_HIP_VERTEX_LANDMARK;
	std::vector<int> lmMap, lmPtr, ePose;
	if (anyLm && Lf > 0)
	{
		if (lmOrderActive)
		{
			lmMap.resize(Lf);
			HIP_TRY(hipMemcpyAsync(lmMap.data(), d_lmMap.data(), sizeof(int) * (size_t)Lf, hipMemcpyDeviceToHost, stream));
		}
		lmPtr.resize((size_t)Lf + 1); ePose.resize(std::max(E, 1));
		HIP_TRY(hipMemcpyAsync(lmPtr.data(), g.lm_ptr, sizeof(int) * ((size_t)Lf + 1), hipMemcpyDeviceToHost, stream));
		if (E) HIP_TRY(hipMemcpyAsync(ePose.data(), g.e_pose, sizeof(int) * (size_t)E, hipMemcpyDeviceToHost, stream));
		sync();
	}
	std::vector<int> ia(n), ib(n);
	auto internal = [&](int kind, int idx) {
		if (kind == CUBA_HIP_VERTEX_POSE) return idx < Pf ? poseNewOfOld[idx] : -1;
		return idx < Lf ? (lmMap.empty() ? idx : lmMap[idx]) : -1;
	};
	for (int k = 0; k < n; k++) { ia[k] = internal(kindA[k], indexA[k]); ib[k] = internal(kindB[k], indexB[k]); }
	// Orientation: every distinct RIGHT vertex costs a column group and a forward path, every left vertex only rows of the extraction.  So
	// the side with fewer distinct vertices goes right (pose 0 against every pose: one block instead of one per segment), and the blocks
	// come back transposed (Sigma_ab = Sigma_ba^T).
	auto distinct = [&](const int32_t* kind, const std::vector<int>& idx) {
		std::vector<long long> v;
		for (int k = 0; k < n; k++) if (ia[k] >= 0 && ib[k] >= 0) v.push_back(2LL * idx[k] + kind[k]);
		std::sort(v.begin(), v.end());
		return (size_t)(std::unique(v.begin(), v.end()) - v.begin());
	};
	const bool swapped = distinct(kindA, ia) < distinct(kindB, ib);
	PairRequest rq;
	if (swapped) pair_pack(*plan, n, kindB, ib.data(), kindA, ia.data(), lmPtr, ePose, rq);
	else pair_pack(*plan, n, kindA, ia.data(), kindB, ib.data(), lmPtr, ePose, rq);
	// workspace budget: the option, or half the free device memory
	size_t budget = (size_t)(covWorkspaceMb * 1048576.0);
	if (covWorkspaceMb <= 0)
	{
		size_t freeB = 0, totalB = 0;
		if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); freeB = 0; }
		budget = freeB / 2;
	}
	// 1-2: linearisation and Schur complement at lambda = 0 in fp64 (computeCovariance's reasons)
	zeroReduced();
	st.mixed = 0;
	linearize(1, 0.0, false);
	st.mixed = mixedPrecision ? 1 : 0;
	int* hflag = (int*)hostStage();
	if (Pf > 0)
	{
		launch_sparse_chol_fill(st, sys, directDev, stream);
		launch_sparse_chol_factor(directDev, directPlan, stream);
		HIP_TRY(hipMemcpyAsync(hflag, directDev.fail, sizeof(int), hipMemcpyDeviceToHost, stream));
		sync();
		if (*hflag) return false;
	}
	const Scalar* W = nullptr;
	if (anyLm && Lf > 0 && E > 0)
	{
		d_covW.resize((size_t)18 * E);
		launch_edge_w(g, d_covW.data(), stream);
		W = d_covW.data();
	}
	const int nDev = (int)(rq.pairRec.size() / 8);
	d_pairOut.resize((size_t)36 * std::max(nDev, 1));
	// the device output is indexed by the caller's pair index k: renumber to a dense range
	std::vector<int> outOf(nDev);
	for (int r = 0; r < nDev; r++) { outOf[r] = rq.pairRec[8 * (size_t)r + 6]; rq.pairRec[8 * (size_t)r + 6] = r; }
	SparseChol dv = directDev;
	if (Pf == 0) dv.T = 0;
	covPairChunks = run_covariance_pairs(dv, *plan, g, sys, W, rq, budget, covPairWork, d_pairOut.data(), stream);
	std::vector<double> h((size_t)36 * nDev);
	if (nDev) downloadAsDouble(d_pairOut.data(), h.data(), h.size());         // (synchronises)
	else HIP_TRY(hipStreamSynchronize(stream));
	covPairsSeconds = std::chrono::duration<double>(Clock::now() - t0).count();
	std::fill(out, out + (size_t)36 * n, 0.0);
	for (int r = 0; r < nDev; r++)
	{
		const int k = outOf[r];
		const double* src = h.data() + 36 * (size_t)r;
		double* dst = out + 36 * (size_t)k;
		if (!swapped) { std::copy(src, src + 36, dst); continue; }
		// the device block is Sigma_ba (rows from b, leading dimension dim(b)); the caller's is its transpose
		const int da = kindA[k] == CUBA_HIP_VERTEX_POSE ? 6 : 3, db = kindB[k] == CUBA_HIP_VERTEX_POSE ? 6 : 3;
		for (int j = 0; j < db; j++)
			for (int i = 0; i < da; i++) dst[j * da + i] = src[i * db + j];
	}
	// (a large request's workspace is not kept for the handle's lifetime: it would stand in the way of later allocations)
	if (covPairWork.X.size() * sizeof(Scalar) > ((size_t)64 << 20)) covPairWork.X.release();
	if (std::getenv("CUBA_HIP_DEBUG"))
		std::fprintf(stderr, "[cuba_hip] covariance pairs: %d pairs, %d blocks%s, %d chunks, %.3f ms\n", n, rq.nBlocks, swapped ? " (sides swapped)" : "", covPairChunks, 1e3 * covPairsSeconds);
	return true;
}
