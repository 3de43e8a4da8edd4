// ba_gate.hip -- edge gating: reprojection edges switched off and on without a new graph (g2o's setLevel / computeActiveErrors flow of
// ORB-SLAM's local bundle adjustment and pose optimisation, which the reference lacks).  A gated edge is an edge of zero information: the
// handle keeps the uploaded information w0 untouched and points DeviceGraph::e_w at a second, live array w_live = mask ? w0 : +0, so no
// other kernel knows of the gate.  Here: the classification pass (lane = sorted edge, like residual_chi2_kernel), the mask's way between
// the caller's edge order and the sorted one, and the active observations per landmark.  Every count is a wave ballot + popcount into
// per-workgroup partials added by a second stage: no atomics, like every other sum of the library.  Below the kernels: the handle's side
// (cuba_hip_gate_edges, cuba_hip_set_edge_active, cuba_hip_get_edge_active, cuba_hip_landmark_active_edges).

#include "ba_solver.hpp"
#include "ba_device.hpp"

namespace cubahip
{

namespace
{
constexpr int GATE_T = 256;

__device__ __forceinline__ int ballot_count(bool p) { return __popcll(__ballot(p)); }

// One pass over the sorted edges.  a.g.e_w is the UPLOADED information.  Six counts per workgroup into a.parts[6 * workgroup ..].
__global__ __launch_bounds__(GATE_T) void edge_gate_kernel(EdgeGateArgs a)
{
	__shared__ int red[GATE_T / WAVE][GATE_COUNTS];
	const DeviceGraph& g = a.g;
	int cnt[GATE_COUNTS] = { 0, 0, 0, 0, 0, 0 };          // wave-uniform
	// (whole waves walk the loop together: the ballots below need every lane of the wave)
	for (int base = g.e_begin + blockIdx.x * GATE_T; base < g.e_end; base += gridDim.x * GATE_T)
	{
		const int e = base + threadIdx.x;
		const bool in = e < g.e_end;
		bool stereo = false, was = true, chiOk = false, depthOk = false;
		Scalar w0 = 0, chi = 0;
		if (in)
		{
			LaneEdge le;
			load_edge(g, g.q, g.t, g.Xw, e, le);
			w0 = le.w; stereo = le.stereo;
			chi = w0 * edge_residual(le.q, le.t, le.cam, le.Xw, le.meas, le.stereo, le.lin.r, le.Xc);
			// (a NaN fails both tests)
			chiOk = !!((double)chi <= (stereo ? a.chi2_stereo : a.chi2_mono));
			depthOk = !a.require_depth || le.Xc[2] > Scalar(0);
			if (a.mask_in) was = a.mask_in[e] != 0;
		}
		const bool pass = chiOk && depthOk;
		const bool now = in && pass && (a.mode != GATE_ONLY_REMOVE || was);
		cnt[0] += ballot_count(now && !stereo);
		cnt[1] += ballot_count(now && stereo);
		cnt[2] += ballot_count(in && depthOk && !chiOk && !stereo);
		cnt[3] += ballot_count(in && depthOk && !chiOk && stereo);
		cnt[4] += ballot_count(in && !depthOk);
		cnt[5] += ballot_count(in && now != was);
		if (in)
		{
			if (a.chi_out) a.chi_out[e] = chi;
			if (a.mode != GATE_DRY_RUN) { a.mask_out[e] = now ? 1 : 0; a.w_live[e] = now ? w0 : Scalar(0); }
		}
	}
	if ((threadIdx.x & (WAVE - 1)) == 0)
#pragma unroll
		for (int k = 0; k < GATE_COUNTS; k++) red[threadIdx.x / WAVE][k] = cnt[k];
	__syncthreads();
	if (threadIdx.x < GATE_COUNTS)
	{
		long long s = 0;
#pragma unroll
		for (int w = 0; w < GATE_T / WAVE; w++) s += red[w][threadIdx.x];
		a.parts[(size_t)GATE_COUNTS * blockIdx.x + threadIdx.x] = s;
	}
}

// second stage: one wave adds the n workgroups' partials, lane-strided, then across the lanes
__global__ __launch_bounds__(WAVE) void gate_counts_kernel(const long long* __restrict__ parts, int n, long long* __restrict__ out)
{
	long long s[GATE_COUNTS] = { 0, 0, 0, 0, 0, 0 };
	for (int i = threadIdx.x; i < n; i += WAVE)
#pragma unroll
		for (int k = 0; k < GATE_COUNTS; k++) s[k] += parts[(size_t)GATE_COUNTS * i + k];
#pragma unroll
	for (int k = 0; k < GATE_COUNTS; k++)
	{
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o);
		if (threadIdx.x == 0) out[k] = s[k];
	}
}

// the mask from the caller's edge order into the sorted one, and the live information with it (w_live = mask ? w0 : +0)
__global__ __launch_bounds__(GATE_T) void gate_apply_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ maskCaller, const Scalar* __restrict__ w0,
	int E, uint8_t* __restrict__ maskSorted, Scalar* __restrict__ w_live)
{
	const int i = blockIdx.x * GATE_T + threadIdx.x;
	if (i >= E) return;
	const bool on = maskCaller[perm[i]] != 0;
	maskSorted[i] = on ? 1 : 0;
	w_live[i] = on ? w0[i] : Scalar(0);
}

// ... and back (the counterpart of unsort_kernel for the mask)
__global__ __launch_bounds__(GATE_T) void gate_unsort_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ maskSorted, int E, uint8_t* __restrict__ maskCaller)
{
	const int i = blockIdx.x * GATE_T + threadIdx.x;
	if (i < E) maskCaller[perm[i]] = maskSorted[i];
}

__device__ __forceinline__ int lane_count(const uint8_t* mask, int e0, int e1)
{
	if (!mask) return e1 - e0;
	int n = 0;
	for (int e = e0; e < e1; e++) n += mask[e] != 0;
	return n;
}

// Lane = landmark l of the CALLER's numbering (row newOfOld[l] of the internal order): the lane walks its edges when they are at most 64.
// The longer ones are the big_lm class of the wave list (every such landmark of an unpartitioned handle is in it): the workgroup kernel
// below counts them, and this one fetches the result.
__global__ __launch_bounds__(GATE_T) void landmark_active_kernel(const int* __restrict__ lm_ptr, const uint8_t* __restrict__ mask, const int* __restrict__ newOfOld,
	const int* __restrict__ bigInternal, int Lt, int* __restrict__ out)
{
	const int l = blockIdx.x * GATE_T + threadIdx.x;
	if (l >= Lt) return;
	const int m = newOfOld ? newOfOld[l] : l;
	const int e0 = lm_ptr[m], e1 = lm_ptr[m + 1];
	out[l] = e1 - e0 > WAVE ? bigInternal[m] : lane_count(mask, e0, e1);
}

// workgroup = one landmark of the big_lm class
__global__ __launch_bounds__(GATE_T) void landmark_active_big_kernel(const int* __restrict__ lm_ptr, const uint8_t* __restrict__ mask, const int* __restrict__ big_lm,
	int* __restrict__ outInternal)
{
	__shared__ int red[GATE_T / WAVE];
	const int m = big_lm[blockIdx.x];
	const int e0 = lm_ptr[m], e1 = lm_ptr[m + 1];
	int n = 0;
	for (int e = e0; e < e1; e += GATE_T) n += ballot_count(e + (int)threadIdx.x < e1 && (!mask || mask[e + threadIdx.x] != 0));
	if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = n;
	__syncthreads();
	if (threadIdx.x == 0) outInternal[m] = red[0] + red[1] + red[2] + red[3];
}

inline dim3 gate_grid(size_t n) { return dim3((unsigned)((n + GATE_T - 1) / GATE_T)); }
}  // namespace

int edge_gate_grid(const DeviceGraph& g)
{
	const int n = g.e_end - g.e_begin;
	return n > 0 ? min((n + GATE_T - 1) / GATE_T, 2048) : 0;
}

void launch_edge_gate(const EdgeGateArgs& a, long long* counts, hipStream_t s)
{
	const int grid = edge_gate_grid(a.g);
	if (grid > 0) hipLaunchKernelGGL(edge_gate_kernel, dim3(grid), dim3(GATE_T), 0, s, a);
	hipLaunchKernelGGL(gate_counts_kernel, dim3(1), dim3(WAVE), 0, s, a.parts, grid, counts);
}

void launch_gate_apply(const uint32_t* perm, const uint8_t* maskCaller, const Scalar* w0, int E, uint8_t* maskSorted, Scalar* w_live, hipStream_t s)
{
	if (E > 0) hipLaunchKernelGGL(gate_apply_kernel, gate_grid(E), dim3(GATE_T), 0, s, perm, maskCaller, w0, E, maskSorted, w_live);
}

void launch_gate_unsort(const uint32_t* perm, const uint8_t* maskSorted, int E, uint8_t* maskCaller, hipStream_t s)
{
	if (E > 0) hipLaunchKernelGGL(gate_unsort_kernel, gate_grid(E), dim3(GATE_T), 0, s, perm, maskSorted, E, maskCaller);
}

void launch_landmark_active(const int* lm_ptr, const uint8_t* mask, const int* newOfOld, int Lt, const int* big_lm, int nBig, int* bigInternal, int* out, hipStream_t s)
{
	if (Lt <= 0) return;
	if (nBig > 0) hipLaunchKernelGGL(landmark_active_big_kernel, dim3(nBig), dim3(GATE_T), 0, s, lm_ptr, mask, big_lm, bigInternal);
	hipLaunchKernelGGL(landmark_active_kernel, gate_grid(Lt), dim3(GATE_T), 0, s, lm_ptr, mask, newOfOld, bigInternal, Lt, out);
}

}  // namespace cubahip

// ---------------------------------------------------------------------------------------------------------------------------------------
// The handle's side.  The mask in the CALLER's edge order (d_gateMaskCaller) is what the gate is: the sorted copy and the live information
// are derived from it and from d_w through the sort permutation, again whenever that permutation or d_w changed (refreshGate, from need()).
// d_w itself is never edited -- a "same values" promise of cuba_hip_set_graph keeps it as the uploaded information.
// ---------------------------------------------------------------------------------------------------------------------------------------
void cuba_hip_solver::requireGateable() const
{
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (partHi >= 0) throw StateError{ "edge gating is not available on a landmark-partitioned handle" };
}

const uint32_t* cuba_hip_solver::permDevice()
{
	if (devTopology) return d_perm.data();
	// (host pipeline: the permutation lives on the host)
	d_gatePerm.uploadRaw(reinterpret_cast<const uint32_t*>(perm.data()), perm.size(), stream);
	return d_gatePerm.data();
}

void cuba_hip_solver::allocGate()
{
	d_wLive.resize(E); d_gateMask.resize(E); d_gateMaskCaller.resize(E);
}

void cuba_hip_solver::gateChanged()
{
	gateActive = true; gateStamp = valuesStamp;
	g.e_w = d_wLive.data();
	covBlocksValid = false;
}

void cuba_hip_solver::refreshGate()
{
	if (!gateActive || gateStamp == valuesStamp) return;
	allocGate();
	launch_gate_apply(permDevice(), d_gateMaskCaller.data(), d_w.data(), E, d_gateMask.data(), d_wLive.data(), stream);
	gateChanged();
}

void cuba_hip_solver::clearGate()
{
	if (!gateActive) return;
	gateActive = false;
	g.e_w = d_w.data();
	covBlocksValid = false;
	sync();
	d_wLive.release(); d_gateMask.release(); d_gateMaskCaller.release(); d_gateCounts.release(); d_gatePerm.release(); d_gateLm.release();
}

void cuba_hip_solver::gateEdges(const double chi2Max[2], bool positiveDepth, int mode, int64_t counts[6], double* chi2PerEdge)
{
	if (mode != GATE_RECLASSIFY && mode != GATE_ONLY_REMOVE && mode != GATE_DRY_RUN) throw ArgError{ "bad gate mode" };
	if (!chi2Max || std::isnan(chi2Max[0]) || std::isnan(chi2Max[1])) throw ArgError{ "chi2_max must be two numbers (+inf: no chi2 test)" };
	requireGateable();
	need();
	const bool dry = mode == GATE_DRY_RUN;
	EdgeGateArgs a;
	a.g = g; a.g.e_w = d_w.data();
	a.chi2_mono = chi2Max[0]; a.chi2_stereo = chi2Max[1];
	a.require_depth = positiveDepth ? 1 : 0; a.mode = mode;
	a.mask_in = gateActive ? d_gateMask.data() : nullptr;
	if (!dry) { allocGate(); a.mask_out = d_gateMask.data(); a.w_live = d_wLive.data(); }
	a.chi_out = chi2PerEdge ? d_perEdge.data() : nullptr;
	d_gateCounts.resize((size_t)GATE_COUNTS * (1 + edge_gate_grid(a.g)));
	a.parts = d_gateCounts.data() + GATE_COUNTS;
	launch_edge_gate(a, d_gateCounts.data(), stream);
	if (!dry)
	{
		launch_gate_unsort(permDevice(), d_gateMask.data(), E, d_gateMaskCaller.data(), stream);
		gateChanged();
	}
	long long h[GATE_COUNTS];
	HIP_TRY(hipMemcpyAsync(h, d_gateCounts.data(), sizeof h, hipMemcpyDeviceToHost, stream));
	if (chi2PerEdge && E)
	{
		d_chiCaller.resize(E);
		topo::launch_unsort(permDevice(), d_perEdge.data(), E, d_chiCaller.data(), stream);
		HIP_TRY(hipMemcpyAsync(chi2PerEdge, d_chiCaller.data(), sizeof(double) * E, hipMemcpyDeviceToHost, stream));
	}
	sync();
	if (counts) for (int k = 0; k < GATE_COUNTS; k++) counts[k] = h[k];
}

void cuba_hip_solver::setEdgeActive(const uint8_t* active)
{
	requireGateable();
	if (!active) { clearGate(); return; }
	need();
	allocGate();
	h_gateMask.resize(E);
	for (int e = 0; e < E; e++) h_gateMask[e] = active[e] ? 1 : 0;
	d_gateMaskCaller.upload(h_gateMask, stream);
	launch_gate_apply(permDevice(), d_gateMaskCaller.data(), d_w.data(), E, d_gateMask.data(), d_wLive.data(), stream);
	gateChanged();
	sync();
}

void cuba_hip_solver::getEdgeActive(uint8_t* active)
{
	requireGateable();
	if (!active && E) throw ArgError{ "null output" };
	if (!E) return;
	if (!gateActive) { std::memset(active, 1, (size_t)E); return; }
	HIP_TRY(hipMemcpyAsync(active, d_gateMaskCaller.data(), (size_t)E, hipMemcpyDeviceToHost, stream));
	sync();
}

void cuba_hip_solver::landmarkActiveEdges(int32_t* perLandmark)
{
	requireGateable();
	if (!perLandmark && Lt) throw ArgError{ "null output" };
	need();
	if (!Lt) return;
	d_gateLm.resize((size_t)2 * Lt);
	launch_landmark_active(d_lmptr.data(), gateActive ? d_gateMask.data() : nullptr, lmOrderActive ? d_lmMap.data() : nullptr, Lt, st.big_lm, st.nBig,
		d_gateLm.data(), d_gateLm.data() + Lt, stream);
	HIP_TRY(hipMemcpyAsync(perLandmark, d_gateLm.data() + Lt, sizeof(int32_t) * (size_t)Lt, hipMemcpyDeviceToHost, stream));
	sync();
}
