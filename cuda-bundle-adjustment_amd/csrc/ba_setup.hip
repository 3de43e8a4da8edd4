// ba_setup.hip -- graph upload (cuba_hip_set_graph) and symbolic structure of the reduced system, on the device (rocPRIM sorts + segment
// kernels of ba_structure.hip) and on the host (the independent cross-check pipeline): counterpart of CudaBlockSolver::initialize /
// buildStructure (/root/reference/src/cuda_bundle_adjustment.cpp:115-366) and HschurSparseBlockMatrix::constructFromVertices.
#include "ba_solver.hpp"

using namespace cubahip;

void cuba_hip_solver::finishValues()
{
	if (!valuesPending) return;
	valuesPending = false;
	HIP_TRY(hipStreamWaitEvent(stream, evValues, 0));
	gatherSortedValues();
	valuesStamp++;          // (the permutation or the sorted values are new: an edge gate derives its copies again, refreshGate)
}

void cuba_hip_solver::gatherSortedValues()
{
	sizeSortedValues();
	topo::launch_gather_edges(d_perm.data(), d_rawEp.data(), d_rawEl.data(), d_rawDim.data(), d_rawMeas.data(), d_rawOmega.data(), E,
		nullptr, nullptr, d_mu.data(), d_mv.data(), d_mr.data(), d_w.data(), stream);
	sortedValuesValid = true;
}

UploadFacts cuba_hip_solver::uploadFacts() const
{
	static const bool noCache = std::getenv("CUBA_HIP_NO_STRUCTURE_CACHE") != nullptr;   // A/B knob for set-up timings
	UploadFacts f{};
	f.haveGraph = haveGraph; f.haveStructure = haveStructure;
	f.Pt = Pt; f.Pf = Pf; f.Lt = Lt; f.Lf = Lf; f.E = E;
	f.partitioned = partHi >= 0;
	f.devTopology = devTopology; f.hostTopoValid = hostTopoValid; f.reorderActive = reorderActive; f.lmOrderActive = lmOrderActive;
	// (a begin without its end: the sorted measurement / information arrays it was going to fill were never gathered -- a "same values"
	// promise for THIS call must not keep them: round-4 advisor)
	f.sortedValuesValid = sortedValuesValid && !valuesPending;
	f.valuesPartial = valuesPartial;
	f.sortedValuesFit = d_mu.size() == (size_t)E && d_w.size() == (size_t)E;
	f.edgesHeld = h_inEp.size() == (size_t)E;
	f.deviceSetup = deviceSetup; f.poseReorder = poseReorder; f.lmReorder = lmReorder;
	f.noCache = noCache;
	return f;
}

// the caller's index arrays are the previous call's, entry by entry (read where needsEdgeCompare says so: the counts are equal then)
bool cuba_hip_solver::sameEdgeArrays(const UploadArrays& in) const
{
	const int32_t* ep = in.ep; const int32_t* el = in.el; const uint8_t* edim = in.edim;
	std::atomic<int> diff{ 0 };
	parallelFor(E, [&](int e) { if (h_inEp[e] != ep[e] || h_inEl[e] != el[e] || h_inDim[e] != edim[e]) diff.store(1, std::memory_order_relaxed); });
	return diff == 0;
}

static void validateEdges(const UploadCall& c, const cuba_hip_solver::UploadArrays& in)
{
	const int32_t* ep = in.ep; const int32_t* el = in.el; const uint8_t* edim = in.edim;
	const int Pt = c.Pt, Pf = c.Pf, Lt = c.Lt, Lf = c.Lf;
	std::atomic<int> bad{ 0 };
	cuba_hip_solver::parallelFor(c.E, [&](int e) {
		if (ep[e] < 0 || ep[e] >= Pt || el[e] < 0 || el[e] >= Lt) bad.store(1, std::memory_order_relaxed);
		else if (edim[e] != 2 && edim[e] != 3) bad.store(2, std::memory_order_relaxed);
		else if (ep[e] >= Pf && el[e] >= Lf) bad.store(3, std::memory_order_relaxed);
	});
	if (bad == 1) throw ArgError{ "edge index out of range" };
	if (bad == 2) throw ArgError{ "edge_dim must be 2 or 3" };
	if (bad == 3) throw ArgError{ "edge with both ends fixed (must be dropped by the caller)" };
}

void cuba_hip_solver::setGraph(int Pt_, int Pf_, int Lt_, int Lf_, const double* q, const double* t, const double* cam, const double* Xw,
	int E_, const int32_t* ep, const int32_t* el, const uint8_t* edim, const double* meas, const double* omega, bool deferValues, int ownLo, int ownHi)
{
	// (a promise covers one call, successful or not: it is gone before the first check that can refuse this one)
	const UploadCall call{ Pt_, Pf_, Lt_, Lf_, E_, ownLo, ownHi, deferValues, hintSameEdges, hintSameValues,
		!q || !t || !cam, !Xw, !ep || !el || !edim || !meas || !omega, sizeof(Scalar) };
	hintSameEdges = hintSameValues = false;
	const UploadArrays in{ q, t, cam, Xw, ep, el, edim, meas, omega };
	// ---- plan and refuse: nothing is touched yet, a rejected call must leave the previous graph fully usable ----
	const auto t0 = Clock::now();
	const UploadFacts facts = uploadFacts();
	const UploadPlan plan = planUpload(facts, call, needsEdgeCompare(facts, call) && sameEdgeArrays(in));
	if (plan.refusal) throw ArgError{ plan.refusal };
	if (!plan.sameEdges) validateEdges(call, in);
	// ---- replace ----
	// (a begin without its end: the old upload must not outlive its arrays' replacement.  Below every refusal: a refused call leaves the
	// begun graph in force, and its values still arrive with the next need())
	if (valuesPending) { HIP_TRY(hipStreamSynchronize(upStream)); valuesPending = false; sortedValuesValid = false; }
	// an edge gate (ba_gate.hip) outlives a call whose edge arrays are the previous call's -- promised or found so above --: its mask is kept
	// in the caller's edge order, and need() derives the live information from the newly uploaded one.  Other edges: all active again.
	if (!plan.sameEdges) clearGate();
	clearFactors();           // (they name poses of the previous graph; need() rebuilds a kept structure unless the same pairs come back)
	// from here on the old graph is being replaced: a failure below (allocation, upload) leaves NO graph
	haveGraph = false;
	haveStructure = false;
	covBlocksValid = false;
	Pt = Pt_; Pf = Pf_; Lt = Lt_; Lf = Lf_; E = E_;
	// (before the sort: the internal landmark order is for whole-range handles -- and a whole upload is one, whatever range was in force)
	partLo = call.ranged() ? ownLo : 0; partHi = call.ranged() ? ownHi : -1;
	lap(nullptr);
	const DeviceGraph gOld = g;
	const bool sameTopology = plan.useDev ? sortEdgesDevice(plan, in) : sortEdgesHost(plan, in);
	uploadState(in);
	allocRunBuffers();
	// (enqueued LAST: the copy engine serves its queue in order, and the small uploads of this call must not wait behind 18 MB)
	if (plan.deferValues) enqueueDeferredValues(in);
	sync(); expectedTicket = 0; ((volatile int*)((char*)h_pinned + 1024))[3] = 0;
	sync();   // host staging vectors go out of scope
	lap("set_graph: alloc + upload + sync");
	publishGraph(plan, gOld, sameTopology);
	prof[0] += std::chrono::duration<double>(Clock::now() - t0).count();
}

// ---- device path: raw arrays go up as they are; sort, gather and the landmark pointers are kernels.  Returns: the structure stays. ----
bool cuba_hip_solver::sortEdgesDevice(const UploadPlan& plan, const UploadArrays& in)
{
	const bool ranged = partHi >= 0;
	if (!plan.keepPoseOrder) resetPoseOrder();
	if (!plan.reuseSort)
	{
		if (!plan.sameEdges) { h_inEp.assign(in.ep, in.ep + E); h_inEl.assign(in.el, in.el + E); h_inDim.assign(in.edim, in.edim + E); }
		d_rawEpCaller.uploadRaw(in.ep, E, stream); d_rawElCaller.uploadRaw(in.el, E, stream); d_rawDim.uploadRaw(in.edim, E, stream);
		d_rawEp.resize(E);
		HIP_TRY(hipMemcpyAsync(d_rawEp.data(), d_rawEpCaller.data(), sizeof(int) * (size_t)E, hipMemcpyDeviceToDevice, stream));
		// internal landmark order from the pose numbering in force (the caller's here; applyPoseOrder renews it under a new one)
		if (plan.lmOrderWanted) computeLandmarkOrder(); else resetLandmarkOrder();
	}
	if (plan.deferValues) { d_rawMeas.resize((size_t)3 * E); d_rawOmega.resize(E); }
	else if (ranged)
	{
		// the values of the rank's own edges only: ids + {u, v, r, omega} packed by the host, spread into the caller-order arrays by a kernel
		// (the other edges' slots read as zeros; no kernel of a partitioned handle looks at them)
		const int32_t* el = in.el; const double* meas = in.meas; const double* omega = in.omega;
		const int ownLo = partLo, ownHi = partHi;
		h_ownIds.clear();
		for (int e = 0; e < E; e++) if (el[e] >= ownLo && el[e] < ownHi) h_ownIds.push_back(e);
		const int n = (int)h_ownIds.size();
		h_ownVals.resize((size_t)4 * n);
		parallelFor(n, [&](int i) {
			const size_t e = (size_t)h_ownIds[i];
			h_ownVals[4 * (size_t)i] = meas[3 * e]; h_ownVals[4 * (size_t)i + 1] = meas[3 * e + 1]; h_ownVals[4 * (size_t)i + 2] = meas[3 * e + 2];
			h_ownVals[4 * (size_t)i + 3] = omega[e];
		});
		d_ownIds.upload(h_ownIds, stream); d_ownVals.upload(h_ownVals, stream);
		d_rawMeas.resize((size_t)3 * E); d_rawOmega.resize(E);
		d_rawMeas.zero(stream); d_rawOmega.zero(stream);
		topo::launch_scatter_values(d_ownIds.data(), d_ownVals.data(), n, d_rawMeas.data(), d_rawOmega.data(), stream);
		cntValueBytes += (int64_t)n * 36;
	}
	else if (!plan.keepValues) { d_rawMeas.uploadRaw(in.meas, (size_t)3 * E, stream); d_rawOmega.uploadRaw(in.omega, E, stream); cntValueBytes += (int64_t)E * 32; }
	lap("set_graph: raw uploads enqueued");
	if (!plan.keepValues) sortedValuesValid = false;
	if (!plan.reuseSort) runDeviceEdgeSort(!plan.deferValues);
	else if (!plan.keepValues && !plan.deferValues) gatherSortedValues();
	if (plan.deferValues) { sizeSortedValues(); valuesPending = true; }      // (finishValues gathers them and marks them valid)
	devTopology = true; hostTopoValid = false;
	lap("set_graph: device sort + gather enqueued");
	return plan.mayKeepStructure && plan.reuseSort;
}

// ---- host path (the independent cross-check pipeline, and graphs without edges): sort and gather here, upload the sorted arrays.  Runs
// in the caller's pose and landmark order.  Returns: the structure stays. ----
bool cuba_hip_solver::sortEdgesHost(const UploadPlan& plan, const UploadArrays& in)
{
	const int32_t* ep = in.ep; const int32_t* el = in.el; const uint8_t* edim = in.edim; const double* meas = in.meas; const double* omega = in.omega;
	const bool reuse = plan.reuseHostSort;
	resetPoseOrder();
	lmOrderActive = false;          // (uploadState leaves the landmark rows as the caller numbers them)
	if (!reuse)
	{
		h_inEp.assign(ep, ep + E); h_inEl.assign(el, el + E); h_inDim.assign(edim, edim + E);
		// sort edges by (landmark, pose, original index): counting sort on the landmark, small sorts inside
		cntEdgeSorts++;
		h_lmptr.assign(Lt + 1, 0);
		for (int e = 0; e < E; e++) h_lmptr[el[e] + 1]++;
		for (int l = 0; l < Lt; l++) h_lmptr[l + 1] += h_lmptr[l];
		perm.assign(E, 0);
		std::vector<int> cursor(h_lmptr.begin(), h_lmptr.end() - 1);
		for (int e = 0; e < E; e++) perm[cursor[el[e]]++] = e;
		std::vector<long long> byEdges(h_lmptr.begin(), h_lmptr.end());    // balance the small sorts by edge count
		parallelRows(Lt, byEdges, [&](int l) {
			std::sort(perm.begin() + h_lmptr[l], perm.begin() + h_lmptr[l + 1],
				[&](int a, int b) { return ep[a] != ep[b] ? ep[a] < ep[b] : a < b; });
		});
	}
	lap("set_graph: validate + sort edges");
	std::vector<int>& sPose = h_spose[reuse ? topoSlot : topoSlot ^ 1];   // the previous call's sorted index arrays stay in the other slot
	std::vector<int>& sLm = h_slm[reuse ? topoSlot : topoSlot ^ 1];
	sPose.resize(E); sLm.resize(E);
	// staging buffers are members: a second set_graph of similar size touches no fresh pages
	std::vector<Scalar>&mu = h_stage[0], &mv = h_stage[1], &mr = h_stage[2], &w = h_stage[3];
	mu.resize(E); mv.resize(E); mr.resize(E); w.resize(E);
	h_epose.resize(E);
	parallelFor(E, [&](int i) {       // random gather through the sort permutation
		const int e = perm[i];
		if (!reuse)
		{
			h_epose[i] = ep[e];
			sPose[i] = ep[e] | (edim[e] == 3 ? STEREO_BIT : 0);
			sLm[i] = el[e];
		}
		mu[i] = meas[3 * (size_t)e]; mv[i] = meas[3 * (size_t)e + 1];
		mr[i] = edim[e] == 3 ? meas[3 * (size_t)e + 2] : 0.0;
		w[i] = omega[e];
	});
	// Same vertices, same edges (in sorted order, same types) as last time: everything build_structure() derives from
	// the topology is still valid on the device -- only the values are new (the samples' warm-up + timed protocol,
	// repeated optimisation of one window).  Decided by comparing the sorted index arrays, 8 bytes per edge.
	const bool sameTopology = plan.mayKeepStructure && hostTopoValid && (reuse || (sPose == h_spose[topoSlot] && sLm == h_slm[topoSlot]));
	if (!reuse) topoSlot ^= 1;
	lap("set_graph: gather sorted arrays");
	if (!reuse || devTopology) { d_epose.upload(sPose, stream); d_elm.upload(sLm, stream); d_lmptr.upload(h_lmptr, stream); }
	d_mu.upload(mu, stream); d_mv.upload(mv, stream); d_mr.upload(mr, stream); d_w.upload(w, stream);
	cntValueBytes += (int64_t)E * 4 * (int64_t)sizeof(Scalar);
	devTopology = false; hostTopoValid = true;
	return sameTopology;
}

// the estimates and cameras go up straight from the caller's arrays when they need neither a conversion (fp64 build) nor a
// row permutation (internal pose order): no staging copy, and page-locked caller memory (cuba_hip_host_alloc) moves by DMA
void cuba_hip_solver::uploadState(const UploadArrays& in)
{
	const size_t nState = (size_t)7 * Pt + (size_t)3 * Lt;
	if (sizeof(Scalar) == sizeof(double) && !reorderActive)
	{
		d_state.resize(nState); d_cam.resize((size_t)5 * Pt);
		Scalar* ds = d_state.data();
		if (Pt)
		{
			HIP_TRY(hipMemcpyAsync(ds, in.q, sizeof(double) * 4 * (size_t)Pt, hipMemcpyHostToDevice, stream));
			HIP_TRY(hipMemcpyAsync(ds + 4 * (size_t)Pt, in.t, sizeof(double) * 3 * (size_t)Pt, hipMemcpyHostToDevice, stream));
			HIP_TRY(hipMemcpyAsync(d_cam.data(), in.cam, sizeof(double) * 5 * (size_t)Pt, hipMemcpyHostToDevice, stream));
		}
		if (Lt) HIP_TRY(hipMemcpyAsync(ds + 7 * (size_t)Pt, in.Xw, sizeof(double) * 3 * (size_t)Lt, hipMemcpyHostToDevice, stream));
	}
	else
	{
		std::vector<Scalar>&state = h_stage[4], &camv = h_stage[5];
		state.resize(nState);
		for (size_t i = 0; i < (size_t)4 * Pt; i++) state[i] = (Scalar)in.q[i];
		for (size_t i = 0; i < (size_t)3 * Pt; i++) state[4 * (size_t)Pt + i] = (Scalar)in.t[i];
		for (size_t i = 0; i < (size_t)3 * Lt; i++) state[7 * (size_t)Pt + i] = (Scalar)in.Xw[i];
		camv.assign(in.cam, in.cam + 5 * (size_t)Pt);
		permuteStateRows(state, camv);          // the caller's rows -> the internal pose order kept from the last call (none: as they are)
		d_state.upload(state, stream);
		d_cam.upload(camv, stream);
	}
	if (lmOrderActive) landmarkRowsInPlace(d_state.data() + 7 * (size_t)Pt, Lt, 3, true);
}

void cuba_hip_solver::allocRunBuffers()
{
	d_backup.resize((size_t)7 * Pt + (size_t)3 * Lt);
	dropSnapshots();
	d_perEdge.resize(E);
	if (!h_pinned)
	{
		// Coherent (fine-grained) mapping: the spin-wait protocol below reads device-written results without a stream
		// synchronisation, which is only defined for coherent host memory (HIP_HOST_COHERENT defaults to 0).
		HIP_TRY(hipHostMalloc((void**)&h_pinned, 4096, hipHostMallocMapped | hipHostMallocCoherent));
		std::memset(h_pinned, 0, 4096);
		void* dev = nullptr;
		HIP_TRY(hipHostGetDevicePointer(&dev, h_pinned, 0));
		slotsDev = (Scalar*)dev; flagsDev = (int*)((char*)dev + 1024);
	}
	d_parts.resize(8192 + (size_t)E + 64); d_maxdiag.resize(64); d_fail.resize(1); d_iters.resize(1); d_kbase.resize(1); d_done.resize(1); d_ticket.resize(1);
	d_fail.zero(stream); d_iters.zero(stream); d_kbase.zero(stream); d_done.zero(stream); d_ticket.zero(stream);
}

// deferValues (cuba_hip_set_graph_begin): meas / omega, 32 bytes per edge, cross on the second stream while the structure analysis runs
void cuba_hip_solver::enqueueDeferredValues(const UploadArrays& in)
{
	if (!upStream) { HIP_TRY(hipStreamCreateWithFlags(&upStream, hipStreamNonBlocking)); HIP_TRY(hipEventCreateWithFlags(&evValues, hipEventDisableTiming)); }
	// (the raw buffers may still be read by a gather of the previous call on the work stream)
	HIP_TRY(hipEventRecord(evValues, stream)); HIP_TRY(hipStreamWaitEvent(upStream, evValues, 0));
	HIP_TRY(hipMemcpyAsync(d_rawMeas.data(), in.meas, sizeof(double) * 3 * (size_t)E, hipMemcpyHostToDevice, upStream));
	HIP_TRY(hipMemcpyAsync(d_rawOmega.data(), in.omega, sizeof(double) * (size_t)E, hipMemcpyHostToDevice, upStream));
	HIP_TRY(hipEventRecord(evValues, upStream));
	cntValueBytes += (int64_t)E * 32;
}

void cuba_hip_solver::publishGraph(const UploadPlan& plan, const DeviceGraph& gOld, bool sameTopology)
{
	g = DeviceGraph();
	g.Pt = Pt; g.Pf = Pf; g.Lt = Lt; g.Lf = Lf; g.E = E;
	g.q = d_state.data(); g.t = d_state.data() + 4 * (size_t)Pt; g.Xw = d_state.data() + 7 * (size_t)Pt;
	g.cam = d_cam.data();
	g.e_pose = d_epose.data(); g.e_lm = d_elm.data(); g.lm_ptr = d_lmptr.data();
	g.e_mu = d_mu.data(); g.e_mv = d_mv.data(); g.e_mr = d_mr.data(); g.e_w = liveInformation();
	g.rk[0] = rk[0]; g.rk[1] = rk[1];
	g.e_begin = 0; g.e_end = E;
	valuesPartial = partHi >= 0 && plan.useDev;          // (a ranged upload; the host pipeline reads the whole arrays)
	if (sameTopology)
	{
		// the captured PCG graphs carry the DeviceGraph by value: they stay usable only if no buffer moved
		DeviceGraph a = gOld, b = g;
		a.rk[0] = a.rk[1] = b.rk[0] = b.rk[1] = RobustKernel();
		if (std::memcmp(&a, &b, sizeof(DeviceGraph)) != 0) dropPcgGraph();
		haveStructure = true;
	}
	coarseValid = false; startRunHistory();
	haveGraph = true;
	lambda = 0;
	for (double& v : prof) v = 0;
	cntPcgIters = cntTrials = cntCoarseRefresh = cntPcgLooks = cntPcgEnqueued = cntPcgUnconverged = 0;
	cntCoarseInline = cntFp32Fallbacks = 0;
	cntBatchFullTrials = cntBatchIterTrials = 0;
	pcgHistory.clear();
	cntUploads++;
	valuesStamp++;          // (the permutation or the sorted values are new: an edge gate derives its copies again, refreshGate)
}

void cuba_hip_solver::buildStructure()
{
	if (!haveGraph) throw StateError{ "set_graph must be called first" };
	if (haveStructure) return;
	if (gjStream) { HIP_TRY(hipStreamSynchronize(gjStream)); pendingInv = -1; assemblePending = false; }   // an overlapped coarse inversion uses the old structure
	if (devTopology && deviceSetup) { buildStructureDevice(); return; }      // (landmark partitions included)
	localRanges = false;
	if (reorderActive) { std::vector<int> id(Pf); for (int i = 0; i < Pf; i++) id[i] = i; applyPoseOrder(id); }   // the host pipeline runs in the caller's order
	ensureHostTopology();
	const auto t0 = Clock::now();
	std::vector<int> nfree(Lf, 0);
	std::vector<long long> pairBase(Lf, 0);
	nmul = 0;
	long long npairs = 0;
	parallelFor(Lf, [&](int l) {
		int n = 0;
		for (int i = h_lmptr[l]; i < h_lmptr[l + 1]; i++) n += h_epose[i] < Pf;   // edges are sorted by pose: the free ones come first
		nfree[l] = n;
	});
	for (int l = 0; l < Lf; l++)
	{
		const int n = nfree[l];
		pairBase[l] = npairs;
		npairs += (long long)n * (n - 1) / 2;
		nmul += (long long)n * (n + 1) / 2;
	}
	if (npairs >= (1LL << 31)) throw ArgError{ "graph too dense: more than 2^31 Schur block products" };
	lap(nullptr);
	// Pattern of Hsc + product lists: bucket the (column, product id) pairs by block row, sort every row on its own
	// (cache resident, rows spread over host threads), then walk the sorted rows: a new column opens a new block,
	// and the products of a block are the consecutive entries with its column, already in landmark order (product
	// ids grow with the landmark index) -- the fixed summation order that makes the results reproducible.
	// per free pose: its edges (sorted-edge ids, ascending = landmark order), over the whole graph
	std::vector<int> peAllPtr(Pf + 1, 0);
	std::vector<int>& peAll = h_work[5];
	{
		// counting sort by pose, split over contiguous edge ranges: per-range histograms, offsets in (pose, range)
		// order, then every range scatters its own edges -- the lists stay in ascending edge order
		const int T = (int)std::min<long long>(HostPool::instance().maxThreads(), E / 50000 + 1);
		std::vector<int> hist((size_t)T * Pf, 0);
		auto range = [&](int t) { return std::make_pair((int)((long long)E * t / T), (int)((long long)E * (t + 1) / T)); };
		HostPool::instance().run(T, [&](int t) {
			int* h = hist.data() + (size_t)t * Pf;
			for (int i = range(t).first; i < range(t).second; i++) if (h_epose[i] < Pf) h[h_epose[i]]++;
		});
		int run = 0;
		for (int ps = 0; ps < Pf; ps++)
		{
			peAllPtr[ps] = run;
			for (int t = 0; t < T; t++) { const int c = hist[(size_t)t * Pf + ps]; hist[(size_t)t * Pf + ps] = run; run += c; }
		}
		peAllPtr[Pf] = run;
		peAll.resize(run);
		HostPool::instance().run(T, [&](int t) {
			int* cur = hist.data() + (size_t)t * Pf;
			for (int i = range(t).first; i < range(t).second; i++) if (h_epose[i] < Pf) peAll[cur[h_epose[i]]++] = i;
		});
	}
	lap("structure:   nfree + pose lists");
	const std::vector<int>& slm = h_slm[topoSlot];          // sorted edge -> landmark (set_graph)
	std::vector<long long> peWeight(peAllPtr.begin(), peAllPtr.end());
	// row i of the pattern collects, for every landmark pose i sees, the poses after it in that landmark's edge list:
	// each row is produced by one thread into its own segment (no atomics)
	// (the pose pairs of the relative-pose edges: off-diagonal seeds, sorted by (row, column))
	h_relSeeds = relSeedKeys();
	std::vector<int> relRowPtr(Pf + 1, 0);
	for (uint64_t k : h_relSeeds) relRowPtr[(size_t)(k >> 32) + 1]++;
	for (int i = 0; i < Pf; i++) relRowPtr[i + 1] += relRowPtr[i];
	std::vector<long long> rowStart(Pf + 1, 0);
	{
		std::vector<long long> cnt(Pf, 1);                   // the diagonal block always exists
		parallelRows(Pf, peWeight, [&](int i) {
			long long c = 1 + (relRowPtr[i + 1] - relRowPtr[i]);
			for (int x = peAllPtr[i]; x < peAllPtr[i + 1]; x++)
			{
				const int e = peAll[x], l = slm[e];
				if (l < Lf) c += nfree[l] - 1 - (e - h_lmptr[l]);
			}
			cnt[i] = c;
		});
		for (int i = 0; i < Pf; i++) rowStart[i + 1] = rowStart[i] + cnt[i];
	}
	lap("structure:   count per row");
	// (the large work arrays are members: rebuilding for the next graph touches no fresh pages)
	// an entry carries its two (sorted) edges along: every pass below streams through memory, nothing is looked up
	// by product id (a product -> edges table is written once per landmark by several rows: cache-line ping-pong)
	std::vector<PatternEntry>& ent = h_ent; ent.resize((size_t)rowStart[Pf]);
	parallelRows(Pf, rowStart, [&](int i) {
		long long slot = rowStart[i];
		ent[slot++] = PatternEntry{ (uint64_t)i << 32, -1, -1 };                    // id 0 = diagonal seed, sorts first
		for (int x = relRowPtr[i]; x < relRowPtr[i + 1]; x++) ent[slot++] = PatternEntry{ (uint64_t)(uint32_t)h_relSeeds[x] << 32, -1, -1 };
		for (int x = peAllPtr[i]; x < peAllPtr[i + 1]; x++)
		{
			const int e = peAll[x], l = slm[e];
			if (l >= Lf) continue;
			const int b0 = h_lmptr[l], n = nfree[l], a2 = e - b0;
			long long idx = pairBase[l] + (long long)a2 * (n - 1) - (long long)a2 * (a2 - 1) / 2;   // id of product (a2, a2 + 1)
			for (int c = a2 + 1; c < n; c++, idx++, slot++)
			{
				ent[slot] = PatternEntry{ ((uint64_t)h_epose[b0 + c] << 32) | (uint64_t)(idx + 1), e, b0 + c };
			}
		}
	});
	lap("structure:   bucket fill");
	// landmark partition (multi-GPU): the PATTERN is global, the product lists cover the landmarks [lo, hi) only --
	// product ids are in landmark order, so that is an id range
	const int lo = std::max(0, partLo), hi = partHi < 0 ? Lt : std::min(Lt, partHi);
	const long long idLo = std::min(lo, Lf) < Lf ? pairBase[std::min(lo, Lf)] : npairs;
	const long long idHi = std::min(hi, Lf) < Lf ? pairBase[std::min(hi, Lf)] : npairs;
	std::vector<int> rowBlocks(Pf, 0);
	std::vector<long long> rowProducts(Pf + 1, 0);
	parallelRows(Pf, rowStart, [&](int i) {
		PatternEntry* e0 = ent.data() + rowStart[i]; PatternEntry* e1 = ent.data() + rowStart[i + 1];
		{
			// order by (column, product id).  The entries were produced in product-id order, so a STABLE counting sort
			// on the column does it in O(n + columns spanned); rows that span far more columns than they have
			// entries (loop closures) fall back to a comparison sort
			const size_t nEnt = (size_t)(e1 - e0);
			uint32_t cmax = (uint32_t)i;
			for (PatternEntry* e = e0; e < e1; e++) cmax = std::max(cmax, (uint32_t)(e->key >> 32));
			const size_t span = (size_t)cmax - (size_t)i + 1;          // columns of an upper-triangular row start at the row
			if (span <= 8 * nEnt + 64)
			{
				thread_local std::vector<PatternEntry> tmp;
				thread_local std::vector<int> cnt;
				tmp.assign(e0, e1);
				cnt.assign(span + 1, 0);
				for (const PatternEntry& x : tmp) cnt[(size_t)(x.key >> 32) - i + 1]++;
				for (size_t c = 0; c < span; c++) cnt[c + 1] += cnt[c];
				for (const PatternEntry& x : tmp) e0[cnt[(size_t)(x.key >> 32) - i]++] = x;
			}
			else std::sort(e0, e1, [](const PatternEntry& x, const PatternEntry& y) { return x.key < y.key; });
		}
		int u = 0; uint32_t last = 0xffffffffu; long long np = 0;
		for (PatternEntry* e = e0; e < e1; e++)
		{
			const uint32_t c = (uint32_t)(e->key >> 32); u += c != last; last = c;
			const long long id = (long long)(uint32_t)e->key - 1;
			np += id >= idLo && id < idHi;
		}
		rowBlocks[i] = u; rowProducts[i + 1] = np;
	});
	lap("structure:   row sorts");
	h_rowptr.assign(Pf + 1, 0);
	for (int i = 0; i < Pf; i++) { h_rowptr[i + 1] = h_rowptr[i] + rowBlocks[i]; rowProducts[i + 1] += rowProducts[i]; }
	const int nblk = h_rowptr[Pf];
	const long long nprodLocal = rowProducts[Pf];
	h_colind.assign(nblk, 0);
	std::vector<int> blkRow(nblk), prodPtr(nblk + 1, 0), odBlocks;
	std::vector<int>&prodEa = h_work[2], &prodEb = h_work[3];
	prodEa.resize((size_t)nprodLocal); prodEb.resize((size_t)nprodLocal);
	parallelRows(Pf, rowStart, [&](int i) {
		int k = h_rowptr[i] - 1; uint32_t last = 0xffffffffu;
		long long out = rowProducts[i];
		for (long long x = rowStart[i]; x < rowStart[i + 1]; x++)
		{
			const uint32_t c = (uint32_t)(ent[x].key >> 32); const uint32_t id = (uint32_t)ent[x].key;
			if (c != last) { k++; h_colind[k] = (int)c; blkRow[k] = i; prodPtr[k] = (int)out; last = c; }
			if (!id) continue;
			if ((long long)id - 1 >= idLo && (long long)id - 1 < idHi) { prodEa[out] = ent[x].ea; prodEb[out] = ent[x].eb; out++; }
		}
	});
	prodPtr[nblk] = (int)nprodLocal;
	lap("structure: Hsc pattern + product blocks");
	// symmetric adjacency over the upper storage
	std::vector<int> adjPtr(Pf + 1, 0);
	for (int i = 0; i < Pf; i++)
		for (int k = h_rowptr[i]; k < h_rowptr[i + 1]; k++)
		{
			adjPtr[i + 1]++;
			if (h_colind[k] != i) adjPtr[h_colind[k] + 1]++;
		}
	for (int i = 0; i < Pf; i++) adjPtr[i + 1] += adjPtr[i];
	std::vector<int> adjBlk(adjPtr[Pf]), adjCol(adjPtr[Pf]);
	{
		std::vector<int> cur(adjPtr.begin(), adjPtr.end() - 1);
		// lower part first (neighbours j < i arrive in increasing j), then the row's own upper part
		for (int i = 0; i < Pf; i++)
			for (int k = h_rowptr[i]; k < h_rowptr[i + 1]; k++)
			{
				const int j = h_colind[k];
				if (j != i) { adjBlk[cur[j]] = k | (int)0x80000000; adjCol[cur[j]] = i; cur[j]++; }
			}
		for (int i = 0; i < Pf; i++)
			for (int k = h_rowptr[i]; k < h_rowptr[i + 1]; k++) { adjBlk[cur[i]] = k; adjCol[cur[i]] = h_colind[k]; cur[i]++; }
	}
	lap("structure: adjacency");
	g.e_begin = h_lmptr[lo]; g.e_end = h_lmptr[hi];
	// blocks with products, longest lists first (the block pass takes them in this order)
	{
		int maxCnt = 0;
		for (int k = 0; k < nblk; k++) maxCnt = std::max(maxCnt, prodPtr[k + 1] - prodPtr[k]);
		std::vector<int> start(maxCnt + 2, 0);                 // stable counting sort by descending list length
		for (int k = 0; k < nblk; k++) { const int c = prodPtr[k + 1] - prodPtr[k]; if (c > 0) start[maxCnt - c + 1]++; }
		for (int c = 0; c <= maxCnt; c++) start[c + 1] += start[c];
		odBlocks.resize(start[maxCnt + 1]);
		for (int k = 0; k < nblk; k++) { const int c = prodPtr[k + 1] - prodPtr[k]; if (c > 0) odBlocks[start[maxCnt - c]++] = k; }
		// (plain row order was measured slower: 174 vs 135 us at KITTI-00 -- the long lists must start first; an XCD-aware order cut the
		// HBM-side fetch 2-3 x and bought nothing: the pass is latency-bound, profiles/r03j_block_order.txt)
		if (rowGroupedBlocks(nprodLocal))
		{
			std::vector<int> cntOf(nblk);
			for (int k = 0; k < nblk; k++) cntOf[k] = prodPtr[k + 1] - prodPtr[k];
			odBlocks = rowGroupedOrder(blkRow.data(), h_colind.data(), cntOf.data(), nblk);
		}
	}
	lap("structure: product lists");
	// per free pose: its edges inside this handle's landmark range (a contiguous run of the global list)
	std::vector<int> pePtr(Pf + 1, 0), peEdge;
	const bool wholeGraph = g.e_begin == 0 && g.e_end == E;      // then the global lists are the lists (no copy)
	if (!wholeGraph)
	{
		for (int i = g.e_begin; i < g.e_end; i++) if (h_epose[i] < Pf) pePtr[h_epose[i] + 1]++;
		for (int i = 0; i < Pf; i++) pePtr[i + 1] += pePtr[i];
		peEdge.resize(pePtr[Pf]);
		std::vector<int> cur(pePtr.begin(), pePtr.end() - 1);
		for (int i = g.e_begin; i < g.e_end; i++) if (h_epose[i] < Pf) peEdge[cur[h_epose[i]]++] = i;
	}
	lap("structure: pose edge lists");
	// wave work list: whole landmarks, at most 64 edges per wave; larger landmarks get a workgroup each
	std::vector<int> waveLm, bigLm;
	{
		int start = -1, cnt = 0;
		auto flush = [&](int end) { if (start >= 0 && cnt > 0) { waveLm.push_back(start); waveLm.push_back(end); } start = -1; cnt = 0; };
		for (int l = lo; l < hi; l++)
		{
			// (the device pipeline packs chunks of WAVE_CHUNK landmarks independently: the same cuts here, so that both
			// pipelines produce the same waves -- the per-wave partial sums of the fused trial tail depend on them)
			if ((l - lo) % topo::WAVE_CHUNK == 0) flush(l);
			const int n = h_lmptr[l + 1] - h_lmptr[l];
			if (n > WAVE)
			{
				flush(l);
				bigLm.push_back(l);
				continue;
			}
			if (n == 0) continue;   // empty landmarks inside a run are harmless (no lanes)
			if (start >= 0 && cnt + n > WAVE) flush(l);
			if (start < 0) start = l;
			cnt += n;
		}
		flush(hi);
	}

	lap("structure: wave list");
	d_waveLm.upload(waveLm, stream); d_bigLm.upload(bigLm, stream);
	d_rowptr.upload(h_rowptr, stream); d_colind.upload(h_colind, stream);
	d_adjPtr.upload(adjPtr, stream); d_adjBlk.upload(adjBlk, stream); d_adjCol.upload(adjCol, stream);
	int ellM = 0, ellOver = 0;
	{
		int maxRow = 0;
		for (int i = 0; i < Pf; i++) maxRow = std::max(maxRow, adjPtr[i + 1] - adjPtr[i]);
		const int M = std::min(3, (maxRow + 19) / 20);
		ellM = M; ellOver = maxRow > 20 * M;
		std::vector<int2> ell((size_t)Pf * M * 20, int2{ 0, -1 });
		for (int i = 0; i < Pf; i++)
		{
			const int n = std::min(adjPtr[i + 1] - adjPtr[i], 20 * M);
			for (int e = 0; e < n; e++) ell[(size_t)i * M * 20 + e] = int2{ adjBlk[adjPtr[i] + e], adjCol[adjPtr[i] + e] };
		}
		d_ell.upload(ell, stream);
	}
	d_blkrow.upload(blkRow, stream); d_odBlocks.upload(odBlocks, stream); d_prodPtr.upload(prodPtr, stream);
	d_prodEa.upload(prodEa, stream); d_prodEb.upload(prodEb, stream); d_pePtr.upload(wholeGraph ? peAllPtr : pePtr, stream); d_peEdge.upload(wholeGraph ? peAll : peEdge, stream);
	const CoarseCfg cc = coarseConfig();
	allocSystem(nblk, cc);
	const int agg = cc.agg, cl = cc.cl, nc = cc.nc;
	lap("structure: uploads + allocs");
	// coarse-matrix assembly lists: fine blocks grouped by the coarse block (I,J) they fall into (both triangles)
	std::vector<int> cbI, cbJ, cbPtr(1, 0), cbBlk, adjRow(adjBlk.size());
	std::vector<Scalar> cbWi, cbWj;
	auto weight = [&](int pose) {     // same formula as agg_weight() on the device
		if (pose == Pf - 1 && Pf % agg == 1) return Scalar(0);
		return Scalar(2 * (pose % agg) + 1 - agg) / Scalar(agg);
	};
	for (int i = 0; i < Pf; i++) for (int a = adjPtr[i]; a < adjPtr[i + 1]; a++) adjRow[a] = i;
	if (nc > 0)
	{
		std::vector<uint64_t> ck; ck.reserve(adjBlk.size());
		for (int i = 0; i < Pf; i++)
			for (int a = adjPtr[i]; a < adjPtr[i + 1]; a++)
				ck.push_back(((uint64_t)((size_t)(i / agg) * nc + adjCol[a] / agg) << 32) | (uint32_t)a);
		std::sort(ck.begin(), ck.end());
		for (size_t x = 0; x < ck.size(); x++)
		{
			const int cbid = (int)(ck[x] >> 32);
			if (x == 0 || cbid != (int)(ck[x - 1] >> 32))
			{
				if (x) cbPtr.push_back((int)cbBlk.size());
				cbI.push_back(cbid / nc); cbJ.push_back(cbid % nc);
			}
			cbBlk.push_back(adjBlk[(uint32_t)ck[x]]);
			if (cl == 2) { cbWi.push_back(weight(adjRow[(uint32_t)ck[x]])); cbWj.push_back(weight(adjCol[(uint32_t)ck[x]])); }
		}
		cbPtr.push_back((int)cbBlk.size());
	}
	d_cbI.upload(cbI, stream); d_cbJ.upload(cbJ, stream); d_cbPtr.upload(cbPtr, stream); d_cbBlk.upload(cbBlk, stream); d_cbWi.upload(cbWi, stream); d_cbWj.upload(cbWj, stream);
	sync();
	lap("structure: coarse lists + sync");
	diagProdBlocks = 0; for (int k : odBlocks) diagProdBlocks += k >= 0 && blkRow[k] == h_colind[k];
	heavyBlocks = 0;        // (the plain list is sorted by length; the tile-grouped one is not: all blocks then take the 16-lane path)
	if (!rowGroupedBlocks(nprodLocal))
		for (int k : odBlocks) heavyBlocks += prodPtr[k + 1] - prodPtr[k] > BP_HEAVY;
	publishStructure(nblk, (int)waveLm.size() / 2, (int)bigLm.size(), (int)odBlocks.size(), (int)cbI.size(), ellM, ellOver, cc);
	hostPatternValid = true;
	const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
	prof[1] += 0.5 * dt; prof[5] += 0.5 * dt;   // pattern of Hsc doubles as the "symbolic" phase of the reduced solver
}

cuba_hip_solver::CoarseCfg cuba_hip_solver::coarseConfig() const
{
	int agg = pcgAggregate;
	const int cl = coarseLinear ? 2 : 1;
	// automatic size: coarse dimension <= ~700-960 (scripts/experiments/agg_sweep.py: iterations vs the O(Nc^3) inversion)
	// (small graphs want smaller aggregates: KITTI-07, 247 free poses: 24 / 16 / 12 / 8 / 6 / 4 poses -> 8.6 / 7.0 / 6.4 / 6.3 / 6.5 / 7.9 ms)
	// (round 4, fp32-stored inverse + unrolled pivot chain: KITTI-07 10 / 8 / 6 / 4 poses -> 4.00 / 3.65 / 3.39 / 4.30 ms, 250 / 212 / 195 / 238 iterations:
	// the floor of the small-graph rule went from 8 to 6, profiles/r04m_sweeps.txt)
	// (large graphs, inversion hidden under the PCG of earlier trials: S2M 44 / 40 / 36 / 32 poses -> 27.1 / 26.35 / 26.7 / 26.4 ms,
	// G4M 88 / 72 / 64 / 56 / 48 -> 65.1 / 59.6 / 54.8 / 54.0 / 58.3 ms: the aggregate count may grow from 115 to 180 with the graph)
	// (round 3, coarse inverse stored in fp32 -- its apply costs half: KITTI-00 24 / 20 / 16 poses -> 8.16 / 8.00 / 7.81 ms, S2M 44 / 40 / 36 /
	// 32 / 28 -> 25.8 / 25.0 / 24.8 / 24.6 / 26.0 ms, G4M 64 / 56 / 48 / 40 -> 51.7 / 50.5 / 52.8 / 58.2 ms: profiles/r03i_agg_sweep.txt)
	const int ncMax = std::min(180, std::max(115, (Pf + 31) / 32));
	if (agg < 0) agg = cl == 2 ? (Pf >= 1320 ? std::max(16, (Pf + ncMax - 1) / ncMax) : std::max(6, (Pf + 27) / 55)) : std::max(12, (Pf + 159) / 160);
	const int spmvRows = spmv_rows_for(Pf);
	if (agg > 0) agg = (agg + spmvRows - 1) / spmvRows * spmvRows;   // aggregates = whole SpMV workgroups (sys.qpart)
	int nc = agg > 0 ? (Pf + agg - 1) / agg : 0;
	// the two-level kernel keeps two coarse vectors in LDS and the dense inverse costs O(Nc^3): a user-chosen aggregate
	// that small for this many poses is widened
	// (round 6: this used to be one loop that doubled the aggregate until BOTH conditions held -- which never happens once the aggregate's
	// own 12 agg numbers exceed the LDS budget (a user-chosen aggregate above ~600 poses, or the automatic one beyond ~47 000 poses): the
	// doubling ran until the integer overflowed and the division below trapped.  Now: the aggregate is capped at 600 poses and widened by
	// doubling only while that helps; failing that, the aggregate size that MINIMISES the footprint (12 (cl Pf / agg + agg) numbers:
	// agg = sqrt(cl Pf)) is tried, first with the configured coarse functions, then with constant ones (half the coarse dimension: good
	// to ~97 000 poses), and only then the preconditioner falls back to block-Jacobi alone -- where the exact solver takes over after
	// the iteration budget anyway.)
	int clOut = cl;
	const int aggMax = 600 / spmvRows * spmvRows;
	auto ncOf = [&](int a) { return (Pf + a - 1) / a; };
	auto fits = [&](int c, int a) { const int n = ncOf(a); return c * n <= 600 && sizeof(Scalar) * (12 * (size_t)c * n + 12 * (size_t)a + 200) <= 60 * 1024; };
	if (agg > aggMax) agg = aggMax;
	if (agg > 0)
	{
		bool ok = false;
		for (int c = cl; c >= 1 && !ok; c--)
		{
			int a = agg;
			while (a < aggMax && !fits(c, a)) a = std::min(aggMax, 2 * a);
			if (!fits(c, a))
			{
				int m = ((int)std::ceil(std::sqrt((double)c * Pf)) + spmvRows - 1) / spmvRows * spmvRows;
				m = std::min(aggMax, std::max(agg, m));
				if (fits(c, m)) a = m;
			}
			if (fits(c, a)) { agg = a; clOut = c; ok = true; }
		}
		if (!ok) agg = 0;
	}
	nc = agg > 0 ? ncOf(agg) : 0;
	if (nc < 2) { agg = 0; nc = 0; }
	return CoarseCfg{ agg, agg > 0 ? clOut : cl, nc, spmvRows };
}

void cuba_hip_solver::allocSystem(int nblk, const CoarseCfg& c)
{
	directRefused = false; directSticky = false; directPlanValid = false;      // (a new structure: the exact solver analyses it afresh at its first use)
	d_red.resize((size_t)36 * nblk + (size_t)12 * Pf);
	d_lmSys.resize((size_t)9 * Lf); d_lmInv.resize((size_t)8 * std::max(Lf, 1)); d_erec.resize((size_t)8 * E); d_xp.resize((size_t)6 * Pf); d_xl.resize((size_t)3 * Lf);
	d_minv.resize((size_t)36 * Pf);
	d_r.resize((size_t)6 * Pf); d_z.resize((size_t)6 * Pf); d_p0.resize((size_t)6 * Pf); d_p1.resize((size_t)6 * Pf); d_ap.resize((size_t)6 * Pf);
	d_red.zero(stream); d_lmSys.zero(stream); d_lmInv.zero(stream); d_xp.zero(stream); d_xl.zero(stream);
	reducedZeroed = true;
	for (auto& b : d_coarse) b.resize((size_t)36 * c.cl * c.cl * c.nc * c.nc);
	{
		const size_t n = (size_t)6 * c.cl * c.nc;
		for (auto& b : d_coarse32) b.resize(fp32Inverse() ? n * ((n + 3) & ~(size_t)3) : 0);
	}
	d_rc.resize((size_t)12 * c.cl * c.nc); d_r2.resize((size_t)6 * Pf);
	maxIterAlloc = pcgMaxIter > 0 ? pcgMaxIter : std::min(32768, std::max(64, 4 * 6 * Pf));
	const int gridSetup = (Pf + PCG_SETUP_POSES - 1) / PCG_SETUP_POSES, gridUpd = (Pf + 39) / 40, gridSpmv = (Pf + c.spmvRows - 1) / c.spmvRows;
	rzStrideCfg = std::max(1, std::max(std::max(gridSetup, gridUpd), c.nc)); pqStrideCfg = std::max(1, gridSpmv);
	d_rz.resize((size_t)5 * rzStrideCfg); d_pq.resize((size_t)4 * pqStrideCfg);
}

std::vector<int> cuba_hip_solver::rowGroupedOrder(const int* blkRow, const int* blkCol, const int* cnt, int nblk) const
{
	// groups are 4 x 4 tiles of the block matrix: a-side records are shared by 4 blocks of a workgroup, b-side records by 4.
	// KITTI-00 linearise + Schur: pieces of one row 102.9 us, 2 x 8 tiles 99.3, 4 x 4 tiles 99.6; S2M 356 / 341.6 / 340.9 us
	// (profiles/r03fin3_block_order_tiles.txt)
	const int tr = 4, tc = 4;
	const long long nColTiles = (Pf + tc - 1) / tc;
	(void)nColTiles;
	// 1. blocks with products grouped by tile, in (tile row, tile column, block id) order, each tile's blocks then by list length
	//    descending (stable).  The blocks come sorted by (row, column) -- BSR order --, so a band of 4 block rows is 4 sorted runs: a
	//    4-way merge on the tile column visits every block once, and a tile holds at most 16 blocks (insertion sort).
	// 2. a tile with all 16 blocks is a whole chunk; the other tiles' blocks, in tile order, are re-chunked (neighbouring tiles share
	//    records too)
	std::vector<int> val; val.reserve(nblk);     // whole chunks, 16 entries each
	std::vector<int> rest; rest.reserve(nblk);
	std::vector<int> chunkStart;                 // chunk c = 16 consecutive entries of `val` from chunkStart[c] (whole chunks) or of `rest` (id - n)
	for (int k0 = 0; k0 < nblk;)
	{
		const int band = blkRow[k0] / tr;
		int head[4], end[4], nr = 0, k = k0;
		while (k < nblk && blkRow[k] / tr == band)
		{
			const int r = blkRow[k], b = k;
			while (k < nblk && blkRow[k] == r) k++;
			head[nr] = b; end[nr] = k; nr++;
		}
		for (;;)
		{
			int ct = 0x7fffffff;
			for (int x = 0; x < nr; x++) if (head[x] < end[x]) ct = std::min(ct, blkCol[head[x]] / tc);
			if (ct == 0x7fffffff) break;
			int tile[16], nt = 0;
			for (int x = 0; x < nr; x++)
				while (head[x] < end[x] && blkCol[head[x]] / tc == ct) { if (cnt[head[x]] > 0) tile[nt++] = head[x]; head[x]++; }
			for (int a2 = 1; a2 < nt; a2++)
			{
				const int v = tile[a2]; int b2 = a2;
				while (b2 > 0 && cnt[tile[b2 - 1]] < cnt[v]) { tile[b2] = tile[b2 - 1]; b2--; }
				tile[b2] = v;
			}
			if (nt == 16) { chunkStart.push_back((int)val.size()); val.insert(val.end(), tile, tile + 16); }
			else rest.insert(rest.end(), tile, tile + nt);
		}
		k0 = k;
	}
	const size_t nWhole = chunkStart.size();
	const size_t n = (size_t)nblk + 1;           // (ids >= n address `rest`)
	for (size_t i = 0; i < rest.size(); i += 16)
	{
		// (a chunk of leftovers: longest list first inside it, ties in the order they came)
		const size_t e = std::min(rest.size(), i + 16);
		for (size_t a2 = i + 1; a2 < e; a2++)
		{
			const int v = rest[a2]; size_t b2 = a2;
			while (b2 > i && cnt[rest[b2 - 1]] < cnt[v]) { rest[b2] = rest[b2 - 1]; b2--; }
			rest[b2] = v;
		}
		chunkStart.push_back((int)(n + i));
	}
	// 3. chunks by their longest list, descending (stable): counting sort over the lengths that occur
	const size_t nChunks = chunkStart.size();
	auto firstOf = [&](size_t c) { return chunkStart[c] < (int)n ? val[chunkStart[c]] : rest[chunkStart[c] - n]; };
	std::vector<std::pair<int, int>> byLen(nChunks);
	for (size_t c = 0; c < nChunks; c++) byLen[c] = std::make_pair(-cnt[firstOf(c)], (int)c);
	std::stable_sort(byLen.begin(), byLen.end(), [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x.first < y.first; });
	std::vector<int> od(nChunks * 16, -1);
	for (size_t o = 0; o < nChunks; o++)
	{
		const size_t c = (size_t)byLen[o].second;
		if (c < nWhole) for (int x = 0; x < 16; x++) od[o * 16 + x] = val[chunkStart[c] + x];
		else
		{
			const size_t b = (size_t)chunkStart[c] - n, e = std::min(rest.size(), b + 16);
			for (size_t x = b; x < e; x++) od[o * 16 + (x - b)] = rest[x];
		}
	}
	return od;
}

void cuba_hip_solver::publishStructure(int nblk, int nWaves, int nBig, int nOd, int nCb, int ellM, int ellOver, const CoarseCfg& c)
{
	const int agg = c.agg, cl = c.cl, nc = c.nc, spmvRows = c.spmvRows;
	const int gridSetup = (Pf + PCG_SETUP_POSES - 1) / PCG_SETUP_POSES, gridUpd = (Pf + 39) / 40, gridSpmv = (Pf + spmvRows - 1) / spmvRows;
	st = DeviceStructure();
	st.nWaves = nWaves; st.wave_lm = d_waveLm.data();
	st.nBig = nBig; st.big_lm = d_bigLm.data();
	st.nblk = nblk; st.hsc_rowptr = d_rowptr.data(); st.hsc_colind = d_colind.data();
	st.adj_ptr = d_adjPtr.data(); st.adj_blk = d_adjBlk.data(); st.adj_col = d_adjCol.data();
	st.ell = d_ell.data(); st.ell_m = ellM; st.ell_over = ellOver;
	st.hsc_blkrow = d_blkrow.data(); st.nOd = nOd; st.nDiagProd = diagProdBlocks; st.od_blocks = d_odBlocks.data(); st.nHeavy = std::min(heavyBlocks, nOd);
	// (whole-wave blocks shorten the longest dependent chain of the block pass: 51 -> 37 us at KITTI-07; on graphs whose pass is bound by its
	// gathers they only add waves: 114 -> 122 us at KITTI-00, 405 -> 411 us at S2M -- profiles/r03z_block_pass_ab.txt)
	if (d_prodEa.size() > ((size_t)1 << 19)) st.nHeavy = 0;
	// (64-byte rows of the landmark inverses: block pass -3 us / landmark pass +5 us at KITTI-00, -16 / +3 us at S2M)
	st.inv_rows8 = Lf >= 250000;
	st.prod_ea = d_prodEa.data(); st.prod_eb = d_prodEb.data();
	if (!localRanges) fillProdLm();          // (a device-built partition needed it earlier)
	st.prod_lm = d_prodLm.data();
	st.prod_beg = localRanges ? d_prodBeg.data() : d_prodPtr.data(); st.prod_end = localRanges ? d_prodEnd.data() : d_prodPtr.data() + 1;
	st.pe_beg = localRanges ? d_peBeg.data() : d_pePtr.data(); st.pe_end = localRanges ? d_peEnd.data() : d_pePtr.data() + 1;
	st.pe_edge = d_peEdge.data(); st.e_rec = d_erec.data();
	st.nCb = nCb; st.cb_I = d_cbI.data(); st.cb_J = d_cbJ.data(); st.cb_ptr = d_cbPtr.data(); st.cb_blk = d_cbBlk.data(); st.cb_wi = d_cbWi.data(); st.cb_wj = d_cbWj.data();
	sys = DeviceSystem();
	sys.hsc = d_red.data(); sys.bsc = d_red.data() + (size_t)36 * nblk; sys.bp = sys.bsc + (size_t)6 * Pf;
	sys.lm_sys = d_lmSys.data(); sys.lm_inv = d_lmInv.data(); sys.xp = d_xp.data(); sys.xl = d_xl.data(); sys.slots = slotsDev; sys.host_flags = flagsDev; sys.parts = d_parts.data();
	sys.maxdiag = d_maxdiag.data(); sys.fail = d_fail.data();
	sys.minv = d_minv.data(); sys.r = d_r.data(); sys.z = d_z.data(); sys.p0 = d_p0.data(); sys.p1 = d_p1.data(); sys.ap = d_ap.data();
	sys.rz = d_rz.data(); sys.pq = d_pq.data(); sys.iters = d_iters.data(); sys.kbase = d_kbase.data(); sys.ticket = d_ticket.data();
	dropPcgGraph();
	firstInvValid = false; firstInvPending = false; prevRunIters.clear();
	sys.rzStride = rzStrideCfg; sys.pqStride = pqStrideCfg; sys.npq = gridSpmv;
	sys.nrz0 = agg > 0 ? nc : gridSetup; sys.nrz = agg > 0 ? nc : gridUpd; sys.done = d_done.data();
	coarseValid = false;
	d_qpart.resize(agg > 0 ? (size_t)(agg / spmvRows) * 6 * cl * nc : 1); d_gjPivots.resize(2 * 32 * 32); sys.gj_pivots = d_gjPivots.data();
	sys.qpart = d_qpart.data();   // [workgroup within its aggregate][coarse unknown]
	d_qpart.zero(stream);        // sets of SpMV workgroups the last aggregate does not have are read as zeros by the two-level kernel
	// (d_lmState: the LM decision state in [0, 9), the run start's chi2 slot group from [16])
	d_lamS.resize(1); d_lmState.resize(32); sys.lam_dev = d_lamS.data();
	// (the row-update launch of the upper-triangle iteration keeps an aggregate's 6 agg row entries in the registers of one workgroup:
	// beyond pcg_rows_max_aggregate() poses -- a user-set pcg_aggregate, or ~120 000 poses with the automatic one -- the two-launch form serves)
	sys.upper = agg > 0 && agg <= pcg_rows_max_aggregate() && (spmvUpper < 0 ? spmvRows == 4 : spmvUpper != 0) ? 1 : 0;
	if (sys.upper)
	{
		d_tq.resize((size_t)6 * nblk); sys.tq = d_tq.data(); d_hrow.release(); sys.hrow = nullptr;
		d_lowpos.resize((size_t)nblk); sys.lowpos = d_lowpos.data();
		DeviceGraph gg; gg.Pf = Pf;
		launch_build_lowpos(gg, st, d_lowpos.data(), stream);
		sys.npq = spmv_upper_grid(Pf);          // (fewer p.Ap partials than the row-sum SpMV leaves: the rings are sized for those)
	}
	else
	{
		d_hrow.resize((size_t)36 * 20 * ellM * Pf); sys.hrow = d_hrow.data();
		d_hrow.zero(stream);         // (padding slots are never written)
	}
	sys.spmv_rows = spmvRows;
	sys.agg = agg; sys.nc = nc; sys.cl = agg > 0 ? cl : 1; sys.inv_agg = agg > 0 ? Scalar(1) / Scalar(agg) : Scalar(0); sys.acinv = d_coarse[0].data(); sys.rc = d_rc.data(); sys.r2 = d_r2.data();
	sys.acinv32 = fp32Inverse() && agg > 0 ? d_coarse32[0].data() : nullptr;
	cutReductionParts();
	haveStructure = true;
	structRelPairs = h_relPairs; cntStructureBuilds++;
}

// Landmark partitions: cut the reduced matrix at block rows into at most `redChunks` ranges of about equal size and group the block list
// of the Schur pass by range.  The cuts depend on the (global) block pattern only, so every rank of a partitioned run makes the same
// ones; inside a range the list keeps its order and its whole-wave blocks stay in front, so every block is computed exactly as in
// one pass.
void cuba_hip_solver::cutReductionParts()
{
	redParts.clear();
	if (partHi < 0 || st.nblk <= 0 || st.nOd <= 0 || Pf <= 0) return;
	const size_t matrixBytes = (size_t)36 * st.nblk * sizeof(Scalar);
	const int want = redChunks > 0 ? redChunks : (int)std::min<size_t>(8, matrixBytes >> 23);
	if (want <= 1) return;
	std::vector<int> rowptr((size_t)Pf + 1), od((size_t)st.nOd);
	HIP_TRY(hipMemcpyAsync(rowptr.data(), d_rowptr.data(), sizeof(int) * rowptr.size(), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(od.data(), d_odBlocks.data(), sizeof(int) * od.size(), hipMemcpyDeviceToHost, stream));
	sync();
	std::vector<int> cut{ 0 };            // first block of every range
	for (int c = 1; c < want; c++)
	{
		const int target = (int)((long long)st.nblk * c / want);
		const int b = *std::lower_bound(rowptr.begin(), rowptr.end(), target);
		if (b > cut.back() && b < st.nblk) cut.push_back(b);
	}
	if (cut.size() < 2) return;
	cut.push_back(st.nblk);
	const int C = (int)cut.size() - 1;
	std::vector<std::vector<int>> lists(C);
	std::vector<int> heavy(C, 0);
	int c = 0;                            // (an unused slot of an XCD-aware order, -1, stays with the entry before it)
	for (int i = 0; i < st.nOd; i++)
	{
		if (od[i] >= 0) c = (int)(std::upper_bound(cut.begin() + 1, cut.end(), od[i]) - (cut.begin() + 1));
		lists[c].push_back(od[i]);
		if (i < st.nHeavy) heavy[c]++;
	}
	od.clear();
	for (int k = 0; k < C; k++)
	{
		RedPart p;
		p.od.begin = (int)od.size(); od.insert(od.end(), lists[k].begin(), lists[k].end()); p.od.end = (int)od.size(); p.od.heavy = heavy[k];
		p.blkBegin = (size_t)cut[k]; p.blkEnd = (size_t)cut[k + 1];
		redParts.push_back(p);
	}
	d_odBlocks.upload(od, stream);
	sync();          // `od` is a local
}

void cuba_hip_solver::fillProdLm()
{
	d_prodLm.resize(d_prodEa.size());
	topo::launch_gather_int(d_prodEa.data(), d_elm.data(), d_prodEa.size(), d_prodLm.data(), stream);
}

void cuba_hip_solver::computeLandmarkOrder()
{
	d_lmFirst.resize(Lt); d_lmLast.resize(Lt); d_lmMap.resize(Lt); d_rawEl.resize(E);
	d_k64a.resize(std::max((size_t)Lf, d_k64a.size())); d_k64b.resize(std::max((size_t)Lf, d_k64b.size()));
	d_v32a.resize(std::max((size_t)Lf, d_v32a.size())); d_v32b.resize(std::max((size_t)Lf, d_v32b.size()));
	sortTemp((size_t)Lf);
	topo::launch_lm_first_last(d_rawEp.data(), d_rawElCaller.data(), E, Lt, d_lmFirst.data(), d_lmLast.data(), stream);
	topo::launch_lm_order_keys(d_lmFirst.data(), d_lmLast.data(), Lf, d_k64a.data(), d_v32a.data(), stream);
	HIP_TRY(topo::sort_u64_u32(d_topoTemp.data(), d_topoTemp.size(), d_k64a.data(), d_k64b.data(), d_v32a.data(), d_v32b.data(), (size_t)Lf, 64, stream));
	topo::launch_lm_order_map(d_v32b.data(), Lf, Lt, d_lmMap.data(), stream);
	topo::launch_remap_landmarks(d_rawElCaller.data(), d_lmMap.data(), E, d_rawEl.data(), stream);
	lmOrderActive = true;
	dropSnapshots();
}

void cuba_hip_solver::switchLandmarkOrder(bool on)
{
	if (on == lmOrderActive || !devTopology || E == 0 || d_rawElCaller.size() != (size_t)E) return;
	Scalar* X = d_state.data() + 7 * (size_t)Pt;
	if (lmOrderActive) landmarkRowsInPlace(X, Lt, 3, false);
	if (on) { computeLandmarkOrder(); landmarkRowsInPlace(X, Lt, 3, true); }
	else resetLandmarkOrder();
	runDeviceEdgeSort();
	sync();
	haveStructure = false; hostTopoValid = false; hostPatternValid = false;
}

void cuba_hip_solver::resetLandmarkOrder()
{
	d_rawEl.resize(E);
	if (E) HIP_TRY(hipMemcpyAsync(d_rawEl.data(), d_rawElCaller.data(), sizeof(int) * (size_t)E, hipMemcpyDeviceToDevice, stream));
	if (lmOrderActive) dropSnapshots();
	lmOrderActive = false;
}

void cuba_hip_solver::landmarkRowsInPlace(Scalar* rows, int nrows, int width, bool toInternal)
{
	const size_t n = (size_t)nrows * width;
	if (!n) return;
	d_rowTmp.resize(std::max(n, d_rowTmp.size()));
	HIP_TRY(hipMemcpyAsync(d_rowTmp.data(), rows, sizeof(Scalar) * n, hipMemcpyDeviceToDevice, stream));
	topo::launch_permute_rows(d_rowTmp.data(), rows, d_lmMap.data(), nrows, width, toInternal, stream);
}

const Scalar* cuba_hip_solver::landmarkRowsForCaller(const Scalar* rows, int nrows, int width)
{
	if (!lmOrderActive || nrows == 0) return rows;
	d_rowTmp.resize(std::max((size_t)nrows * width, d_rowTmp.size()));
	topo::launch_permute_rows(rows, d_rowTmp.data(), d_lmMap.data(), nrows, width, false, stream);
	return d_rowTmp.data();
}

void cuba_hip_solver::resetPoseOrder()
{
	if (reorderActive) dropSnapshots();          // (they hold rows in the order that ends here)
	reorderActive = false;
	poseOrderChanged();
	poseNewOfOld.resize(Pf); poseOldOfNew.resize(Pf);
	for (int i = 0; i < Pf; i++) poseNewOfOld[i] = poseOldOfNew[i] = i;
}

void cuba_hip_solver::permuteStateRows(std::vector<Scalar>& state, std::vector<Scalar>& camv) const
{
	permutePoseArray(state.data(), 4, true);
	permutePoseArray(state.data() + 4 * (size_t)Pt, 3, true);
	permutePoseArray(camv.data(), 5, true);
}

void cuba_hip_solver::runDeviceEdgeSort(bool withValues)
{
	if (withValues && valuesPending) { valuesPending = false; HIP_TRY(hipStreamWaitEvent(stream, evValues, 0)); }     // (a re-sort under a new pose order: the values must have landed)
	sizeSortedValues();
	d_k64a.resize(E); d_k64b.resize(E); d_v32a.resize(E); d_perm.resize(E); d_counters.resize(topo::CNT_COUNT);
	d_epose.resize(E); d_elm.resize(E); d_lmptr.resize((size_t)Lt + 1);
	d_counters.zero(stream);
	topo::launch_edge_keys(d_rawEp.data(), d_rawEl.data(), d_rawDim.data(), E, Pt, Pf, Lt, Lf, d_k64a.data(), d_v32a.data(), d_counters.data(), stream);
	const size_t tb = topo::sort_temp_bytes(E);
	d_topoTemp.resize(std::max(tb, d_topoTemp.size()));
	HIP_TRY(topo::sort_u64_u32(d_topoTemp.data(), d_topoTemp.size(), d_k64a.data(), d_k64b.data(), d_v32a.data(), d_perm.data(), E, 32 + bitsFor(Lt), stream));
	topo::launch_gather_edges(d_perm.data(), d_rawEp.data(), d_rawEl.data(), d_rawDim.data(), d_rawMeas.data(), d_rawOmega.data(), E,
		d_epose.data(), d_elm.data(), withValues ? d_mu.data() : nullptr, d_mv.data(), d_mr.data(), d_w.data(), stream);
	topo::launch_segment_ptr(d_elm.data(), E, Lt, d_lmptr.data(), stream);
	if (withValues) sortedValuesValid = true;
	cntEdgeSorts++;
	valuesStamp++;          // (the permutation or the sorted values are new: an edge gate derives its copies again, refreshGate)
}

std::vector<int> cuba_hip_solver::chainOrder(const std::vector<int>& rowptr, const std::vector<int>& colind, const std::vector<int>& prodPtr) const
{
	const int n = Pf;
	std::vector<int> adjP(n + 1, 0);
	for (int i = 0; i < n; i++)
		for (int k = rowptr[i]; k < rowptr[i + 1]; k++) if (colind[k] != i) { adjP[i + 1]++; adjP[colind[k] + 1]++; }
	for (int i = 0; i < n; i++) adjP[i + 1] += adjP[i];
	std::vector<int> adjJ(adjP[n]), adjW(adjP[n]), cur(adjP.begin(), adjP.end() - 1);
	std::vector<long long> deg(n, 0);
	for (int i = 0; i < n; i++)
		for (int k = rowptr[i]; k < rowptr[i + 1]; k++)
		{
			const int j = colind[k];
			if (j == i) continue;
			const int w = std::max(1, prodPtr[k + 1] - prodPtr[k]);
			adjJ[cur[i]] = j; adjW[cur[i]++] = w; adjJ[cur[j]] = i; adjW[cur[j]++] = w;
			deg[i] += w; deg[j] += w;
		}
	std::vector<char> visited(n, 0);
	std::vector<int> order; order.reserve(n);
	std::vector<std::pair<int, int>> heap;            // (weight, -pose) of unvisited poses next to visited ones
	int at = -1;
	for (int i = 0; i < n; i++) if (deg[i] > 0 && (at < 0 || deg[i] < deg[at])) at = i;
	if (at < 0) at = 0;
	int nextUnvisited = 0;
	while ((int)order.size() < n)
	{
		visited[at] = 1; order.push_back(at);
		int best = -1, bw = -1;
		for (int x = adjP[at]; x < adjP[at + 1]; x++)
		{
			const int j = adjJ[x];
			if (visited[j]) continue;
			heap.emplace_back(adjW[x], -j); std::push_heap(heap.begin(), heap.end());
			if (adjW[x] > bw || (adjW[x] == bw && j < best)) { best = j; bw = adjW[x]; }
		}
		if (best >= 0) { at = best; continue; }
		at = -1;
		while (!heap.empty())
		{
			std::pop_heap(heap.begin(), heap.end());
			const int j = -heap.back().second; heap.pop_back();
			if (!visited[j]) { at = j; break; }
		}
		if (at < 0)
		{
			while (nextUnvisited < n && visited[nextUnvisited]) nextUnvisited++;
			if (nextUnvisited >= n) break;
			at = nextUnvisited;
		}
	}
	std::vector<int> newOfOld(n);
	for (int k = 0; k < n; k++) newOfOld[order[k]] = k;
	return newOfOld;
}

void cuba_hip_solver::applyPoseOrder(const std::vector<int>& newOfOld)
{
	std::vector<Scalar> state(d_state.size()), camv((size_t)5 * Pt);
	HIP_TRY(hipMemcpyAsync(state.data(), d_state.data(), sizeof(Scalar) * state.size(), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(camv.data(), d_cam.data(), sizeof(Scalar) * camv.size(), hipMemcpyDeviceToHost, stream));
	sync();
	// back to the caller's order with the order in force, then into the new one
	permutePoseArray(state.data(), 4, false); permutePoseArray(state.data() + 4 * (size_t)Pt, 3, false); permutePoseArray(camv.data(), 5, false);
	poseNewOfOld = newOfOld;
	reorderActive = false;
	poseOrderChanged();
	for (int i = 0; i < Pf; i++) { poseOldOfNew[newOfOld[i]] = i; if (newOfOld[i] != i) reorderActive = true; }
	permuteStateRows(state, camv);
	d_state.upload(state, stream); d_cam.upload(camv, stream);
	d_poseMap.upload(poseNewOfOld, stream);
	topo::launch_remap_poses(d_rawEpCaller.data(), d_poseMap.data(), E, Pf, d_rawEp.data(), stream);
	if (lmOrderActive || landmarkOrderAllowed())
	{
		// (the landmark rows just went up in the order that ends here)
		if (lmOrderActive) landmarkRowsInPlace(d_state.data() + 7 * (size_t)Pt, Lt, 3, false);
		computeLandmarkOrder();
		landmarkRowsInPlace(d_state.data() + 7 * (size_t)Pt, Lt, 3, true);
	}
	runDeviceEdgeSort();
	sync();          // the host vectors above go out of scope
	dropSnapshots(); // (round-3 advisor: a snapshot taken in the previous order would assign pose rows to the wrong poses)
	haveStructure = false; hostTopoValid = false; hostPatternValid = false;
}

bool cuba_hip_solver::tryReorder(int nblk, int farBlocks)
{
	const int offDiag = nblk - Pf;
	if (!poseReorder || Pf < 48 || offDiag <= 0 || 2 * (long long)farBlocks < offDiag) return false;
	std::vector<int> rp((size_t)Pf + 1), ci(nblk), pp((size_t)nblk + 1);
	HIP_TRY(hipMemcpyAsync(rp.data(), d_rowptr.data(), sizeof(int) * rp.size(), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(ci.data(), d_colind.data(), sizeof(int) * ci.size(), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(pp.data(), d_prodPtr.data(), sizeof(int) * pp.size(), hipMemcpyDeviceToHost, stream));
	sync();
	const std::vector<int> order = chainOrder(rp, ci, pp);
	// worth it only if the new order really is more local
	long long farNew = 0;
	for (int i = 0; i < Pf; i++)
		for (int k = rp[i]; k < rp[i + 1]; k++) farNew += std::abs(order[i] - order[ci[k]]) > farOffset();
	if (std::getenv("CUBA_HIP_DEBUG")) std::fprintf(stderr, "[cuba_hip] pose order: %d of %d off-diagonal blocks far from the diagonal, %lld after the walk\n", farBlocks, offDiag, farNew);
	if (2 * farNew >= farBlocks) return false;
	applyPoseOrder(order);
	return true;
}

void cuba_hip_solver::ensureHostTopology()
{
	if (hostTopoValid || !devTopology) return;
	std::vector<uint32_t> p32(E);
	h_lmptr.resize((size_t)Lt + 1);
	std::vector<int>&sPose = h_spose[topoSlot], &sLm = h_slm[topoSlot];
	sPose.resize(E); sLm.resize(E);
	if (E)
	{
		HIP_TRY(hipMemcpyAsync(p32.data(), d_perm.data(), sizeof(uint32_t) * E, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(sPose.data(), d_epose.data(), sizeof(int) * E, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(sLm.data(), d_elm.data(), sizeof(int) * E, hipMemcpyDeviceToHost, stream));
	}
	HIP_TRY(hipMemcpyAsync(h_lmptr.data(), d_lmptr.data(), sizeof(int) * ((size_t)Lt + 1), hipMemcpyDeviceToHost, stream));
	sync();
	perm.assign(p32.begin(), p32.end());
	h_epose.resize(E);
	for (int i = 0; i < E; i++) h_epose[i] = sPose[i] & ~STEREO_BIT;
	hostTopoValid = true;
}

void cuba_hip_solver::buildStructureDevice()
{
	const auto t0 = Clock::now();
	lap(nullptr);
	int* cnt = d_counters.data();
	d_counters.zero(stream);
	sortTemp((size_t)std::max(E, Lf + 1));
	// 1. per landmark: free-pose edges, pose pairs; exclusive scan -> first product id of every landmark
	d_lmNfree.resize(Lf); d_pairCount.resize((size_t)Lf + 1); d_lmPairBase.resize((size_t)Lf + 1);
	d_freeCount.resize((size_t)Lf + 1); d_freeScan.resize((size_t)Lf + 1);
	topo::launch_lm_pairs(d_lmptr.data(), d_epose.data(), Lf, Pf, d_lmNfree.data(), d_pairCount.data(), d_freeCount.data(), stream);
	HIP_TRY(topo::exclusive_scan_i64(d_topoTemp.data(), d_topoTemp.size(), d_pairCount.data(), d_lmPairBase.data(), (size_t)Lf + 1, stream));
	HIP_TRY(topo::exclusive_scan_i64(d_topoTemp.data(), d_topoTemp.size(), d_freeCount.data(), d_freeScan.data(), (size_t)Lf + 1, stream));
	// 2. per free pose: its edges in ascending (= landmark) order -- a stable sort by pose
	d_k32a.resize(E); d_k32b.resize(E); d_v32a.resize(E); d_v32b.resize(E); d_tmpI0.resize(E);
	topo::launch_pose_keys(d_epose.data(), E, Pf, d_k32a.data(), d_v32a.data(), stream);
	HIP_TRY(topo::sort_u32_u32(d_topoTemp.data(), d_topoTemp.size(), d_k32a.data(), d_k32b.data(), d_v32a.data(), d_v32b.data(), E, bitsFor(Pf), stream));
	d_peEdge.resize(E); d_pePtr.resize((size_t)Pf + 1);
	topo::launch_copy_u32_to_int(d_v32b.data(), d_peEdge.data(), E, stream);
	topo::launch_copy_u32_to_int(d_k32b.data(), d_tmpI0.data(), E, stream);
	topo::launch_segment_ptr(d_tmpI0.data(), E, Pf, d_pePtr.data(), stream);
	// 3. wave work list, pass 1 (counts per chunk of landmarks) + scan
	// landmark partition (multi-GPU): the block PATTERN, the adjacency and the coarse lists are global -- every rank must hold the same
	// reduced-system layout --, the wave list covers the landmarks [lo, hi) only, and the product / pose-edge lists (in landmark
	// order) are walked over the sub-ranges that belong to those landmarks
	const int lo = std::max(0, partLo), hi = partHi < 0 ? Lt : std::min(Lt, partHi);
	localRanges = partHi >= 0;
	const int nChunks = (hi - lo + topo::WAVE_CHUNK - 1) / topo::WAVE_CHUNK;
	d_chunk.resize((size_t)2 * std::max(1, nChunks));
	if (nChunks == 0) d_chunk.zero(stream);
	topo::launch_wave_count(d_lmptr.data(), lo, hi, d_chunk.data(), stream);
	topo::launch_wave_scan(d_chunk.data(), nChunks, cnt, stream);
	// ---- synchronisation 1: number of products, of free-pose edges, of waves ------------------------------------------
	int hc[topo::CNT_COUNT];
	long long npairs = 0, nFreeEdges = 0;      // sums over the free landmarks of n (n - 1) / 2 and of n (n = edges with a free pose)
	HIP_TRY(hipMemcpyAsync(&npairs, d_lmPairBase.data() + Lf, sizeof(long long), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(&nFreeEdges, d_freeScan.data() + Lf, sizeof(long long), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(hc, cnt, sizeof hc, hipMemcpyDeviceToHost, stream));
	int eRange[2] = { 0, E };
	if (localRanges)
	{
		HIP_TRY(hipMemcpyAsync(&eRange[0], d_lmptr.data() + lo, sizeof(int), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(&eRange[1], d_lmptr.data() + hi, sizeof(int), hipMemcpyDeviceToHost, stream));
	}
	sync();
	lap("structure (device): pairs, pose lists, wave counts");
	if (Lf == 0) npairs = 0;
	// the pose pairs of the relative-pose edges: off-diagonal seeds of the pattern, in the internal pose order in force
	h_relSeeds = relSeedKeys();
	const int nRelSeeds = (int)h_relSeeds.size(), nSeeds = Pf + nRelSeeds;
	if (npairs >= (1LL << 31) - nSeeds) throw ArgError{ "graph too dense: more than 2^31 Schur block products" };
	nmul = npairs + nFreeEdges;
	const int nWaves = hc[topo::CNT_NWAVES], nBig = hc[topo::CNT_NBIG];
	d_waveLm.resize((size_t)2 * nWaves); d_bigLm.resize(nBig);
	topo::launch_wave_write(d_lmptr.data(), lo, hi, d_chunk.data(), d_waveLm.data(), d_bigLm.data(), stream);
	g.e_begin = eRange[0]; g.e_end = eRange[1];
	if (localRanges)
	{
		d_peBeg.resize(Pf); d_peEnd.resize(Pf);
		topo::launch_segment_subrange(d_pePtr.data(), Pf, d_peEdge.data(), g.e_begin, g.e_end, d_peBeg.data(), d_peEnd.data(), stream);
	}
	// 4. pattern entries (diagonal seeds + one per product), sorted by (row, column); head flags; block index of every entry
	const size_t nEnt = (size_t)nSeeds + (size_t)npairs;
	if (nRelSeeds) d_relSeeds.upload(h_relSeeds, stream);
	d_k64a.resize(nEnt); d_k64b.resize(nEnt); d_v64a.resize(nEnt); d_v64b.resize(nEnt);
	sortTemp(nEnt);
	topo::launch_pattern_entries(d_lmptr.data(), d_epose.data(), d_elm.data(), d_lmNfree.data(), d_lmPairBase.data(), E, Lf, Pf, d_k64a.data(), d_v64a.data(),
		nRelSeeds ? d_relSeeds.data() : nullptr, nRelSeeds, stream);
	HIP_TRY(topo::sort_u64_u64(d_topoTemp.data(), d_topoTemp.size(), d_k64a.data(), d_k64b.data(), d_v64a.data(), d_v64b.data(), nEnt, 32 + bitsFor(Pf), stream));
	d_tmpI0.resize(std::max(nEnt, (size_t)E)); d_tmpI1.resize(std::max(nEnt, (size_t)E));
	topo::launch_entry_heads(d_k64b.data(), nEnt, d_tmpI0.data(), stream);
	int nblk = 0;
	if (nEnt)
	{
		HIP_TRY(topo::inclusive_scan_i32(d_topoTemp.data(), d_topoTemp.size(), d_tmpI0.data(), d_tmpI1.data(), nEnt, stream));
		// ---- synchronisation 2: number of blocks ------------------------------------------------------------------
		// (off-diagonal seeds: the product positions need the number of seeds before every entry)
		if (nRelSeeds)
		{
			d_relSeedFlag.resize(nEnt); d_relSeedScan.resize(nEnt);
			topo::launch_seed_flags(d_v64b.data(), nEnt, d_relSeedFlag.data(), stream);
			HIP_TRY(topo::inclusive_scan_i32(d_topoTemp.data(), d_topoTemp.size(), d_relSeedFlag.data(), d_relSeedScan.data(), nEnt, stream));
		}
		nblk = readBack(d_tmpI1.data() + (nEnt - 1));
	}
	lap("structure (device): entries sorted, blocks counted");
	// 5. blocks + product lists, row pointers
	d_colind.resize(nblk); d_blkrow.resize(nblk); d_prodPtr.resize((size_t)nblk + 1); d_prodEa.resize((size_t)npairs); d_prodEb.resize((size_t)npairs);
	d_rowptr.resize((size_t)Pf + 1);
	if (nblk == 0) { d_prodPtr.zero(stream); d_rowptr.zero(stream); }
	topo::launch_blocks_from_entries(d_k64b.data(), d_v64b.data(), d_tmpI1.data(), nEnt, nSeeds, nRelSeeds ? d_relSeedScan.data() : nullptr,
		d_colind.data(), d_blkrow.data(), d_prodPtr.data(),
		d_prodEa.data(), d_prodEb.data(), stream);
	topo::launch_segment_ptr(d_blkrow.data(), nblk, Pf, d_rowptr.data(), stream);
	// (the tile order of the Schur block pass -- a host computation over the block list -- needs only what exists from here on: its
	// inputs start their way to a page-locked staging block now, and the host works on them while the device runs steps 6-8)
	const bool earlyTiles = rowGroupedBlocks(npairs) && nblk > 0 && !localRanges;
	if (earlyTiles)
	{
		if (tileStageCap < (size_t)3 * nblk + 1)
		{
			if (h_tileStage) (void)hipHostFree(h_tileStage);
			h_tileStage = nullptr; tileStageCap = 0;
			HIP_TRY(hipHostMalloc((void**)&h_tileStage, sizeof(int) * ((size_t)3 * nblk + 1), hipHostMallocDefault));
			tileStageCap = (size_t)3 * nblk + 1;
		}
		if (!evTileInputs) HIP_TRY(hipEventCreateWithFlags(&evTileInputs, hipEventDisableTiming));
		HIP_TRY(hipMemcpyAsync(h_tileStage, d_blkrow.data(), sizeof(int) * nblk, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(h_tileStage + nblk, d_colind.data(), sizeof(int) * nblk, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(h_tileStage + 2 * (size_t)nblk, d_prodPtr.data(), sizeof(int) * ((size_t)nblk + 1), hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipEventRecord(evTileInputs, stream));
	}
	// 6. blocks with products, longest list first
	const size_t n32 = std::max((size_t)std::max(nblk, E), (size_t)2 * nblk);
	d_k32a.resize(n32); d_k32b.resize(n32); d_v32a.resize(n32); d_v32b.resize(n32);
	sortTemp(n32);
	d_odBlocks.resize(nblk);
	if (localRanges)
	{
		fillProdLm();
		d_prodBeg.resize(nblk); d_prodEnd.resize(nblk);
		topo::launch_segment_subrange(d_prodPtr.data(), nblk, d_prodLm.data(), lo, hi, d_prodBeg.data(), d_prodEnd.data(), stream);
	}
	topo::launch_od_keys(localRanges ? d_prodBeg.data() : d_prodPtr.data(), localRanges ? d_prodEnd.data() : d_prodPtr.data() + 1,
		d_blkrow.data(), d_colind.data(), nblk, farOffset(), BP_HEAVY, d_k32a.data(), d_v32a.data(), cnt, stream);
	if (nblk) HIP_TRY(topo::sort_u32_u32(d_topoTemp.data(), d_topoTemp.size(), d_k32a.data(), d_k32b.data(), d_v32a.data(), d_v32b.data(), nblk, 32, stream));
	topo::launch_copy_u32_to_int(d_v32b.data(), d_odBlocks.data(), nblk, stream);
	// 7. symmetric adjacency: the lower part of every row comes from the (column, row)-sorted list of the off-diagonal blocks
	const int nAdj = std::max(0, 2 * nblk - Pf);
	d_lowerPtr.resize((size_t)Pf + 1); d_adjPtr.resize((size_t)Pf + 1); d_adjBlk.resize(nAdj); d_adjCol.resize(nAdj); d_adjRow.resize(nAdj);
	// (both scratch arrays serve step 8 as well: head flags / their scan over the nAdj = 2 nblk - Pf adjacency entries, which
	// exceeds E and Pf + npairs when most pose pairs share a single landmark)
	d_tmpI0.resize(std::max(std::max((size_t)nblk, (size_t)nAdj), d_tmpI0.size())); d_tmpI1.resize(std::max((size_t)nAdj, d_tmpI1.size()));
	d_k64a.resize(std::max((size_t)nblk, d_k64a.size())); d_k64b.resize(std::max((size_t)nblk, d_k64b.size()));
	topo::launch_transpose_keys(d_colind.data(), d_blkrow.data(), nblk, d_k64a.data(), d_v32a.data(), stream);
	if (nblk) HIP_TRY(topo::sort_u64_u32(d_topoTemp.data(), d_topoTemp.size(), d_k64a.data(), d_k64b.data(), d_v32a.data(), d_v32b.data(), nblk, 64, stream));
	topo::launch_keys_hi(d_k64b.data(), nblk, Pf, d_tmpI0.data(), stream);
	topo::launch_segment_ptr(d_tmpI0.data(), nblk, Pf, d_lowerPtr.data(), stream);
	topo::launch_adj_ptr(d_rowptr.data(), d_lowerPtr.data(), Pf, d_adjPtr.data(), cnt, stream);
	topo::launch_adj_fill(d_rowptr.data(), d_colind.data(), d_blkrow.data(), d_lowerPtr.data(), d_k64b.data(), d_v32b.data(), nblk, d_adjPtr.data(),
		d_adjBlk.data(), d_adjCol.data(), d_adjRow.data(), stream);
	// 8. coarse-matrix assembly lists: adjacency entries grouped by the coarse block they fall into (stable: entry order kept)
	const CoarseCfg cc = coarseConfig();
	d_cbI.resize(nAdj); d_cbJ.resize(nAdj); d_cbPtr.resize((size_t)nAdj + 1); d_cbBlk.resize(nAdj);
	d_cbWi.resize(cc.cl == 2 ? nAdj : 0); d_cbWj.resize(cc.cl == 2 ? nAdj : 0);
	if (cc.nc > 0 && nAdj > 0)
	{
		topo::launch_coarse_keys(d_adjRow.data(), d_adjCol.data(), nAdj, cc.agg, cc.nc, d_k32a.data(), d_v32a.data(), stream);
		HIP_TRY(topo::sort_u32_u32(d_topoTemp.data(), d_topoTemp.size(), d_k32a.data(), d_k32b.data(), d_v32a.data(), d_v32b.data(), nAdj, bitsFor((long long)cc.nc * cc.nc), stream));
		topo::launch_heads_u32(d_k32b.data(), nAdj, d_tmpI0.data(), stream);
		HIP_TRY(topo::inclusive_scan_i32(d_topoTemp.data(), d_topoTemp.size(), d_tmpI0.data(), d_tmpI1.data(), nAdj, stream));
		topo::launch_coarse_lists(d_k32b.data(), d_v32b.data(), d_tmpI1.data(), d_adjBlk.data(), d_adjRow.data(), d_adjCol.data(), nAdj, cc.agg, cc.nc, Pf, cc.cl,
			d_cbI.data(), d_cbJ.data(), d_cbPtr.data(), d_cbBlk.data(), d_cbWi.data(), d_cbWj.data(), cnt, stream);
	}
	allocSystem(nblk, cc);
	// ---- synchronisation 3: widest adjacency row, numbers of product blocks and of coarse blocks -----------------------------
	HIP_TRY(hipMemcpyAsync(hc, cnt, sizeof hc, hipMemcpyDeviceToHost, stream));
	std::vector<int> earlyOd;
	if (earlyTiles)
	{
		HIP_TRY(hipEventSynchronize(evTileInputs));
		const int* pp = h_tileStage + 2 * (size_t)nblk;
		std::vector<int> len(nblk);
		for (int k = 0; k < nblk; k++) len[k] = pp[k + 1] - pp[k];
		earlyOd = rowGroupedOrder(h_tileStage, h_tileStage + nblk, len.data(), nblk);
	}
	sync();
	lap("structure (device): adjacency, coarse lists, allocations");
	const int maxRow = hc[topo::CNT_MAXROW];
	const int ellM = std::min(3, (maxRow + 19) / 20), ellOver = maxRow > 20 * ellM;
	d_ell.resize((size_t)Pf * ellM * 20);
	topo::launch_ell(d_adjPtr.data(), d_adjBlk.data(), d_adjCol.data(), Pf, ellM, d_ell.data(), stream);
	if (!reorderActive && !reorderTried && tryReorder(nblk, hc[topo::CNT_FARBLOCKS]))
	{
		reorderTried = true;
		buildStructureDevice();            // once more, now in the internal pose order
		return;
	}
	reorderTried = false;
	diagProdBlocks = hc[topo::CNT_DIAGPROD]; heavyBlocks = hc[topo::CNT_NHEAVY];
	int nOdList = hc[topo::CNT_NOD];
	if (earlyTiles)
	{
		d_odBlocks.upload(earlyOd, stream);
		sync();          // `earlyOd` is a local
		nOdList = (int)earlyOd.size(); heavyBlocks = 0;
	}
	else if (rowGroupedBlocks(npairs) && nblk > 0)
	{
		// (landmark partitions: the list lengths are those of the rank's sub-ranges, known only after step 6)
		std::vector<int> hRow(nblk), hBeg(nblk), hEnd(nblk), hCol;
		hCol.resize(nblk); HIP_TRY(hipMemcpyAsync(hCol.data(), d_colind.data(), sizeof(int) * nblk, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(hRow.data(), d_blkrow.data(), sizeof(int) * nblk, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(hBeg.data(), localRanges ? d_prodBeg.data() : d_prodPtr.data(), sizeof(int) * nblk, hipMemcpyDeviceToHost, stream));
		HIP_TRY(hipMemcpyAsync(hEnd.data(), localRanges ? d_prodEnd.data() : d_prodPtr.data() + 1, sizeof(int) * nblk, hipMemcpyDeviceToHost, stream));
		sync();
		for (int k = 0; k < nblk; k++) hEnd[k] -= hBeg[k];          // list lengths
		const std::vector<int> od = rowGroupedOrder(hRow.data(), hCol.data(), hEnd.data(), nblk);
		d_odBlocks.upload(od, stream);
		sync();          // `od` is a local: the copy must have left it (round-3 advisor)
		nOdList = (int)od.size(); heavyBlocks = 0;
	}
	lap("structure (device): block order of the Schur pass");
	publishStructure(nblk, nWaves, nBig, nOdList, cc.nc > 0 ? hc[topo::CNT_NCB] : 0, ellM, ellOver, cc);
	hostPatternValid = false;
	lap("structure (device): published");
	if (std::getenv("CUBA_HIP_DEBUG")) std::fprintf(stderr, "[cuba_hip] structure (device): nblk %d products %lld waves %d big %d od %d coarse blocks %d max row %d\n",
		nblk, npairs, nWaves, nBig, hc[topo::CNT_NOD], hc[topo::CNT_NCB], maxRow);
	const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
	prof[1] += 0.5 * dt; prof[5] += 0.5 * dt;
}

std::vector<cuba_hip_solver::CallerBlock> cuba_hip_solver::callerBlocks()
{
	ensureHostPattern();
	std::vector<CallerBlock> b; b.reserve(h_colind.size());
	for (int i = 0; i < Pf; i++)
		for (int k = h_rowptr[i]; k < h_rowptr[i + 1]; k++)
		{
			int r = poseOldOfNew[i], c = poseOldOfNew[h_colind[k]];
			const bool tr = r > c;
			if (tr) std::swap(r, c);
			b.push_back(CallerBlock{ ((uint64_t)(uint32_t)r << 32) | (uint32_t)c, k, tr });
		}
	std::sort(b.begin(), b.end(), [](const CallerBlock& x, const CallerBlock& y) { return x.key < y.key; });
	return b;
}

void cuba_hip_solver::ensureHostPattern()
{
	if (hostPatternValid) return;
	h_rowptr.resize((size_t)Pf + 1); h_colind.resize(st.nblk);
	HIP_TRY(hipMemcpyAsync(h_rowptr.data(), d_rowptr.data(), sizeof(int) * h_rowptr.size(), hipMemcpyDeviceToHost, stream));
	if (st.nblk) HIP_TRY(hipMemcpyAsync(h_colind.data(), d_colind.data(), sizeof(int) * h_colind.size(), hipMemcpyDeviceToHost, stream));
	sync();
	hostPatternValid = true;
}
