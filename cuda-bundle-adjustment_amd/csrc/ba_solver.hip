// ba_solver.hip -- the C ABI (include/cuba_hip.h) over the solver handle of ba_solver.hpp.
//
// There is deliberately no CPU fallback: every entry point fails with CUBA_HIP_ERR_NO_DEVICE / CUBA_HIP_ERR_RUNTIME when no gfx950 device
// is usable.
#include "ba_solver.hpp"

using namespace cubahip;


// -----------------------------------------------------------------------------------------------------
// C ABI
// -----------------------------------------------------------------------------------------------------
namespace cubahip_host
{
std::atomic<int> g_liveHandles{ 0 };
}

namespace
{
std::string g_createError;

template <typename F>
int guarded(cuba_hip_solver* s, F&& f)
{
	if (!s) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	try
	{
		if (hipSetDevice(s->device) != hipSuccess) { s->lastError = "hipSetDevice failed"; return CUBA_HIP_ERR_RUNTIME; }
		f();
		return CUBA_HIP_OK;
	}
	catch (const HipError& e)
	{
		char buf[512];
		std::snprintf(buf, sizeof buf, "HIP error %d (%s) in `%s` at %s:%d", (int)e.code, hipGetErrorString(e.code), e.what, e.file, e.line);
		s->lastError = buf;
		return CUBA_HIP_ERR_RUNTIME;
	}
	catch (const StateError& e) { s->lastError = e.msg; return CUBA_HIP_ERR_STATE; }
	catch (const ArgError& e) { s->lastError = e.msg; return CUBA_HIP_ERR_INVALID_ARGUMENT; }
	catch (const std::exception& e) { s->lastError = e.what(); return CUBA_HIP_ERR_RUNTIME; }
}
}  // namespace

namespace
{
std::mutex g_pinMutex;
std::vector<void*> g_pinned;      // blocks handed out by cuba_hip_host_alloc that really are page-locked
}

extern "C" {

void* cuba_hip_host_alloc(size_t bytes)
{
	void* p = nullptr;
	int n = 0;
	if (bytes && hipGetDeviceCount(&n) == hipSuccess && n > 0 && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess && p)
	{
		std::lock_guard<std::mutex> lk(g_pinMutex);
		g_pinned.push_back(p);
		return p;
	}
	(void)hipGetLastError();
	return std::malloc(bytes ? bytes : 1);
}

void cuba_hip_host_free(void* p)
{
	if (!p) return;
	{
		std::lock_guard<std::mutex> lk(g_pinMutex);
		auto it = std::find(g_pinned.begin(), g_pinned.end(), p);
		if (it != g_pinned.end()) { g_pinned.erase(it); (void)hipHostFree(p); return; }
	}
	std::free(p);
}

const char* cuba_hip_version(void) { return sizeof(Scalar) == 8 ? "cuba-hip 0.1 (gfx950, fp64)" : "cuba-hip 0.1 (gfx950, fp32)"; }
int cuba_hip_scalar_size(void) { return (int)sizeof(Scalar); }

int cuba_hip_create(int device, cuba_hip_solver** out)
{
	if (!out) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CUBA_HIP_ERR_NO_DEVICE;
	if (device < 0 || device >= n) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (hipSetDevice(device) != hipSuccess) return CUBA_HIP_ERR_RUNTIME;
	cuba_hip_solver* s = new (std::nothrow) cuba_hip_solver;
	if (!s) return CUBA_HIP_ERR_RUNTIME;
	s->device = device;
	if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { delete s; return CUBA_HIP_ERR_RUNTIME; }
	s->ownStream = true;
	g_liveHandles.fetch_add(1, std::memory_order_relaxed);
	*out = s;
	return CUBA_HIP_OK;
}

int cuba_hip_destroy(cuba_hip_solver* s)
{
	if (!s) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	(void)hipSetDevice(s->device);
	(void)hipStreamSynchronize(s->stream);
	delete s;
	g_liveHandles.fetch_sub(1, std::memory_order_relaxed);
	return CUBA_HIP_OK;
}

const char* cuba_hip_last_error(const cuba_hip_solver* s) { return s ? s->lastError.c_str() : "null solver handle"; }

int cuba_hip_set_stream(cuba_hip_solver* s, void* hip_stream)
{
	return guarded(s, [&] {
		s->sync();
		if (s->ownStream && s->stream) { HIP_TRY(hipStreamDestroy(s->stream)); s->ownStream = false; }
		s->stream = (hipStream_t)hip_stream;
	});
}

int cuba_hip_set_option(cuba_hip_solver* s, const char* key, double value)
{
	return guarded(s, [&] {
		if (!key) throw ArgError{ "null key" };
		const std::string k(key);
		if (k == "pcg_tol") s->pcgTol = value;
		else if (k == "pcg_max_iter") { s->pcgMaxIter = (int)value; s->haveStructure = false; }
		else if (k == "heuristics") { s->heuristics = value != 0; s->firstInvValid = false; s->firstInvPending = false; }
		else if (k == "precond_fp32") { s->precondFp32 = value != 0; s->haveStructure = false; s->coarseValid = false; s->dropPcgGraph(); }
		else if (k == "pose_reorder") { s->poseReorder = value != 0; s->haveStructure = false; }
		else if (k == "device_setup") { s->deviceSetup = value != 0; s->haveStructure = false; }
		else if (k == "mixed_precision") s->mixedPrecision = value != 0 && sizeof(Scalar) == 8;
		else if (k == "pcg_accept_unconverged") s->acceptUnconverged = value != 0;
		else if (k == "direct_fallback") { s->directFallback = value != 0; s->directSticky = false; }
		else if (k == "direct_after") s->directAfter = (int)value;
		else if (k == "direct_max_tiles") { s->directMaxTiles = (int)value; s->directRefused = false; s->directPlanValid = false; }
		else if (k == "direct_slack") { s->directSlack = (int)value; s->directRefused = false; s->directPlanValid = false; }
		else if (k == "reduced_solver")
		{
			if (value != 0 && value != 1) throw ArgError{ "reduced_solver: 0 = block PCG with the exact solver as fallback, 1 = exact sparse Cholesky for every solve" };
			s->directAlways = value != 0;
		}
		else if (k == "pcg_aggregate") { s->pcgAggregate = (int)value; s->haveStructure = false; }
		else if (k == "coarse_linear") { s->coarseLinear = value != 0; s->haveStructure = false; }
		else if (k == "covariance_workspace_mb")
		{
			if (value < 0 || value > (double)(1 << 30)) throw ArgError{ "covariance_workspace_mb must lie in 0 .. 2^30 (0 = automatic)" };
			s->covWorkspaceMb = value;
		}
		else if (k == "landmark_reorder") s->lmReorder = value != 0;         // (takes effect with the next cuba_hip_set_graph: setGraph's lmOrderFits)
		else if (k == "reduction_chunks")
		{
			if (value < 0 || value > 64) throw ArgError{ "reduction_chunks must lie in 0 .. 64" };
			s->redChunks = (int)value; s->haveStructure = false;
		}
		else if (k == "spmv_upper") { s->spmvUpper = (int)value; s->haveStructure = false; s->dropPcgGraph(); }
		else if (k == "pcg_graph") { s->useGraph = value != 0; s->dropPcgGraph(); }
		else if (k == "profile") s->profile = value != 0;
		else throw ArgError{ "unknown option: " + k };
	});
}


int cuba_hip_hint_unchanged(cuba_hip_solver* s, int same_edges, int same_values)
{
	return guarded(s, [&] { s->hintSameEdges = same_edges != 0; s->hintSameValues = same_edges != 0 && same_values != 0; });
}

int cuba_hip_set_graph(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf, const double* q, const double* t, const double* cam,
	const double* Xw, int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim,
	const double* meas, const double* omega)
{
	return guarded(s, [&] { s->setGraph(Pt, Pf, Lt, Lf, q, t, cam, Xw, E, edge_pose, edge_landmark, edge_dim, meas, omega); });
}

int cuba_hip_set_graph_begin(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf, const double* q, const double* t, const double* cam,
	const double* Xw, int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim,
	const double* meas, const double* omega)
{
	return guarded(s, [&] { s->setGraph(Pt, Pf, Lt, Lf, q, t, cam, Xw, E, edge_pose, edge_landmark, edge_dim, meas, omega, true); });
}

int cuba_hip_set_graph_partition(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf,
	const double* q, const double* t, const double* cam, const double* Xw,
	int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim,
	const double* meas, const double* omega, int landmark_begin, int landmark_end)
{
	return guarded(s, [&] {
		if (landmark_end < 0) throw ArgError{ "bad landmark range" };
		s->setGraph(Pt, Pf, Lt, Lf, q, t, cam, Xw, E, edge_pose, edge_landmark, edge_dim, meas, omega, false, landmark_begin, landmark_end);
	});
}

int cuba_hip_set_graph_end(cuba_hip_solver* s)
{
	return guarded(s, [&] {
		if (!s->haveGraph) throw StateError{ "set_graph_begin must be called first" };
		if (s->upStream) HIP_TRY(hipStreamSynchronize(s->upStream));      // the caller's meas / omega are free again
		s->finishValues();
	});
}

int cuba_hip_set_robust_kernel(cuba_hip_solver* s, int edge_type, int kind, double delta)
{
	return guarded(s, [&] {
		if (edge_type < 0 || edge_type > 1 || kind < 0 || kind > 2) throw ArgError{ "bad robust kernel" };
		s->rk[edge_type] = RobustKernel{ kind, (Scalar)delta };
	});
}

int cuba_hip_build_structure(cuba_hip_solver* s) { return guarded(s, [&] { s->buildStructure(); s->sync(); }); }

int cuba_hip_compute_errors(cuba_hip_solver* s, double* chi2)
{
	return guarded(s, [&] { if (!chi2) throw ArgError{ "null output" }; *chi2 = s->computeErrors(); });
}

int cuba_hip_build_system(cuba_hip_solver* s) { return guarded(s, [&] { s->need(); }); }

int cuba_hip_max_diagonal(cuba_hip_solver* s, double* v)
{
	return guarded(s, [&] { if (!v) throw ArgError{ "null output" }; *v = s->maxDiagonal(); });
}

int cuba_hip_set_lambda(cuba_hip_solver* s, double lambda) { return guarded(s, [&] { s->lambda = lambda; }); }
int cuba_hip_restore_diagonal(cuba_hip_solver* s) { return guarded(s, [&] { s->lambda = 0; }); }

int cuba_hip_schur(cuba_hip_solver* s) { return guarded(s, [&] { s->schur(); }); }

int cuba_hip_schur_parts(cuba_hip_solver* s, int* n_parts)
{
	return guarded(s, [&] { s->need(); if (n_parts) *n_parts = s->schurParts(); });
}

int cuba_hip_schur_part(cuba_hip_solver* s, int part, size_t ranges[4])
{
	return guarded(s, [&] { size_t r[4]; s->schurPart(part, r); if (ranges) std::copy(r, r + 4, ranges); });
}

int cuba_hip_solve_reduced(cuba_hip_solver* s, int* ok)
{
	return guarded(s, [&] { const bool r = s->solveReduced(); if (ok) *ok = r ? 1 : 0; });
}

int cuba_hip_back_substitute(cuba_hip_solver* s) { return guarded(s, [&] { s->backSubstitute(); }); }

int cuba_hip_solve(cuba_hip_solver* s, int* ok)
{
	return guarded(s, [&] { const bool r = s->solve(); if (ok) *ok = r ? 1 : 0; });
}

int cuba_hip_update(cuba_hip_solver* s) { return guarded(s, [&] { s->update(); }); }

int cuba_hip_compute_scale(cuba_hip_solver* s, double lambda, double* scale)
{
	return guarded(s, [&] {
		if (!scale) throw ArgError{ "null output" };
		*scale = s->computeScale(lambda);
	});
}

int cuba_hip_snapshot_state_slot(cuba_hip_solver* s, int slot)
{
	return guarded(s, [&] {
		if (slot < 0 || slot >= CUBA_HIP_SNAPSHOT_SLOTS) throw ArgError{ "snapshot slot out of range" };
		s->need();
		DevBuf<Scalar>& b = s->d_snapshots[slot];
		b.resize(s->d_state.size());
		HIP_TRY(hipMemcpyAsync(b.data(), s->d_state.data(), s->d_state.size() * sizeof(Scalar), hipMemcpyDeviceToDevice, s->stream));
	});
}

int cuba_hip_restore_state_slot(cuba_hip_solver* s, int slot)
{
	return guarded(s, [&] {
		s->need();
		const auto it = s->d_snapshots.find(slot);
		if (it == s->d_snapshots.end() || it->second.size() != s->d_state.size()) throw StateError{ "no snapshot of this graph's estimates in that slot (cuba_hip_snapshot_state)" };
		HIP_TRY(hipMemcpyAsync(s->d_state.data(), it->second.data(), s->d_state.size() * sizeof(Scalar), hipMemcpyDeviceToDevice, s->stream));
	});
}

int cuba_hip_snapshot_state(cuba_hip_solver* s) { return cuba_hip_snapshot_state_slot(s, 0); }
int cuba_hip_restore_state(cuba_hip_solver* s) { return cuba_hip_restore_state_slot(s, 0); }

int cuba_hip_push(cuba_hip_solver* s) { return guarded(s, [&] { s->push(); }); }
int cuba_hip_pop(cuba_hip_solver* s) { return guarded(s, [&] { s->pop(); }); }

int cuba_hip_optimize(cuba_hip_solver* s, int niterations, double* chi2_per_iter, int* n_done)
{
	return guarded(s, [&] {
		if (niterations < 0) throw ArgError{ "negative iteration count" };
		const int n = s->optimize(niterations, chi2_per_iter);
		if (n_done) *n_done = n;
	});
}

int cuba_hip_optimize_batch(cuba_hip_solver** handles, int n, int niterations, double* chi2_per_iter, int* n_done, int* batched_solves)
{
	if (!handles || n <= 0 || n > CUBA_HIP_BATCH_MAX || !n_done) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	for (int i = 0; i < n; i++)
	{
		if (!handles[i]) return CUBA_HIP_ERR_INVALID_ARGUMENT;
		for (int j = 0; j < i; j++) if (handles[j] == handles[i]) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	}
	// (an error is recorded on the first handle: cuba_hip_last_error(handles[0]))
	return guarded(handles[0], [&] {
		if (niterations < 0) throw ArgError{ "negative iteration count" };
		const int b = cuba_hip_optimize_batch_impl(handles, n, niterations, chi2_per_iter, n_done);
		if (batched_solves) *batched_solves = b;
	});
}

int cuba_hip_get_solution(cuba_hip_solver* s, double* q, double* t, double* Xw)
{
	return guarded(s, [&] {
		if (!s->haveGraph) throw StateError{ "set_graph must be called first" };
		const Scalar* base = s->d_state.data();
		if (q) { s->downloadAsDouble(base, q, (size_t)4 * s->Pt); s->permutePoseArray(q, 4, false); }
		if (t) { s->downloadAsDouble(base + 4 * (size_t)s->Pt, t, (size_t)3 * s->Pt); s->permutePoseArray(t, 3, false); }
		if (Xw) s->downloadAsDouble(s->landmarkRowsForCaller(base + 7 * (size_t)s->Pt, s->Lt, 3), Xw, (size_t)3 * s->Lt);
	});
}

int cuba_hip_set_solution(cuba_hip_solver* s, const double* q, const double* t, const double* Xw)
{
	return guarded(s, [&] {
		if (!s->haveGraph) throw StateError{ "set_graph must be called first" };
		s->buildStructure();          // the internal pose order (if any) is decided there
		Scalar* base = s->d_state.data();
		if (q) { std::vector<double> v(q, q + (size_t)4 * s->Pt); s->permutePoseArray(v.data(), 4, true); s->uploadFromDouble(base, v.data(), v.size()); }
		if (t) { std::vector<double> v(t, t + (size_t)3 * s->Pt); s->permutePoseArray(v.data(), 3, true); s->uploadFromDouble(base + 4 * (size_t)s->Pt, v.data(), v.size()); }
		if (Xw)
		{
			s->uploadFromDouble(base + 7 * (size_t)s->Pt, Xw, (size_t)3 * s->Lt);
			if (s->lmOrderActive) s->landmarkRowsInPlace(base + 7 * (size_t)s->Pt, s->Lt, 3, true);
		}
	});
}

int cuba_hip_chi_squares(cuba_hip_solver* s, double* out)
{
	return guarded(s, [&] { if (!out && s->E) throw ArgError{ "null output" }; s->chiSquares(out); });
}

int cuba_hip_chi_squares_begin(cuba_hip_solver* s, double* out)
{
	return guarded(s, [&] { if (!out && s->E) throw ArgError{ "null output" }; s->chiSquares(out, false); });     // (the host set-up path has finished when this returns)
}

int cuba_hip_chi_squares_end(cuba_hip_solver* s)
{
	return guarded(s, [&] { s->sync(); });
}

int cuba_hip_gate_edges(cuba_hip_solver* s, const double chi2_max[2], int require_positive_depth, int mode, int64_t counts[6], double* chi2_per_edge)
{
	return guarded(s, [&] { s->gateEdges(chi2_max, require_positive_depth != 0, mode, counts, chi2_per_edge); });
}

int cuba_hip_set_edge_active(cuba_hip_solver* s, const uint8_t* active) { return guarded(s, [&] { s->setEdgeActive(active); }); }
int cuba_hip_get_edge_active(cuba_hip_solver* s, uint8_t* active) { return guarded(s, [&] { s->getEdgeActive(active); }); }
int cuba_hip_landmark_active_edges(cuba_hip_solver* s, int32_t* per_landmark) { return guarded(s, [&] { s->landmarkActiveEdges(per_landmark); }); }

int cuba_hip_triangulate_landmarks(cuba_hip_solver* s, const uint8_t* select, int refine_iterations, double min_parallax_deg,
	const double chi2_max[2], int dry_run, int32_t* status, int64_t counts[CUBA_HIP_TRI_STATUSES], double* xyz)
{
	return guarded(s, [&] { s->triangulateLandmarks(select, refine_iterations, min_parallax_deg, chi2_max, dry_run != 0, status, counts, xyz); });
}

int cuba_hip_refine_poses(cuba_hip_solver* s, const uint8_t* select, int rounds, int iterations, int robust_rounds, const double chi2_max[2],
	int min_inliers, int dry_run, int32_t* status, int64_t counts[CUBA_HIP_POSEREF_STATUSES], int32_t* inliers, double* chi2, double* q, double* t,
	uint8_t* edge_inlier)
{
	return guarded(s, [&] { s->refinePoses(select, rounds, iterations, robust_rounds, chi2_max, min_inliers, dry_run != 0, status, counts, inliers, chi2, q, t, edge_inlier); });
}

int cuba_hip_localize_poses(cuba_hip_solver* s, const uint8_t* select, int hypotheses, uint64_t seed, const double chi2_max[2], int min_inliers,
	int dry_run, int32_t* status, int64_t counts[CUBA_HIP_POSELOC_STATUSES], int32_t* inliers, double* cost, int32_t* winner, double* q, double* t,
	uint8_t* edge_inlier)
{
	return guarded(s, [&] { s->localizePoses(select, hypotheses, seed, chi2_max, min_inliers, dry_run != 0, status, counts, inliers, cost, winner, q, t, edge_inlier); });
}

int cuba_hip_get_profile(cuba_hip_solver* s, double seconds[CUBA_HIP_PROFILE_ITEMS])
{
	return guarded(s, [&] { for (int i = 0; i < CUBA_HIP_PROFILE_ITEMS; i++) seconds[i] = s->prof[i]; });
}

int cuba_hip_get_counters(cuba_hip_solver* s, int64_t c[8])
{
	return guarded(s, [&] {
		c[0] = s->cntPcgIters; c[1] = s->cntTrials; c[2] = s->st.nblk; c[3] = s->nmul;
		c[4] = s->cntCoarseRefresh; c[5] = s->cntPcgLooks; c[6] = s->cntPcgEnqueued; c[7] = 6 * (int64_t)s->sys.cl * s->sys.nc;
	});
}

int cuba_hip_get_counter(cuba_hip_solver* s, const char* name, int64_t* value)
{
	return guarded(s, [&] {
		if (!name || !value) throw ArgError{ "null argument" };
		const std::string k(name);
		if (k == "pcg_iterations") *value = s->cntPcgIters;
		else if (k == "lm_trials") *value = s->cntTrials;
		else if (k == "coarse_refreshes") *value = s->cntCoarseRefresh;
		else if (k == "coarse_inline_inversions") *value = s->cntCoarseInline;
		else if (k == "pcg_host_looks") *value = s->cntPcgLooks;
		else if (k == "pcg_iterations_enqueued") *value = s->cntPcgEnqueued;
		else if (k == "pcg_unconverged_solves") *value = s->cntPcgUnconverged;
		else if (k == "pcg_graph_instantiations") *value = s->gb.builds.load();
		else if (k == "precond_fp32_fallbacks") *value = s->cntFp32Fallbacks;
		else if (k == "pcg_iterations_plain_launches") *value = s->cntPcgPlain;
		else if (k == "batch_full_trials") *value = s->cntBatchFullTrials;
		else if (k == "batch_iteration_trials") *value = s->cntBatchIterTrials;
		else if (k == "host_looks") *value = s->cntHostLooks;
		else if (k == "exact_solve_fallbacks") *value = s->cntDirect;
		else if (k == "exact_solve_failures") *value = s->cntDirectFailed;
		else if (k == "graph_uploads") *value = s->cntUploads;
		else if (k == "structure_builds") *value = s->cntStructureBuilds;
		else if (k == "value_bytes_uploaded") *value = s->cntValueBytes;
		else if (k == "edge_sorts") *value = s->cntEdgeSorts;
		else if (k == "late_decision_records") *value = s->cntLateRecords;
		else if (k == "covariance_ns") *value = (int64_t)(1e9 * s->covSeconds);
		else if (k == "covariance_pairs_ns") *value = (int64_t)(1e9 * s->covPairsSeconds);
		else if (k == "covariance_pairs_chunks") *value = s->covPairChunks;
		else throw ArgError{ "unknown counter: " + k };
	});
}

int cuba_hip_get_pcg_history(cuba_hip_solver* s, int32_t* iterations, int capacity, int* n_solves, int64_t* n_unconverged)
{
	return guarded(s, [&] {
		const int n = (int)s->pcgHistory.size();
		if (n_solves) *n_solves = n;
		if (n_unconverged) *n_unconverged = s->cntPcgUnconverged;
		if (iterations) for (int i = 0; i < std::min(n, capacity); i++) iterations[i] = s->pcgHistory[i];
	});
}

int cuba_hip_get_hsc_structure(cuba_hip_solver* s, int32_t* row_ptr, int32_t* col_ind, int* nblk)
{
	return guarded(s, [&] {
		s->need();
		s->ensureHostPattern();
		if (nblk) *nblk = (int)s->h_colind.size();
		if (!s->reorderActive)
		{
			if (row_ptr) std::memcpy(row_ptr, s->h_rowptr.data(), sizeof(int) * s->h_rowptr.size());
			if (col_ind) std::memcpy(col_ind, s->h_colind.data(), sizeof(int) * s->h_colind.size());
			return;
		}
		const auto blocks = s->callerBlocks();
		if (row_ptr)
		{
			for (int i = 0; i <= s->Pf; i++) row_ptr[i] = 0;
			for (const auto& b : blocks) row_ptr[(int)(b.key >> 32) + 1]++;
			for (int i = 0; i < s->Pf; i++) row_ptr[i + 1] += row_ptr[i];
		}
		if (col_ind) for (size_t k = 0; k < blocks.size(); k++) col_ind[k] = (int)(uint32_t)blocks[k].key;
	});
}

int cuba_hip_get_array(cuba_hip_solver* s, int which, double* out, size_t* count)
{
	return guarded(s, [&] {
		s->need();
		const Scalar* src = nullptr; size_t n = 0;
		switch (which)
		{
		case CUBA_HIP_ARRAY_BP: src = s->sys.bp; n = (size_t)6 * s->Pf; break;
		case CUBA_HIP_ARRAY_BSC: src = s->sys.bsc; n = (size_t)6 * s->Pf; break;
		case CUBA_HIP_ARRAY_XP: src = s->sys.xp; n = (size_t)6 * s->Pf; break;
		case CUBA_HIP_ARRAY_XL: src = s->sys.xl; n = (size_t)3 * s->Lf; break;
		case CUBA_HIP_ARRAY_LM_SYS: src = s->sys.lm_sys; n = (size_t)9 * s->Lf; break;
		case CUBA_HIP_ARRAY_HSC: src = s->sys.hsc; n = (size_t)36 * s->st.nblk; break;
		default: throw ArgError{ "unknown array id" };
		}
		if (count) *count = n;
		if (out && n)
		{
			// (landmark-indexed arrays: back to the caller's landmark numbering)
			if (which == CUBA_HIP_ARRAY_XL) src = s->landmarkRowsForCaller(src, s->Lf, 3);
			else if (which == CUBA_HIP_ARRAY_LM_SYS) src = s->landmarkRowsForCaller(src, s->Lf, 9);
			s->downloadAsDouble(src, out, n);
			if (s->reorderActive)
			{
				// back to the caller's pose numbering
				if (which == CUBA_HIP_ARRAY_BP || which == CUBA_HIP_ARRAY_BSC || which == CUBA_HIP_ARRAY_XP) s->permutePoseArray(out, 6, false);
				else if (which == CUBA_HIP_ARRAY_HSC)
				{
					const std::vector<double> v(out, out + n);
					const auto blocks = s->callerBlocks();
					for (size_t k = 0; k < blocks.size(); k++)
					{
						const double* src36 = v.data() + 36 * (size_t)blocks[k].src;
						double* dst = out + 36 * k;
						for (int c = 0; c < 6; c++)
							for (int r = 0; r < 6; r++) dst[c * 6 + r] = blocks[k].transposed ? src36[r * 6 + c] : src36[c * 6 + r];
					}
				}
			}
		}
	});
}

// marginal covariances (g2o's SparseOptimizer::computeMarginals; the reference has none): ba_covariance.hip
int cuba_hip_compute_covariance(cuba_hip_solver* s, double* pose_cov, double* landmark_cov, int* not_positive_definite)
{
	return guarded(s, [&] {
		const bool ok = s->computeCovariance(pose_cov, landmark_cov);
		if (!ok) s->lastError = "marginal covariances: non-positive pivot (the undamped reduced matrix is not positive definite)";
		if (not_positive_definite) *not_positive_definite = ok ? 0 : 1;
	});
}

int cuba_hip_get_covariance_blocks(cuba_hip_solver* s, double* values)
{
	return guarded(s, [&] { s->covarianceBlocks(values); });
}

int cuba_hip_compute_covariance_pairs(cuba_hip_solver* s, int n, const int32_t* kind_a, const int32_t* index_a, const int32_t* kind_b,
	const int32_t* index_b, double* out, int* not_positive_definite)
{
	return guarded(s, [&] {
		const bool ok = s->computeCovariancePairs(n, kind_a, index_a, kind_b, index_b, out);
		if (!ok) s->lastError = "covariance pairs: non-positive pivot (the undamped reduced matrix is not positive definite)";
		if (not_positive_definite) *not_positive_definite = ok ? 0 : 1;
	});
}

// the per-factor chi2 of one kind (cubahip::FACTOR_*)
static int factor_chi_squares(cuba_hip_solver* s, int kind, double* out)
{
	return guarded(s, [&] {
		if (!s->haveGraph) throw StateError{ "set_graph must be called first" };
		if (s->factorSets[kind]->n() > 0 && !out) throw ArgError{ "null output" };
		s->factorChiSquares(kind, out);
	});
}

int cuba_hip_set_pose_priors(cuba_hip_solver* s, int n, const int32_t* pose, const double* q, const double* t, const double* info)
{
	return guarded(s, [&] { s->setPosePriors(n, pose, q, t, info); });
}

int cuba_hip_prior_chi_squares(cuba_hip_solver* s, double* chi2_per_prior) { return factor_chi_squares(s, cubahip::FACTOR_PRIORS, chi2_per_prior); }

int cuba_hip_set_relative_pose_edges(cuba_hip_solver* s, int n, const int32_t* pose_i, const int32_t* pose_j, const double* q, const double* t, const double* info)
{
	return guarded(s, [&] { s->setRelativePoseEdges(n, pose_i, pose_j, q, t, info); });
}

int cuba_hip_set_pose_factor_robust_kernels(cuba_hip_solver* s, int factor_type, int n, const int32_t* kind, const double* delta)
{
	return guarded(s, [&] { s->setPoseFactorRobustKernels(factor_type, n, kind, delta); });
}

int cuba_hip_relative_pose_chi_squares(cuba_hip_solver* s, double* chi2_per_edge) { return factor_chi_squares(s, cubahip::FACTOR_REL, chi2_per_edge); }

int cuba_hip_set_landmark_priors(cuba_hip_solver* s, int n, const int32_t* landmark, const double* xyz, const double* info, const int32_t* kind, const double* delta)
{
	return guarded(s, [&] { s->setLandmarkPriors(n, landmark, xyz, info, kind, delta); });
}

int cuba_hip_landmark_prior_chi_squares(cuba_hip_solver* s, double* chi2_per_prior) { return factor_chi_squares(s, cubahip::FACTOR_LMP, chi2_per_prior); }

int cuba_hip_set_position_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* position, const double* lever_arm, const double* info,
	const int32_t* kind, const double* delta)
{
	return guarded(s, [&] { s->setPositionFactors(n, pose, position, lever_arm, info, kind, delta); });
}

int cuba_hip_position_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor) { return factor_chi_squares(s, cubahip::FACTOR_POS, chi2_per_factor); }

int cuba_hip_set_direction_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* world_dir, const double* measured_dir, const double* info,
	const int32_t* kind, const double* delta)
{
	return guarded(s, [&] { s->setDirectionFactors(n, pose, world_dir, measured_dir, info, kind, delta); });
}

int cuba_hip_direction_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor) { return factor_chi_squares(s, cubahip::FACTOR_DIR, chi2_per_factor); }

int cuba_hip_set_range_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* anchor, const double* range, const double* lever_arm, const double* info,
	const int32_t* kind, const double* delta)
{
	return guarded(s, [&] { s->setRangeFactors(n, pose, anchor, range, lever_arm, info, kind, delta); });
}

int cuba_hip_range_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor) { return factor_chi_squares(s, cubahip::FACTOR_RNG, chi2_per_factor); }

int cuba_hip_set_pose_range_factors(cuba_hip_solver* s, int n, const int32_t* pose_i, const int32_t* pose_j, const double* range, const double* lever_arm_i,
	const double* lever_arm_j, const double* info, const int32_t* kind, const double* delta)
{
	return guarded(s, [&] { s->setPoseRangeFactors(n, pose_i, pose_j, range, lever_arm_i, lever_arm_j, info, kind, delta); });
}

int cuba_hip_pose_range_factor_chi_squares(cuba_hip_solver* s, double* chi2_per_factor) { return factor_chi_squares(s, cubahip::FACTOR_PRNG, chi2_per_factor); }

int cuba_hip_time_kernels(cuba_hip_solver* s, int reps, double ms_per_launch[CUBA_HIP_TIMED_KERNELS])
{
	return guarded(s, [&] {
		if (reps <= 0 || !ms_per_launch) throw ArgError{ "bad arguments" };
		s->timeKernels(reps, ms_per_launch);
	});
}

int cuba_hip_set_partition(cuba_hip_solver* s, int landmark_begin, int landmark_end)
{
	return guarded(s, [&] {
		if (!s->haveGraph) throw StateError{ "set_graph must be called first" };
		// (after a rank's upload the device holds the values of that rank's landmarks only: any other range would silently evaluate zeros)
		if (s->valuesPartial && (landmark_end < 0 || landmark_begin < s->partLo || landmark_end > s->partHi))
			throw StateError{ "cuba_hip_set_graph_partition uploaded this range's values only: a wider range needs a new upload" };
		if (landmark_begin == 0 && landmark_end == -1)          // remove the restriction: the handle evaluates the whole graph again
		{
			if (s->partHi >= 0) s->haveStructure = false;
			s->partLo = 0; s->partHi = -1;
			s->switchLandmarkOrder(s->landmarkOrderAllowed());      // (back to the internal landmark order a partition had ended)
			return;
		}
		if (landmark_begin < 0 || landmark_end > s->Lt || landmark_begin > landmark_end) throw ArgError{ "bad landmark range" };
		if (s->gateActive) throw StateError{ "a landmark partition is not available on a handle with gated edges (cuba_hip_set_edge_active(s, NULL) first)" };
		for (const FactorSet* set : s->factorSets)
			if (set->n() > 0) throw StateError{ std::string("a landmark partition is not available on a handle with ") + set->plural };
		if (s->partHi >= 0 && landmark_begin == s->partLo && landmark_end == s->partHi) return;      // (cuba_hip_set_graph_partition set it already)
		s->partLo = landmark_begin; s->partHi = landmark_end;
		s->haveStructure = false;
		// the range is in the caller's landmark numbering: unless it is the whole range, the internal landmark order ends here (rows of the
		// estimates back to the caller's order, edges sorted again)
		s->switchLandmarkOrder(s->landmarkOrderAllowed());
	});
}

int cuba_hip_assemble(cuba_hip_solver* s) { return guarded(s, [&] { s->assemble(); }); }

int cuba_hip_max_diagonal_parts(cuba_hip_solver* s, double* pose_part, double* landmark_part)
{
	return guarded(s, [&] { if (!pose_part || !landmark_part) throw ArgError{ "null output" }; s->maxDiagonalParts(pose_part, landmark_part); });
}

int cuba_hip_compute_scale_parts(cuba_hip_solver* s, double lambda, double* pose_part, double* landmark_part)
{
	return guarded(s, [&] { if (!pose_part || !landmark_part) throw ArgError{ "null output" }; s->scaleParts(lambda, pose_part, landmark_part); });
}

int cuba_hip_device_pointer(cuba_hip_solver* s, int which, void** device_ptr, size_t* count)
{
	return guarded(s, [&] {
		s->need();
		Scalar* p = nullptr; size_t n = 0;
		switch (which)
		{
		case CUBA_HIP_ARRAY_BP: p = s->sys.bp; n = (size_t)6 * s->Pf; break;
		case CUBA_HIP_ARRAY_BSC: p = s->sys.bsc; n = (size_t)6 * s->Pf; break;
		case CUBA_HIP_ARRAY_XP: p = s->sys.xp; n = (size_t)6 * s->Pf; break;
		case CUBA_HIP_ARRAY_XL: p = s->sys.xl; n = (size_t)3 * s->Lf; break;
		case CUBA_HIP_ARRAY_LM_SYS: p = s->sys.lm_sys; n = (size_t)9 * s->Lf; break;
		case CUBA_HIP_ARRAY_HSC: p = s->sys.hsc; n = (size_t)36 * s->st.nblk; break;
		case CUBA_HIP_ARRAY_STATE: p = s->d_state.data(); n = s->d_state.size(); break;
		default: throw ArgError{ "unknown array id" };
		}
		if (device_ptr) *device_ptr = p;
		if (count) *count = n;
	});
}

int cuba_hip_get_sizes(cuba_hip_solver* s, int sizes[5])
{
	return guarded(s, [&] {
		if (!s->haveGraph) throw StateError{ "set_graph must be called first" };
		sizes[0] = s->Pt; sizes[1] = s->Pf; sizes[2] = s->Lt; sizes[3] = s->Lf; sizes[4] = s->E;
	});
}

}  // extern "C"

namespace
{
// What the debug hooks of the exact solver build from a dense matrix: the reduced system as the library would hold it -- the 6 x 6 blocks
// on or above the diagonal that are not identically zero (the diagonal ones always), one block per (row, column) -- its plan, and the
// device views the fill and the factorisation read.
struct DebugSystem
{
	SparseCholPlan plan;
	std::vector<int> blkrow, colind;
	DevBuf<Scalar> dBlocks, dB, dTiles, dTilesT, dY, dRinv;
	DevBuf<int> dRow, dCol, dFail, dColPtr, dRowIdx, dColOf, dGPtr, dGather, dLvlTiles, dLvlCols, dBlkTile, dPos;
	SparseChol d;
	DeviceStructure st;
	DeviceSystem sys;
};

// false: the factor needs more than 2^22 tiles
bool debug_system(int n, const double* A, const double* b, int slack, int32_t stats[4], DebugSystem& q)
{
	const int P = n / 6;
	std::vector<Scalar> blocks; std::vector<int> rowptr(1, 0);
	for (int bi = 0; bi < P; bi++)
	{
		for (int bj = bi; bj < P; bj++)
		{
			bool any = bi == bj;
			for (int c = 0; c < 6 && !any; c++) for (int r = 0; r < 6; r++) any = any || A[(size_t)(6 * bj + c) * n + 6 * bi + r] != 0.0;
			if (!any) continue;
			q.blkrow.push_back(bi); q.colind.push_back(bj);
			for (int c = 0; c < 6; c++) for (int r = 0; r < 6; r++) blocks.push_back((Scalar)A[(size_t)(6 * bj + c) * n + 6 * bi + r]);
		}
		rowptr.push_back((int)q.colind.size());
	}
	SparseCholPlan& plan = q.plan;
	if (!sparse_chol_plan(P, rowptr.data(), q.colind.data(), slack, (size_t)1 << 22, plan)) return false;
	if (stats) { stats[0] = plan.T; stats[1] = plan.nTiles; stats[2] = plan.nLevels; stats[3] = plan.slack; }
	std::vector<Scalar> hb(b, b + n);
	q.dBlocks.upload(blocks, nullptr); q.dB.upload(hb, nullptr); q.dRow.upload(q.blkrow, nullptr); q.dCol.upload(q.colind, nullptr);
	q.dColPtr.upload(plan.colPtr, nullptr); q.dRowIdx.upload(plan.rowIdx, nullptr); q.dColOf.upload(plan.colOfTile, nullptr); q.dGPtr.upload(plan.gPtr, nullptr);
	q.dGather.upload(plan.gather, nullptr); q.dLvlTiles.upload(plan.wgRec, nullptr); q.dLvlCols.upload(plan.lvlCols, nullptr);
	q.dBlkTile.upload(plan.blkTile, nullptr); q.dPos.upload(plan.posOfSeg, nullptr);
	q.dTiles.resize((size_t)SC_TT * ((size_t)plan.nTiles + 1)); q.dTilesT.resize((size_t)SC_TT * plan.nTiles);
	q.dY.resize((size_t)SC_T * plan.T); q.dRinv.resize((size_t)SC_T * plan.T); q.dFail.resize(1);
	SparseChol& d = q.d;
	d.tiles = q.dTiles.data(); d.tilesT = q.dTilesT.data(); d.y = q.dY.data(); d.rinv = q.dRinv.data(); d.fail = q.dFail.data();
	d.colPtr = q.dColPtr.data(); d.rowIdx = q.dRowIdx.data(); d.colOfTile = q.dColOf.data(); d.gPtr = q.dGPtr.data(); d.gather = q.dGather.data();
	d.wgRec = q.dLvlTiles.data(); d.lvlCols = q.dLvlCols.data(); d.blkTile = q.dBlkTile.data(); d.posOfSeg = q.dPos.data();
	d.T = plan.T; d.Pf = P; d.nTiles = plan.nTiles;
	q.st.nblk = (int)q.blkrow.size(); q.st.hsc_blkrow = q.dRow.data(); q.st.hsc_colind = q.dCol.data();
	q.sys.hsc = q.dBlocks.data(); q.sys.bsc = q.dB.data();
	return true;
}
}  // namespace

extern "C" {

int cuba_hip_debug_dense_inverse(int device, int n, const double* A, double* Ainv)
{
	if (n <= 0 || !A || !Ainv) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (hipSetDevice(device) != hipSuccess) return CUBA_HIP_ERR_NO_DEVICE;
	try
	{
		const size_t nn = (size_t)n * n;
		std::vector<Scalar> h(A, A + nn);
		DevBuf<Scalar> w0, w1;
		w0.upload(h, nullptr); w1.resize(nn);
		DevBuf<Scalar> piv; piv.resize(2 * 32 * 32);
		Scalar* res = launch_dense_inverse(w0.data(), w1.data(), n, piv.data(), nullptr);
		launch_coarse_finish(res, res, n, nullptr);
		HIP_TRY(hipMemcpy(h.data(), res, sizeof(Scalar) * nn, hipMemcpyDeviceToHost));
		for (size_t i = 0; i < nn; i++) Ainv[i] = (double)h[i];
		return CUBA_HIP_OK;
	}
	catch (const HipError&) { return CUBA_HIP_ERR_RUNTIME; }
}

int cuba_hip_debug_dense_solve(int device, int n, const double* A, const double* b, double* x, int* not_positive_definite)
{
	return cuba_hip_debug_sparse_solve(device, n, A, b, x, not_positive_definite, -1, nullptr);
}

int cuba_hip_debug_sparse_solve(int device, int n, const double* A, const double* b, double* x, int* not_positive_definite, int slack, int32_t stats[4])
{
	if (n <= 0 || n % 6 != 0 || !A || !b || !x) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (hipSetDevice(device) != hipSuccess) return CUBA_HIP_ERR_NO_DEVICE;
	try
	{
		DebugSystem q;
		if (!debug_system(n, A, b, slack, stats, q)) return CUBA_HIP_ERR_RUNTIME;
		DevBuf<Scalar> dX; dX.resize(n);
		launch_sparse_chol_fill(q.st, q.sys, q.d, nullptr);
		launch_sparse_chol_solve(q.d, q.plan, dX.data(), nullptr);
		std::vector<Scalar> hx(n); int flag = 0;
		HIP_TRY(hipMemcpy(hx.data(), dX.data(), sizeof(Scalar) * n, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(&flag, q.dFail.data(), sizeof(int), hipMemcpyDeviceToHost));
		for (int i = 0; i < n; i++) x[i] = (double)hx[i];
		if (not_positive_definite) *not_positive_definite = flag;
		return CUBA_HIP_OK;
	}
	catch (const HipError&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (const std::exception&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (...) { return CUBA_HIP_ERR_RUNTIME; }
}

int cuba_hip_debug_selected_inverse(int device, int n, const double* A, double* sigma, int* not_positive_definite, int slack, int32_t stats[4])
{
	if (n <= 0 || n % 6 != 0 || !A || !sigma) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (sizeof(Scalar) != 8) return CUBA_HIP_ERR_INVALID_ARGUMENT;          // (as cuba_hip_compute_covariance in the fp32 library)
	if (hipSetDevice(device) != hipSuccess) return CUBA_HIP_ERR_NO_DEVICE;
	try
	{
		const size_t nn = (size_t)n * n;
		std::fill(sigma, sigma + nn, 0.0);
		if (not_positive_definite) *not_positive_definite = 0;
		const int P = n / 6;
		const std::vector<double> zeros(n, 0.0);
		DebugSystem q;
		if (!debug_system(n, A, zeros.data(), slack, stats, q)) return CUBA_HIP_ERR_RUNTIME;
		// cuba_hip_solver::computeCovariance's calls, in its order
		launch_sparse_chol_fill(q.st, q.sys, q.d, nullptr);
		launch_sparse_chol_factor(q.d, q.plan, nullptr);
		int flag = 0;
		HIP_TRY(hipMemcpy(&flag, q.dFail.data(), sizeof(int), hipMemcpyDeviceToHost));
		if (flag)
		{
			if (not_positive_definite) *not_positive_definite = 1;
			return CUBA_HIP_OK;
		}
		SelInvPlan sp;
		if (!selinv_plan(q.plan, sp)) return CUBA_HIP_ERR_RUNTIME;
		DevBuf<int> dSelInts; DevBuf<Scalar> dSigma, dPose, dBlk;
		SelInv v;
		upload_selinv_plan(sp, dSelInts, v, nullptr);
		// (all-ones bytes, a NaN: a tile, block or element the kernels should have written and did not shows up in the output)
		dSigma.resize((size_t)SC_TT * std::max(1, q.plan.nTiles)); dPose.resize((size_t)36 * P); dBlk.resize((size_t)36 * q.st.nblk);
		HIP_TRY(hipMemset(dSigma.data(), 0xff, sizeof(Scalar) * dSigma.size()));
		HIP_TRY(hipMemset(dPose.data(), 0xff, sizeof(Scalar) * dPose.size()));
		HIP_TRY(hipMemset(dBlk.data(), 0xff, sizeof(Scalar) * dBlk.size()));
		v.sigma = dSigma.data();
		launch_selinv(q.d, q.plan, sp, v, nullptr);
		launch_selinv_extract(q.st, q.d, v, dPose.data(), dBlk.data(), P, nullptr);
		std::vector<Scalar> hp(dPose.size()), hb(dBlk.size());
		HIP_TRY(hipMemcpy(hp.data(), dPose.data(), sizeof(Scalar) * hp.size(), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(hb.data(), dBlk.data(), sizeof(Scalar) * hb.size(), hipMemcpyDeviceToHost));
		// scattered as extracted (6 x 6 column-major blocks): the off-diagonal blocks of the pattern and their transposes, then the pose
		// blocks on the diagonal -- nothing symmetrised here, so a diagonal block shows the kernels' own symmetry
		for (int b = 0; b < q.st.nblk; b++)
		{
			const int bi = q.blkrow[b], bj = q.colind[b];
			if (bi == bj) continue;
			for (int c = 0; c < 6; c++)
				for (int r = 0; r < 6; r++)
				{
					const double val = (double)hb[36 * (size_t)b + 6 * c + r];
					sigma[(size_t)(6 * bj + c) * n + 6 * bi + r] = val;
					sigma[(size_t)(6 * bi + r) * n + 6 * bj + c] = val;
				}
		}
		for (int p = 0; p < P; p++)
			for (int c = 0; c < 6; c++)
				for (int r = 0; r < 6; r++) sigma[(size_t)(6 * p + c) * n + 6 * p + r] = (double)hp[36 * (size_t)p + 6 * c + r];
		return CUBA_HIP_OK;
	}
	catch (const HipError&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (const std::exception&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (...) { return CUBA_HIP_ERR_RUNTIME; }
}

}  // extern "C"

namespace
{
// the patterns the library itself hands to sparse_chol_plan (Hsc's h_rowptr / h_colind), and nothing else: rows that start at 0 and
// never shrink, each led by its own diagonal block, columns strictly increasing and below n_poses (sparse_chol_plan indexes by them)
bool pattern_ok(int n_poses, const int32_t* row_ptr, const int32_t* col_ind)
{
	if (row_ptr[0] != 0) return false;
	for (int i = 0; i < n_poses; i++)
	{
		if (row_ptr[i + 1] <= row_ptr[i] || col_ind[row_ptr[i]] != i) return false;
		for (int k = row_ptr[i] + 1; k < row_ptr[i + 1]; k++)
			if (col_ind[k] <= col_ind[k - 1] || col_ind[k] >= n_poses) return false;
	}
	return true;
}

// pose pairs (block_i = left, block_j = right) of a debug hook, packed as the handle packs a request of free poses
void debug_pack(const SparseCholPlan& plan, int n_pairs, const int32_t* block_i, const int32_t* block_j, PairRequest& rq)
{
	const std::vector<int> zeros((size_t)std::max(n_pairs, 1), 0), none;
	pair_pack(plan, n_pairs, zeros.data(), block_i, zeros.data(), block_j, none, none, rq);
}
}  // namespace

extern "C" {

int cuba_hip_debug_inverse_blocks(int device, int n, const double* A, int n_pairs, const int32_t* block_i, const int32_t* block_j, double* out,
	int* not_positive_definite, int slack, int32_t stats[4])
{
	if (n <= 0 || n % 6 != 0 || !A || n_pairs < 0 || (n_pairs > 0 && (!block_i || !block_j || !out))) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (sizeof(Scalar) != 8) return CUBA_HIP_ERR_INVALID_ARGUMENT;          // (as cuba_hip_compute_covariance_pairs in the fp32 library)
	const int P = n / 6;
	for (int k = 0; k < n_pairs; k++)
		if (block_i[k] < 0 || block_i[k] >= P || block_j[k] < 0 || block_j[k] >= P) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (hipSetDevice(device) != hipSuccess) return CUBA_HIP_ERR_NO_DEVICE;
	try
	{
		std::fill(out, out + (size_t)36 * n_pairs, 0.0);
		if (not_positive_definite) *not_positive_definite = 0;
		const std::vector<double> zeros(n, 0.0);
		DebugSystem q;
		if (!debug_system(n, A, zeros.data(), slack, stats, q)) return CUBA_HIP_ERR_RUNTIME;
		// cuba_hip_solver::computeCovariancePairs' calls, in its order
		launch_sparse_chol_fill(q.st, q.sys, q.d, nullptr);
		launch_sparse_chol_factor(q.d, q.plan, nullptr);
		int flag = 0;
		HIP_TRY(hipMemcpy(&flag, q.dFail.data(), sizeof(int), hipMemcpyDeviceToHost));
		if (flag)
		{
			if (not_positive_definite) *not_positive_definite = 1;
			return CUBA_HIP_OK;
		}
		PairRequest rq;
		debug_pack(q.plan, n_pairs, block_i, block_j, rq);
		size_t freeB = 0, totalB = 0;
		HIP_TRY(hipMemGetInfo(&freeB, &totalB));
		PairWork w;
		DevBuf<Scalar> dOut;
		dOut.resize((size_t)36 * std::max(n_pairs, 1));
		// (all-ones bytes, a NaN: an output the kernels should have written and did not shows up)
		HIP_TRY(hipMemset(dOut.data(), 0xff, sizeof(Scalar) * dOut.size()));
		const int chunks = run_covariance_pairs(q.d, q.plan, DeviceGraph(), DeviceSystem(), nullptr, rq, freeB / 2, w, dOut.data(), nullptr);
		(void)chunks;
		std::vector<Scalar> h((size_t)36 * n_pairs);
		if (n_pairs) HIP_TRY(hipMemcpy(h.data(), dOut.data(), sizeof(Scalar) * h.size(), hipMemcpyDeviceToHost));
		HIP_TRY(hipDeviceSynchronize());
		for (size_t i = 0; i < h.size(); i++) out[i] = (double)h[i];
		return CUBA_HIP_OK;
	}
	catch (const HipError&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (const std::exception&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (...) { return CUBA_HIP_ERR_RUNTIME; }
}

// The pair solve's symbolic phase alone (host only), all blocks in one chunk.  which: 0 header {blocks, slots, forward records, forward
// gather entries, backward records, backward gather entries}, 1 pairs {block, column, 0, 0}, 2 fwdPtr, 3 fwdCols, 4 bwdPtr, 5 bwdCols,
// 6 slotPtr, 7 slotCols, 8 fLvlPtr, 9 fRec, 10 fGather, 11 bLvlPtr, 12 bRec, 13 bGather
int cuba_hip_debug_pair_plan(int n_poses, const int32_t* row_ptr, const int32_t* col_ind, int slack, int n_pairs, const int32_t* block_i,
	const int32_t* block_j, int which, int32_t* out, size_t capacity, size_t* count)
{
	if (n_poses <= 0 || !row_ptr || !col_ind || !count || n_pairs < 0 || (n_pairs > 0 && (!block_i || !block_j))) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (which < 0 || which > 13) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (!pattern_ok(n_poses, row_ptr, col_ind)) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	for (int k = 0; k < n_pairs; k++)
		if (block_i[k] < 0 || block_i[k] >= n_poses || block_j[k] < 0 || block_j[k] >= n_poses) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	try
	{
		SparseCholPlan plan;
		if (!sparse_chol_plan(n_poses, row_ptr, col_ind, slack, (size_t)1 << 22, plan)) return CUBA_HIP_ERR_RUNTIME;
		PairRequest rq;
		debug_pack(plan, n_pairs, block_i, block_j, rq);
		PairPlan pl;
		if (!pair_plan(plan, rq, 0, rq.nBlocks, pl)) return CUBA_HIP_ERR_RUNTIME;
		std::vector<int> pairs((size_t)4 * n_pairs, 0);
		for (size_t r = 0; r < rq.pairRec.size(); r += 8)
		{
			const int k = rq.pairRec[r + 6];
			pairs[4 * (size_t)k] = rq.pairRec[r + 2]; pairs[4 * (size_t)k + 1] = rq.pairRec[r + 3];
		}
		const std::vector<int> header{ rq.nBlocks, (int)pl.slots(), (int)(pl.fRec.size() / 4), (int)(pl.fGather.size() / 2), (int)(pl.bRec.size() / 4),
			(int)(pl.bGather.size() / 2) };
		const std::vector<int>* src[] = { &header, &pairs, &pl.fwdPtr, &pl.fwdCols, &pl.bwdPtr, &pl.bwdCols, &pl.slotPtr, &pl.slotCols,
			&pl.fLvlPtr, &pl.fRec, &pl.fGather, &pl.bLvlPtr, &pl.bRec, &pl.bGather };
		*count = src[which]->size();
		if (out) std::memcpy(out, src[which]->data(), sizeof(int) * std::min(capacity, src[which]->size()));
		return CUBA_HIP_OK;
	}
	catch (const std::exception&) { return CUBA_HIP_ERR_RUNTIME; }
	catch (...) { return CUBA_HIP_ERR_RUNTIME; }
}

// The symbolic phase alone (host only: needs no device).  which: 0 header {T, nTiles, nLevels, slack, gather entries, nblk}, 1 posOfSeg,
// 2 colPtr, 3 rowIdx, 4 gPtr, 5 gather (4 ints per entry), 6 lvlPtr, 7 lvlTiles, 8 lvlColPtr, 9 lvlCols, 10 blkTile;
// the selected inversion's plan on top of it (SelInvPlan): 11 header {nLevels, off-diagonal tiles, gather entries, tile products (low,
// high 31 bits)}, 12 stepPtr, 13 offRec (4 ints per tile), 14 colStepPtr, 15 cols, 16 gather (2 ints per entry)
int cuba_hip_debug_sparse_plan(int n_poses, const int32_t* row_ptr, const int32_t* col_ind, int slack, int which, int32_t* out, size_t capacity, size_t* count)
{
	if (n_poses <= 0 || !row_ptr || !col_ind || !count) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (which < 0 || which > 16) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (!pattern_ok(n_poses, row_ptr, col_ind)) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	static thread_local SparseCholPlan plan;
	static thread_local SelInvPlan sel;
	static thread_local bool selValid = false;
	static thread_local std::vector<int> key;
	try
	{
		std::vector<int> k(row_ptr, row_ptr + n_poses + 1);
		k.insert(k.end(), col_ind, col_ind + row_ptr[n_poses]);
		k.push_back(slack);
		if (k != key)
		{
			key.clear(); selValid = false;
			if (!sparse_chol_plan(n_poses, row_ptr, col_ind, slack, (size_t)1 << 22, plan)) return CUBA_HIP_ERR_RUNTIME;
			key.swap(k);
		}
		if (which >= 11 && !selValid)
		{
			if (!selinv_plan(plan, sel)) return CUBA_HIP_ERR_RUNTIME;          // (a tile the recurrence needs is missing: a bug)
			selValid = true;
		}
		const std::vector<int> header{ plan.T, plan.nTiles, plan.nLevels, plan.slack, (int)(plan.gather.size() / 4), (int)plan.blkTile.size() };
		const std::vector<int> selHeader{ sel.nLevels, (int)(sel.offRec.size() / 4), (int)(sel.gather.size() / 2), (int)(sel.products & 0x7fffffff), (int)(sel.products >> 31) };
		const std::vector<int>* src[] = { &header, &plan.posOfSeg, &plan.colPtr, &plan.rowIdx, &plan.gPtr, &plan.gather, &plan.lvlPtr, &plan.lvlTiles,
			&plan.lvlColPtr, &plan.lvlCols, &plan.blkTile, &selHeader, &sel.stepPtr, &sel.offRec, &sel.colStepPtr, &sel.cols, &sel.gather };
		*count = src[which]->size();
		if (out) std::memcpy(out, src[which]->data(), sizeof(int) * std::min(capacity, src[which]->size()));
		return CUBA_HIP_OK;
	}
	catch (const std::exception&) { key.clear(); selValid = false; return CUBA_HIP_ERR_RUNTIME; }
	catch (...) { key.clear(); selValid = false; return CUBA_HIP_ERR_RUNTIME; }
}

// The PCG configuration in force (read-only): {agg, cl, nc, spmv_rows, upper, ell_m, ell_over, coarse inverse stored in fp32, row entries
// per thread of the upper-triangle row update (0 when that iteration is off)}, and the internal order of the free poses
int cuba_hip_debug_pcg_config(cuba_hip_solver* s, int32_t cfg[9], int32_t* pose_order, size_t capacity, size_t* count)
{
	return guarded(s, [&] {
		if (!cfg) throw ArgError{ "null output" };
		s->need();
		const DeviceSystem& y = s->sys;
		const int32_t v[9] = { y.agg, y.cl, y.nc, y.spmv_rows, y.upper, s->st.ell_m, s->st.ell_over, y.acinv32 != nullptr ? 1 : 0,
			y.upper ? pcg_rows_entries_per_thread(y) : 0 };
		std::memcpy(cfg, v, sizeof v);
		if (count) *count = s->poseOldOfNew.size();
		if (pose_order) std::memcpy(pose_order, s->poseOldOfNew.data(), sizeof(int32_t) * std::min(capacity, s->poseOldOfNew.size()));
	});
}

// The ring of decision records of the handle's last device-decided run (LM_RING x LM_REC doubles; zeros before its first run)
int cuba_hip_debug_lm_records(cuba_hip_solver* s, double* out, size_t capacity, size_t* count)
{
	return guarded(s, [&] {
		if (!count) throw ArgError{ "null output" };
		*count = (size_t)LM_RING * LM_REC;
		if (!out) return;
		s->sync();
		std::atomic_thread_fence(std::memory_order_acquire);
		for (size_t i = 0; i < std::min(capacity, *count); i++) out[i] = s->h_lmRing ? ((const volatile double*)s->h_lmRing)[i] : 0.0;
	});
}

// The decision kernels of a device-decided run on SCRIPTED sums, no handle and no graph: the start of a run (start_mode 0: the state as
// lmRunBegin's host branch writes it, from F0 and lam0; 1: launch_lm_run_init over chi_slots[NSLOT] and maxdiag_bits[64] with tau), then per
// trial t, in stream order, launch_reduce_report with a decision over the partial sums a[a_off[t], a_off[t + 1]) (landmark part of the
// denominator), b (chi2), c (pose part) -- or launch_lm_decide_failed where ok[t] == 0 -- and launch_restore_if_rejected on a scratch
// state / backup pair of scratch_count numbers.  Every trial is fed, whatever the host logic (LmRun::absorb, niter iterations) makes of
// the records.  out_start[10]: the 9 state numbers and the damping as the kernels read it after the start.  out[32 t ..]: [0, 9) state,
// [9, 17) the trial's ring record, 17 the damping as the kernels read it, 18..20 the three sums from their slot groups, 21 slots 1..NSLOT-1
// of the three groups all zero (-1: a failed trial has no sums), 22 scratch state == backup, 23 scratch state as it was before the trial,
// 24 the host absorbed the record (0: it had stopped before; -1: the record's tag was not the trial's), 25 done, 26 stop, 27 rejRun,
// 28 a chi2 was written for this trial, 29 that chi2, 30 the host's damping, 31 the host's F
int cuba_hip_debug_lm_script(int device, int start_mode, double F0, double lam0, const double* chi_slots, const uint64_t* maxdiag_bits, double tau, double tag_base,
	int niter, int n_trials, const int32_t* ok, const double* a, const int32_t* a_off, const double* b, const int32_t* b_off, const double* c, const int32_t* c_off,
	size_t scratch_count, double* out_start, double* out)
{
	constexpr int MAX_TRIALS = 512, MAX_PARTS = 1 << 16, GUARD = 64, STRIDE = 32;
	constexpr size_t MAX_SCRATCH = (size_t)1 << 20;
	if (start_mode < 0 || start_mode > 1 || n_trials < 0 || n_trials > MAX_TRIALS || niter < 0 || niter > MAX_TRIALS) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (!out_start || (n_trials > 0 && (!ok || !a_off || !b_off || !c_off || !out))) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (start_mode == 1 && (!chi_slots || !maxdiag_bits)) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (scratch_count > MAX_SCRATCH) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	if (!(tag_base >= 0 && tag_base <= 9e15)) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	const int32_t* offs[3] = { a_off, b_off, c_off };
	const double* src[3] = { a, b, c };
	for (int k = 0; k < 3 && n_trials > 0; k++)
	{
		if (offs[k][0] != 0) return CUBA_HIP_ERR_INVALID_ARGUMENT;
		for (int t = 0; t < n_trials; t++)
			if (offs[k][t + 1] < offs[k][t] || offs[k][t + 1] - offs[k][t] > MAX_PARTS) return CUBA_HIP_ERR_INVALID_ARGUMENT;
		if (offs[k][n_trials] > 0 && !src[k]) return CUBA_HIP_ERR_INVALID_ARGUMENT;
	}
	if (hipSetDevice(device) != hipSuccess) return CUBA_HIP_ERR_NO_DEVICE;
	double* ringHost = nullptr;
	try
	{
		hipStream_t st = nullptr;
		DevBuf<double> dState; dState.resize(16); dState.zero(st);
		DevBuf<Scalar> dLam; dLam.resize(1); dLam.zero(st);
		DevBuf<Scalar> dSlots; dSlots.resize(4 * NSLOT);
		DevBuf<Scalar> dParts; dParts.resize(3 * (size_t)MAX_PARTS + 4 * GUARD);
		DevBuf<Scalar> dScratch, dBackup;
		HIP_TRY(hipHostMalloc((void**)&ringHost, sizeof(double) * LM_RING * LM_REC, hipHostMallocMapped | hipHostMallocCoherent));
		std::memset(ringHost, 0, sizeof(double) * LM_RING * LM_REC);
		LmDevice lm; lm.state = dState.data(); lm.lam = dLam.data();
		HIP_TRY(hipHostGetDevicePointer((void**)&lm.ring, ringHost, 0));
		const DeviceSystem sys{};                       // (host_flags null: nothing is published)
		cuba_hip_solver::LmRun r;
		r.niter = niter; r.stop = niter <= 0; r.tagBase = tag_base; r.lm = lm;
		std::vector<double> chi2((size_t)std::max(niter, 1), 0.0);
		r.chi2Out = chi2.data();
		if (start_mode == 1)
		{
			std::vector<Scalar> hs(chi_slots, chi_slots + NSLOT);
			DevBuf<Scalar> dChi; dChi.upload(hs, st);
			DevBuf<unsigned long long> dMax; dMax.resize(64);
			HIP_TRY(hipMemcpyAsync(dMax.data(), maxdiag_bits, sizeof(unsigned long long) * 64, hipMemcpyHostToDevice, st));
			launch_lm_run_init(dChi.data(), dMax.data(), lm, tau, tag_base, cuba_hip_solver::LmRun::maxq, st);
			HIP_TRY(hipStreamSynchronize(st));
		}
		else
		{
			const double st9[9] = { F0, lam0, 2.0, 0.0, 0.0, 1.0, 0.0, (double)cuba_hip_solver::LmRun::maxq, tag_base };
			const Scalar l1 = (Scalar)lam0;
			HIP_TRY(hipMemcpy(dState.data(), st9, sizeof st9, hipMemcpyHostToDevice));
			HIP_TRY(hipMemcpy(dLam.data(), &l1, sizeof l1, hipMemcpyHostToDevice));
			r.F = F0; r.lam = lam0;
		}
		{
			Scalar l1 = 0;
			HIP_TRY(hipMemcpy(out_start, dState.data(), sizeof(double) * 9, hipMemcpyDeviceToHost));
			HIP_TRY(hipMemcpy(&l1, dLam.data(), sizeof l1, hipMemcpyDeviceToHost));
			out_start[9] = (double)l1;
		}
		std::vector<Scalar> hScratch(scratch_count), hBackup(scratch_count), hGot(scratch_count), hParts, hSlots(4 * NSLOT);
		for (size_t i = 0; i < scratch_count; i++) { hScratch[i] = (Scalar)(1 + i % 251); hBackup[i] = -(Scalar)(1 + i % 127); }
		dBackup.upload(hBackup, st);
		for (int t = 0; t < n_trials; t++)
		{
			double* o = out + (size_t)STRIDE * t;
			std::fill(o, o + STRIDE, 0.0);
			dScratch.upload(hScratch, st);
			if (ok[t])
			{
				// [guard | a | guard | b | guard | c | guard]: a read outside an array changes its total
				const int n[3] = { a_off[t + 1] - a_off[t], b_off[t + 1] - b_off[t], c_off[t + 1] - c_off[t] };
				hParts.assign((size_t)n[0] + n[1] + n[2] + 4 * GUARD, (Scalar)1048576);
				size_t at[3], pos = GUARD;
				for (int k = 0; k < 3; k++)
				{
					at[k] = pos;
					for (int i = 0; i < n[k]; i++) hParts[pos + i] = (Scalar)src[k][offs[k][t] + i];
					pos += (size_t)n[k] + GUARD;
				}
				HIP_TRY(hipMemcpyAsync(dParts.data(), hParts.data(), sizeof(Scalar) * hParts.size(), hipMemcpyHostToDevice, st));
				std::fill(hSlots.begin(), hSlots.end(), (Scalar)77);
				HIP_TRY(hipMemcpyAsync(dSlots.data(), hSlots.data(), sizeof(Scalar) * hSlots.size(), hipMemcpyHostToDevice, st));
				launch_reduce_report(sys, dParts.data() + at[0], n[0], dSlots.data() + NSLOT, dParts.data() + at[1], n[1], dSlots.data(),
					dParts.data() + at[2], n[2], dSlots.data() + 3 * NSLOT, &lm, 0, st);
			}
			else launch_lm_decide_failed(sys, lm, st);
			launch_restore_if_rejected(dScratch.data(), dBackup.data(), scratch_count, lm, st);
			HIP_TRY(hipStreamSynchronize(st));
			HIP_TRY(hipMemcpy(o, dState.data(), sizeof(double) * 9, hipMemcpyDeviceToHost));
			std::atomic_thread_fence(std::memory_order_acquire);
			const volatile double* rec = ringHost + (size_t)(t % LM_RING) * LM_REC;
			for (int i = 0; i < LM_REC; i++) o[9 + i] = rec[i];
			Scalar l1 = 0;
			HIP_TRY(hipMemcpy(&l1, dLam.data(), sizeof l1, hipMemcpyDeviceToHost));
			o[17] = (double)l1;
			if (ok[t])
			{
				HIP_TRY(hipMemcpy(hSlots.data(), dSlots.data(), sizeof(Scalar) * hSlots.size(), hipMemcpyDeviceToHost));
				o[18] = (double)hSlots[NSLOT]; o[19] = (double)hSlots[0]; o[20] = (double)hSlots[3 * NSLOT];
				bool zero = true;
				for (int g = 0; g < 4; g++)
					for (int i = 1; i < NSLOT; i++) if (g != 2 && hSlots[g * NSLOT + i] != Scalar(0)) zero = false;
				o[21] = zero ? 1.0 : 0.0;
			}
			else o[21] = -1.0;
			if (scratch_count) HIP_TRY(hipMemcpy(hGot.data(), dScratch.data(), sizeof(Scalar) * scratch_count, hipMemcpyDeviceToHost));
			o[22] = hGot == hBackup ? 1.0 : 0.0;
			o[23] = hGot == hScratch ? 1.0 : 0.0;
			if (!r.stop && r.seen == t)
			{
				const int doneBefore = r.done;
				if (!r.absorb(rec)) o[24] = -1.0;
				else
				{
					o[24] = 1.0;
					if (r.done > doneBefore) { o[28] = 1.0; o[29] = chi2[doneBefore]; }
				}
			}
			o[25] = r.done; o[26] = r.stop ? 1.0 : 0.0; o[27] = r.rejRun; o[30] = r.lam; o[31] = r.F;
		}
		(void)hipHostFree(ringHost);
		return CUBA_HIP_OK;
	}
	catch (const HipError&) { if (ringHost) (void)hipHostFree(ringHost); return CUBA_HIP_ERR_RUNTIME; }
	catch (const std::exception&) { if (ringHost) (void)hipHostFree(ringHost); return CUBA_HIP_ERR_RUNTIME; }
	catch (...) { if (ringHost) (void)hipHostFree(ringHost); return CUBA_HIP_ERR_RUNTIME; }
}

int cuba_hip_begin_run(cuba_hip_solver* s)
{
	return guarded(s, [&] { s->need(); s->coarseValid = false; s->startRunHistory(); });
}

int cuba_hip_get_stream(cuba_hip_solver* s, void** hip_stream)
{
	return guarded(s, [&] { if (!hip_stream) throw ArgError{ "null output" }; *hip_stream = (void*)s->stream; });
}

int cuba_hip_evaluate_device(cuba_hip_solver* s, double lambda, int with_scale, void** device_scalars3)
{
	return guarded(s, [&] {
		s->need();
		if (!device_scalars3) throw ArgError{ "null output" };
		s->d_eval.resize(4);
		launch_residual_chi2(s->g, s->d_parts.data(), s->slotsDev, nullptr, s->stream, s->factors());
		if (with_scale) launch_pose_scale(s->g, s->sys, lambda, s->slotsDev + 3 * NSLOT, s->stream);
		launch_collect_eval(s->sys, s->d_eval.data(), s->stream);
		*device_scalars3 = s->d_eval.data();
	});
}

int cuba_hip_reduction_buffer(cuba_hip_solver* s, void** device_ptr, size_t* count)
{
	return guarded(s, [&] {
		s->need();
		if (device_ptr) *device_ptr = s->d_red.data();
		if (count) *count = s->d_red.size();
	});
}

}  // extern "C"
