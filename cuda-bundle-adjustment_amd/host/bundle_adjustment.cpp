// bundle_adjustment.cpp -- host C++ layer: cuba::CudaBundleAdjustment implemented over the C ABI
// (include/cuba_hip.h).  Plain C++17, no HIP headers: everything device-side happens behind the ABI.
//
// Behavioural counterpart of CudaBundleAdjustmentImpl and of the host half of CudaBlockSolver
// (/root/reference/src/cuda_bundle_adjustment.cpp:115-261 initialize, :512-543 finalize/getChiSqs,
// :677-903 graph containers + LM entry).  Differences, all deliberate:
//   * edges are kept in insertion order (the reference iterates unordered_sets, so its edge order and
//     hence its last-bit results change from run to run);
//   * the device handle is created lazily in optimize(), so graph editing and initialize() work on a
//     machine without a GPU;
//   * failures raise std::runtime_error instead of being printed and ignored.

#include "cuda_bundle_adjustment.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <cstddef>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "cuba_hip.h"
#include "../csrc/host_pool.hpp"

namespace cuba
{
namespace
{

// Staging arrays that cross the C ABI live in page-locked memory (cuba_hip_host_alloc; plain malloc without a device): the
// 18 MB of measurements a KITTI-00-sized initialize() hands over then move at full PCIe rate.
template <class T>
struct PinnedAllocator
{
	using value_type = T;
	PinnedAllocator() = default;
	template <class U> PinnedAllocator(const PinnedAllocator<U>&) {}
	T* allocate(size_t n)
	{
		void* p = cuba_hip_host_alloc(n * sizeof(T));
		if (!p) throw std::bad_alloc();
		return static_cast<T*>(p);
	}
	void deallocate(T* p, size_t) { cuba_hip_host_free(p); }
	template <class U> bool operator==(const PinnedAllocator<U>&) const { return true; }
	template <class U> bool operator!=(const PinnedAllocator<U>&) const { return false; }
};
template <class T> using PinnedVector = std::vector<T, PinnedAllocator<T>>;

const char* const kProfileKeys[CUBA_HIP_PROFILE_ITEMS] = {
	"0: Initialize Optimizer", "1: Build Structure", "2: Compute Error", "3: Build System",
	"4: Schur Complement", "5: Symbolic Decomposition", "6: Numerical Decomposition", "7: Update Solution"
};

// insertion-ordered pointer set: dense vector (erased slots become null) + hash index, so that the linear sweep in
// initialize() touches contiguous memory
template <class T>
class OrderedSet
{
public:
	bool insert(T* p)
	{
		if (!index_.emplace(p, items_.size()).second) return false;
		items_.push_back(p);
		return true;
	}
	bool erase(T* p)
	{
		auto it = index_.find(p);
		if (it == index_.end()) return false;
		items_[it->second] = nullptr;
		index_.erase(it);
		return true;
	}
	bool contains(T* p) const { return index_.count(p) != 0; }
	size_t size() const { return index_.size(); }
	void clear() { index_.clear(); items_.clear(); }
	const std::vector<T*>& slots() const { return items_; }   // may contain nullptr
private:
	std::unordered_map<T*, size_t> index_;
	std::vector<T*> items_;
};

// ---- the factor kinds -------------------------------------------------------------------------------
// Everything the host layer does with a factor exists once (HipBundleAdjustment: addFactor, upload, readChiSquares, dropFactorsOf,
// clear; below the class: the three public functions of every kind); FactorKind<F> holds what is a kind's own:
//   fn, noun, ofA   "cuba::addX", "a factor" / "an edge" / "a prior" and "a factor" / ..., for the messages
//   kernelType      -1: kind | delta travel inside the setter (null | null when no factor has a kernel); otherwise the factor type
//                   under which cuba_hip_set_pose_factor_robust_kernels takes them after the setter, and only when some factor has one
//   inBlockPattern  its pose pairs are part of the reduced matrix's pattern: on a graph upload the set goes up again before
//                   cuba_hip_build_structure
//   set             fields -> flat arrays -> the C setter; setName, chiSquares, chiName: the setter's name and the chi2 reader
// What a factor hangs on -- one pose, one landmark, two different poses -- is read off its struct (`vertex`, or `vertexI` and `vertexJ`).
// A new kind: its struct in the header, its FactorKind and its place in FactorLists here, its three public functions at the end of the file.
template <class F> struct FactorKind;

template <class F> auto ends(const F& f) -> std::array<decltype(F::vertex), 1> { return { f.vertex }; }
template <class F> auto ends(const F& f) -> std::array<decltype(F::vertexI), 2> { return { f.vertexI, f.vertexJ }; }
template <class V, size_t N> bool distinctVertices(const std::array<V*, N>& e) { return e.front() && e.back() && (N == 1 || e.front() != e.back()); }
inline const char* whatItNeeds(const std::array<PoseVertex*, 1>&) { return "a pose vertex"; }
inline const char* whatItNeeds(const std::array<LandmarkVertex*, 1>&) { return "a landmark vertex"; }
inline const char* whatItNeeds(const std::array<PoseVertex*, 2>&) { return "two different pose vertices"; }

// one field of every factor of a set as the C ABI takes it, factor after factor
struct Values { const double* p; size_t n; };
template <size_t N> Values values(const std::array<double, N>& a) { return { a.data(), N }; }
inline Values values(const double& x) { return { &x, 1 }; }
inline Values values(const Array<double, 3>& v) { return { v.data(), 3 }; }
inline Values values(const PoseVertex::Rotation& q) { return { q.coeffs().data(), 4 }; }       // (x, y, z, w)
template <class F, class M> std::vector<double> column(const std::vector<F*>& factors, M F::* field)
{
	const size_t w = factors.empty() ? 0 : values(factors[0]->*field).n;
	std::vector<double> a(w * factors.size());
	for (size_t k = 0; k < factors.size(); k++) std::copy_n(values(factors[k]->*field).p, w, a.begin() + w * k);
	return a;
}

template <> struct FactorKind<PosePrior>
{
	static constexpr const char* fn = "cuba::addPosePrior", *noun = "a prior", *ofA = "a prior";
	static constexpr int kernelType = 0;
	static constexpr bool inBlockPattern = false;
	static constexpr const char* setName = "cuba_hip_set_pose_priors", *chiName = "cuba_hip_prior_chi_squares";
	static constexpr auto chiSquares = cuba_hip_prior_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<PosePrior*>& f, const int32_t* pose, const int32_t*, const int32_t*, const double*)
	{
		return cuba_hip_set_pose_priors(s, (int)f.size(), pose, column(f, &PosePrior::q).data(), column(f, &PosePrior::t).data(), column(f, &PosePrior::information).data());
	}
};
template <> struct FactorKind<RelativePoseEdge>
{
	static constexpr const char* fn = "cuba::addRelativePoseEdge", *noun = "an edge", *ofA = "a relative-pose edge";
	static constexpr int kernelType = 1;
	static constexpr bool inBlockPattern = true;
	static constexpr const char* setName = "cuba_hip_set_relative_pose_edges", *chiName = "cuba_hip_relative_pose_chi_squares";
	static constexpr auto chiSquares = cuba_hip_relative_pose_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<RelativePoseEdge*>& f, const int32_t* pi, const int32_t* pj, const int32_t*, const double*)
	{
		return cuba_hip_set_relative_pose_edges(s, (int)f.size(), pi, pj, column(f, &RelativePoseEdge::q).data(), column(f, &RelativePoseEdge::t).data(),
			column(f, &RelativePoseEdge::information).data());
	}
};
template <> struct FactorKind<LandmarkPrior>
{
	static constexpr const char* fn = "cuba::addLandmarkPrior", *noun = "a prior", *ofA = "a prior";
	static constexpr int kernelType = -1;
	static constexpr bool inBlockPattern = false;
	static constexpr const char* setName = "cuba_hip_set_landmark_priors", *chiName = "cuba_hip_landmark_prior_chi_squares";
	static constexpr auto chiSquares = cuba_hip_landmark_prior_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<LandmarkPrior*>& f, const int32_t* lm, const int32_t*, const int32_t* kind, const double* delta)
	{
		return cuba_hip_set_landmark_priors(s, (int)f.size(), lm, column(f, &LandmarkPrior::position).data(), column(f, &LandmarkPrior::information).data(), kind, delta);
	}
};
template <> struct FactorKind<PositionFactor>
{
	static constexpr const char* fn = "cuba::addPositionFactor", *noun = "a factor", *ofA = "a factor";
	static constexpr int kernelType = -1;
	static constexpr bool inBlockPattern = false;
	static constexpr const char* setName = "cuba_hip_set_position_factors", *chiName = "cuba_hip_position_factor_chi_squares";
	static constexpr auto chiSquares = cuba_hip_position_factor_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<PositionFactor*>& f, const int32_t* pose, const int32_t*, const int32_t* kind, const double* delta)
	{
		return cuba_hip_set_position_factors(s, (int)f.size(), pose, column(f, &PositionFactor::position).data(), column(f, &PositionFactor::leverArm).data(),
			column(f, &PositionFactor::information).data(), kind, delta);
	}
};
template <> struct FactorKind<DirectionFactor>
{
	static constexpr const char* fn = "cuba::addDirectionFactor", *noun = "a factor", *ofA = "a factor";
	static constexpr int kernelType = -1;
	static constexpr bool inBlockPattern = false;
	static constexpr const char* setName = "cuba_hip_set_direction_factors", *chiName = "cuba_hip_direction_factor_chi_squares";
	static constexpr auto chiSquares = cuba_hip_direction_factor_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<DirectionFactor*>& f, const int32_t* pose, const int32_t*, const int32_t* kind, const double* delta)
	{
		return cuba_hip_set_direction_factors(s, (int)f.size(), pose, column(f, &DirectionFactor::worldDirection).data(), column(f, &DirectionFactor::measurement).data(),
			column(f, &DirectionFactor::information).data(), kind, delta);
	}
};
template <> struct FactorKind<RangeFactor>
{
	static constexpr const char* fn = "cuba::addRangeFactor", *noun = "a factor", *ofA = "a factor";
	static constexpr int kernelType = -1;
	static constexpr bool inBlockPattern = false;
	static constexpr const char* setName = "cuba_hip_set_range_factors", *chiName = "cuba_hip_range_factor_chi_squares";
	static constexpr auto chiSquares = cuba_hip_range_factor_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<RangeFactor*>& f, const int32_t* pose, const int32_t*, const int32_t* kind, const double* delta)
	{
		return cuba_hip_set_range_factors(s, (int)f.size(), pose, column(f, &RangeFactor::anchor).data(), column(f, &RangeFactor::range).data(),
			column(f, &RangeFactor::leverArm).data(), column(f, &RangeFactor::information).data(), kind, delta);
	}
};
template <> struct FactorKind<PoseRangeFactor>
{
	static constexpr const char* fn = "cuba::addPoseRangeFactor", *noun = "a factor", *ofA = "a factor";
	static constexpr int kernelType = -1;
	static constexpr bool inBlockPattern = true;
	static constexpr const char* setName = "cuba_hip_set_pose_range_factors", *chiName = "cuba_hip_pose_range_factor_chi_squares";
	static constexpr auto chiSquares = cuba_hip_pose_range_factor_chi_squares;
	static int set(cuba_hip_solver* s, const std::vector<PoseRangeFactor*>& f, const int32_t* pi, const int32_t* pj, const int32_t* kind, const double* delta)
	{
		return cuba_hip_set_pose_range_factors(s, (int)f.size(), pi, pj, column(f, &PoseRangeFactor::range).data(), column(f, &PoseRangeFactor::leverArmI).data(),
			column(f, &PoseRangeFactor::leverArmJ).data(), column(f, &PoseRangeFactor::information).data(), kind, delta);
	}
};

// the factors of one kind as an object keeps them
template <class F>
struct FactorList
{
	using Kind = FactorKind<F>;
	std::vector<F*> items, uploaded;      // in the caller's order; the set the last initialize() handed to the device
	std::map<const F*, double> chi;       // per object of `uploaded`, from the last optimize()
	bool onDevice = false, dirty = false;
	void add(F* f) { if (std::find(items.begin(), items.end(), f) == items.end()) items.push_back(f); }
	void remove(F* f) { items.erase(std::remove(items.begin(), items.end(), f), items.end()); }
	template <class Pred> void removeIf(Pred&& pred) { items.erase(std::remove_if(items.begin(), items.end(), pred), items.end()); }
	double chiSquared(const F* f) const
	{
		const auto it = chi.find(f);
		return it == chi.end() ? 0.0 : it->second;
	}
	// an upload's first and last step; false: nothing to send (sent already, or no such factors now nor at the last initialize(), which
	// would have to be cleared on the device)
	bool beginUpload()
	{
		if (!dirty) return false;
		dirty = false;
		chi.clear();
		uploaded.clear();
		return !items.empty() || onDevice;
	}
	void endUpload() { onDevice = !items.empty(); uploaded = items; }
	// after optimize(): read(out[uploaded.size()]) fetches the chi2 of the uploaded set
	template <class Read> void readChi(Read&& read)
	{
		if (uploaded.empty()) return;
		std::vector<double> c(uploaded.size());
		read(c.data());
		for (size_t k = 0; k < c.size(); k++) chi[uploaded[k]] = c[k];
	}
};

// All kinds of an object.  The order of this tuple is the order of the C ABI calls, and part of the contract (tests/golden/host_factor_calls.txt):
//   on a graph upload  the kinds in the block pattern -- relative-pose edges, range factors between poses -- before the structure build;
//   before every solve all kinds: priors, relative-pose edges, landmark priors, position, direction, range, pose range (a set that went
//                      up already, or is empty on both sides, sends nothing);
//   after a solve      the chi2 of the kinds outside the block pattern, then of those in it.
using FactorLists = std::tuple<FactorList<PosePrior>, FactorList<RelativePoseEdge>, FactorList<LandmarkPrior>, FactorList<PositionFactor>,
	FactorList<DirectionFactor>, FactorList<RangeFactor>, FactorList<PoseRangeFactor>>;

class HipBundleAdjustment final : public CudaBundleAdjustment
{
public:
	~HipBundleAdjustment() override
	{
		if (solver_) cuba_hip_destroy(solver_);
	}

	// ---- graph editing (ref :681-764) -----------------------------------------------------------
	void addPoseVertex(PoseVertex* v) override { poses_.insert({ v->id, v }); posesDirty_ = true; }
	void addLandmarkVertex(LandmarkVertex* v) override { landmarks_.insert({ v->id, v }); landmarksDirty_ = true; }

	void addMonocularEdge(MonoEdge* e) override
	{
		mono_.insert(e); edgesDirty_ = true;
		e->vertexP->edges.insert(e);
		e->vertexL->edges.insert(e);
	}

	void addStereoEdge(StereoEdge* e) override
	{
		stereo_.insert(e); edgesDirty_ = true;
		e->vertexP->edges.insert(e);
		e->vertexL->edges.insert(e);
	}

	PoseVertex* poseVertex(int id) const override { return poses_.at(id); }
	LandmarkVertex* landmarkVertex(int id) const override { return landmarks_.at(id); }

	void removePoseVertex(PoseVertex* v) override
	{
		auto it = poses_.find(v->id);
		if (it == poses_.end()) return;
		const std::vector<BaseEdge*> incident(it->second->edges.begin(), it->second->edges.end());
		for (BaseEdge* e : incident) removeEdge(e);
		dropFactorsOf(it->second);
		poses_.erase(it);
		posesDirty_ = true;
	}

	void removeLandmarkVertex(LandmarkVertex* v) override
	{
		auto it = landmarks_.find(v->id);
		if (it == landmarks_.end()) return;
		const std::vector<BaseEdge*> incident(it->second->edges.begin(), it->second->edges.end());
		for (BaseEdge* e : incident) removeEdge(e);
		dropFactorsOf(it->second);
		landmarks_.erase(it);
		landmarksDirty_ = true;
	}

	void removeEdge(BaseEdge* e) override
	{
		if (PoseVertex* p = e->poseVertex()) p->edges.erase(e);
		if (LandmarkVertex* l = e->landmarkVertex()) l->edges.erase(e);
		edgesDirty_ = true;
		if (inactiveEdges_.erase(e)) maskDirty_ = true;          // (the level leaves with the edge)
		if (e->dim() == 2) mono_.erase(static_cast<MonoEdge*>(e));
		else if (e->dim() == 3) stereo_.erase(static_cast<StereoEdge*>(e));
	}

	size_t nposes() const override { return poses_.size(); }
	size_t nlandmarks() const override { return landmarks_.size(); }
	size_t nedges() const override { return mono_.size() + stereo_.size(); }

	void setRobustKernels(RobustKernelType kernelType, double delta, EdgeType edgeType) override
	{
		const int et = static_cast<int>(edgeType);
		if (et < 0 || et >= 2) throw std::invalid_argument("setRobustKernels: bad edge type");
		robustKind_[et] = static_cast<int>(kernelType);
		robustDelta_[et] = delta;
	}

	// ---- initialize: graph -> solver-order flat arrays (ref CudaBlockSolver::initialize :115-261) ----
	void initialize() override
	{
		covPoseIndex_.clear(); covLmIndex_.clear();          // (marginal covariances describe the graph they were computed on)
		forEachKind([](auto& list) { list.dirty = true; });      // (the factors as they stand now go to the device with the next solve)
		poseIdx_.clear(); landmarkIdx_.clear();              // (the factors' vertex indices: rebuilt from the vertices active now by the first factor that asks)
		const auto t0 = std::chrono::steady_clock::now();
		static const bool dbg = std::getenv("CUBA_HIP_DEBUG") != nullptr;
		auto tl = t0;
		auto lap = [&](const char* what) {
			if (!dbg) return;
			const auto now = std::chrono::steady_clock::now();
			std::fprintf(stderr, "[cuba host]   initialize: %-22s %7.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - tl).count());
			tl = now;
		};
		// (results of the previous optimize() stay queryable: when the edge list is rebuilt below, the old one is set aside
		// -- a move -- instead of being indexed here: the index over 561 k edges costs more than the rest of initialize())
		// the previous flattening is kept for comparison: when neither the edge set nor the active vertices (and their
		// free / fixed split) changed, the edge -> vertex indices are still right and only the values are read again
		std::vector<PoseVertex*> prevPoses;
		std::vector<LandmarkVertex*> prevLandmarks;
		prevPoses.swap(activePoses_); prevLandmarks.swap(activeLandmarks_);
		const int prevFreeP = numFreePoses_, prevFreeL = numFreeLandmarks_;

		// vertices in id order (the reference walks its std::maps), free ones first, vertices without edges left out
		// (ref :128-200).  The id-ordered pointer lists are cached between calls as long as no vertex was added or
		// removed, and the sweep over them (one dependent load per vertex) is split over a few host threads.
		// (no vertex and no edge added or removed since the last call: the active lists can only have changed through `fixed` flags,
		// which the single-pass variant of indexVertices checks while it reads the values)
		const bool stableP = !posesDirty_ && !edgesDirty_ && !prevPoses.empty(), stableL = !landmarksDirty_ && !edgesDirty_ && !prevLandmarks.empty();
		if (posesDirty_) { poseList_.clear(); for (const auto& kv : poses_) poseList_.push_back(kv.second); posesDirty_ = false; }
		if (landmarksDirty_) { landmarkList_.clear(); for (const auto& kv : landmarks_) landmarkList_.push_back(kv.second); landmarksDirty_ = false; }
		numFreePoses_ = indexVertices(poseList_, activePoses_, stableP ? &prevPoses : nullptr, prevFreeP, [&](size_t n) { q_.resize(4 * n); t_.resize(3 * n); cam_.resize(5 * n); },
			[&](PoseVertex* v, size_t i) {
				v->iP = static_cast<int>(i);
				const double* qc = v->q.coeffs().data();       // (x, y, z, w)
				std::copy(qc, qc + 4, q_.begin() + 4 * i);
				std::copy(v->t.data(), v->t.data() + 3, t_.begin() + 3 * i);
				const double c[5] = { v->camera.fx, v->camera.fy, v->camera.cx, v->camera.cy, v->camera.bf };
				std::copy(c, c + 5, cam_.begin() + 5 * i);
			});
		lap("poses");
		numFreeLandmarks_ = indexVertices(landmarkList_, activeLandmarks_, stableL ? &prevLandmarks : nullptr, prevFreeL, [&](size_t n) { Xw_.resize(3 * n); },
			[&](LandmarkVertex* v, size_t i) {
				v->iL = static_cast<int>(i);
				std::copy(v->Xw.data(), v->Xw.data() + 3, Xw_.begin() + 3 * i);
			});
		// edges: mono first, then stereo, insertion order inside each type; edges with both ends fixed are inactive
		// (ref :204-243).  561 k edges mean 561 k dependent pointer loads (edge -> vertex -> index), so the sweep is
		// split over a few host threads: count the active edges per chunk, prefix-sum, fill.
		lap("landmarks");
		const bool sameTopology = !edgesDirty_ && !activeEdges_.empty() && prevFreeP == numFreePoses_ && prevFreeL == numFreeLandmarks_ &&
			prevPoses == activePoses_ && prevLandmarks == activeLandmarks_;
		lap("same-topology check");
		if (sameTopology)
		{
			// the values are re-read from the caller's edge objects (they are the caller's to change); whether any of them differs from
			// what the device already holds falls out of the copy, and saves the library 32 bytes per edge of PCIe when none does
			const size_t nAct = activeEdges_.size();
			const unsigned T = hostThreads(nAct);
			std::atomic<int> changed{ 0 };
			forThreads(T, [&](unsigned t) {
				const size_t oEnd = nAct * (t + 1) / T;
				bool diff = false;
				for (size_t o = nAct * t / T; o < oEnd; o++)
				{
					// every edge object is its own cache miss: keep a dozen of them in flight
					if (o + kPrefetch < oEnd) { const char* nx = reinterpret_cast<const char*>(activeEdges_[o + kPrefetch]); __builtin_prefetch(nx); __builtin_prefetch(nx + 64); }
					double m0, m1, m2, w;
					if (edgeDim_[o] == 2)
					{
						const MonoEdge* m = static_cast<const MonoEdge*>(activeEdges_[o]);
						m0 = m->measurement[0]; m1 = m->measurement[1]; m2 = 0.0; w = m->information;
					}
					else
					{
						const StereoEdge* m = static_cast<const StereoEdge*>(activeEdges_[o]);
						m0 = m->measurement[0]; m1 = m->measurement[1]; m2 = m->measurement[2]; w = m->information;
					}
					// (bitwise: a NaN that stays a NaN is "unchanged", -0.0 vs 0.0 is a change)
					diff |= std::memcmp(&meas_[3 * o], &m0, 8) != 0 || std::memcmp(&meas_[3 * o + 1], &m1, 8) != 0 || std::memcmp(&meas_[3 * o + 2], &m2, 8) != 0 ||
						std::memcmp(&omega_[o], &w, 8) != 0;
					meas_[3 * o] = m0; meas_[3 * o + 1] = m1; meas_[3 * o + 2] = m2; omega_[o] = w;
				}
				if (diff) changed.store(1, std::memory_order_relaxed);
			});
			if (changed.load()) valuesChangedSinceUpload_ = true;      // (several initialize() calls may pass before the next upload)
		}
		else
		{
		const auto& ms = mono_.slots();
		const auto& ss = stereo_.slots();
		const size_t nM = ms.size(), nAll = nM + ss.size();
		auto edgeAt = [&](size_t k) -> BaseEdge* { return k < nM ? static_cast<BaseEdge*>(ms[k]) : static_cast<BaseEdge*>(ss[k - nM]); };
		auto isActive = [&](BaseEdge* e) { return e && !(e->poseVertex()->fixed && e->landmarkVertex()->fixed); };
		const unsigned T = hostThreads(nAll);
		std::vector<size_t> cnt(T + 1, 0);
		auto chunk = [&](unsigned t) { return std::make_pair(nAll * t / T, nAll * (t + 1) / T); };
		forThreads(T, [&](unsigned t) {
			size_t c = 0;
			for (size_t k = chunk(t).first; k < chunk(t).second; k++)
			{
				if (k + kPrefetch < chunk(t).second) if (const BaseEdge* nx = edgeAt(k + kPrefetch)) __builtin_prefetch(nx);
				c += isActive(edgeAt(k));
			}
			cnt[t + 1] = c;
		});
		for (unsigned t = 0; t < T; t++) cnt[t + 1] += cnt[t];
		const size_t nAct = cnt[T];
		if (!chiIndexBuilt_ && chiEdges_.empty()) chiEdges_ = std::move(activeEdges_);   // pending per-edge results refer to the old list
		activeEdges_.resize(nAct); edgePose_.resize(nAct); edgeLandmark_.resize(nAct); edgeDim_.resize(nAct);
		meas_.resize(3 * nAct); omega_.resize(nAct);
		forThreads(T, [&](unsigned t) {
			size_t o = cnt[t];
			for (size_t k = chunk(t).first; k < chunk(t).second; k++)
			{
				if (k + kPrefetch < chunk(t).second) if (const BaseEdge* nx = edgeAt(k + kPrefetch)) { __builtin_prefetch(nx); __builtin_prefetch(reinterpret_cast<const char*>(nx) + 64); }
				BaseEdge* e = edgeAt(k);
				if (!isActive(e)) continue;
				activeEdges_[o] = e;
				edgePose_[o] = e->poseVertex()->iP;
				edgeLandmark_[o] = e->landmarkVertex()->iL;
				if (k < nM)
				{
					const MonoEdge* m = ms[k];
					edgeDim_[o] = 2; meas_[3 * o] = m->measurement[0]; meas_[3 * o + 1] = m->measurement[1]; meas_[3 * o + 2] = 0.0;
					omega_[o] = m->information;
				}
				else
				{
					const StereoEdge* m = ss[k - nM];
					edgeDim_[o] = 3; meas_[3 * o] = m->measurement[0]; meas_[3 * o + 1] = m->measurement[1]; meas_[3 * o + 2] = m->measurement[2];
					omega_[o] = m->information;
				}
				o++;
			}
		});
		}
		if (!sameTopology) edgesChangedSinceUpload_ = valuesChangedSinceUpload_ = true;
		edgesDirty_ = false;
		lap("edges");

		stats_.clear();
		graphDirty_ = true;
		initialized_ = true;
		initSeconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	}

	// ---- optimize: the LM loop runs behind the ABI (ref :793-857) -----------------------------------
	void prepareOptimize()
	{
		if (!initialized_) throw std::runtime_error("optimize() called before initialize()");
		static const bool dbg = std::getenv("CUBA_HIP_DEBUG") != nullptr;      // phase breakdown of the contract wall on stderr
		auto tl = std::chrono::steady_clock::now();
		auto lap = [&](const char* what) {
			if (!dbg) return;
			const auto now = std::chrono::steady_clock::now();
			std::fprintf(stderr, "[cuba host] %-28s %7.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - tl).count());
			tl = now;
		};
		if (dbg) std::fprintf(stderr, "[cuba host] %-28s %7.3f ms\n", "initialize()", 1e3 * initSeconds_);
		if (!solver_)
		{
			const char* dev = std::getenv("CUBA_HIP_DEVICE");
			check(cuba_hip_create(dev ? std::atoi(dev) : 0, &solver_), "cuba_hip_create");
			if (const char* p = std::getenv("CUBA_HIP_PROFILE")) check(cuba_hip_set_option(solver_, "profile", std::atof(p)), "set_option");
			if (const char* p = std::getenv("CUBA_HIP_PCG_TOL")) check(cuba_hip_set_option(solver_, "pcg_tol", std::atof(p)), "set_option");
			if (const char* p = std::getenv("CUBA_HIP_HEURISTICS")) check(cuba_hip_set_option(solver_, "heuristics", std::atof(p)), "set_option");      // (0: no run-to-run memories, samples/edit_fuzz.cpp)
		}
		for (int et = 0; et < 2; et++) check(cuba_hip_set_robust_kernel(solver_, et, robustKind_[et], robustDelta_[et]), "set_robust_kernel");
		if (graphDirty_)
		{
			// what initialize() learned while it re-read the graph: the index arrays / the edge values are those of the last upload
			// (the promise refers to ONE upload: the handle counts its uploads, and a count that is not the one recorded with the flags
			// -- a handle that was recreated, an upload this object does not know of -- voids it: round-3 advisor)
			int64_t uploadsNow = -1;
			(void)cuba_hip_get_counter(solver_, "graph_uploads", &uploadsNow);
			if (uploadsNow != uploadGeneration_) uploadedOnce_ = false;
			const bool sameEdges = uploadedOnce_ && !edgesChangedSinceUpload_;
			check(cuba_hip_hint_unchanged(solver_, sameEdges ? 1 : 0, sameEdges && !valuesChangedSinceUpload_ ? 1 : 0), "cuba_hip_hint_unchanged");
			// two-step upload: the measurements / information (32 of the 41 bytes per edge; page-locked staging arrays of this object,
			// untouched until the next initialize()) cross PCIe on a second stream while the structure analysis runs on the index arrays
			check(cuba_hip_set_graph_begin(solver_, static_cast<int>(activePoses_.size()), numFreePoses_,
				static_cast<int>(activeLandmarks_.size()), numFreeLandmarks_, q_.data(), t_.data(), cam_.data(), Xw_.data(),
				static_cast<int>(activeEdges_.size()), edgePose_.data(), edgeLandmark_.data(), edgeDim_.data(), meas_.data(), omega_.data()),
				"cuba_hip_set_graph_begin");
			// (an upload clears the handle's relative-pose edges and range factors between poses; their pose pairs are part of the block
			// pattern, so they go up before the structure analysis: an unchanged pair set then keeps the structure of the previous initialize())
			forEachKind([](auto& list) { if (inBlockPattern(list)) { list.onDevice = false; list.dirty = true; } });
			forEachKind([this](auto& list) { if (inBlockPattern(list)) upload(list); });
			check(cuba_hip_build_structure(solver_), "cuba_hip_build_structure");
			check(cuba_hip_set_graph_end(solver_), "cuba_hip_set_graph_end");
			graphDirty_ = false;
			forEachKind([](auto& list) { if (!inBlockPattern(list)) list.dirty = true; });          // (an upload clears the handle's other factors too)
			uploadedOnce_ = true; edgesChangedSinceUpload_ = valuesChangedSinceUpload_ = false;       // from here on the device holds exactly these edges and values
			(void)cuba_hip_get_counter(solver_, "graph_uploads", &uploadGeneration_);
			maskDirty_ = true;          // (the edge order may be another, and the handle drops its mask with other edges)
		}
		lap("create + set_graph");
		forEachKind([this](auto& list) { upload(list); });
		sendEdgeMask();
	}

	// ---- edge gating (extension: cuba::gateEdges and friends) ----------------------------------------
	// The levels are kept per edge OBJECT (inactiveEdges_: the edges at level 1), as the factor lists are kept per factor, and go to
	// the handle as a mask over the active edges after every upload of the graph and after every change by hand.  An object that never
	// gates sends nothing.
	void sendEdgeMask()
	{
		if (!maskDirty_) return;
		maskDirty_ = false;
		if (inactiveEdges_.empty() && !deviceGated_) return;
		bool any = false;
		edgeMask_.assign(activeEdges_.size(), 1);
		for (size_t o = 0; o < activeEdges_.size(); o++) if (inactiveEdges_.count(activeEdges_[o])) { edgeMask_[o] = 0; any = true; }
		check(cuba_hip_set_edge_active(solver_, any ? edgeMask_.data() : nullptr), "cuba_hip_set_edge_active");
		deviceGated_ = any;
	}
	EdgeGateResult gateEdges(const EdgeGate& gate)
	{
		prepareOptimize();            // (the graph and the levels set by hand go up first)
		const double thr[2] = { gate.chi2Mono, gate.chi2Stereo };
		int64_t c[6] = { 0, 0, 0, 0, 0, 0 };
		gateChi_.assign(activeEdges_.size(), 0.0);
		check(cuba_hip_gate_edges(solver_, thr, gate.positiveDepth ? 1 : 0, static_cast<int>(gate.mode), c, gateChi_.data()), "cuba_hip_gate_edges");
		gateChiEdges_ = activeEdges_; gateChiIndex_.clear();          // (the edge -> value index is built by the first edgeGateChiSquared)
		if (gate.mode != EdgeGateMode::DRY_RUN)
		{
			edgeMask_.assign(activeEdges_.size(), 1);
			check(cuba_hip_get_edge_active(solver_, edgeMask_.data()), "cuba_hip_get_edge_active");
			for (size_t o = 0; o < activeEdges_.size(); o++)
				if (edgeMask_[o]) inactiveEdges_.erase(activeEdges_[o]); else inactiveEdges_.insert(activeEdges_[o]);
			deviceGated_ = true;
		}
		return { c[0], c[1], c[2], c[3], c[4], c[5] };
	}
	void setEdgeActive(const BaseEdge* e, bool active)
	{
		if (!e) return;
		if (active ? inactiveEdges_.erase(e) != 0 : inactiveEdges_.insert(e).second) maskDirty_ = true;
	}
	bool edgeActive(const BaseEdge* e) const { return inactiveEdges_.count(e) == 0; }
	double edgeGateChiSquared(const BaseEdge* e) const
	{
		if (gateChiIndex_.empty()) for (size_t o = 0; o < gateChiEdges_.size(); o++) gateChiIndex_[gateChiEdges_[o]] = gateChi_[o];
		const auto it = gateChiIndex_.find(e);
		return it == gateChiIndex_.end() ? 0.0 : it->second;
	}
	// ---- landmark triangulation (extension: cuba::triangulateLandmarks) --------------------------------
	// One call behind the ABI.  The accepted positions go into the vertex objects (and the staging array of the next upload): the next
	// initialize() reads the estimates from there, and the handle already holds them.
	TriangulationResult triangulateLandmarks(const TriangulationOptions& o, const std::vector<LandmarkVertex*>* subset)
	{
		prepareOptimize();            // (the graph and the levels set by hand go up first)
		const size_t nL = activeLandmarks_.size();
		std::vector<uint8_t> select;
		if (subset)
		{
			select.assign(nL, 0);
			for (const LandmarkVertex* v : *subset)
				if (v && v->iL >= 0 && static_cast<size_t>(v->iL) < nL && activeLandmarks_[v->iL] == v) select[v->iL] = 1;
		}
		const double thr[2] = { o.chi2Mono, o.chi2Stereo };
		int64_t c[CUBA_HIP_TRI_STATUSES] = { 0, 0, 0, 0, 0, 0, 0, 0 };
		triStatus_.assign(nL, CUBA_HIP_TRI_NOT_SELECTED);
		std::vector<double> xyz(3 * nL);
		check(cuba_hip_triangulate_landmarks(solver_, subset ? select.data() : nullptr, o.refineIterations, o.minParallaxDeg, thr, o.dryRun ? 1 : 0,
			triStatus_.data(), c, xyz.data()), "cuba_hip_triangulate_landmarks");
		triLandmarks_ = activeLandmarks_; triIndex_.clear();          // (the vertex -> status index is built by the first triangulationStatus)
		if (!o.dryRun)
			for (size_t i = 0; i < nL; i++)
				if (triStatus_[i] == CUBA_HIP_TRI_OK)
					for (int k = 0; k < 3; k++) activeLandmarks_[i]->Xw.data()[k] = Xw_[3 * i + k] = xyz[3 * i + k];
		TriangulationResult r;
		for (int k = 0; k < CUBA_HIP_TRI_STATUSES; k++) r.counts[k] = c[k];
		return r;
	}
	TriangulationStatus triangulationStatus(const LandmarkVertex* v) const
	{
		if (triIndex_.empty()) for (size_t i = 0; i < triLandmarks_.size(); i++) triIndex_[triLandmarks_[i]] = triStatus_[i];
		const auto it = triIndex_.find(v);
		return it == triIndex_.end() ? TriangulationStatus::NOT_SELECTED : static_cast<TriangulationStatus>(it->second);
	}
	// ---- pose refinement with the landmarks held (extension: cuba::refinePoses) ---------------------------
	// One call behind the ABI.  The refined poses go into the vertex objects (and the staging arrays of the next upload): the next
	// initialize() reads the estimates from there, and the handle already holds them.
	PoseRefinementResult refinePoses(const PoseRefinementOptions& o, const std::vector<PoseVertex*>* subset)
	{
		if (o.rounds < 1 || o.rounds > 4 || o.iterations < 1 || o.iterations > 32 || o.robustRounds < 0 || o.robustRounds > o.rounds || o.minInliers < 0 ||
			std::isnan(o.chi2Mono) || std::isnan(o.chi2Stereo))
			throw std::invalid_argument("cuba::refinePoses: rounds 1 ... 4, iterations 1 ... 32, robustRounds 0 ... rounds, minInliers >= 0, thresholds not NaN");
		prepareOptimize();            // (the graph and the levels set by hand go up first)
		const size_t nP = activePoses_.size();
		std::vector<uint8_t> select;
		if (subset)
		{
			select.assign(nP, 0);
			for (const PoseVertex* v : *subset)
				if (v && v->iP >= 0 && static_cast<size_t>(v->iP) < nP && activePoses_[v->iP] == v) select[v->iP] = 1;
		}
		const double thr[2] = { o.chi2Mono, o.chi2Stereo };
		int64_t c[CUBA_HIP_POSEREF_STATUSES] = { 0, 0, 0, 0, 0, 0 };
		refStatus_.assign(nP, CUBA_HIP_POSEREF_NOT_SELECTED);
		std::vector<double> q(4 * nP), t(3 * nP);
		check(cuba_hip_refine_poses(solver_, subset ? select.data() : nullptr, o.rounds, o.iterations, o.robustRounds, thr, o.minInliers, o.dryRun ? 1 : 0,
			refStatus_.data(), c, nullptr, nullptr, q.data(), t.data(), nullptr), "cuba_hip_refine_poses");
		refPoses_ = activePoses_; refIndex_.clear();          // (the vertex -> row index is built by the first poseRefinementStatus)
		if (!o.dryRun)
			for (size_t i = 0; i < nP; i++)
				if (refStatus_[i] == CUBA_HIP_POSEREF_OK)
				{
					double* qc = activePoses_[i]->q.coeffs().data();
					for (int k = 0; k < 4; k++) qc[k] = q_[4 * i + k] = q[4 * i + k];
					for (int k = 0; k < 3; k++) activePoses_[i]->t.data()[k] = t_[3 * i + k] = t[3 * i + k];
				}
		PoseRefinementResult r;
		for (int k = 0; k < CUBA_HIP_POSEREF_STATUSES; k++) r.counts[k] = c[k];
		return r;
	}
	size_t refinementRow(const PoseVertex* v) const
	{
		if (refIndex_.empty()) for (size_t i = 0; i < refPoses_.size(); i++) refIndex_[refPoses_[i]] = i;
		const auto it = refIndex_.find(v);
		return it == refIndex_.end() ? refPoses_.size() : it->second;
	}
	PoseRefinementStatus poseRefinementStatus(const PoseVertex* v) const
	{
		const size_t i = refinementRow(v);
		return i == refPoses_.size() ? PoseRefinementStatus::NOT_SELECTED : static_cast<PoseRefinementStatus>(refStatus_[i]);
	}
	// ---- pose localisation from scratch (extension: cuba::localizePoses) -----------------------------------
	// One call behind the ABI.  The winners go into the vertex objects (and the staging arrays of the next upload), as refinePoses' do.
	PoseLocalizationResult localizePoses(const PoseLocalizationOptions& o, const std::vector<PoseVertex*>* subset)
	{
		if (o.hypotheses < 1 || o.hypotheses > 4096 || o.minInliers < 0 || !std::isfinite(o.chi2Mono) || !std::isfinite(o.chi2Stereo) ||
			!(o.chi2Mono > 0) || !(o.chi2Stereo > 0))
			throw std::invalid_argument("cuba::localizePoses: hypotheses 1 ... 4096, minInliers >= 0, thresholds finite and positive");
		prepareOptimize();            // (the graph and the levels set by hand go up first)
		const size_t nP = activePoses_.size();
		std::vector<uint8_t> select;
		if (subset)
		{
			select.assign(nP, 0);
			for (const PoseVertex* v : *subset)
				if (v && v->iP >= 0 && static_cast<size_t>(v->iP) < nP && activePoses_[v->iP] == v) select[v->iP] = 1;
		}
		const double thr[2] = { o.chi2Mono, o.chi2Stereo };
		int64_t c[CUBA_HIP_POSELOC_STATUSES] = { 0, 0, 0, 0, 0, 0 };
		locStatus_.assign(nP, CUBA_HIP_POSELOC_NOT_SELECTED);
		std::vector<double> q(4 * nP), t(3 * nP);
		check(cuba_hip_localize_poses(solver_, subset ? select.data() : nullptr, o.hypotheses, static_cast<uint64_t>(o.seed), thr, o.minInliers, o.dryRun ? 1 : 0,
			locStatus_.data(), c, nullptr, nullptr, nullptr, q.data(), t.data(), nullptr), "cuba_hip_localize_poses");
		locPoses_ = activePoses_; locIndex_.clear();          // (the vertex -> row index is built by the first poseLocalizationStatus)
		if (!o.dryRun)
			for (size_t i = 0; i < nP; i++)
				if (locStatus_[i] == CUBA_HIP_POSELOC_OK)
				{
					double* qc = activePoses_[i]->q.coeffs().data();
					for (int k = 0; k < 4; k++) qc[k] = q_[4 * i + k] = q[4 * i + k];
					for (int k = 0; k < 3; k++) activePoses_[i]->t.data()[k] = t_[3 * i + k] = t[3 * i + k];
				}
		PoseLocalizationResult r;
		for (int k = 0; k < CUBA_HIP_POSELOC_STATUSES; k++) r.counts[k] = c[k];
		return r;
	}
	PoseLocalizationStatus poseLocalizationStatus(const PoseVertex* v) const
	{
		if (locIndex_.empty()) for (size_t i = 0; i < locPoses_.size(); i++) locIndex_[locPoses_[i]] = i;
		const auto it = locIndex_.find(v);
		return it == locIndex_.end() ? PoseLocalizationStatus::NOT_SELECTED : static_cast<PoseLocalizationStatus>(locStatus_[it->second]);
	}
	int activeObservations(const LandmarkVertex* v) const
	{
		int n = 0;
		if (v && landmarks_.count(v->id) && landmarks_.at(v->id) == v)
			for (const BaseEdge* e : v->edges)
				n += !(e->poseVertex()->fixed && v->fixed) && inactiveEdges_.count(e) == 0;
		return n;
	}

	// ---- factors (FactorKind, FactorLists above) -----------------------------------------------------
	FactorLists factors_;
	template <class Fn> void forEachKind(Fn&& fn) { std::apply([&](auto&... list) { (fn(list), ...); }, factors_); }
	template <class F> static constexpr bool inBlockPattern(const FactorList<F>&) { return FactorKind<F>::inBlockPattern; }
	// (public: the extension functions below remove and look up through it)
	template <class F> FactorList<F>& list() { return std::get<FactorList<F>>(factors_); }
	template <class F> const FactorList<F>& list() const { return std::get<FactorList<F>>(factors_); }

	template <class F> void addFactor(F* f)
	{
		using K = FactorKind<F>;
		using Ends = decltype(ends(*f));
		if (!f || !distinctVertices(ends(*f))) throw std::invalid_argument(std::string(K::fn) + ": " + K::noun + " needs " + whatItNeeds(Ends()));
		list<F>().add(f);
	}
	// a removed vertex takes its factors with it (initialize() would refuse them: their vertex is not part of the graph)
	void dropFactorsOf(const void* vertex)
	{
		forEachKind([vertex](auto& list) {
			list.removeIf([vertex](const auto* f) { for (const void* v : ends(*f)) if (v == vertex) return true; return false; });
		});
	}
	// index of a factor's vertex among the active ones (each map is built with the first factor of an initialize() that asks);
	// `refusal`: the message for a vertex that is not part of the graph
	template <class V> static int32_t indexIn(std::map<const V*, int32_t>& index, const std::vector<V*>& active, const V* v, const std::string& refusal)
	{
		if (index.empty())
			for (size_t i = 0; i < active.size(); i++) index[active[i]] = (int32_t)i;
		const auto it = index.find(v);
		if (it == index.end()) throw std::invalid_argument(refusal);
		return it->second;
	}
	int32_t vertexIndex(const PoseVertex* v, const std::string& refusal) { return indexIn(poseIdx_, activePoses_, v, refusal); }
	int32_t vertexIndex(const LandmarkVertex* v, const std::string& refusal) { return indexIn(landmarkIdx_, activeLandmarks_, v, refusal); }
	// kind | delta of a set of factors as the C ABI takes them; any: a factor has a kernel
	struct FactorKernels { std::vector<int32_t> kind; std::vector<double> delta; bool any = false; };
	template <class F> static FactorKernels packKernels(const std::vector<F*>& factors)
	{
		const size_t n = factors.size();
		FactorKernels r{ std::vector<int32_t>(n), std::vector<double>(n) };
		for (size_t k = 0; k < n; k++)
		{
			r.kind[k] = static_cast<int32_t>(factors[k]->kernel); r.delta[k] = factors[k]->delta;
			r.any = r.any || factors[k]->kernel != PoseFactorKernel::NONE;
		}
		return r;
	}
	// the set as it stands goes to the device, if it changed since it last went (an empty set that replaces one: the clearing call)
	template <class F> void upload(FactorList<F>& list)
	{
		using K = FactorKind<F>;
		if (!list.beginUpload()) return;
		const std::vector<F*>& factors = list.items;
		const size_t n = factors.size();
		constexpr bool binary = std::tuple_size<decltype(ends(*factors[0]))>::value == 2;
		std::vector<int32_t> vertex[2] = { std::vector<int32_t>(n), std::vector<int32_t>(binary ? n : 0) };
		const std::string refusal = std::string(K::fn) + (binary ? ": a vertex of " : ": the vertex of ") + K::ofA + " is not part of the graph";
		for (size_t k = 0; k < n; k++)
		{
			const auto e = ends(*factors[k]);
			for (size_t s = 0; s < e.size(); s++) vertex[s][k] = vertexIndex(e[s], refusal);
		}
		const FactorKernels r = packKernels(factors);
		const bool inside = K::kernelType < 0 && r.any;
		check(K::set(solver_, factors, vertex[0].data(), vertex[1].data(), inside ? r.kind.data() : nullptr, inside ? r.delta.data() : nullptr), K::setName);
		// (the pose factors' kernels follow the set they belong to; a set without any sends nothing: the handle has none after the setter)
		if (K::kernelType >= 0 && r.any)
			check(cuba_hip_set_pose_factor_robust_kernels(solver_, K::kernelType, (int)n, r.kind.data(), r.delta.data()), "cuba_hip_set_pose_factor_robust_kernels");
		list.endUpload();
	}
	// after a solve: the chi2 of the uploaded sets
	void readChiSquares()
	{
		for (const bool pattern : { false, true })
			forEachKind([&](auto& list) {
				using K = typename std::decay_t<decltype(list)>::Kind;
				if (K::inBlockPattern == pattern) list.readChi([&](double* c) { check(K::chiSquares(solver_, c), K::chiName); });
			});
	}

	// (optimize() in three steps, so that cuba::optimizeBatch can run the middle one for several objects at once)
	void optimize(int niterations) override
	{
		prepareOptimize();
		std::vector<double> chi2(std::max(niterations, 1), 0.0);
		int done = 0;
		check(cuba_hip_optimize(solver_, niterations, chi2.data(), &done), "cuba_hip_optimize");
		finishOptimize(chi2.data(), done);
	}

	cuba_hip_solver* handle() const { return solver_; }

	// ---- marginal covariances (extension: cuba::computeCovariances) --------------------------------
	bool computeCovariances(bool landmarks)
	{
		prepareOptimize();            // (the graph goes up first if initialize() changed it: the covariance is that of the current estimate)
		covPoseIndex_.clear(); covLmIndex_.clear();
		poseCov_.assign(36 * activePoses_.size(), 0.0);
		lmCov_.assign(landmarks ? 9 * activeLandmarks_.size() : 0, 0.0);
		int notPd = 0;
		check(cuba_hip_compute_covariance(solver_, poseCov_.data(), landmarks ? lmCov_.data() : nullptr, &notPd), "cuba_hip_compute_covariance");
		if (notPd) return false;
		for (int i = 0; i < numFreePoses_; i++) covPoseIndex_[activePoses_[i]] = (size_t)i;
		if (landmarks) for (int i = 0; i < numFreeLandmarks_; i++) covLmIndex_[activeLandmarks_[i]] = (size_t)i;
		return true;
	}
	bool computeCrossCovariances(const std::vector<CovariancePair>& pairs, std::vector<std::array<double, 36>>& out)
	{
		prepareOptimize();            // (as computeCovariances: the estimate on the device is the current one)
		std::map<const PoseVertex*, int> poseIdx;
		std::map<const LandmarkVertex*, int> lmIdx;
		for (size_t i = 0; i < activePoses_.size(); i++) poseIdx[activePoses_[i]] = (int)i;
		for (size_t i = 0; i < activeLandmarks_.size(); i++) lmIdx[activeLandmarks_[i]] = (int)i;
		const size_t n = pairs.size();
		std::vector<int32_t> kind[2], index[2];
		for (int s = 0; s < 2; s++) { kind[s].resize(std::max<size_t>(n, 1)); index[s].resize(std::max<size_t>(n, 1)); }
		for (size_t k = 0; k < n; k++)
			for (int s = 0; s < 2; s++)
			{
				const CovarianceVertex& v = s ? pairs[k].second : pairs[k].first;
				if (v.pose)
				{
					const auto it = poseIdx.find(v.pose);
					if (it == poseIdx.end()) throw std::invalid_argument("cuba::computeCrossCovariances: a pose vertex of pair " + std::to_string(k) + " is not part of the graph");
					kind[s][k] = CUBA_HIP_VERTEX_POSE; index[s][k] = it->second;
				}
				else
				{
					const auto it = v.landmark ? lmIdx.find(v.landmark) : lmIdx.end();
					if (it == lmIdx.end()) throw std::invalid_argument("cuba::computeCrossCovariances: a landmark vertex of pair " + std::to_string(k) + " is not part of the graph");
					kind[s][k] = CUBA_HIP_VERTEX_LANDMARK; index[s][k] = it->second;
				}
			}
		std::vector<double> blocks(36 * std::max<size_t>(n, 1), 0.0);
		int notPd = 0;
		check(cuba_hip_compute_covariance_pairs(solver_, (int)n, kind[0].data(), index[0].data(), kind[1].data(), index[1].data(), blocks.data(), &notPd),
			"cuba_hip_compute_covariance_pairs");
		if (notPd) return false;
		out.resize(n);
		for (size_t k = 0; k < n; k++) std::copy(blocks.begin() + 36 * k, blocks.begin() + 36 * (k + 1), out[k].begin());
		return true;
	}
	bool poseCovariance(const PoseVertex* v, double out[36]) const { return covBlock(covPoseIndex_, poseCov_, v, 36, out); }
	bool landmarkCovariance(const LandmarkVertex* v, double out[9]) const { return covBlock(covLmIndex_, lmCov_, v, 9, out); }

	void finishOptimize(const double* chi2, int done)
	{
		static const bool dbg = std::getenv("CUBA_HIP_DEBUG") != nullptr;
		auto tl = std::chrono::steady_clock::now();
		auto lap = [&](const char* what) {
			if (!dbg) return;
			const auto now = std::chrono::steady_clock::now();
			std::fprintf(stderr, "[cuba host] %-28s %7.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - tl).count());
			tl = now;
		};
		for (int i = 0; i < done; i++) stats_.push_back({ i, chi2[i] });
		readChiSquares();

		// finalize (ref :512-526): estimates back into the caller's vertices
		check(cuba_hip_get_solution(solver_, q_.data(), t_.data(), Xw_.data()), "cuba_hip_get_solution");
		lap("get_solution");
		// per-edge chi2 (ref getChiSqs :528-543): evaluated and copied by the device while the host writes the estimates back
		perEdgeChi_.resize(activeEdges_.size());
		check(cuba_hip_chi_squares_begin(solver_, perEdgeChi_.data()), "cuba_hip_chi_squares_begin");
		for (size_t i = 0; i < activePoses_.size(); i++)
		{
			double* qc = activePoses_[i]->q.coeffs().data();
			for (int k = 0; k < 4; k++) qc[k] = q_[4 * i + k];
			for (int k = 0; k < 3; k++) activePoses_[i]->t.data()[k] = t_[3 * i + k];
		}
		{
			const size_t nL = activeLandmarks_.size();
			const unsigned T = hostThreads(nL);
			forThreads(T, [&](unsigned t) {       // one scattered store per landmark object: split over the pool
				const size_t iEnd = nL * (t + 1) / T;
				for (size_t i = nL * t / T; i < iEnd; i++)
				{
					if (i + kPrefetch < iEnd) __builtin_prefetch(activeLandmarks_[i + kPrefetch]->Xw.data(), 1);
					for (int k = 0; k < 3; k++) activeLandmarks_[i]->Xw.data()[k] = Xw_[3 * i + k];
				}
			});
		}

		lap("write-back into vertices");
		check(cuba_hip_chi_squares_end(solver_), "cuba_hip_chi_squares_end");
		lap("chi_squares (rest)");
		chiSqs_.clear();
		chiEdges_.clear();
		chiIndexBuilt_ = false;          // the edge -> value index is built on the first chiSquared() query

		double prof[CUBA_HIP_PROFILE_ITEMS];
		check(cuba_hip_get_profile(solver_, prof), "cuba_hip_get_profile");
		prof[0] += initSeconds_;
		initSeconds_ = 0;
		timeProfile_.clear();
		for (int i = 0; i < CUBA_HIP_PROFILE_ITEMS; i++) timeProfile_[kProfileKeys[i]] = prof[i];
	}

	void clear() override
	{
		covPoseIndex_.clear(); covLmIndex_.clear();
		poses_.clear(); landmarks_.clear(); mono_.clear(); stereo_.clear(); stats_.clear();
		forEachKind([](auto& list) { list.items.clear(); list.chi.clear(); });
		inactiveEdges_.clear(); maskDirty_ = true; gateChi_.clear(); gateChiEdges_.clear(); gateChiIndex_.clear();
		triStatus_.clear(); triLandmarks_.clear(); triIndex_.clear();
		refStatus_.clear(); refPoses_.clear(); refIndex_.clear();
		locStatus_.clear(); locPoses_.clear(); locIndex_.clear();
		posesDirty_ = landmarksDirty_ = edgesDirty_ = true;
		initialized_ = false;
	}

	const BatchStatistics& batchStatistics() const override { return stats_; }
	const TimeProfile& timeProfile() const override { return timeProfile_; }

	double chiSquared(const BaseEdge* e) const override
	{
		buildChiIndex();
		auto it = chiSqs_.find(e);
		return it == chiSqs_.end() ? 0.0 : it->second;
	}

private:
	static constexpr size_t kPrefetch = 12;      // objects ahead of the one being read in the pointer-chasing loops
	static unsigned hostThreads(size_t items)
	{
		static const size_t grain = std::getenv("CUBA_HOST_GRAIN") ? (size_t)std::max(1000, std::atoi(std::getenv("CUBA_HOST_GRAIN"))) : 20000;   // items per host thread
		return (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)cubahip::HostPool::instance().maxThreads(), items / grain + 1));
	}

	template <class Fn>
	static void forThreads(unsigned T, Fn&& fn)
	{
		cubahip::HostPool::instance().run((int)T, [&](int t) { fn((unsigned)t); });   // persistent pool shared with the device library
	}

	// active = [free vertices in list order | fixed vertices in list order], vertices without edges skipped;
	// emit(v, solver index) runs once per active vertex.  Returns the number of free ones.
	// prev (optional): the active list of the previous call, valid as long as no `fixed` flag changed -- then ONE pass over it
	// re-reads the values (and checks the flags); otherwise the two passes over the whole list.
	template <class V, class Resize, class Emit>
	static int indexVertices(const std::vector<V*>& list, std::vector<V*>& active, const std::vector<V*>* prev, int prevFree, Resize&& resize, Emit&& emit)
	{
		if (prev)
		{
			const size_t m = prev->size();
			const unsigned Tp = hostThreads(m);
			resize(m);
			std::vector<char> bad(Tp, 0);
			forThreads(Tp, [&](unsigned t) {
				const size_t iEnd = m * (t + 1) / Tp;
				for (size_t i = m * t / Tp; i < iEnd; i++)
				{
					if (i + kPrefetch < iEnd) { const char* nx = reinterpret_cast<const char*>((*prev)[i + kPrefetch]); __builtin_prefetch(nx); __builtin_prefetch(nx + 64); }
					V* v = (*prev)[i];
					if (v->edges.empty() || v->fixed != (i >= (size_t)prevFree)) { bad[t] = 1; break; }
					emit(v, i);
				}
			});
			bool ok = true;
			for (char b : bad) ok = ok && !b;
			if (ok) { active = *prev; return prevFree; }
		}
		const size_t n = list.size();
		const unsigned T = hostThreads(n);
		std::vector<size_t> nFree(T + 1, 0), nFixed(T + 1, 0);
		forThreads(T, [&](unsigned t) {
			size_t a = 0, b = 0;
			const size_t kEnd = n * (t + 1) / T;
			for (size_t k = n * t / T; k < kEnd; k++)
			{
				if (k + kPrefetch < kEnd) { const char* nx = reinterpret_cast<const char*>(list[k + kPrefetch]); __builtin_prefetch(nx); __builtin_prefetch(nx + 64); }
				const V* v = list[k];
				if (v->edges.empty()) continue;
				(v->fixed ? b : a)++;
			}
			nFree[t + 1] = a; nFixed[t + 1] = b;
		});
		for (unsigned t = 0; t < T; t++) { nFree[t + 1] += nFree[t]; nFixed[t + 1] += nFixed[t]; }
		const size_t freeTotal = nFree[T];
		active.resize(freeTotal + nFixed[T]);
		resize(active.size());
		forThreads(T, [&](unsigned t) {
			size_t a = nFree[t], b = freeTotal + nFixed[t];
			const size_t kEnd = n * (t + 1) / T;
			for (size_t k = n * t / T; k < kEnd; k++)
			{
				if (k + kPrefetch < kEnd) { const char* nx = reinterpret_cast<const char*>(list[k + kPrefetch]); __builtin_prefetch(nx); __builtin_prefetch(nx + 64); }
				V* v = list[k];
				if (v->edges.empty()) continue;
				const size_t i = v->fixed ? b++ : a++;
				active[i] = v;
				emit(v, i);
			}
		});
		return static_cast<int>(freeTotal);
	}

	void buildChiIndex() const
	{
		if (chiIndexBuilt_) return;
		const std::vector<BaseEdge*>& edges = chiEdges_.empty() ? activeEdges_ : chiEdges_;   // set aside by initialize()?
		chiSqs_.reserve(perEdgeChi_.size());
		for (size_t i = 0; i < perEdgeChi_.size(); i++) chiSqs_[edges[i]] = perEdgeChi_[i];
		chiEdges_.clear(); chiEdges_.shrink_to_fit();
		chiIndexBuilt_ = true;
	}

	void check(int status, const char* what) const
	{
		if (status == CUBA_HIP_OK) return;
		std::string msg = std::string(what) + " failed (status " + std::to_string(status) + ")";
		if (solver_) { msg += ": "; msg += cuba_hip_last_error(solver_); }
		else if (status == CUBA_HIP_ERR_NO_DEVICE) msg += ": no HIP device visible";
		throw std::runtime_error(msg);
	}

	std::map<int, PoseVertex*> poses_;
	std::map<int, LandmarkVertex*> landmarks_;
	std::vector<PoseVertex*> poseList_;           // the maps' values in id order, rebuilt when a vertex was added / removed
	std::vector<LandmarkVertex*> landmarkList_;
	bool posesDirty_ = true, landmarksDirty_ = true;
	bool edgesDirty_ = true;                      // an edge was added / removed since the last initialize()
	OrderedSet<MonoEdge> mono_;
	OrderedSet<StereoEdge> stereo_;
	int robustKind_[2] = { 0, 0 };
	double robustDelta_[2] = { 0, 0 };

	// flattened problem (solver order)
	std::vector<PoseVertex*> activePoses_;
	std::map<const PoseVertex*, int32_t> poseIdx_;            // active pose -> solver index, for the factors of this initialize()
	std::vector<LandmarkVertex*> activeLandmarks_;
	std::map<const LandmarkVertex*, int32_t> landmarkIdx_;    // the same for the landmark priors
	std::vector<BaseEdge*> activeEdges_;
	int numFreePoses_ = 0, numFreeLandmarks_ = 0;
	PinnedVector<double> q_, t_, cam_, Xw_, meas_, omega_;
	PinnedVector<int32_t> edgePose_, edgeLandmark_;
	PinnedVector<uint8_t> edgeDim_;
	bool initialized_ = false, graphDirty_ = false;
	double initSeconds_ = 0;

	template <class V>
	static bool covBlock(const std::unordered_map<const void*, size_t>& index, const std::vector<double>& cov, const V* v, int n, double* out)
	{
		const auto it = index.find(v);
		if (it == index.end()) return false;          // fixed, not part of the last computation, or nothing computed
		std::copy(cov.begin() + (size_t)n * it->second, cov.begin() + (size_t)n * (it->second + 1), out);
		return true;
	}
	std::unordered_map<const void*, size_t> covPoseIndex_, covLmIndex_;      // free vertex -> row of the last computation
	std::vector<double> poseCov_, lmCov_;

	cuba_hip_solver* solver_ = nullptr;
	bool uploadedOnce_ = false, edgesChangedSinceUpload_ = true, valuesChangedSinceUpload_ = true;    // what cuba_hip_hint_unchanged may promise
	int64_t uploadGeneration_ = -1;          // "graph_uploads" of the handle right after the upload those flags describe
	BatchStatistics stats_;
	TimeProfile timeProfile_;
	PinnedVector<double> perEdgeChi_;
	mutable std::unordered_map<const BaseEdge*, double> chiSqs_;
	mutable bool chiIndexBuilt_ = true;
	mutable std::vector<BaseEdge*> chiEdges_;   // edge list the pending per-edge results refer to, once initialize() replaced activeEdges_

	std::unordered_set<const BaseEdge*> inactiveEdges_;      // the edges switched off (level 1)
	bool maskDirty_ = false, deviceGated_ = false;           // the handle's mask is not inactiveEdges_ / the handle holds a mask
	std::vector<uint8_t> edgeMask_;
	std::vector<double> gateChi_;                            // ungated chi2 of the last gateEdges, over gateChiEdges_
	std::vector<BaseEdge*> gateChiEdges_;
	mutable std::unordered_map<const BaseEdge*, double> gateChiIndex_;
	std::vector<int32_t> triStatus_;                         // statuses of the last triangulateLandmarks, over triLandmarks_
	std::vector<LandmarkVertex*> triLandmarks_;
	mutable std::unordered_map<const LandmarkVertex*, int32_t> triIndex_;
	std::vector<int32_t> refStatus_;                         // statuses of the last refinePoses, over refPoses_
	std::vector<PoseVertex*> refPoses_;
	mutable std::unordered_map<const PoseVertex*, size_t> refIndex_;
	std::vector<int32_t> locStatus_;                         // statuses of the last localizePoses, over locPoses_
	std::vector<PoseVertex*> locPoses_;
	mutable std::unordered_map<const PoseVertex*, size_t> locIndex_;
};

}  // namespace

CudaBundleAdjustment::Ptr CudaBundleAdjustment::createChecked(const size_t* layout, int n)
{
	// the layouts THIS library was compiled with (see the inline create() in the header)
	const size_t mine[8] = { sizeof(PoseVertex), alignof(PoseVertex), offsetof(PoseVertex, t), offsetof(PoseVertex, camera),
		sizeof(LandmarkVertex), offsetof(LandmarkVertex, fixed), sizeof(MonoEdge), sizeof(StereoEdge) };
	bool same = layout && n == 8;
	for (int i = 0; same && i < 8; i++) same = layout[i] == mine[i];
	if (!same)
		throw std::runtime_error("cuba::CudaBundleAdjustment::create: the application and libcuda_bundle_adjustment.so were compiled with "
			"different Eigen headers (vertex / edge layouts differ); rebuild one of them against the other's Eigen");
	return std::make_unique<HipBundleAdjustment>();
}

CudaBundleAdjustment::~CudaBundleAdjustment() = default;

// Extension (no counterpart in the reference's API): optimize() of several objects in ONE device launch chain (cuba_hip_optimize_batch).
// Every object ends exactly where its own optimize(niterations) would have ended -- estimates written back into its vertices,
// batchStatistics(), chiSquared() -- bit for bit; objects the device library cannot batch are run one after the other by it.
void optimizeBatch(CudaBundleAdjustment* const* objects, int n, int niterations)
{
	if (n <= 0) return;
	std::vector<HipBundleAdjustment*> impl((size_t)n);
	std::vector<cuba_hip_solver*> handles((size_t)n);
	for (int i = 0; i < n; i++)
	{
		impl[i] = dynamic_cast<HipBundleAdjustment*>(objects[i]);
		if (!impl[i]) throw std::runtime_error("cuba::optimizeBatch: not an object of this library");
		impl[i]->prepareOptimize();
		handles[i] = impl[i]->handle();
	}
	std::vector<double> chi2((size_t)n * std::max(niterations, 1), 0.0);
	std::vector<int> done((size_t)n, 0);
	const int rc = cuba_hip_optimize_batch(handles.data(), n, niterations, chi2.data(), done.data(), nullptr);
	if (rc != CUBA_HIP_OK) throw std::runtime_error(std::string("cuba_hip_optimize_batch failed: ") + cuba_hip_last_error(handles[0]));
	for (int i = 0; i < n; i++) impl[i]->finishOptimize(chi2.data() + (size_t)i * std::max(niterations, 1), done[i]);
}

// Extension (g2o's SparseOptimizer::computeMarginals; the reference has none): marginal covariances of the free poses (6 x 6, tangent
// [omega, upsilon] of the pose update) and, with `landmarks`, of the free landmarks (3 x 3) at the object's current estimate --
// the inverse of the undamped Gauss-Newton Hessian (cuba_hip_compute_covariance).  false: that Hessian is not positive definite.
bool computeCovariances(CudaBundleAdjustment* object, bool landmarks)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::computeCovariances: not an object of this library");
	return impl->computeCovariances(landmarks);
}

bool computeCrossCovariances(CudaBundleAdjustment* object, const std::vector<CovariancePair>& pairs, std::vector<std::array<double, 36>>& out)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::computeCrossCovariances: not an object of this library");
	return impl->computeCrossCovariances(pairs, out);
}

bool poseCovariance(const CudaBundleAdjustment* object, const PoseVertex* v, double cov[36])
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl && impl->poseCovariance(v, cov);
}

bool landmarkCovariance(const CudaBundleAdjustment* object, const LandmarkVertex* v, double cov[9])
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl && impl->landmarkCovariance(v, cov);
}

// Extensions (the reference has no factors besides the reprojection edges): add / remove / chi2 of every factor kind, the same three
// for all of them.  A factor takes effect at the next initialize(); an object of another library is refused by add and ignored by the
// other two (remove: nothing to do, chi2: 0).
namespace
{
template <class F> void addFactor(CudaBundleAdjustment* object, F* f)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error(std::string(FactorKind<F>::fn) + ": not an object of this library");
	impl->addFactor(f);
}
template <class F> void removeFactor(CudaBundleAdjustment* object, F* f)
{
	if (auto* impl = dynamic_cast<HipBundleAdjustment*>(object)) impl->list<F>().remove(f);
}
template <class F> double factorChiSquared(const CudaBundleAdjustment* object, const F* f)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl ? impl->list<F>().chiSquared(f) : 0.0;
}
}  // namespace

// Extension (g2o's setLevel / computeActiveErrors; the reference has none): edges switched off and on without a new topology.
EdgeGateResult gateEdges(CudaBundleAdjustment* object, const EdgeGate& gate)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::gateEdges: not an object of this library");
	return impl->gateEdges(gate);
}
void setEdgeActive(CudaBundleAdjustment* object, const BaseEdge* edge, bool active)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::setEdgeActive: not an object of this library");
	impl->setEdgeActive(edge, active);
}
bool edgeActive(const CudaBundleAdjustment* object, const BaseEdge* edge)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return !impl || impl->edgeActive(edge);
}
double edgeGateChiSquared(const CudaBundleAdjustment* object, const BaseEdge* edge)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl ? impl->edgeGateChiSquared(edge) : 0.0;
}
int activeObservations(const CudaBundleAdjustment* object, const LandmarkVertex* v)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl ? impl->activeObservations(v) : 0;
}

// Extension (g2o's StructureOnlySolver<3> / ORB-SLAM's CreateNewMapPoints; the reference has none): landmarks from their edges and the poses.
TriangulationResult triangulateLandmarks(CudaBundleAdjustment* object, const TriangulationOptions& options, const std::vector<LandmarkVertex*>* subset)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::triangulateLandmarks: not an object of this library");
	return impl->triangulateLandmarks(options, subset);
}
TriangulationStatus triangulationStatus(const CudaBundleAdjustment* object, const LandmarkVertex* v)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl ? impl->triangulationStatus(v) : TriangulationStatus::NOT_SELECTED;
}

// Extension (g2o's motion-only bundle adjustment / ORB-SLAM's PoseOptimization; the reference has none): poses from their edges and the landmarks.
PoseRefinementResult refinePoses(CudaBundleAdjustment* object, const PoseRefinementOptions& options, const std::vector<PoseVertex*>* subset)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::refinePoses: not an object of this library");
	return impl->refinePoses(options, subset);
}
PoseRefinementStatus poseRefinementStatus(const CudaBundleAdjustment* object, const PoseVertex* v)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl ? impl->poseRefinementStatus(v) : PoseRefinementStatus::NOT_SELECTED;
}

// Extension (the PnP-RANSAC half of ORB-SLAM's relocalisation; the reference has none): poses from their edges and the landmarks alone.
PoseLocalizationResult localizePoses(CudaBundleAdjustment* object, const PoseLocalizationOptions& options, const std::vector<PoseVertex*>* subset)
{
	auto* impl = dynamic_cast<HipBundleAdjustment*>(object);
	if (!impl) throw std::runtime_error("cuba::localizePoses: not an object of this library");
	return impl->localizePoses(options, subset);
}
PoseLocalizationStatus poseLocalizationStatus(const CudaBundleAdjustment* object, const PoseVertex* v)
{
	const auto* impl = dynamic_cast<const HipBundleAdjustment*>(object);
	return impl ? impl->poseLocalizationStatus(v) : PoseLocalizationStatus::NOT_SELECTED;
}

void addPosePrior(CudaBundleAdjustment* object, PosePrior* prior) { addFactor(object, prior); }
void removePosePrior(CudaBundleAdjustment* object, PosePrior* prior) { removeFactor(object, prior); }
double priorChiSquared(const CudaBundleAdjustment* object, const PosePrior* prior) { return factorChiSquared(object, prior); }

void addRelativePoseEdge(CudaBundleAdjustment* object, RelativePoseEdge* edge) { addFactor(object, edge); }
void removeRelativePoseEdge(CudaBundleAdjustment* object, RelativePoseEdge* edge) { removeFactor(object, edge); }
double relativePoseChiSquared(const CudaBundleAdjustment* object, const RelativePoseEdge* edge) { return factorChiSquared(object, edge); }

void addLandmarkPrior(CudaBundleAdjustment* object, LandmarkPrior* prior) { addFactor(object, prior); }
void removeLandmarkPrior(CudaBundleAdjustment* object, LandmarkPrior* prior) { removeFactor(object, prior); }
double landmarkPriorChiSquared(const CudaBundleAdjustment* object, const LandmarkPrior* prior) { return factorChiSquared(object, prior); }

void addPositionFactor(CudaBundleAdjustment* object, PositionFactor* factor) { addFactor(object, factor); }
void removePositionFactor(CudaBundleAdjustment* object, PositionFactor* factor) { removeFactor(object, factor); }
double positionFactorChiSquared(const CudaBundleAdjustment* object, const PositionFactor* factor) { return factorChiSquared(object, factor); }

void addDirectionFactor(CudaBundleAdjustment* object, DirectionFactor* factor) { addFactor(object, factor); }
void removeDirectionFactor(CudaBundleAdjustment* object, DirectionFactor* factor) { removeFactor(object, factor); }
double directionFactorChiSquared(const CudaBundleAdjustment* object, const DirectionFactor* factor) { return factorChiSquared(object, factor); }

void addRangeFactor(CudaBundleAdjustment* object, RangeFactor* factor) { addFactor(object, factor); }
void removeRangeFactor(CudaBundleAdjustment* object, RangeFactor* factor) { removeFactor(object, factor); }
double rangeFactorChiSquared(const CudaBundleAdjustment* object, const RangeFactor* factor) { return factorChiSquared(object, factor); }

void addPoseRangeFactor(CudaBundleAdjustment* object, PoseRangeFactor* factor) { addFactor(object, factor); }
void removePoseRangeFactor(CudaBundleAdjustment* object, PoseRangeFactor* factor) { removeFactor(object, factor); }
double poseRangeFactorChiSquared(const CudaBundleAdjustment* object, const PoseRangeFactor* factor) { return factorChiSquared(object, factor); }

}  // namespace cuba
