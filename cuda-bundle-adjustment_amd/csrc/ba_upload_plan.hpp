// ba_upload_plan.hpp -- what one cuba_hip_set_graph[_begin / _partition] call refuses, and what it reuses of the previous upload: a pure
// function of what the handle had (UploadFacts), what the call asks (UploadCall) and one data-dependent bit (the caller's index arrays
// equal the previous call's).  No HIP, no member of cuba_hip_solver: cuba_hip_solver::setGraph (ba_setup.hip) fills the two structs, acts
// on the plan step by step and decides nothing itself; host/test/upload_plan_test.cpp enumerates every combination on the CPU.
#pragma once
#include <cstddef>

namespace cubahip {

constexpr int UPLOAD_POSE_LIMIT = 0x40000000;          // (= STEREO_BIT, ba_kernels.hpp: a sorted edge carries its pose index below that bit)

// what the handle had when the call arrived
struct UploadFacts
{
	bool haveGraph, haveStructure;
	int Pt, Pf, Lt, Lf, E;
	bool partitioned;            // a landmark range is in force (partHi >= 0), set by a ranged upload or by cuba_hip_set_partition
	bool devTopology;            // the sort in force was made on the device
	bool hostTopoValid;          // ... and the host arrays describe it (made there, or read back)
	bool reorderActive;          // an internal pose order is in force
	bool lmOrderActive;          // an internal landmark order is in force
	bool sortedValuesValid;      // the sorted values of the previous upload are gathered (false while a two-step upload is open)
	bool valuesPartial;          // ... but only those of a rank's own landmarks crossed PCIe
	bool sortedValuesFit;        // the sorted value buffers have E entries
	bool edgesHeld;              // the host copy of the previous call's index arrays has E entries
	bool deviceSetup, poseReorder, lmReorder;          // the options
	bool noCache;                // CUBA_HIP_NO_STRUCTURE_CACHE: the A/B knob for set-up timings
};

// what the call asks
struct UploadCall
{
	int Pt, Pf, Lt, Lf, E;
	int ownLo, ownHi;            // ownHi >= 0: cuba_hip_set_graph_partition
	bool deferValues;            // cuba_hip_set_graph_begin
	bool hintEdges, hintValues;  // the cuba_hip_hint_unchanged promise, taken (and so consumed) at the top of setGraph
	bool nullPoseArray, nullLandmarkArray, nullEdgeArray;
	size_t scalarSize;
	bool ranged() const { return ownHi >= 0; }
};

struct UploadPlan
{
	const char* const refusal;   // nullptr, or the text of CUBA_HIP_ERR_INVALID_ARGUMENT; every decision below is false then
	const bool sameEdges;        // the caller's index arrays are the previous call's, compared or promised: ONLY this decides the gate
	const bool useDev;           // device pipeline (the host pipeline: "device_setup" = 0, or a graph without edges)
	const bool lmOrderWanted;    // the internal landmark order a fresh handle would choose for the new counts and range
	const bool keepPoseOrder;    // device pipeline: the internal pose order found for this very topology stays
	const bool reuseSort;        // device pipeline: permutation and sorted index arrays stay
	const bool reuseHostSort;    // host pipeline: the same
	const bool keepValues;       // the sorted values stay: nothing of meas / omega crosses PCIe
	const bool deferValues;      // meas / omega cross on the second stream, enqueued last; need() gathers them
	const bool mayKeepStructure; // the symbolic structure stays if the sort does (host pipeline: or sorts to the same arrays)
};

inline const char* uploadRefusal(const UploadCall& c)
{
	if (c.ranged() && (c.ownLo < 0 || c.ownHi > c.Lt || c.ownLo > c.ownHi)) return "bad landmark range";
	if (c.Pt < 0 || c.Lt < 0 || c.E < 0 || c.Pf < 0 || c.Pf > c.Pt || c.Lf < 0 || c.Lf > c.Lt) return "bad vertex counts";
	if (c.Pt >= UPLOAD_POSE_LIMIT) return "too many poses";
	// the per-edge linearisation record carries 2*landmark+stereo in a Scalar slot: exact in fp32 only below 2^24
	if (c.scalarSize == 4 && c.Lt >= (1 << 23)) return "fp32 build: at most 2^23 - 1 landmarks";
	if ((c.Pt && c.nullPoseArray) || (c.Lt && c.nullLandmarkArray) || (c.E && c.nullEdgeArray)) return "null array";
	return nullptr;
}

inline bool sameCounts(const UploadFacts& f, const UploadCall& c) { return f.Pt == c.Pt && f.Pf == c.Pf && f.Lt == c.Lt && f.Lf == c.Lf && f.E == c.E; }

// the index arrays of this call may be the previous call's at all
// (a ranged upload changes what the handle evaluates: nothing of the previous call is reused, and the sort runs in the caller's landmark order)
inline bool edgesComparable(const UploadFacts& f, const UploadCall& c)
{
	return !uploadRefusal(c) && !f.noCache && !c.ranged() && f.haveGraph && f.edgesHeld && sameCounts(f, c);
}

// ... and nobody promised it: the caller's arrays are compared with the host copy, E entries each
inline bool needsEdgeCompare(const UploadFacts& f, const UploadCall& c) { return edgesComparable(f, c) && !c.hintEdges; }

// edgesEqual: the outcome of that comparison (read only where needsEdgeCompare)
inline UploadPlan planUpload(const UploadFacts& f, const UploadCall& c, bool edgesEqual)
{
	if (const char* refusal = uploadRefusal(c)) return UploadPlan{ refusal, false, false, false, false, false, false, false, false, false };
	// the very same index arrays as in the previous call (re-initialisation of an unchanged graph): the sort, the permutation and the
	// sorted index arrays are all still valid -- where they exist in the form this call needs, below
	const bool sameEdges = edgesComparable(f, c) && (c.hintEdges || edgesEqual);
	const bool promisedValues = sameEdges && c.hintEdges && c.hintValues;
	const bool mayKeepStructure = !f.noCache && !c.ranged() && f.haveStructure && !f.partitioned && sameCounts(f, c);
	const bool useDev = f.deviceSetup && c.E > 0;
	// (a landmark partition names its range in the caller's numbering: only the whole range leaves the internal order alone)
	const bool lmOrderWanted = f.lmReorder && c.Lf > 1 && c.E > 0 && (!c.ranged() || (c.ownLo <= 0 && c.ownHi >= c.Lt));
	// ---- device pipeline ----
	// (the kept sort carries the landmark order it was made under: a changed "landmark_reorder", or a landmark partition in force until
	// this call, takes effect here)
	const bool lmOrderFits = f.lmOrderActive == lmOrderWanted;
	// (an internal pose order found for this very topology is kept -- while "pose_reorder" is on --; otherwise it starts over as the identity)
	const bool keepPoseOrder = useDev && f.reorderActive && f.poseReorder && sameEdges && f.devTopology && mayKeepStructure && lmOrderFits;
	const bool reuseSort = useDev && sameEdges && f.devTopology && (keepPoseOrder || !f.reorderActive) && lmOrderFits;
	const bool keepValues = promisedValues && reuseSort && f.sortedValuesValid && !f.valuesPartial && f.sortedValuesFit;
	const bool deferValues = useDev && c.deferValues && !c.ranged() && !keepValues;
	// ---- host pipeline ----
	// the host-side sort of the previous call does not exist (device path), or it was read back from a device sort in an internal pose or
	// landmark order, which the host pipeline leaves: its indices do not name the rows this call uploads
	const bool reuseHostSort = !useDev && sameEdges && f.hostTopoValid && !f.reorderActive && !f.lmOrderActive;
	return UploadPlan{ nullptr, sameEdges, useDev, lmOrderWanted, keepPoseOrder, reuseSort, reuseHostSort, keepValues, deferValues, mayKeepStructure };
}

}  // namespace cubahip
