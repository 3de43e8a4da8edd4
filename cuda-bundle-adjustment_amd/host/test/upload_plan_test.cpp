// upload_plan_test.cpp -- every combination of what a handle can have and what a cuba_hip_set_graph call can ask, through planUpload
// (csrc/ba_upload_plan.hpp), without a GPU: tests/test_upload_plan.py.  The enumeration also visits states no handle reaches (an internal
// landmark order without a device sort, say): the invariants hold there too, so no argument about reachability is needed.
// Each invariant names the defect it guards; prints "FAILED <invariant>: <case>" for the first case that breaks one and exits 1.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "ba_upload_plan.hpp"

using namespace cubahip;

enum Form { ONE_CALL, BEGIN, RANGED_PART, RANGED_WHOLE, FORMS };
static const char* const FORM_NAMES[FORMS] = { "one call", "begin", "ranged over a part", "ranged over the whole range" };
static const char* const FACT_NAMES[16] = { "haveGraph", "haveStructure", "sameCounts", "partitioned", "devTopology", "hostTopoValid", "reorderActive",
	"lmOrderActive", "sortedValuesValid", "valuesPartial", "sortedValuesFit", "edgesHeld", "deviceSetup", "poseReorder", "lmReorder", "noCache" };
enum { HAVE_GRAPH, HAVE_STRUCTURE, SAME_COUNTS, PARTITIONED, DEV_TOPOLOGY, HOST_TOPO_VALID, REORDER_ACTIVE, LM_ORDER_ACTIVE, SORTED_VALUES_VALID,
	VALUES_PARTIAL, SORTED_VALUES_FIT, EDGES_HELD, DEVICE_SETUP, POSE_REORDER, LM_REORDER, NO_CACHE };

struct Case { unsigned bits; Form form; bool empty, hintEdges, hintValues, edgesEqual; };

static UploadCall callOf(const Case& k)
{
	UploadCall c{};
	c.Pt = 5; c.Pf = 4; c.Lt = 10; c.Lf = 8; c.E = k.empty ? 0 : 20;
	c.ownLo = 0; c.ownHi = k.form == RANGED_PART ? 6 : k.form == RANGED_WHOLE ? c.Lt : -1;
	c.deferValues = k.form == BEGIN;
	c.hintEdges = k.hintEdges; c.hintValues = k.hintValues;
	c.scalarSize = 8;
	return c;
}

static UploadFacts factsOf(const Case& k)
{
	const auto bit = [&](int b) { return (k.bits >> b & 1) != 0; };
	const UploadCall c = callOf(k);
	UploadFacts f{};
	f.haveGraph = bit(HAVE_GRAPH); f.haveStructure = bit(HAVE_STRUCTURE);
	f.Pt = bit(SAME_COUNTS) ? c.Pt : c.Pt + 1; f.Pf = c.Pf; f.Lt = c.Lt; f.Lf = c.Lf; f.E = c.E;
	f.partitioned = bit(PARTITIONED); f.devTopology = bit(DEV_TOPOLOGY); f.hostTopoValid = bit(HOST_TOPO_VALID);
	f.reorderActive = bit(REORDER_ACTIVE); f.lmOrderActive = bit(LM_ORDER_ACTIVE);
	f.sortedValuesValid = bit(SORTED_VALUES_VALID); f.valuesPartial = bit(VALUES_PARTIAL); f.sortedValuesFit = bit(SORTED_VALUES_FIT);
	f.edgesHeld = bit(EDGES_HELD); f.deviceSetup = bit(DEVICE_SETUP); f.poseReorder = bit(POSE_REORDER); f.lmReorder = bit(LM_REORDER);
	f.noCache = bit(NO_CACHE);
	return f;
}

static UploadPlan planOf(const Case& k) { return planUpload(factsOf(k), callOf(k), k.edgesEqual); }

static std::string describe(const Case& k)
{
	std::string s = std::string(FORM_NAMES[k.form]) + (k.empty ? ", no edges" : "") + (k.hintEdges ? ", edges promised" : "")
		+ (k.hintValues ? ", values promised" : "") + (k.edgesEqual ? ", edges equal" : ", edges differ") + "; facts:";
	for (int b = 0; b < 16; b++) if (k.bits >> b & 1) s += std::string(" ") + FACT_NAMES[b];
	return s;
}

static std::map<std::string, std::string> failures;          // invariant -> first case that broke it
static void expect(bool ok, const char* invariant, const Case& k) { if (!ok && !failures.count(invariant)) failures[invariant] = describe(k); }
static void expectText(bool ok, const char* invariant, const char* what) { if (!ok && !failures.count(invariant)) failures[invariant] = what; }

static bool sameDecisions(const UploadPlan& a, const UploadPlan& b)
{
	return a.sameEdges == b.sameEdges && a.useDev == b.useDev && a.lmOrderWanted == b.lmOrderWanted && a.keepPoseOrder == b.keepPoseOrder
		&& a.reuseSort == b.reuseSort && a.reuseHostSort == b.reuseHostSort && a.keepValues == b.keepValues && a.deferValues == b.deferValues
		&& a.mayKeepStructure == b.mayKeepStructure;
}

static void refusals()
{
	const char* inv = "refusals: today's checks, order and texts, whatever the hints";
	struct R { const char* name; void (*breakIt)(UploadCall&); const char* text; };
	const R list[] = {
		{ "range below 0", [](UploadCall& c) { c.ownLo = -1; c.ownHi = 4; }, "bad landmark range" },
		{ "range past the landmarks", [](UploadCall& c) { c.ownHi = c.Lt + 1; }, "bad landmark range" },
		{ "range backwards", [](UploadCall& c) { c.ownLo = 5; c.ownHi = 4; }, "bad landmark range" },
		{ "range AND counts: the range is seen first", [](UploadCall& c) { c.ownLo = 5; c.ownHi = 4; c.Pf = c.Pt + 1; }, "bad landmark range" },
		{ "more free poses than poses", [](UploadCall& c) { c.Pf = c.Pt + 1; }, "bad vertex counts" },
		{ "negative edges", [](UploadCall& c) { c.E = -1; }, "bad vertex counts" },
		{ "more free landmarks than landmarks", [](UploadCall& c) { c.Lf = c.Lt + 1; }, "bad vertex counts" },
		{ "too many poses", [](UploadCall& c) { c.Pt = UPLOAD_POSE_LIMIT; }, "too many poses" },
		{ "fp32 landmark limit", [](UploadCall& c) { c.scalarSize = 4; c.Lt = 1 << 23; }, "fp32 build: at most 2^23 - 1 landmarks" },
		{ "null pose array", [](UploadCall& c) { c.nullPoseArray = true; }, "null array" },
		{ "null landmark array", [](UploadCall& c) { c.nullLandmarkArray = true; }, "null array" },
		{ "null edge array", [](UploadCall& c) { c.nullEdgeArray = true; }, "null array" },
	};
	Case k{ 0xffffu & ~(1u << NO_CACHE) & ~(1u << PARTITIONED), ONE_CALL, false, false, false, true };
	for (const R& r : list)
		for (int hints = 0; hints < 4; hints++)
		{
			k.hintEdges = hints & 1; k.hintValues = hints >> 1;
			UploadCall c = callOf(k);
			r.breakIt(c);
			const UploadPlan p = planUpload(factsOf(k), c, true);
			expectText(p.refusal && !std::strcmp(p.refusal, r.text), inv, r.name);
			// (a refused call must not read the caller's arrays -- they may be the null ones -- and decides nothing)
			expectText(!needsEdgeCompare(factsOf(k), c) && sameDecisions(p, UploadPlan{ p.refusal, false, false, false, false, false, false, false, false, false }), inv, r.name);
		}
	// the limits themselves are accepted on the other side
	UploadCall c = callOf(k);
	c.Lt = 1 << 23;
	expectText(!planUpload(factsOf(k), c, true).refusal, inv, "2^23 landmarks in the fp64 build");
	c = callOf(k); c.E = 0; c.nullEdgeArray = true;
	expectText(!planUpload(factsOf(k), c, true).refusal, inv, "null edge arrays of a graph without edges");
}

int main()
{
	long long cases = 0;
	const char* const DECISIONS[9] = { "sameEdges", "useDev", "lmOrderWanted", "keepPoseOrder", "reuseSort", "reuseHostSort", "keepValues", "deferValues", "mayKeepStructure" };
	long long seenTrue[9] = {}, seenFalse[9] = {};
	bool gateKeptWithoutHostSort = false;
	for (unsigned bits = 0; bits < (1u << 16); bits++)
		for (int form = 0; form < FORMS; form++)
			for (int rest = 0; rest < 16; rest++)
			{
				const Case k{ bits, (Form)form, (rest & 1) != 0, (rest & 2) != 0, (rest & 4) != 0, (rest & 8) != 0 };
				const UploadFacts f = factsOf(k);
				const UploadCall c = callOf(k);
				const UploadPlan p = planOf(k);
				cases++;
				expect(!p.refusal, "every enumerated call is a valid one", k);
				const bool d[9] = { p.sameEdges, p.useDev, p.lmOrderWanted, p.keepPoseOrder, p.reuseSort, p.reuseHostSort, p.keepValues, p.deferValues, p.mayKeepStructure };
				for (int i = 0; i < 9; i++) (d[i] ? seenTrue : seenFalse)[i]++;

				// a ranged upload changes what the handle evaluates: it reuses nothing of the previous call and defers nothing
				// (guards: a rank keeping the sort or the values of a whole upload, whose landmark order is not the caller's)
				if (c.ranged())
					expect(!p.sameEdges && !p.keepPoseOrder && !p.reuseSort && !p.reuseHostSort && !p.keepValues && !p.deferValues && !p.mayKeepStructure,
						"a ranged call reuses nothing and defers nothing", k);

				// guards: the mutant "keepValues whenever edges are promised" (new values under a promise of the edges alone ran on the old ones),
				// the begin-without-end values that were never gathered, and the half-filled values a ranged upload leaves
				if (p.keepValues)
					expect(c.hintEdges && c.hintValues && p.reuseSort && f.sortedValuesValid && !f.valuesPartial && f.sortedValuesFit,
						"keepValues implies promised values, reuseSort, sortedValuesValid, not valuesPartial", k);

				// guards: "landmark_reorder" not taking effect with an upload of the same index arrays (reorder_options, hsc in the last bits),
				// and a whole upload after a ranged one keeping a sort made in the caller's landmark order (partition, check 5)
				if (p.reuseSort)
					expect(p.sameEdges && f.devTopology && p.useDev && f.lmOrderActive == p.lmOrderWanted,
						"reuseSort implies sameEdges, devTopology, useDev and the landmark order a fresh upload would choose", k);

				// guards: "pose_reorder" = 0 not taking effect with an upload of the same index arrays (reorder_options, check 5)
				if (p.keepPoseOrder)
					expect(f.poseReorder && f.reorderActive && p.reuseSort, "keepPoseOrder implies poseReorder, reorderActive and reuseSort", k);
				// (and an order that is not kept ends: the sort made under it goes with it)
				if (f.reorderActive && !p.keepPoseOrder) expect(!p.reuseSort, "a pose order that ends takes its sort along", k);

				// guards: chi2 5e13 (orders, check 4) -- the host pipeline reusing a host topology read back from a device sort in an internal
				// order for rows it uploads in the caller's
				if (p.reuseHostSort)
					expect(!p.useDev && p.sameEdges && f.hostTopoValid && !f.reorderActive && !f.lmOrderActive,
						"reuseHostSort implies hostTopoValid and no internal pose or landmark order", k);

				// the gate is kept exactly when the edges are the previous call's, on either pipeline and whatever can be reused of the sort
				// (guards: the two meanings of the old sameInput -- a host-path upload that cannot reuse its sort must still keep the mask)
				{
					Case plain = k;
					plain.bits &= ~(1u << DEV_TOPOLOGY | 1u << HOST_TOPO_VALID | 1u << REORDER_ACTIVE | 1u << LM_ORDER_ACTIVE | 1u << DEVICE_SETUP
						| 1u << HAVE_STRUCTURE | 1u << PARTITIONED | 1u << SORTED_VALUES_VALID | 1u << VALUES_PARTIAL | 1u << SORTED_VALUES_FIT
						| 1u << POSE_REORDER | 1u << LM_REORDER);
					const bool spec = !f.noCache && !c.ranged() && f.haveGraph && f.edgesHeld && sameCounts(f, c) && (c.hintEdges || k.edgesEqual);
					expect(p.sameEdges == spec && p.sameEdges == planOf(plain).sameEdges, "the gate is kept exactly when sameEdges, on either path", k);
					if (p.sameEdges && !p.useDev && !p.reuseHostSort) gateKeptWithoutHostSort = true;
				}

				// with the no-cache knob nothing is reused (the A/B knob of the set-up timings must time a fresh upload)
				if (f.noCache)
					expect(!p.sameEdges && !p.keepPoseOrder && !p.reuseSort && !p.reuseHostSort && !p.keepValues && !p.mayKeepStructure,
						"with the no-cache knob nothing is reused", k);

				// the structure: only at unchanged counts, on a whole-range handle that has one
				if (p.mayKeepStructure) expect(f.haveStructure && !f.partitioned && sameCounts(f, c) && !c.ranged(), "mayKeepStructure implies a structure at these counts, unpartitioned", k);

				// the second stream carries the values only when the caller asked for it and they are needed
				if (p.deferValues) expect(c.deferValues && p.useDev && !p.keepValues && c.E > 0, "deferValues implies a begin on the device pipeline that needs the values", k);

				// the device pipeline: the option, and edges to sort; the landmark order: never for a part of the range
				expect(p.useDev == (f.deviceSetup && c.E > 0), "useDev is device_setup and a graph with edges", k);
				if (k.form == RANGED_PART) expect(!p.lmOrderWanted, "a part of the landmark range keeps the caller's landmark order", k);

				// the E-long comparison runs exactly when its outcome is read ...
				{
					Case other = k; other.edgesEqual = !k.edgesEqual;
					const bool read = !sameDecisions(p, planOf(other));
					expect(!read || needsEdgeCompare(f, c), "the comparison's outcome is read only where needsEdgeCompare", k);
					// ... and when today's code runs it: the counts are equal, a graph exists, the call is not ranged, caching is on, no promise
					expect(needsEdgeCompare(f, c) == (sameCounts(f, c) && f.haveGraph && f.edgesHeld && !c.ranged() && !f.noCache && !c.hintEdges),
						"needsEdgeCompare: equal counts, a graph, not ranged, caching on, not promised", k);
				}

				// a promise of values without one of the edges is no promise (cuba_hip_hint_unchanged stores none)
				if (!c.hintEdges) expect(!p.keepValues, "values are never kept without promised edges", k);
			}
	refusals();
	// every decision is taken both ways somewhere: an invariant over a constant says nothing
	for (int i = 0; i < 9; i++)
		expectText(seenTrue[i] > 0 && seenFalse[i] > 0, "every decision is true somewhere and false somewhere", DECISIONS[i]);
	expectText(gateKeptWithoutHostSort, "the gate is kept exactly when sameEdges, on either path", "no case keeps the gate without reusing the host sort");
	for (const auto& kv : failures) std::printf("FAILED %s: %s\n", kv.first.c_str(), kv.second.c_str());
	if (!failures.empty()) return 1;
	std::printf("upload plan: %lld cases, all invariants hold\n", cases);
	return 0;
}
