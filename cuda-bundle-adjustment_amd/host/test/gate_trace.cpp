// gate_trace.cpp -- the edge levels of the host layer (../bundle_adjustment.cpp: cuba::gateEdges, setEdgeActive, edgeActive,
// activeObservations) without a GPU: the public API on a graph of two poses, two landmarks and four edges, linked against the recording
// stand-in fake_cuba_hip.cpp, which prints every C ABI call.  This program prints a marker line per step and the levels after it;
// tests/test_host_edge_gating.py reads the output.
#include <cstdio>
#include <vector>

#include <cuda_bundle_adjustment.h>

using namespace cuba;
using V3 = Array<double, 3>;
using V2 = Array<double, 2>;

static std::vector<MonoEdge*> all;

static void show(const char* step, const CudaBundleAdjustment* ba, const LandmarkVertex* l0, const LandmarkVertex* l1)
{
	std::printf("# %s: active", step);
	for (const MonoEdge* e : all) std::printf(" %d", edgeActive(ba, e) ? 1 : 0);
	std::printf(", observations %d %d\n", activeObservations(ba, l0), activeObservations(ba, l1));
}

int main()
{
	CameraParams cam; cam.fx = cam.fy = 500; cam.cx = cam.cy = 250; cam.bf = 50;
	PoseVertex p0(0, Eigen::Quaterniond(1, 0, 0, 0), V3(0, 0, 0), cam, true), p1(1, Eigen::Quaterniond(1, 0, 0, 0), V3(1, 0, 0), cam, false);
	LandmarkVertex l0(0, V3(0, 0, 5), false), l1(1, V3(1, 0, 6), false);
	MonoEdge e00(V2(250, 250), 1.0, &p0, &l0), e10(V2(350, 250), 1.0, &p1, &l0), e01(V2(333, 250), 1.0, &p0, &l1), e11(V2(416, 250), 1.0, &p1, &l1);
	all = { &e00, &e10, &e01, &e11 };
	auto ba = CudaBundleAdjustment::create();
	ba->addPoseVertex(&p0); ba->addPoseVertex(&p1); ba->addLandmarkVertex(&l0); ba->addLandmarkVertex(&l1);
	for (MonoEdge* e : all) ba->addMonocularEdge(e);

	std::printf("# no gate: nothing of it crosses the C ABI\n");
	ba->initialize(); ba->optimize(1);
	show("plain", ba.get(), &l0, &l1);

	std::printf("# a level set by hand goes up with the next optimize, once\n");
	setEdgeActive(ba.get(), &e10, false);
	show("e10 off", ba.get(), &l0, &l1);
	ba->optimize(1);
	ba->optimize(1);

	std::printf("# gateEdges: dry run, then a classification (the stand-in keeps every edge: e10 comes back)\n");
	EdgeGate dry; dry.mode = EdgeGateMode::DRY_RUN;
	gateEdges(ba.get(), dry);
	show("dry run", ba.get(), &l0, &l1);
	const EdgeGateResult r = gateEdges(ba.get(), EdgeGate());
	std::printf("# counts %lld %lld %lld %lld %lld %lld, ungated chi2 %g %g %g %g\n", r.activeMono, r.activeStereo, r.gatedChi2Mono, r.gatedChi2Stereo, r.gatedDepth,
		r.changed, edgeGateChiSquared(ba.get(), &e00), edgeGateChiSquared(ba.get(), &e10), edgeGateChiSquared(ba.get(), &e01), edgeGateChiSquared(ba.get(), &e11));
	show("classified", ba.get(), &l0, &l1);

	std::printf("# the levels survive a change of the graph that keeps the edge; the level of an edge that leaves goes with it\n");
	setEdgeActive(ba.get(), &e01, false); setEdgeActive(ba.get(), &e11, false);
	ba->removeEdge(&e11);
	ba->initialize(); ba->optimize(1);
	show("e11 removed", ba.get(), &l0, &l1);
	ba->addMonocularEdge(&e11);
	ba->initialize(); ba->optimize(1);
	show("e11 back", ba.get(), &l0, &l1);

	std::printf("# the last level switched on again: the handle's gate is cleared\n");
	setEdgeActive(ba.get(), &e01, true);
	ba->optimize(1);
	ba->optimize(1);

	std::printf("# clear() drops all levels\n");
	setEdgeActive(ba.get(), &e00, false);
	ba->clear();
	show("cleared", ba.get(), &l0, &l1);
	return 0;
}
