// triangulate_trace.cpp -- landmark triangulation in the host layer (../bundle_adjustment.cpp: cuba::triangulateLandmarks,
// triangulationStatus) without a GPU: the public API on a graph of two poses, five landmarks (the last one fixed) and ten edges, linked
// against the recording stand-ins fake_cuba_hip.cpp and fake_cuba_hip_triangulate.cpp, which print every C ABI call.  This program prints
// a marker line per step, then every vertex's status and Xw; tests/test_host_triangulation.py reads the output.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <cuda_bundle_adjustment.h>

using namespace cuba;
using V3 = Array<double, 3>;
using V2 = Array<double, 2>;

static std::vector<LandmarkVertex*> lms;

static void show(const char* step, const CudaBundleAdjustment* ba)
{
	std::printf("# %s: status", step);
	for (const LandmarkVertex* l : lms) std::printf(" %d", static_cast<int>(triangulationStatus(ba, l)));
	std::printf(", Xw");
	for (const LandmarkVertex* l : lms) std::printf(" %g %g %g", l->Xw.data()[0], l->Xw.data()[1], l->Xw.data()[2]);
	std::printf("\n");
}

static void counts(const TriangulationResult& r)
{
	std::printf("# counts");
	for (int k = 0; k < 8; k++) std::printf(" %lld", r.counts[k]);
	std::printf("\n");
}

// an implementation of the interface that is not this library's
struct Foreign : CudaBundleAdjustment
{
	BatchStatistics stats; TimeProfile profile;
	void addPoseVertex(PoseVertex*) override {}
	void addLandmarkVertex(LandmarkVertex*) override {}
	void addMonocularEdge(MonoEdge*) override {}
	void addStereoEdge(StereoEdge*) override {}
	PoseVertex* poseVertex(int) const override { return nullptr; }
	LandmarkVertex* landmarkVertex(int) const override { return nullptr; }
	void removePoseVertex(PoseVertex*) override {}
	void removeLandmarkVertex(LandmarkVertex*) override {}
	void removeEdge(BaseEdge*) override {}
	size_t nposes() const override { return 0; }
	size_t nlandmarks() const override { return 0; }
	size_t nedges() const override { return 0; }
	void setRobustKernels(RobustKernelType, double, EdgeType) override {}
	void initialize() override {}
	void optimize(int) override {}
	void clear() override {}
	const BatchStatistics& batchStatistics() const override { return stats; }
	const TimeProfile& timeProfile() const override { return profile; }
	double chiSquared(const BaseEdge*) const override { return 0; }
};

int main()
{
	CameraParams cam; cam.fx = cam.fy = 500; cam.cx = cam.cy = 250; cam.bf = 50;
	PoseVertex p0(0, Eigen::Quaterniond(1, 0, 0, 0), V3(0, 0, 0), cam, true), p1(1, Eigen::Quaterniond(1, 0, 0, 0), V3(1, 0, 0), cam, false);
	// (ids out of order: the solver numbers the free landmarks by id -- 3, 5, 7, 9 -> 0, 1, 2, 3 -- and the fixed one last)
	LandmarkVertex l7(7, V3(7, 0, 5), false), l3(3, V3(3, 0, 5), false), l9(9, V3(9, 0, 5), false), l5(5, V3(5, 0, 5), false), l1(1, V3(1, 0, 5), true);
	lms = { &l7, &l3, &l9, &l5, &l1 };
	std::vector<MonoEdge> edges;
	edges.reserve(10);
	for (LandmarkVertex* l : lms) { edges.emplace_back(V2(250, 250), 1.0, &p0, l); edges.emplace_back(V2(350, 250), 1.0, &p1, l); }
	auto ba = CudaBundleAdjustment::create();
	ba->addPoseVertex(&p0); ba->addPoseVertex(&p1);
	for (LandmarkVertex* l : lms) ba->addLandmarkVertex(l);
	for (MonoEdge& e : edges) ba->addMonocularEdge(&e);
	ba->initialize();
	show("before", ba.get());

	std::printf("# all landmarks with the default options\n");
	counts(triangulateLandmarks(ba.get(), TriangulationOptions()));
	show("all", ba.get());

	std::printf("# a dry run on a subset with options of its own\n");
	TriangulationOptions o; o.refineIterations = 3; o.minParallaxDeg = 0.5; o.chi2Mono = 4; o.chi2Stereo = 6; o.dryRun = true;
	l9.Xw = V3(-9, 0, 5);
	std::vector<LandmarkVertex*> subset = { &l9, &l3, nullptr };
	counts(triangulateLandmarks(ba.get(), o, &subset));
	show("dry run", ba.get());

	std::printf("# the same subset for real\n");
	o.dryRun = false;
	counts(triangulateLandmarks(ba.get(), o, &subset));
	show("subset", ba.get());

	std::printf("# the next optimize starts from the accepted positions\n");
	ba->optimize(1);
	show("optimized", ba.get());

	std::printf("# an object of another library is refused\n");
	Foreign other;
	try { triangulateLandmarks(&other, TriangulationOptions()); std::printf("no exception\n"); }
	catch (const std::runtime_error& e) { std::printf("std::runtime_error: %s\n", e.what()); }
	std::printf("# foreign status %d\n", static_cast<int>(triangulationStatus(&other, &l3)));

	std::printf("# clear() drops the statuses\n");
	ba->clear();
	show("cleared", ba.get());
	return 0;
}
