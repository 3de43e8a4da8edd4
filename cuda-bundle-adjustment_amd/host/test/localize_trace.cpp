// localize_trace.cpp -- pose localisation in the host layer (../bundle_adjustment.cpp: cuba::localizePoses, poseLocalizationStatus) without a
// GPU: the public API on a graph of four free poses, three landmarks (the last one fixed) and twelve edges, linked against the recording
// stand-ins fake_cuba_hip*.cpp, which print every C ABI call.  This program prints a marker line per step, then every pose vertex's status,
// q and t; tests/test_host_pose_localization.py reads the output.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <cuda_bundle_adjustment.h>

using namespace cuba;
using V3 = Array<double, 3>;
using V2 = Array<double, 2>;

static std::vector<PoseVertex*> poses;

static void show(const char* step, const CudaBundleAdjustment* ba)
{
	std::printf("# %s: status", step);
	for (const PoseVertex* p : poses) std::printf(" %d", static_cast<int>(poseLocalizationStatus(ba, p)));
	std::printf(", qt");
	for (const PoseVertex* p : poses)
		std::printf(" %g %g %g %g %g %g %g", p->q.coeffs().data()[0], p->q.coeffs().data()[1], p->q.coeffs().data()[2], p->q.coeffs().data()[3],
			p->t.data()[0], p->t.data()[1], p->t.data()[2]);
	std::printf("\n");
}

static void counts(const PoseLocalizationResult& r)
{
	std::printf("# counts");
	for (int k = 0; k < 6; k++) std::printf(" %lld", r.counts[k]);
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
	const Eigen::Quaterniond half(0.5, 0.5, 0.5, 0.5);       // (w, x, y, z)
	// (ids out of order: the solver numbers the free poses by id -- 3, 5, 7, 9 -> 0, 1, 2, 3)
	PoseVertex p7(7, half, V3(7, 0, 0), cam, false), p3(3, half, V3(3, 0, 0), cam, false), p9(9, half, V3(9, 0, 0), cam, false), p5(5, half, V3(5, 0, 0), cam, false);
	poses = { &p7, &p3, &p9, &p5 };
	LandmarkVertex l0(0, V3(0, 0, 5), false), l1(1, V3(1, 0, 5), false), l2(2, V3(2, 0, 5), true);
	std::vector<LandmarkVertex*> lms = { &l0, &l1, &l2 };
	std::vector<MonoEdge> edges;
	edges.reserve(12);
	for (PoseVertex* p : poses) for (LandmarkVertex* l : lms) edges.emplace_back(V2(250, 250), 1.0, p, l);
	auto ba = CudaBundleAdjustment::create();
	for (PoseVertex* p : poses) ba->addPoseVertex(p);
	for (LandmarkVertex* l : lms) ba->addLandmarkVertex(l);
	for (MonoEdge& e : edges) ba->addMonocularEdge(&e);
	ba->initialize();
	show("before", ba.get());

	std::printf("# all poses with the default options\n");
	counts(localizePoses(ba.get(), PoseLocalizationOptions()));
	show("all", ba.get());

	std::printf("# a dry run on a subset with options of its own\n");
	PoseLocalizationOptions o; o.hypotheses = 77; o.seed = 18446744073709551557ULL; o.chi2Mono = 4; o.chi2Stereo = 6; o.minInliers = 5; o.dryRun = true;
	p9.t = V3(-9, 0, 0);
	std::vector<PoseVertex*> subset = { &p9, &p3, nullptr };
	counts(localizePoses(ba.get(), o, &subset));
	show("dry run", ba.get());

	std::printf("# the same subset for real\n");
	o.dryRun = false;
	counts(localizePoses(ba.get(), o, &subset));
	show("subset", ba.get());

	std::printf("# the next optimize starts from the new poses\n");
	ba->optimize(1);
	show("optimized", ba.get());

	std::printf("# options out of range are refused before any call\n");
	for (int k = 0; k < 9; k++)
	{
		PoseLocalizationOptions bad;
		if (k == 0) bad.hypotheses = 0;
		if (k == 1) bad.hypotheses = 4097;
		if (k == 2) bad.minInliers = -1;
		if (k == 3) bad.chi2Mono = std::nan("");
		if (k == 4) bad.chi2Stereo = std::nan("");
		if (k == 5) bad.chi2Mono = INFINITY;
		if (k == 6) bad.chi2Stereo = INFINITY;
		if (k == 7) bad.chi2Mono = 0;
		if (k == 8) bad.chi2Stereo = -1;
		try { localizePoses(ba.get(), bad); std::printf("no exception\n"); }
		catch (const std::invalid_argument&) { std::printf("std::invalid_argument %d\n", k); }
	}
	show("refused", ba.get());

	std::printf("# an object of another library is refused\n");
	Foreign other;
	try { localizePoses(&other, PoseLocalizationOptions()); std::printf("no exception\n"); }
	catch (const std::runtime_error& e) { std::printf("std::runtime_error: %s\n", e.what()); }
	std::printf("# foreign status %d\n", static_cast<int>(poseLocalizationStatus(&other, &p3)));

	std::printf("# clear() drops the statuses\n");
	ba->clear();
	show("cleared", ba.get());
	return 0;
}
