// outlier_gating.cpp -- ORB-SLAM's outlier handling between two runs, without a new topology: a first robust optimisation, then every
// reprojection edge whose chi-squared exceeds 5.991 (monocular) / 7.815 (stereo) or whose point is not in front of its camera is switched
// off ON THE DEVICE (cuba::gateEdges; g2o's setLevel(1) / computeActiveErrors, which the reference lacks), then a second optimisation on
// the survivors -- no removeEdge, no initialize(), no new structure (compare samples/local_ba_flow.cpp, which removes the edges).  With
// --rounds N the flow of ORB-SLAM's pose optimisation instead: N rounds of optimisation + classification, in which an edge that has
// recovered comes back.  Prints the objective per iteration, the counts of every classification and the landmarks left with fewer than
// two active observations (the ones ORB-SLAM culls); tests/test_host_edge_gating.py checks the numbers against the same flow driven
// through the C ABI from Python.
//
//   usage: outlier_gating graph.json [iters1=5] [iters2=10] [--rounds N]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <opencv2/core.hpp>
#include <cuda_bundle_adjustment.h>

template <int N>
static cuba::Array<double, N> readVec(const cv::FileNode& node)
{
	cuba::Array<double, N> a;
	int k = 0;
	for (const auto& v : node) { if (k >= N) break; a[k++] = double(v); }
	return a;
}

// the iterations of the last optimize(): batchStatistics() collects those of every run since initialize()
static void printRun(const cuba::CudaBundleAdjustment& ba, const char* what, size_t& shown)
{
	const auto& stats = ba.batchStatistics();
	for (; shown < stats.size(); shown++) std::printf("%s iter: %2d, chi2: %.6f\n", what, stats[shown].iteration + 1, stats[shown].chi2);
}

static void printCounts(const char* what, int round, const cuba::EdgeGateResult& r)
{
	std::printf("%s %d: active %lld %lld, gated by chi2 %lld %lld, gated by depth %lld, changed %lld\n", what, round, r.activeMono, r.activeStereo,
		r.gatedChi2Mono, r.gatedChi2Stereo, r.gatedDepth, r.changed);
}

int main(int argc, char** argv)
{
	int rounds = 0;
	std::vector<const char*> args;
	for (int i = 1; i < argc; i++)
	{
		if (!std::strcmp(argv[i], "--rounds") && i + 1 < argc) rounds = std::atoi(argv[++i]);
		else args.push_back(argv[i]);
	}
	if (args.empty()) { std::printf("usage: %s graph.json [iters1=5] [iters2=10] [--rounds N]\n", argv[0]); return 0; }
	const int iters1 = args.size() > 1 ? std::atoi(args[1]) : 5, iters2 = args.size() > 2 ? std::atoi(args[2]) : 10;
	cv::FileStorage fs(args[0], cv::FileStorage::READ);
	if (!fs.isOpened()) { std::fprintf(stderr, "cannot open %s\n", args[0]); return 1; }
	cuba::CameraParams cam;
	cam.fx = fs["fx"]; cam.fy = fs["fy"]; cam.cx = fs["cx"]; cam.cy = fs["cy"]; cam.bf = fs["bf"];

	std::vector<std::unique_ptr<cuba::PoseVertex>> poses;
	std::vector<std::unique_ptr<cuba::LandmarkVertex>> landmarks;
	std::vector<std::unique_ptr<cuba::MonoEdge>> mono;
	std::vector<std::unique_ptr<cuba::StereoEdge>> stereo;
	auto ba = cuba::CudaBundleAdjustment::create();
	for (const auto& n : fs["pose_vertices"])
	{
		poses.push_back(std::make_unique<cuba::PoseVertex>(int(n["id"]), Eigen::Quaterniond(readVec<4>(n["q"])), readVec<3>(n["t"]), cam, int(n["fixed"]) != 0));
		ba->addPoseVertex(poses.back().get());
	}
	for (const auto& n : fs["landmark_vertices"])
	{
		landmarks.push_back(std::make_unique<cuba::LandmarkVertex>(int(n["id"]), readVec<3>(n["Xw"]), int(n["fixed"]) != 0));
		ba->addLandmarkVertex(landmarks.back().get());
	}
	for (const auto& n : fs["monocular_edges"])
	{
		mono.push_back(std::make_unique<cuba::MonoEdge>(readVec<2>(n["measurement"]), double(n["information"]),
			ba->poseVertex(int(n["vertexP"])), ba->landmarkVertex(int(n["vertexL"]))));
		ba->addMonocularEdge(mono.back().get());
	}
	for (const auto& n : fs["stereo_edges"])
	{
		stereo.push_back(std::make_unique<cuba::StereoEdge>(readVec<3>(n["measurement"]), double(n["information"]),
			ba->poseVertex(int(n["vertexP"])), ba->landmarkVertex(int(n["vertexL"]))));
		ba->addStereoEdge(stereo.back().get());
	}
	ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(5.991), cuba::EdgeType::MONOCULAR);
	ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(7.815), cuba::EdgeType::STEREO);
	ba->initialize();

	const cuba::EdgeGate gate;          // 5.991 / 7.815, positive depth, every edge judged afresh
	size_t shown = 0;
	if (rounds > 0)
	{
		// pose-optimisation style: every round optimises, then classifies ALL edges -- one that fits again is let back in
		for (int r = 0; r < rounds; r++)
		{
			ba->optimize(iters2);
			printRun(*ba, ("round " + std::to_string(r)).c_str(), shown);
			printCounts("round", r, cuba::gateEdges(ba.get(), gate));
		}
	}
	else
	{
		ba->optimize(iters1);
		printRun(*ba, "stage1", shown);
		printCounts("gate", 0, cuba::gateEdges(ba.get(), gate));
		ba->optimize(iters2);
		printRun(*ba, "stage2", shown);
	}

	size_t off = 0, weak = 0;
	double worst = 0;
	for (const auto& e : mono) if (!cuba::edgeActive(ba.get(), e.get())) { off++; worst = std::max(worst, cuba::edgeGateChiSquared(ba.get(), e.get())); }
	for (const auto& e : stereo) if (!cuba::edgeActive(ba.get(), e.get())) { off++; worst = std::max(worst, cuba::edgeGateChiSquared(ba.get(), e.get())); }
	for (const auto& v : landmarks) if (!v->edges.empty() && cuba::activeObservations(ba.get(), v.get()) < 2) weak++;
	std::printf("switched off %zu of %zu edges (largest chi2 %.6f)\n", off, mono.size() + stereo.size(), worst);
	std::printf("landmarks with fewer than two active observations: %zu\n", weak);
	return 0;
}
