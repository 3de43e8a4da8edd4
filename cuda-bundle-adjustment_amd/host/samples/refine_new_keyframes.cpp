// refine_new_keyframes.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets) as a small window and
// optimises it twice.  Run A starts from the file's estimate.  Run B gives every third free pose the value of the pose before it in the
// file -- a new keyframe whose start is a zero-motion guess --, refines ONLY those on the device against the file's landmarks, all of
// them held (cuba::refinePoses with a subset: outlier rounds of Levenberg-Marquardt trials per pose, ORB-SLAM's PoseOptimization) and
// then optimises.  A pose that is not accepted keeps its guess and is reported in the counts.
// Prints the counts per status and both runs' objective per iteration.
//
//   usage: refine_new_keyframes graph.json [iterations=10] [rounds=4] [trials=10] [robust_rounds=2] [min_inliers=10] [chi2_mono=5.991] [chi2_stereo=7.815]
//   output: "refined <n> of <m>: ok .. not_selected .. fixed .. few_observations .. singular .. few_inliers ..",
//           "A iter: <i>, chi2: <F>" and "B iter: <i>, chi2: <F>" per iteration, "final chi2 A <F> B <F>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include <opencv2/core.hpp>   // mini_opencv stand-in (JSON reader) unless real OpenCV is on the include path

#include <cuda_bundle_adjustment.h>

namespace
{
template <int N>
cuba::Array<double, N> readVec(const cv::FileNode& node)
{
	cuba::Array<double, N> a;
	int k = 0;
	for (const auto& v : node) { if (k >= N) break; a[k++] = double(v); }
	return a;
}

struct Window
{
	std::vector<std::unique_ptr<cuba::PoseVertex>> poses;
	std::vector<std::unique_ptr<cuba::LandmarkVertex>> landmarks;
	std::vector<std::unique_ptr<cuba::MonoEdge>> mono;
	std::vector<std::unique_ptr<cuba::StereoEdge>> stereo;
	cuba::CudaBundleAdjustment::Ptr ba;
};

bool load(const char* path, Window& w)
{
	cv::FileStorage fs(path, cv::FileStorage::READ);
	if (!fs.isOpened()) return false;
	cuba::CameraParams cam;
	cam.fx = fs["fx"]; cam.fy = fs["fy"]; cam.cx = fs["cx"]; cam.cy = fs["cy"]; cam.bf = fs["bf"];
	w.ba = cuba::CudaBundleAdjustment::create();
	for (const auto& n : fs["pose_vertices"])
	{
		const Eigen::Quaterniond q(readVec<4>(n["q"]));
		w.poses.push_back(std::make_unique<cuba::PoseVertex>(int(n["id"]), q, readVec<3>(n["t"]), cam, int(n["fixed"]) != 0));
		w.ba->addPoseVertex(w.poses.back().get());
	}
	for (const auto& n : fs["landmark_vertices"])
	{
		w.landmarks.push_back(std::make_unique<cuba::LandmarkVertex>(int(n["id"]), readVec<3>(n["Xw"]), int(n["fixed"]) != 0));
		w.ba->addLandmarkVertex(w.landmarks.back().get());
	}
	for (const auto& n : fs["monocular_edges"])
	{
		w.mono.push_back(std::make_unique<cuba::MonoEdge>(readVec<2>(n["measurement"]), double(n["information"]),
			w.ba->poseVertex(int(n["vertexP"])), w.ba->landmarkVertex(int(n["vertexL"]))));
		w.ba->addMonocularEdge(w.mono.back().get());
	}
	for (const auto& n : fs["stereo_edges"])
	{
		w.stereo.push_back(std::make_unique<cuba::StereoEdge>(readVec<3>(n["measurement"]), double(n["information"]),
			w.ba->poseVertex(int(n["vertexP"])), w.ba->landmarkVertex(int(n["vertexL"]))));
		w.ba->addStereoEdge(w.stereo.back().get());
	}
	w.ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(5.991), cuba::EdgeType::MONOCULAR);
	w.ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(7.815), cuba::EdgeType::STEREO);
	return true;
}

double run(const char* tag, Window& w, int iterations)
{
	w.ba->optimize(iterations);
	double last = 0;
	for (const auto& s : w.ba->batchStatistics()) { std::printf("%s iter: %2d, chi2: %.6f\n", tag, s.iteration, s.chi2); last = s.chi2; }
	return last;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2)
	{
		std::printf("usage: %s graph.json [iterations=10] [rounds=4] [trials=10] [robust_rounds=2] [min_inliers=10] [chi2_mono=5.991] [chi2_stereo=7.815]\n", argv[0]);
		return 0;
	}
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	cuba::PoseRefinementOptions options;
	if (argc > 3) options.rounds = std::atoi(argv[3]);
	if (argc > 4) options.iterations = std::atoi(argv[4]);
	if (argc > 5) options.robustRounds = std::atoi(argv[5]);
	if (argc > 6) options.minInliers = std::atoi(argv[6]);
	if (argc > 7) options.chi2Mono = std::atof(argv[7]);
	if (argc > 8) options.chi2Stereo = std::atof(argv[8]);

	Window a, b;
	if (!load(argv[1], a) || !load(argv[1], b)) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }

	a.ba->initialize();
	const double chiA = run("A", a, iterations);

	// (the guesses are taken from window A's copy of the file, so that a guess never copies another guess)
	std::vector<cuba::PoseVertex*> fresh;
	size_t k = 0;
	for (size_t i = 1; i < b.poses.size(); i++)
		if (!b.poses[i]->fixed && k++ % 3 == 0) fresh.push_back(b.poses[i].get());
	Window file;
	if (!load(argv[1], file)) return 1;
	for (size_t i = 1; i < b.poses.size(); i++)
		for (cuba::PoseVertex* v : fresh)
			if (v == b.poses[i].get()) { v->q = file.poses[i - 1]->q; v->t = file.poses[i - 1]->t; }
	b.ba->initialize();
	const cuba::PoseRefinementResult r = cuba::refinePoses(b.ba.get(), options, &fresh);
	static const char* const names[6] = { "ok", "not_selected", "fixed", "few_observations", "singular", "few_inliers" };
	std::printf("refined %lld of %zu:", r.count(cuba::PoseRefinementStatus::OK), fresh.size());
	for (int s = 0; s < 6; s++) std::printf(" %s %lld", names[s], r.counts[s]);
	std::printf("\n");
	const double chiB = run("B", b, iterations);
	std::printf("final chi2 A %.6f B %.6f\n", chiA, chiB);
	return 0;
}
