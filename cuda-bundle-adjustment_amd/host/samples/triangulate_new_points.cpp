// triangulate_new_points.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets) as a small window and
// optimises it twice.  Run A starts from the file's estimate.  Run B gives every third free landmark a useless start -- Xw = (0, 0, 0),
// a map point that has just been created --, triangulates ONLY those on the device from the file's poses and their observations
// (cuba::triangulateLandmarks with a subset: linear start, Gauss-Newton refinement, acceptance tests) and then optimises.  A landmark
// that is not accepted keeps its zeros, is reported in the counts and weighs on run B's objective; a real pipeline would drop it.
// Prints the counts per status and both runs' objective per iteration.
//
//   usage: triangulate_new_points graph.json [iterations=10] [refine=5] [min_parallax_deg=1] [chi2_mono=5.991] [chi2_stereo=7.815]
//   output: "triangulated <n> of <m>: ok .. not_selected .. fixed .. few_observations .. low_parallax .. singular .. behind_camera .. chi2 ..",
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
		std::printf("usage: %s graph.json [iterations=10] [refine=5] [min_parallax_deg=1] [chi2_mono=5.991] [chi2_stereo=7.815]\n", argv[0]);
		return 0;
	}
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	cuba::TriangulationOptions options;
	if (argc > 3) options.refineIterations = std::atoi(argv[3]);
	if (argc > 4) options.minParallaxDeg = std::atof(argv[4]);
	if (argc > 5) options.chi2Mono = std::atof(argv[5]);
	if (argc > 6) options.chi2Stereo = std::atof(argv[6]);

	Window a, b;
	if (!load(argv[1], a) || !load(argv[1], b)) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }

	a.ba->initialize();
	const double chiA = run("A", a, iterations);

	std::vector<cuba::LandmarkVertex*> fresh;
	size_t k = 0;
	for (const auto& l : b.landmarks)
		if (!l->fixed && k++ % 3 == 0) { l->Xw = cuba::Array<double, 3>(0.0, 0.0, 0.0); fresh.push_back(l.get()); }
	b.ba->initialize();
	const cuba::TriangulationResult r = cuba::triangulateLandmarks(b.ba.get(), options, &fresh);
	static const char* const names[8] = { "ok", "not_selected", "fixed", "few_observations", "low_parallax", "singular", "behind_camera", "chi2" };
	std::printf("triangulated %lld of %zu:", r.count(cuba::TriangulationStatus::OK), fresh.size());
	for (int s = 0; s < 8; s++) std::printf(" %s %lld", names[s], r.counts[s]);
	std::printf("\n");
	const double chiB = run("B", b, iterations);
	std::printf("final chi2 A %.6f B %.6f\n", chiA, chiB);
	return 0;
}
