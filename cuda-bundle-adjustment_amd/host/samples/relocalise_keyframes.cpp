// relocalise_keyframes.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets) as a small window and
// optimises it twice.  Run A starts from the file's estimate.  Run B throws the poses of every third free keyframe away -- sets them to
// NaN: a relocalisation after tracking loss, a keyframe joined from another map --, gives ONLY those a value on the device from their
// 2-D - 3-D matches against the file's landmarks (cuba::localizePoses with a subset: a deterministic P3P RANSAC per pose), refines them
// with the landmarks held (cuba::refinePoses) and then optimises: ORB-SLAM's Relocalization followed by the window's bundle adjustment.
// Prints the counts per status, both runs' objective per iteration and how far run B's relocalised poses end from run A's.
//
//   usage: relocalise_keyframes graph.json [iterations=10] [hypotheses=256] [seed=0] [min_inliers=10] [chi2_mono=5.991] [chi2_stereo=7.815]
//   output: "localised <n> of <m>: ok .. not_selected .. fixed .. few_observations .. no_solution .. few_inliers ..",
//           "refined <n> of <m>", "A iter: <i>, chi2: <F>" and "B iter: <i>, chi2: <F>" per iteration, "final chi2 A <F> B <F>",
//           "largest distance of a relocalised pose from run A's (rotation angle in rad, translation relative to max(1, |t|)): <d>"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
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

// the larger of the rotation angle between two poses and |ta - tb|_inf / max(1, |tb|_inf)
double distance(const cuba::PoseVertex& a, const cuba::PoseVertex& b)
{
	const double* qa = a.q.coeffs().data();
	const double* qb = b.q.coeffs().data();
	double dot = 0, na = 0, nb = 0, dt = 0, tb = 1;
	for (int k = 0; k < 4; k++) { dot += qa[k] * qb[k]; na += qa[k] * qa[k]; nb += qb[k] * qb[k]; }
	for (int k = 0; k < 3; k++) { dt = std::max(dt, std::fabs(a.t.data()[k] - b.t.data()[k])); tb = std::max(tb, std::fabs(b.t.data()[k])); }
	const double c = std::min(1.0, std::fabs(dot) / std::sqrt(na * nb));
	const double d = std::max(2 * std::acos(c), dt / tb);
	return std::isnan(d) ? std::numeric_limits<double>::infinity() : d;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2)
	{
		std::printf("usage: %s graph.json [iterations=10] [hypotheses=256] [seed=0] [min_inliers=10] [chi2_mono=5.991] [chi2_stereo=7.815]\n", argv[0]);
		return 0;
	}
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	cuba::PoseLocalizationOptions options;
	if (argc > 3) options.hypotheses = std::atoi(argv[3]);
	if (argc > 4) options.seed = std::strtoull(argv[4], nullptr, 10);
	if (argc > 5) options.minInliers = std::atoi(argv[5]);
	if (argc > 6) options.chi2Mono = std::atof(argv[6]);
	if (argc > 7) options.chi2Stereo = std::atof(argv[7]);

	Window a, b;
	if (!load(argv[1], a) || !load(argv[1], b)) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }

	a.ba->initialize();
	const double chiA = run("A", a, iterations);

	std::vector<cuba::PoseVertex*> lost;
	std::vector<size_t> rows;
	size_t k = 0;
	const double nan = std::numeric_limits<double>::quiet_NaN();
	for (size_t i = 1; i < b.poses.size(); i++)
		if (!b.poses[i]->fixed && k++ % 3 == 0)
		{
			cuba::PoseVertex* v = b.poses[i].get();
			for (int c = 0; c < 4; c++) v->q.coeffs().data()[c] = nan;
			for (int c = 0; c < 3; c++) v->t.data()[c] = nan;
			lost.push_back(v); rows.push_back(i);
		}
	b.ba->initialize();
	const cuba::PoseLocalizationResult r = cuba::localizePoses(b.ba.get(), options, &lost);
	static const char* const names[6] = { "ok", "not_selected", "fixed", "few_observations", "no_solution", "few_inliers" };
	std::printf("localised %lld of %zu:", r.count(cuba::PoseLocalizationStatus::OK), lost.size());
	for (int s = 0; s < 6; s++) std::printf(" %s %lld", names[s], r.counts[s]);
	std::printf("\n");
	for (const cuba::PoseVertex* v : lost)
		if (cuba::poseLocalizationStatus(b.ba.get(), v) != cuba::PoseLocalizationStatus::OK)
			std::printf("pose %d is still lost (status %d): fix it or take it out before optimising\n", v->id, static_cast<int>(cuba::poseLocalizationStatus(b.ba.get(), v)));
	cuba::PoseRefinementOptions refine;
	refine.minInliers = options.minInliers; refine.chi2Mono = options.chi2Mono; refine.chi2Stereo = options.chi2Stereo;
	const cuba::PoseRefinementResult rr = cuba::refinePoses(b.ba.get(), refine, &lost);
	std::printf("refined %lld of %zu\n", rr.count(cuba::PoseRefinementStatus::OK), lost.size());
	const double chiB = run("B", b, iterations);
	std::printf("final chi2 A %.6f B %.6f\n", chiA, chiB);
	double worst = 0;
	for (size_t i : rows) worst = std::max(worst, distance(*b.poses[i], *a.poses[i]));
	std::printf("largest distance of a relocalised pose from run A's (rotation angle in rad, translation relative to max(1, |t|)): %.3e\n", worst);
	return 0;
}
