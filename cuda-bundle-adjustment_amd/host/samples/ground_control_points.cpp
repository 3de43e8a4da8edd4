// ground_control_points.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), frees every pose and every
// landmark and holds the gauge with landmark position priors instead (cuba::addLandmarkPrior; g2o's unary XYZ prior edge): a handful of
// "surveyed" ground-control points, evenly spread over the observed landmarks, each at the landmark's initial position with a
// centimetre-level information.  One of them -- the second -- is given a grossly wrong survey (metres off); under the Cauchy kernel it is
// weighted down instead of bending the map.  Prints the LM objective per iteration (edges plus priors), every control point's chi2 at
// the result (the gross one stands out), its estimate and its marginal covariance, which the priors alone make well defined.
//
//   usage: ground_control_points graph.json [iterations=10] [points=8] [kernel=3] [delta=3]
//          kernel: 0 none, 1 Huber, 2 Tukey, 3 Cauchy
//   output: "iter: <i>, chi2: <F>" per iteration, then per control point "control point <landmark id> chi2 <r^T Omega r>",
//           "control point <id> estimate <x> <y> <z>" and "control point <id> covariance" followed by its 9 numbers (column-major)
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
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2) { std::printf("usage: %s graph.json [iterations=10] [points=8] [kernel=3] [delta=3]\n", argv[0]); return 0; }
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	const int points = argc > 3 ? std::max(3, std::atoi(argv[3])) : 8;
	const int kernel = argc > 4 ? std::atoi(argv[4]) : 3;
	const double delta = argc > 5 ? std::atof(argv[5]) : 3.0;

	cv::FileStorage fs(argv[1], cv::FileStorage::READ);
	if (!fs.isOpened()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
	cuba::CameraParams cam;
	cam.fx = fs["fx"]; cam.fy = fs["fy"]; cam.cx = fs["cx"]; cam.cy = fs["cy"]; cam.bf = fs["bf"];

	std::vector<std::unique_ptr<cuba::PoseVertex>> poses;
	std::vector<std::unique_ptr<cuba::LandmarkVertex>> landmarks;
	std::vector<std::unique_ptr<cuba::MonoEdge>> mono;
	std::vector<std::unique_ptr<cuba::StereoEdge>> stereo;
	auto ba = cuba::CudaBundleAdjustment::create();
	for (const auto& n : fs["pose_vertices"])
	{
		const Eigen::Quaterniond q(readVec<4>(n["q"]));
		poses.push_back(std::make_unique<cuba::PoseVertex>(int(n["id"]), q, readVec<3>(n["t"]), cam, false));     // every pose free
		ba->addPoseVertex(poses.back().get());
	}
	for (const auto& n : fs["landmark_vertices"])
	{
		landmarks.push_back(std::make_unique<cuba::LandmarkVertex>(int(n["id"]), readVec<3>(n["Xw"]), false));     // every landmark free
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

	// the control points: evenly spread over the landmarks that are observed (file order), surveyed to a centimetre (information 1e4 I)
	std::vector<cuba::LandmarkVertex*> observed;
	for (const auto& l : landmarks) if (!l->edges.empty()) observed.push_back(l.get());
	if ((int)observed.size() < points) { std::fprintf(stderr, "the graph has fewer than %d observed landmarks\n", points); return 1; }
	std::vector<std::unique_ptr<cuba::LandmarkPrior>> priors;
	for (int j = 0; j < points; j++)
	{
		auto p = std::make_unique<cuba::LandmarkPrior>();
		p->vertex = observed[(size_t)j * observed.size() / (size_t)points];
		p->position = p->vertex->Xw;
		if (j == 1) { p->position[0] += 5.0; p->position[1] -= 3.0; p->position[2] += 4.0; }      // the gross one
		p->information = { 1e4, 0, 0, 0, 1e4, 0, 0, 0, 1e4 };
		p->kernel = static_cast<cuba::PoseFactorKernel>(kernel);
		p->delta = delta;
		cuba::addLandmarkPrior(ba.get(), p.get());
		priors.push_back(std::move(p));
	}
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	for (const auto& p : priors) std::printf("control point %d chi2 %.17g\n", p->vertex->id, cuba::landmarkPriorChiSquared(ba.get(), p.get()));
	for (const auto& p : priors) std::printf("control point %d estimate %.17g %.17g %.17g\n", p->vertex->id, p->vertex->Xw[0], p->vertex->Xw[1], p->vertex->Xw[2]);
	if (!cuba::computeCovariances(ba.get(), true))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	for (const auto& p : priors)
	{
		double C[9];
		if (!cuba::landmarkCovariance(ba.get(), p->vertex, C)) { std::printf("no covariance of control point %d\n", p->vertex->id); return 3; }
		std::printf("control point %d covariance\n", p->vertex->id);
		for (int k = 0; k < 9; k++) std::printf("%.17g%c", C[k], k % 3 == 2 ? '\n' : ' ');
	}
	return 0;
}
