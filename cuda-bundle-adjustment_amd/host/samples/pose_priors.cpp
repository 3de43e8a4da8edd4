// pose_priors.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), frees every pose and holds the
// gauge with SE(3) pose priors instead (cuba::addPosePrior; g2o's unary pose edges): a strong prior anchors the first pose at its initial
// value, loose full-pose priors -- GPS / INS-like readings -- sit on every k-th pose.  Prints the LM objective per iteration (edges plus
// priors), every prior's chi2 at the result and the marginal covariance of the last pose, which the priors alone make well defined.
//
//   usage: pose_priors graph.json [iterations=10] [k=5] [huber=1]
//   output: "iter: <i>, chi2: <F>" per iteration, "prior <pose id> chi2 <r^T Omega r>" per prior, then
//           "last pose <id> covariance" followed by its 36 numbers (column-major, tangent [omega, upsilon])
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

std::array<double, 36> diagonalInformation(double rot, double trans)
{
	std::array<double, 36> o{};
	for (int i = 0; i < 3; i++) { o[7 * i] = rot; o[7 * (3 + i)] = trans; }
	return o;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2) { std::printf("usage: %s graph.json [iterations=10] [k=5] [huber=1]\n", argv[0]); return 0; }
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	const int every = argc > 3 ? std::max(1, std::atoi(argv[3])) : 5;
	const bool huber = argc > 4 ? std::atoi(argv[4]) != 0 : true;

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
	if (huber)
	{
		ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(5.991), cuba::EdgeType::MONOCULAR);
		ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(7.815), cuba::EdgeType::STEREO);
	}
	// the anchor, then a loose prior on every k-th pose, each at the pose's initial value
	std::vector<std::unique_ptr<cuba::PosePrior>> priors;
	for (size_t i = 0; i < poses.size(); i += (size_t)every)
	{
		auto p = std::make_unique<cuba::PosePrior>();
		p->vertex = poses[i].get();
		p->q = poses[i]->q;
		p->t = poses[i]->t;
		p->information = i == 0 ? diagonalInformation(1e8, 1e8) : diagonalInformation(1e2, 1.0);
		cuba::addPosePrior(ba.get(), p.get());
		priors.push_back(std::move(p));
	}
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	for (const auto& p : priors) std::printf("prior %d chi2 %.17g\n", p->vertex->id, cuba::priorChiSquared(ba.get(), p.get()));
	if (!cuba::computeCovariances(ba.get(), false))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	double C[36];
	if (!cuba::poseCovariance(ba.get(), poses.back().get(), C)) { std::printf("no covariance of the last pose\n"); return 3; }
	std::printf("last pose %d covariance\n", poses.back()->id);
	for (int k = 0; k < 36; k++) std::printf("%.17g%c", C[k], k % 6 == 5 ? '\n' : ' ');
	return 0;
}
