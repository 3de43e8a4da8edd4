// pose_uncertainty.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), optimises it and prints the
// 1-sigma uncertainty of every camera centre from the marginal pose covariances (cuba::computeCovariances / cuba::poseCovariance; the
// capability of g2o's computeMarginals).
//
// The pose covariance is expressed in the tangent [omega, upsilon] of the solver's update T <- exp(xi) T (T world -> camera).  To first
// order the camera centre c = -R^T t then moves by -R^T upsilon, so its covariance in world coordinates is R^T Sigma_upsilon R.
//
//   usage: pose_uncertainty graph.json [iterations=10] [huber=1]
//   output: one line per pose, "pose <id> sigma <sx> <sy> <sz>" (world axes), or "pose <id> fixed"
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

// rotation matrix of the unit quaternion (x, y, z, w), row-major
void quatToRot(const double* q, double R[9])
{
	const double x = q[0], y = q[1], z = q[2], w = q[3];
	R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
	R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
	R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2) { std::printf("usage: %s graph.json [iterations=10] [huber=1]\n", argv[0]); return 0; }
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	const bool huber = argc > 3 ? std::atoi(argv[3]) != 0 : true;

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
		poses.push_back(std::make_unique<cuba::PoseVertex>(int(n["id"]), q, readVec<3>(n["t"]), cam, int(n["fixed"]) != 0));
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
	ba->initialize();
	ba->optimize(iterations);
	std::printf("poses %zu  landmarks %zu  edges %zu  final chi2 %.6f\n", ba->nposes(), ba->nlandmarks(), ba->nedges(),
		ba->batchStatistics().empty() ? 0.0 : ba->batchStatistics().back().chi2);
	if (!cuba::computeCovariances(ba.get(), false))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	for (const auto& p : poses)
	{
		double C[36], R[9];
		if (!cuba::poseCovariance(ba.get(), p.get(), C)) { std::printf("pose %d fixed\n", p->id); continue; }
		quatToRot(p->q.coeffs().data(), R);
		double s[3];
		for (int a = 0; a < 3; a++)
		{
			// (R^T Sigma_upsilon R)_aa = sum_ij R_ia Sigma_ij R_ja; Sigma_upsilon = rows / columns 3..5, column-major
			double v = 0;
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++) v += R[3 * i + a] * C[6 * (3 + j) + 3 + i] * R[3 * j + a];
			s[a] = std::sqrt(std::max(v, 0.0));
		}
		std::printf("pose %d sigma %.9e %.9e %.9e\n", p->id, s[0], s[1], s[2]);
	}
	return 0;
}
