// drift_uncertainty.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), optimises it and prints, for every
// k-th free pose, the 1-sigma uncertainty of its camera centre RELATIVE to the first free pose's centre (the drift of a trajectory), from
// the cross covariances of non-co-visible pose pairs (cuba::computeCrossCovariances).
//
// To first order (see pose_uncertainty.cpp) a camera centre moves by -A upsilon, A = R^T, so
//   Cov(c_k - c_0) = A_k S_kk A_k^T + A_0 S_00 A_0^T - A_k S_k0 A_0^T - A_0 S_0k A_k^T,   S = the upsilon rows / columns of the pose blocks.
// The first free pose is the free pose with the smallest id.
//
//   usage: drift_uncertainty graph.json [iterations=10] [huber=1] [every=1]
//   output: one line per reported pose, "pose <id> drift <sx> <sy> <sz>" (world axes)
#include <algorithm>
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
	if (argc < 2) { std::printf("usage: %s graph.json [iterations=10] [huber=1] [every=1]\n", argv[0]); return 0; }
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	const bool huber = argc > 3 ? std::atoi(argv[3]) != 0 : true;
	const int every = argc > 4 ? std::max(1, std::atoi(argv[4])) : 1;

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
	// the free poses by id, the first of them as the reference
	std::vector<const cuba::PoseVertex*> free;
	for (const auto& p : poses) if (!p->fixed) free.push_back(p.get());
	std::sort(free.begin(), free.end(), [](const cuba::PoseVertex* a, const cuba::PoseVertex* b) { return a->id < b->id; });
	if (free.empty()) { std::printf("no free pose\n"); return 0; }
	std::vector<const cuba::PoseVertex*> report;
	for (size_t i = 0; i < free.size(); i += every) report.push_back(free[i]);
	// per reported pose k: (k, k) and (k, 0); the reference pose is the one right-hand side of every (k, 0) pair
	std::vector<cuba::CovariancePair> pairs;
	for (const auto* p : report) { pairs.push_back({ p, p }); pairs.push_back({ p, free[0] }); }
	std::vector<std::array<double, 36>> S;
	if (!cuba::computeCrossCovariances(ba.get(), pairs, S))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	double R0[9];
	quatToRot(free[0]->q.coeffs().data(), R0);
	const std::array<double, 36>& S00 = S[0];                   // (the first reported pose is free[0]: pair 0 is (0, 0))
	for (size_t r = 0; r < report.size(); r++)
	{
		const std::array<double, 36>& Skk = S[2 * r];
		const std::array<double, 36>& Sk0 = S[2 * r + 1];
		double Rk[9];
		quatToRot(report[r]->q.coeffs().data(), Rk);
		// A = R^T: A(a, i) = R[3 i + a]; the upsilon block of a column-major 6 x 6 block B is B[6 (3 + j) + 3 + i]
		auto ups = [](const std::array<double, 36>& B, int i, int j) { return B[6 * (3 + j) + 3 + i]; };
		double s[3];
		for (int a = 0; a < 3; a++)
		{
			double v = 0;
			for (int i = 0; i < 3; i++)
				for (int j = 0; j < 3; j++)
				{
					v += Rk[3 * i + a] * ups(Skk, i, j) * Rk[3 * j + a] + R0[3 * i + a] * ups(S00, i, j) * R0[3 * j + a];
					v -= 2 * Rk[3 * i + a] * ups(Sk0, i, j) * R0[3 * j + a];          // (the two cross terms are transposes: equal diagonals)
				}
			s[a] = std::sqrt(std::max(v, 0.0));
		}
		std::printf("pose %d drift %.9e %.9e %.9e\n", report[r]->id, s[0], s[1], s[2]);
	}
	return 0;
}
