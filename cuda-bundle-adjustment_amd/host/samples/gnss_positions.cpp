// gnss_positions.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), frees every pose and every landmark
// and geo-references the block with position factors instead (cuba::addPositionFactor): every `stride`-th pose (file order) carries a
// "GNSS fix" of its antenna -- the world position of the point `a` of the camera frame (the lever arm, 0.1 -0.2 0.5 m), taken from the
// pose's initial estimate, with a centimetre-level information.  A position fix knows no orientation: the lever arm is what ties it to the
// rotation, and the fixes together are the gauge of a graph without a fixed vertex.  One fix -- the second -- is grossly wrong (metres
// off, a multipath jump); under the Cauchy kernel it is weighted down instead of bending the trajectory.  Prints the LM objective per
// iteration (edges plus factors), every fix's chi2 at the result (the gross one stands out), the camera centre -R^T t of its pose and
// the pose's marginal covariance, which the fixes alone make well defined.
//
//   usage: gnss_positions graph.json [iterations=10] [stride=5] [kernel=3] [delta=3]
//          kernel: 0 none, 1 Huber, 2 Tukey, 3 Cauchy
//   output: "iter: <i>, chi2: <F>" per iteration, then per fix "fix <pose id> chi2 <r^T Omega r>", "fix <pose id> position <x> <y> <z>"
//           and "fix <pose id> covariance" followed by its 36 numbers (column-major, [omega, upsilon] tangent)
#include <array>
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

// R^T (a - t) of the world -> camera pose [R | t] of v: the world position of the point a of the camera frame
std::array<double, 3> worldPosition(const cuba::PoseVertex& v, const std::array<double, 3>& a)
{
	const double* c = v.q.coeffs().data();      // (x, y, z, w)
	const double x = c[0], y = c[1], z = c[2], w = c[3];
	const double R[3][3] = {
		{ 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w) },
		{ 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w) },
		{ 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) } };
	const double d[3] = { a[0] - v.t[0], a[1] - v.t[1], a[2] - v.t[2] };
	return { R[0][0] * d[0] + R[1][0] * d[1] + R[2][0] * d[2], R[0][1] * d[0] + R[1][1] * d[1] + R[2][1] * d[2], R[0][2] * d[0] + R[1][2] * d[1] + R[2][2] * d[2] };
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2) { std::printf("usage: %s graph.json [iterations=10] [stride=5] [kernel=3] [delta=3]\n", argv[0]); return 0; }
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	const int stride = argc > 3 ? std::max(1, std::atoi(argv[3])) : 5;
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

	// the fixes: every stride-th pose with an edge (file order), the antenna 0.1 -0.2 0.5 m off the camera centre, good to a centimetre
	// (information 1e4 I)
	const std::array<double, 3> arm = { 0.1, -0.2, 0.5 };
	std::vector<cuba::PoseVertex*> observed;
	for (const auto& p : poses) if (!p->edges.empty()) observed.push_back(p.get());
	std::vector<std::unique_ptr<cuba::PositionFactor>> fixes;
	for (size_t j = 0; j < observed.size(); j += (size_t)stride)
	{
		auto f = std::make_unique<cuba::PositionFactor>();
		f->vertex = observed[j];
		f->leverArm = arm;
		f->position = worldPosition(*f->vertex, arm);
		if (fixes.size() == 1) { f->position[0] += 5.0; f->position[1] -= 3.0; f->position[2] += 4.0; }      // the gross one
		f->information = { 1e4, 0, 0, 0, 1e4, 0, 0, 0, 1e4 };
		f->kernel = static_cast<cuba::PoseFactorKernel>(kernel);
		f->delta = delta;
		cuba::addPositionFactor(ba.get(), f.get());
		fixes.push_back(std::move(f));
	}
	if (fixes.size() < 3) { std::fprintf(stderr, "fewer than 3 fixes: the gauge of a free graph needs three\n"); return 1; }
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	for (const auto& f : fixes) std::printf("fix %d chi2 %.17g\n", f->vertex->id, cuba::positionFactorChiSquared(ba.get(), f.get()));
	for (const auto& f : fixes)
	{
		const std::array<double, 3> c = worldPosition(*f->vertex, { 0.0, 0.0, 0.0 });
		std::printf("fix %d position %.17g %.17g %.17g\n", f->vertex->id, c[0], c[1], c[2]);
	}
	if (!cuba::computeCovariances(ba.get(), false))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	for (const auto& f : fixes)
	{
		double C[36];
		if (!cuba::poseCovariance(ba.get(), f->vertex, C)) { std::printf("no covariance of the pose of fix %d\n", f->vertex->id); return 3; }
		std::printf("fix %d covariance\n", f->vertex->id);
		for (int k = 0; k < 36; k++) std::printf("%.17g%c", C[k], k % 6 == 5 ? '\n' : ' ');
	}
	return 0;
}
