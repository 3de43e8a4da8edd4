// gravity_aligned.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), frees every pose and every landmark
// and geo-references the block by two GNSS fixes and gravity: position factors (cuba::addPositionFactor) on the first and the last pose
// with an edge (file order) only, and a direction factor (cuba::addDirectionFactor) on every `stride`-th such pose -- the world vector
// d = (0, 0, -1) as an accelerometer sees it in the camera frame, m = R d of the pose's initial estimate, with the rank-2 information
// (I - m m^T) / sigma^2, sigma = 0.01.  Two fixes alone leave the rotation of the whole graph about the line through them free; one gravity
// reading off that line closes it, so the graph needs no fixed vertex and its geo-reference does not depend on the trajectory's shape.
// One reading -- the second -- is grossly wrong (the sensor was accelerating); under the Cauchy kernel it is weighted down instead of
// tilting its pose.  Prints the LM objective per iteration (edges plus factors), every reading's chi2 at the result (the gross one stands
// out), the tilt error of its pose -- the angle between R d at the result and the clean reading -- and the pose's marginal covariance.
//
//   usage: gravity_aligned graph.json [iterations=10] [stride=5] [kernel=3] [delta=3]
//          kernel: 0 none, 1 Huber, 2 Tukey, 3 Cauchy
//   output: "iter: <i>, chi2: <F>" per iteration, then per reading "gravity <pose id> chi2 <r^T Omega r>", "gravity <pose id> tilt <radians>"
//           and "gravity <pose id> covariance" followed by its 36 numbers (column-major, [omega, upsilon] tangent)
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

// the rotation of the world -> camera pose of v, row-major
void rotation(const cuba::PoseVertex& v, double R[3][3])
{
	const double* c = v.q.coeffs().data();      // (x, y, z, w)
	const double x = c[0], y = c[1], z = c[2], w = c[3];
	const double M[3][3] = {
		{ 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w) },
		{ 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w) },
		{ 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) } };
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) R[i][j] = M[i][j];
}

// R d: the world vector d in the camera frame of v
std::array<double, 3> inCamera(const cuba::PoseVertex& v, const std::array<double, 3>& d)
{
	double R[3][3];
	rotation(v, R);
	return { R[0][0] * d[0] + R[0][1] * d[1] + R[0][2] * d[2], R[1][0] * d[0] + R[1][1] * d[1] + R[1][2] * d[2], R[2][0] * d[0] + R[2][1] * d[1] + R[2][2] * d[2] };
}

// -R^T t: the camera centre of v
std::array<double, 3> centre(const cuba::PoseVertex& v)
{
	double R[3][3];
	rotation(v, R);
	return { -(R[0][0] * v.t[0] + R[1][0] * v.t[1] + R[2][0] * v.t[2]), -(R[0][1] * v.t[0] + R[1][1] * v.t[1] + R[2][1] * v.t[2]),
		-(R[0][2] * v.t[0] + R[1][2] * v.t[1] + R[2][2] * v.t[2]) };
}

std::array<double, 3> normalised(const std::array<double, 3>& a)
{
	const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
	return { a[0] / n, a[1] / n, a[2] / n };
}

// the angle between a and b
double angle(const std::array<double, 3>& a, const std::array<double, 3>& b)
{
	const double c[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
	return std::atan2(std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
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

	std::vector<cuba::PoseVertex*> observed;
	for (const auto& p : poses) if (!p->edges.empty()) observed.push_back(p.get());
	if (observed.size() < 3) { std::fprintf(stderr, "fewer than 3 poses with edges\n"); return 1; }

	// two fixes only: the camera centres of the first and the last pose with an edge, good to a centimetre (information 1e4 I)
	std::vector<std::unique_ptr<cuba::PositionFactor>> fixes;
	for (cuba::PoseVertex* v : { observed.front(), observed.back() })
	{
		auto f = std::make_unique<cuba::PositionFactor>();
		f->vertex = v;
		f->position = centre(*v);
		f->information = { 1e4, 0, 0, 0, 1e4, 0, 0, 0, 1e4 };
		cuba::addPositionFactor(ba.get(), f.get());
		fixes.push_back(std::move(f));
	}

	// the gravity readings: every stride-th pose with an edge, d = (0, 0, -1), sigma = 0.01 across the reading and nothing along it
	const std::array<double, 3> down = { 0.0, 0.0, -1.0 };
	const double sigma = 0.01;
	std::vector<std::unique_ptr<cuba::DirectionFactor>> readings;
	std::vector<std::array<double, 3>> clean;
	for (size_t j = 0; j < observed.size(); j += (size_t)stride)
	{
		auto f = std::make_unique<cuba::DirectionFactor>();
		f->vertex = observed[j];
		f->worldDirection = down;
		std::array<double, 3> m = inCamera(*f->vertex, down);
		clean.push_back(m);
		if (readings.size() == 1) m = normalised({ m[0] + 0.5, m[1] - 0.3, m[2] + 0.4 });      // the gross one
		f->measurement = m;
		for (int c = 0; c < 3; c++)
			for (int r = 0; r < 3; r++) f->information[3 * c + r] = ((r == c ? 1.0 : 0.0) - m[r] * m[c]) / (sigma * sigma);
		f->kernel = static_cast<cuba::PoseFactorKernel>(kernel);
		f->delta = delta;
		cuba::addDirectionFactor(ba.get(), f.get());
		readings.push_back(std::move(f));
	}
	if (readings.size() < 2) { std::fprintf(stderr, "fewer than 2 gravity readings\n"); return 1; }
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	for (const auto& f : readings) std::printf("gravity %d chi2 %.17g\n", f->vertex->id, cuba::directionFactorChiSquared(ba.get(), f.get()));
	for (size_t k = 0; k < readings.size(); k++)
		std::printf("gravity %d tilt %.17g\n", readings[k]->vertex->id, angle(inCamera(*readings[k]->vertex, down), clean[k]));
	if (!cuba::computeCovariances(ba.get(), false))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	for (const auto& f : readings)
	{
		double C[36];
		if (!cuba::poseCovariance(ba.get(), f->vertex, C)) { std::printf("no covariance of the pose of reading %d\n", f->vertex->id); return 3; }
		std::printf("gravity %d covariance\n", f->vertex->id);
		for (int k = 0; k < 36; k++) std::printf("%.17g%c", C[k], k % 6 == 5 ? '\n' : ' ');
	}
	return 0;
}
