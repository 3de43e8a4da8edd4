// odometer_scale.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets) as a MONOCULAR one -- a stereo edge is
// taken without its disparity --, fixes the first pose with an edge (file order), frees every other pose and every landmark, and blows the
// whole estimate up by `scale0` about the fixed pose's camera centre: for the reprojection edges alone that is as good an estimate as the
// file's, since a monocular graph with one fixed pose has its gauge but not its size.  Range factors between poses
// (cuba::addPoseRangeFactor) give it that: the travelled distance of a wheel odometer between consecutive keyframes -- the distance of the
// wheel point (lever arm 0 / 0.3 / -0.2 in the camera frame) of pose k from that of pose k + 1 (file order) at the FILE's estimate,
// sigma = 0.02 m, no kernel, no orientation.  One more factor is a peer range between the second pose and the middle one, grossly wrong
// (a reflection: 5 m long); under the Cauchy kernel it is weighted down instead of bending the trajectory.
// Prints the LM objective per iteration (edges plus factors), the recovered scale -- the spread of the camera centres about their mean
// against the file's --, every factor's chi2 at the result and which of them a gate of `gate` rejects; then removes those factors
// (cuba::removePoseRangeFactor), runs again and prints the same; last the final keyframe leaves: the pose is removed (removePoseVertex), the
// factors touching it go with it without being removed one by one, and a third run prints the same again.
//
//   usage: odometer_scale graph.json [iterations=10] [kernel=3] [delta=3] [scale0=1.05] [gate=25]
//          kernel (of the peer range): 0 none, 1 Huber, 2 Tukey, 3 Cauchy
//   output: "iter: <i>, chi2: <F>" per iteration, "scale <s>", per factor "range <pose id i> <pose id j> chi2 <Omega r^2>", per factor beyond the
//           gate "gated <pose id i> <pose id j>", then "refit iter: <i>, chi2: <F>", "refit scale <s>" and "refit range <i> <j> chi2 <Omega r^2>",
//           then "dropped <pose id>" and "dropped iter: ..." / "dropped range ..." in the same form (0 for the factors that went with the pose)
#include <algorithm>
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
using Vec3 = std::array<double, 3>;

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

// R^T (a - t): the world position of the point a of the camera frame of v (a = 0: the camera centre)
Vec3 inWorld(const cuba::PoseVertex& v, const Vec3& a)
{
	double R[3][3];
	rotation(v, R);
	const double d[3] = { a[0] - v.t[0], a[1] - v.t[1], a[2] - v.t[2] };
	return { R[0][0] * d[0] + R[1][0] * d[1] + R[2][0] * d[2], R[0][1] * d[0] + R[1][1] * d[1] + R[2][1] * d[2], R[0][2] * d[0] + R[1][2] * d[1] + R[2][2] * d[2] };
}

// t = -R c of the pose whose camera centre is c
void setCentre(cuba::PoseVertex& v, const Vec3& c)
{
	double R[3][3];
	rotation(v, R);
	for (int i = 0; i < 3; i++) v.t[i] = -(R[i][0] * c[0] + R[i][1] * c[1] + R[i][2] * c[2]);
}

double distance(const Vec3& a, const Vec3& b)
{
	return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
}

// root of the summed squared distances of the points from their mean
double spread(const std::vector<Vec3>& pts)
{
	Vec3 m = { 0, 0, 0 };
	for (const Vec3& p : pts)
		for (int i = 0; i < 3; i++) m[i] += p[i] / (double)pts.size();
	double s = 0;
	for (const Vec3& p : pts)
		for (int i = 0; i < 3; i++) s += (p[i] - m[i]) * (p[i] - m[i]);
	return std::sqrt(s);
}

std::vector<Vec3> centres(const std::vector<cuba::PoseVertex*>& poses)
{
	std::vector<Vec3> c;
	for (const cuba::PoseVertex* v : poses) c.push_back(inWorld(*v, { 0, 0, 0 }));
	return c;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc < 2) { std::printf("usage: %s graph.json [iterations=10] [kernel=3] [delta=3] [scale0=1.05] [gate=25]\n", argv[0]); return 0; }
	const int iterations = argc > 2 ? std::atoi(argv[2]) : 10;
	const int kernel = argc > 3 ? std::atoi(argv[3]) : 3;
	const double delta = argc > 4 ? std::atof(argv[4]) : 3.0;
	const double scale0 = argc > 5 ? std::atof(argv[5]) : 1.05;
	const double gate = argc > 6 ? std::atof(argv[6]) : 25.0;

	cv::FileStorage fs(argv[1], cv::FileStorage::READ);
	if (!fs.isOpened()) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
	cuba::CameraParams cam;
	cam.fx = fs["fx"]; cam.fy = fs["fy"]; cam.cx = fs["cx"]; cam.cy = fs["cy"]; cam.bf = fs["bf"];

	std::vector<std::unique_ptr<cuba::PoseVertex>> poses;
	std::vector<std::unique_ptr<cuba::LandmarkVertex>> landmarks;
	std::vector<std::unique_ptr<cuba::MonoEdge>> mono;
	auto ba = cuba::CudaBundleAdjustment::create();
	for (const auto& n : fs["pose_vertices"])
	{
		const Eigen::Quaterniond q(readVec<4>(n["q"]));
		poses.push_back(std::make_unique<cuba::PoseVertex>(int(n["id"]), q, readVec<3>(n["t"]), cam, false));
		ba->addPoseVertex(poses.back().get());
	}
	for (const auto& n : fs["landmark_vertices"])
	{
		landmarks.push_back(std::make_unique<cuba::LandmarkVertex>(int(n["id"]), readVec<3>(n["Xw"]), false));     // every landmark free
		ba->addLandmarkVertex(landmarks.back().get());
	}
	// monocular edges only: a stereo edge gives its (u, v) and keeps its disparity to itself
	for (const char* list : { "monocular_edges", "stereo_edges" })
		for (const auto& n : fs[list])
		{
			mono.push_back(std::make_unique<cuba::MonoEdge>(readVec<2>(n["measurement"]), double(n["information"]),
				ba->poseVertex(int(n["vertexP"])), ba->landmarkVertex(int(n["vertexL"]))));
			ba->addMonocularEdge(mono.back().get());
		}
	ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(5.991), cuba::EdgeType::MONOCULAR);

	std::vector<cuba::PoseVertex*> observed;
	for (const auto& p : poses) if (!p->edges.empty()) observed.push_back(p.get());
	if (observed.size() < 4) { std::fprintf(stderr, "fewer than 4 poses with edges\n"); return 1; }
	observed[0]->fixed = true;          // the gauge: one fixed pose, every other free

	// the odometer: the distance of the wheel points of consecutive keyframes at the file's estimate; then the gross peer range
	const std::vector<Vec3> fileCentres = centres(observed);
	const double fileSpread = spread(fileCentres);
	const Vec3 arm = { 0.0, 0.3, -0.2 };
	const double sigma = 0.02;
	std::vector<std::unique_ptr<cuba::PoseRangeFactor>> ranges;
	const auto measure = [&](cuba::PoseVertex* vi, cuba::PoseVertex* vj) {
		auto f = std::make_unique<cuba::PoseRangeFactor>();
		f->vertexI = vi; f->vertexJ = vj;
		f->leverArmI = arm; f->leverArmJ = arm;
		f->range = distance(inWorld(*vi, arm), inWorld(*vj, arm));
		f->information = 1.0 / (sigma * sigma);
		return f;
	};
	for (size_t k = 0; k + 1 < observed.size(); k++) ranges.push_back(measure(observed[k], observed[k + 1]));
	ranges.push_back(measure(observed[observed.size() / 2], observed[1]));
	ranges.back()->range += 5.0;
	ranges.back()->kernel = static_cast<cuba::PoseFactorKernel>(kernel);
	ranges.back()->delta = delta;
	for (const auto& f : ranges) cuba::addPoseRangeFactor(ba.get(), f.get());

	// the start: the file's estimate blown up by scale0 about the fixed pose's camera centre (camera centres and landmarks; the rotations stay)
	const Vec3 c0 = fileCentres[0];
	for (const auto& p : poses)
	{
		if (p.get() == observed[0]) continue;
		const Vec3 c = inWorld(*p, { 0, 0, 0 });
		setCentre(*p, { c0[0] + scale0 * (c[0] - c0[0]), c0[1] + scale0 * (c[1] - c0[1]), c0[2] + scale0 * (c[2] - c0[2]) });
	}
	for (const auto& l : landmarks)
		for (int i = 0; i < 3; i++) l->Xw[i] = c0[i] + scale0 * (l->Xw[i] - c0[i]);
	std::printf("start scale %.17g\n", spread(centres(observed)) / fileSpread);

	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	std::printf("scale %.17g\n", spread(centres(observed)) / fileSpread);
	std::vector<size_t> gated;
	for (size_t k = 0; k < ranges.size(); k++)
	{
		const double e = cuba::poseRangeFactorChiSquared(ba.get(), ranges[k].get());
		std::printf("range %d %d chi2 %.17g\n", ranges[k]->vertexI->id, ranges[k]->vertexJ->id, e);
		if (e > gate) gated.push_back(k);
	}
	for (size_t k : gated) std::printf("gated %d %d\n", ranges[k]->vertexI->id, ranges[k]->vertexJ->id);

	// without the gated factors, from where the first run ended
	for (size_t k : gated) cuba::removePoseRangeFactor(ba.get(), ranges[k].get());
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("refit iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	std::printf("refit scale %.17g\n", spread(centres(observed)) / fileSpread);
	for (size_t k = 0; k < ranges.size(); k++)
		std::printf("refit range %d %d chi2 %.17g\n", ranges[k]->vertexI->id, ranges[k]->vertexJ->id, cuba::poseRangeFactorChiSquared(ba.get(), ranges[k].get()));

	// the last keyframe leaves the graph: its edges and the factors touching it go with it (the objects stay the caller's)
	cuba::PoseVertex* gone = observed.back();
	ba->removePoseVertex(gone);
	std::printf("dropped %d\n", gone->id);
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("dropped iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	for (size_t k = 0; k < ranges.size(); k++)
		std::printf("dropped range %d %d chi2 %.17g\n", ranges[k]->vertexI->id, ranges[k]->vertexJ->id, cuba::poseRangeFactorChiSquared(ba.get(), ranges[k].get()));
	return 0;
}
