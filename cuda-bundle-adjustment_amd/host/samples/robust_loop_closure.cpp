// robust_loop_closure.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), frees every pose but the first
// and adds SE(3) relative-pose edges (cuba::addRelativePoseEdge): odometry between consecutive poses, the true loop closure between the
// first and the last pose and one FALSE closure between the poses a quarter and three quarters along the trajectory, as place recognition
// delivers them now and then.  The measurements are the relative poses of the initial estimate; the false closure's is off by 0.2 rad and
// (0.5, 0, 1) m.  Three runs, each from the initial estimate:
//   reference  odometry + the true closure
//   plain      + the false closure, no robust kernel: at full quadratic weight it bends the trajectory
//   cauchy     + the false closure, cuba::PoseFactorKernel::CAUCHY (delta^2 = 12.592, the 95 % quantile of chi2 with 6 degrees of freedom) on
//              both closures: the false one is weighted down as its chi2 grows, the true one keeps a weight near 1
//
//   usage: robust_loop_closure graph.json [iterations=10] [huber=1]
//   output: per run "run <name>", "iter: <i>, chi2: <F>" per iteration, "relative <id i> <id j> chi2 <r^T Omega r>" per relative-pose edge
//           (the plain value, also under a kernel) and, for the two runs with the false closure,
//           "distance <name> <max |t - t_reference| over the poses>"
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

std::array<double, 36> diagonalInformation(double rot, double trans)
{
	std::array<double, 36> o{};
	for (int i = 0; i < 3; i++) { o[7 * i] = rot; o[7 * (3 + i)] = trans; }
	return o;
}

struct Pose { double q[4], t[3]; };          // (x, y, z, w), world -> camera

Pose poseOf(const cuba::PoseVertex* v)
{
	Pose p;
	for (int i = 0; i < 4; i++) p.q[i] = v->q.coeffs().data()[i];
	for (int i = 0; i < 3; i++) p.t[i] = v->t.data()[i];
	return p;
}

void rotate(const double q[4], const double v[3], double o[3])
{
	const double a[3] = { 2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0]) };
	o[0] = v[0] + q[3] * a[0] + (q[1] * a[2] - q[2] * a[1]);
	o[1] = v[1] + q[3] * a[1] + (q[2] * a[0] - q[0] * a[2]);
	o[2] = v[2] + q[3] * a[2] + (q[0] * a[1] - q[1] * a[0]);
}

Pose mul(const Pose& a, const Pose& b)          // a o b
{
	Pose r;
	r.q[0] = a.q[3] * b.q[0] + b.q[3] * a.q[0] + (a.q[1] * b.q[2] - a.q[2] * b.q[1]);
	r.q[1] = a.q[3] * b.q[1] + b.q[3] * a.q[1] + (a.q[2] * b.q[0] - a.q[0] * b.q[2]);
	r.q[2] = a.q[3] * b.q[2] + b.q[3] * a.q[2] + (a.q[0] * b.q[1] - a.q[1] * b.q[0]);
	r.q[3] = a.q[3] * b.q[3] - (a.q[0] * b.q[0] + a.q[1] * b.q[1] + a.q[2] * b.q[2]);
	rotate(a.q, b.t, r.t);
	for (int i = 0; i < 3; i++) r.t[i] += a.t[i];
	return r;
}

Pose inverse(const Pose& a)
{
	Pose r;
	r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
	double v[3];
	rotate(r.q, a.t, v);
	for (int i = 0; i < 3; i++) r.t[i] = -v[i];
	return r;
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
		poses.push_back(std::make_unique<cuba::PoseVertex>(int(n["id"]), q, readVec<3>(n["t"]), cam, poses.empty()));     // every pose free but the first
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
	if (poses.size() < 8) { std::fprintf(stderr, "the graph needs at least eight poses\n"); return 1; }
	if (huber)
	{
		ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(5.991), cuba::EdgeType::MONOCULAR);
		ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(7.815), cuba::EdgeType::STEREO);
	}
	// relative-pose edges: the measurement is `offset` o T_j T_i^-1 of the initial estimate
	std::vector<std::unique_ptr<cuba::RelativePoseEdge>> rel;
	Pose identity{ { 0, 0, 0, 1 }, { 0, 0, 0 } };
	auto makeEdge = [&](size_t i, size_t j, const std::array<double, 36>& info, const Pose& offset) {
		auto e = std::make_unique<cuba::RelativePoseEdge>();
		e->vertexI = poses[i].get(); e->vertexJ = poses[j].get();
		const Pose z = mul(offset, mul(poseOf(poses[j].get()), inverse(poseOf(poses[i].get()))));
		cuba::Array<double, 4> q; cuba::Array<double, 3> t;
		for (int k = 0; k < 4; k++) q[k] = z.q[k];
		for (int k = 0; k < 3; k++) t[k] = z.t[k];
		e->q = Eigen::Quaterniond(q); e->t = t;
		e->information = info;
		rel.push_back(std::move(e));
		return rel.back().get();
	};
	for (size_t i = 0; i + 1 < poses.size(); i++) cuba::addRelativePoseEdge(ba.get(), makeEdge(i, i + 1, diagonalInformation(1e4, 1e2), identity));
	const std::array<double, 36> closureInfo = diagonalInformation(1e5, 1e3);
	cuba::RelativePoseEdge* closure = makeEdge(0, poses.size() - 1, closureInfo, identity);
	cuba::addRelativePoseEdge(ba.get(), closure);
	const Pose wrong{ { 0, std::sin(0.1), 0, std::cos(0.1) }, { 0.5, 0, 1.0 } };
	cuba::RelativePoseEdge* falseClosure = makeEdge(poses.size() / 4, 3 * poses.size() / 4, closureInfo, wrong);          // (not added yet)

	// every run starts from the initial estimate
	std::vector<Pose> start;
	for (const auto& p : poses) start.push_back(poseOf(p.get()));
	std::vector<decltype(cuba::LandmarkVertex::Xw)> startXw;
	for (const auto& l : landmarks) startXw.push_back(l->Xw);
	std::vector<Pose> reference;
	auto run = [&](const char* name, size_t nEdges) {
		for (size_t i = 0; i < poses.size(); i++)
		{
			cuba::Array<double, 4> q; cuba::Array<double, 3> t;
			for (int k = 0; k < 4; k++) q[k] = start[i].q[k];
			for (int k = 0; k < 3; k++) t[k] = start[i].t[k];
			poses[i]->q = Eigen::Quaterniond(q); poses[i]->t = t;
		}
		for (size_t i = 0; i < landmarks.size(); i++) landmarks[i]->Xw = startXw[i];
		ba->initialize();
		ba->optimize(iterations);
		std::printf("run %s\n", name);
		for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
		for (size_t k = 0; k < nEdges; k++)
			std::printf("relative %d %d chi2 %.17g\n", rel[k]->vertexI->id, rel[k]->vertexJ->id, cuba::relativePoseChiSquared(ba.get(), rel[k].get()));
		if (reference.empty()) { for (const auto& p : poses) reference.push_back(poseOf(p.get())); return; }
		double d = 0;
		for (size_t i = 0; i < poses.size(); i++)
			for (int k = 0; k < 3; k++) d = std::max(d, std::fabs(poses[i]->t.data()[k] - reference[i].t[k]));
		std::printf("distance %s %.17g\n", name, d);
	};
	run("reference", rel.size() - 1);
	cuba::addRelativePoseEdge(ba.get(), falseClosure);
	run("plain", rel.size());
	for (cuba::RelativePoseEdge* e : { closure, falseClosure }) { e->kernel = cuba::PoseFactorKernel::CAUCHY; e->delta = std::sqrt(12.592); }
	run("cauchy", rel.size());
	return 0;
}
