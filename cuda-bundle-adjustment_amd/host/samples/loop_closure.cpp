// loop_closure.cpp -- reads a bundle-adjustment graph (the JSON schema of the reference's datasets), frees every pose but the first and
// adds SE(3) relative-pose edges (cuba::addRelativePoseEdge; g2o's binary SE(3) edges): odometry between consecutive poses and, after a
// gate, one loop closure between the first and the last pose.  The measurements are the relative poses of the initial estimate.
//   1. odometry only: optimise, then gate the closure with cuba::computeCrossCovariances -- the Mahalanobis distance of the closure's
//      residual r = log(T_last T_first^-1 Zbar^-1) under Sigma_r + Omega^-1, Sigma_r = J Sigma J^T the covariance of the pair's relative
//      pose (J = [-Ad(T_last T_first^-1), I] to first order);
//   2. with the closure: optimise again from there.
//
//   usage: loop_closure graph.json [iterations=10] [huber=1]
//   output: "gate mahalanobis2 <d2>", "last pose sigma before <6 numbers>", "iter: <i>, chi2: <F>" per iteration of the second run,
//           "relative <id i> <id j> chi2 <r^T Omega r>" per relative-pose edge, "last pose sigma after <6 numbers>", then
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

// [omega, upsilon] = log of a pose: omega from the quaternion, upsilon = J_w^-1 t
void se3Log(const Pose& p, double r[6])
{
	double q[4] = { p.q[0], p.q[1], p.q[2], p.q[3] };
	const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) * (q[3] < 0 ? -1 : 1);
	for (double& v : q) v /= nq;
	const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
	const double s = n < 1e-4 ? 2 / q[3] * (1 - (n / q[3]) * (n / q[3]) / 3) : 2 * std::atan2(n, q[3]) / n;
	const double w[3] = { s * q[0], s * q[1], s * q[2] };
	const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = std::sqrt(th2);
	const double d = th < 0.25 ? 1.0 / 12 + th2 * (1.0 / 720 + th2 * (1.0 / 30240)) : (1 - 0.5 * th * std::cos(0.5 * th) / std::sin(0.5 * th)) / th2;
	// A t = t - w x t / 2 + d w x (w x t)
	const double* t = p.t;
	const double c1[3] = { w[1] * t[2] - w[2] * t[1], w[2] * t[0] - w[0] * t[2], w[0] * t[1] - w[1] * t[0] };
	const double c2[3] = { w[1] * c1[2] - w[2] * c1[1], w[2] * c1[0] - w[0] * c1[2], w[0] * c1[1] - w[1] * c1[0] };
	for (int i = 0; i < 3; i++) { r[i] = w[i]; r[3 + i] = t[i] - 0.5 * c1[i] + d * c2[i]; }
}

// Ad of a pose, column-major 6 x 6: [[R, 0], [[t]x R, R]]
void adjoint(const Pose& m, double Ad[36])
{
	double R[3][3];
	for (int c = 0; c < 3; c++)
	{
		const double e[3] = { c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0 };
		double v[3];
		rotate(m.q, e, v);
		for (int r = 0; r < 3; r++) R[r][c] = v[r];
	}
	for (int k = 0; k < 36; k++) Ad[k] = 0;
	const double* t = m.t;
	const double T[3][3] = { { 0, -t[2], t[1] }, { t[2], 0, -t[0] }, { -t[1], t[0], 0 } };
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 3; c++)
		{
			Ad[6 * c + r] = R[r][c]; Ad[6 * (3 + c) + 3 + r] = R[r][c];
			Ad[6 * c + 3 + r] = T[r][0] * R[0][c] + T[r][1] * R[1][c] + T[r][2] * R[2][c];
		}
}

// x^T S^-1 x for a symmetric positive definite column-major 6 x 6 S (Gaussian elimination)
double mahalanobis2(const double S[36], const double x[6])
{
	double A[6][7];
	for (int r = 0; r < 6; r++) { for (int c = 0; c < 6; c++) A[r][c] = S[6 * c + r]; A[r][6] = x[r]; }
	for (int k = 0; k < 6; k++)
		for (int r = k + 1; r < 6; r++)
		{
			const double f = A[r][k] / A[k][k];
			for (int c = k; c < 7; c++) A[r][c] -= f * A[k][c];
		}
	double y[6];
	for (int r = 5; r >= 0; r--)
	{
		double s = A[r][6];
		for (int c = r + 1; c < 6; c++) s -= A[r][c] * y[c];
		y[r] = s / A[r][r];
	}
	double d = 0;
	for (int r = 0; r < 6; r++) d += x[r] * y[r];
	return d;
}

void printSigma(const char* what, const std::array<double, 36>& S)
{
	std::printf("last pose sigma %s", what);
	for (int k = 0; k < 6; k++) std::printf(" %.9e", std::sqrt(std::max(S[7 * k], 0.0)));
	std::printf("\n");
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
	if (poses.size() < 3) { std::fprintf(stderr, "the graph needs at least three poses\n"); return 1; }
	if (huber)
	{
		ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(5.991), cuba::EdgeType::MONOCULAR);
		ba->setRobustKernels(cuba::RobustKernelType::HUBER, std::sqrt(7.815), cuba::EdgeType::STEREO);
	}
	// relative-pose edges: the measurement is T_j T_i^-1 of the initial estimate
	std::vector<std::unique_ptr<cuba::RelativePoseEdge>> rel;
	auto makeEdge = [&](size_t i, size_t j, const std::array<double, 36>& info) {
		auto e = std::make_unique<cuba::RelativePoseEdge>();
		e->vertexI = poses[i].get(); e->vertexJ = poses[j].get();
		const Pose z = mul(poseOf(poses[j].get()), inverse(poseOf(poses[i].get())));
		cuba::Array<double, 4> q; cuba::Array<double, 3> t;
		for (int k = 0; k < 4; k++) q[k] = z.q[k];
		for (int k = 0; k < 3; k++) t[k] = z.t[k];
		e->q = Eigen::Quaterniond(q); e->t = t;
		e->information = info;
		rel.push_back(std::move(e));
		return rel.back().get();
	};
	for (size_t i = 0; i + 1 < poses.size(); i++) cuba::addRelativePoseEdge(ba.get(), makeEdge(i, i + 1, diagonalInformation(1e4, 1e2)));
	const std::array<double, 36> closureInfo = diagonalInformation(1e5, 1e3);
	cuba::RelativePoseEdge* closure = makeEdge(0, poses.size() - 1, closureInfo);          // (not added yet)

	// 1. odometry only, then the gate
	ba->initialize();
	ba->optimize(iterations);
	const cuba::PoseVertex *first = poses.front().get(), *last = poses.back().get();
	std::vector<cuba::CovariancePair> pairs = { { first, first }, { first, last }, { last, last } };
	std::vector<std::array<double, 36>> S;
	if (!cuba::computeCrossCovariances(ba.get(), pairs, S))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	{
		Pose zbar;
		for (int k = 0; k < 4; k++) zbar.q[k] = closure->q.coeffs().data()[k];
		for (int k = 0; k < 3; k++) zbar.t[k] = closure->t.data()[k];
		const Pose m = mul(poseOf(last), inverse(poseOf(first)));
		double r[6], Ad[36], Sr[36];
		se3Log(mul(m, inverse(zbar)), r);
		adjoint(m, Ad);
		// Sigma_r = Ad S_ii Ad^T - Ad S_ij - S_ji Ad^T + S_jj, plus the measurement's own covariance Omega^-1 (diagonal here)
		auto at = [](const std::array<double, 36>& B, int r, int c) { return B[6 * c + r]; };
		for (int a = 0; a < 6; a++)
			for (int b = 0; b < 6; b++)
			{
				double v = at(S[2], a, b);
				for (int k = 0; k < 6; k++)
				{
					v -= Ad[6 * k + a] * at(S[1], k, b) + at(S[1], k, a) * Ad[6 * k + b];
					for (int l = 0; l < 6; l++) v += Ad[6 * k + a] * at(S[0], k, l) * Ad[6 * l + b];
				}
				Sr[6 * b + a] = v + (a == b ? 1.0 / closureInfo[7 * a] : 0.0);
			}
		std::printf("gate mahalanobis2 %.9e\n", mahalanobis2(Sr, r));
	}
	printSigma("before", S[2]);

	// 2. with the closure, from the estimate of the first run
	cuba::addRelativePoseEdge(ba.get(), closure);
	ba->initialize();
	ba->optimize(iterations);
	for (const auto& s : ba->batchStatistics()) std::printf("iter: %d, chi2: %.17g\n", s.iteration + 1, s.chi2);
	for (const auto& e : rel) std::printf("relative %d %d chi2 %.17g\n", e->vertexI->id, e->vertexJ->id, cuba::relativePoseChiSquared(ba.get(), e.get()));
	if (!cuba::computeCovariances(ba.get(), false))
	{
		std::printf("the Hessian at the estimate is not positive definite: no covariances\n");
		return 2;
	}
	double C[36];
	if (!cuba::poseCovariance(ba.get(), last, C)) { std::printf("no covariance of the last pose\n"); return 3; }
	std::array<double, 36> Ca;
	for (int k = 0; k < 36; k++) Ca[k] = C[k];
	printSigma("after", Ca);
	std::printf("last pose %d covariance\n", last->id);
	for (int k = 0; k < 36; k++) std::printf("%.17g%c", C[k], k % 6 == 5 ? '\n' : ' ');
	return 0;
}
