// ba_types.hpp -- user-facing graph types of the cuba:: bundle-adjustment API (MI355X build).
//
// Source-compatible with the type header of fixstars/cuda-bundle-adjustment
// (/root/reference/include/cuda_bundle_adjustment_types.h:30-247): same names, members, constructors
// and ownership rules, so code written against the reference (e.g. its samples) compiles unchanged.
// The caller allocates and owns every vertex and edge; the optimiser keeps raw pointers, fills
// PoseVertex::iP / LandmarkVertex::iL and the per-vertex edge sets, and writes the optimised
// q / t / Xw back into the vertices.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <unordered_set>
#include <vector>

#include <Eigen/Core>
#include <Eigen/Geometry>

namespace cuba
{

// ---- aliases (types.h:36-43) ---------------------------------------------------------------------
template <class T, int N> using Array = Eigen::Matrix<T, N, 1>;
template <class T> using Set = std::unordered_set<T>;
template <class T> using UniquePtr = std::unique_ptr<T>;

// ---- pinhole / rectified-stereo intrinsics (types.h:51-62) ---------------------------------------
struct CameraParams
{
	double fx = 0;   // focal length x [px]
	double fy = 0;   // focal length y [px]
	double cx = 0;   // principal point x [px]
	double cy = 0;   // principal point y [px]
	double bf = 0;   // stereo baseline times fx
	CameraParams() = default;
};

struct PoseVertex;
struct LandmarkVertex;

// ---- edges (types.h:73-148) ----------------------------------------------------------------------
struct BaseEdge
{
	virtual PoseVertex* poseVertex() const = 0;
	virtual LandmarkVertex* landmarkVertex() const = 0;
	virtual int dim() const = 0;            // 2 = monocular, 3 = stereo
	virtual ~BaseEdge() = default;
};

template <int DIM>
struct Edge : BaseEdge
{
	using Measurement = Array<double, DIM>;
	using Information = double;             // isotropic information (a scalar, as in the reference)

	Edge() : measurement(Measurement()), information(Information()), vertexP(nullptr), vertexL(nullptr) {}
	Edge(const Measurement& m, Information I, PoseVertex* vertexP, LandmarkVertex* vertexL)
		: measurement(m), information(I), vertexP(vertexP), vertexL(vertexL) {}

	PoseVertex* poseVertex() const override { return vertexP; }
	LandmarkVertex* landmarkVertex() const override { return vertexL; }
	int dim() const override { return DIM; }

	Measurement measurement;
	Information information;
	PoseVertex* vertexP;
	LandmarkVertex* vertexL;
};

using MonoEdge = Edge<2>;
using StereoEdge = Edge<3>;

enum class EdgeType { MONOCULAR = 0, STEREO = 1, COUNT = 2 };

// ---- vertices (types.h:156-208) -------------------------------------------------------------------
struct PoseVertex
{
	using Quaternion = Eigen::Quaterniond;
	using Rotation = Quaternion;
	using Translation = Array<double, 3>;

	PoseVertex() : q(Rotation()), t(Translation()), fixed(false), id(-1), iP(-1) {}
	PoseVertex(int id, const Rotation& q, const Translation& t, const CameraParams& camera, bool fixed = false)
		: q(q), t(t), camera(camera), fixed(fixed), id(id), iP(-1) {}

	Rotation q;              // world -> camera rotation
	Translation t;           // world -> camera translation
	CameraParams camera;
	bool fixed;              // held constant during optimisation
	int id;
	int iP;                  // solver index, assigned by initialize()
	Set<BaseEdge*> edges;    // incident edges, maintained by add*/remove*
};

struct LandmarkVertex
{
	using Point3D = Array<double, 3>;

	LandmarkVertex() : Xw(Point3D()), fixed(false), id(-1), iL(-1) {}
	LandmarkVertex(int id, const Point3D& Xw, bool fixed = false) : Xw(Xw), fixed(fixed), id(id), iL(-1) {}

	Point3D Xw;
	bool fixed;
	int id;
	int iL;                  // solver index, assigned by initialize()
	Set<BaseEdge*> edges;
};

// ---- robust kernels / statistics (types.h:213-236) -------------------------------------------------
enum class RobustKernelType { NONE = 0, HUBER = 1, TUKEY = 2 };

struct BatchInfo
{
	int iteration;
	double chi2;             // robust objective after the iteration
};

using BatchStatistics = std::vector<BatchInfo>;
using TimeProfile = std::map<std::string, double>;

// ---- edge gating (extension: cuba::gateEdges, bundle_adjustment.hpp; the reference has no counterpart) ----------
// RECLASSIFY judges every edge afresh (gated edges can come back), ONLY_REMOVE never re-admits one, DRY_RUN only counts.
enum class EdgeGateMode { RECLASSIFY = 0, ONLY_REMOVE = 1, DRY_RUN = 2 };

struct EdgeGate
{
	double chi2Mono = 5.991, chi2Stereo = 7.815;   // an edge stays active iff its omega |r|^2 is at most this (infinity: no chi2 test)
	bool positiveDepth = true;                     // ... and its point lies in front of the camera
	EdgeGateMode mode = EdgeGateMode::RECLASSIFY;
};

struct EdgeGateResult
{
	long long activeMono = 0, activeStereo = 0;
	long long gatedChi2Mono = 0, gatedChi2Stereo = 0;   // in front of the camera, chi2 above the threshold
	long long gatedDepth = 0;                           // not in front of the camera, whatever the chi2
	long long changed = 0;                              // edges whose state changed (DRY_RUN: would change)
};

// ---- landmark triangulation (extension: cuba::triangulateLandmarks, bundle_adjustment.hpp; the reference has no counterpart) ----------
struct TriangulationOptions
{
	int refineIterations = 5;                      // Gauss-Newton steps per landmark behind the linear start (0 ... 16)
	double minParallaxDeg = 1.0;                   // two views closer than this are LOW_PARALLAX (<= 0: no such test)
	double chi2Mono = 5.991, chi2Stereo = 7.815;   // a landmark is accepted only if every active edge stays at or below this (infinity: no chi2 test)
	bool dryRun = false;                           // only the statuses and counts: no position changes
};

// the statuses in the order they are decided (CUBA_HIP_TRI_* of cuba_hip.h)
enum class TriangulationStatus { OK = 0, NOT_SELECTED, FIXED, FEW_OBSERVATIONS, LOW_PARALLAX, SINGULAR, BEHIND_CAMERA, CHI2 };

struct TriangulationResult
{
	long long counts[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };      // landmarks per TriangulationStatus
	long long count(TriangulationStatus s) const { return counts[static_cast<int>(s)]; }
};

// ---- pose refinement with the landmarks held (extension: cuba::refinePoses, bundle_adjustment.hpp; the reference has no counterpart) ----
struct PoseRefinementOptions
{
	int rounds = 4;                                // outlier rounds (1 ... 4): the edges are classified again at the start of each and once more at the end
	int iterations = 10;                           // Levenberg-Marquardt trials per round (1 ... 32), a fixed count
	int robustRounds = 2;                          // the rounds below this one use the robust kernels, the later ones none (0 ... rounds)
	double chi2Mono = 5.991, chi2Stereo = 7.815;   // from round 1 on an edge is in only at or below this (infinity: no chi2 test)
	int minInliers = 10;                           // a pose left with fewer edges (and always: fewer than 3) is FEW_INLIERS and keeps its value
	bool dryRun = false;                           // only the statuses and counts: no pose changes
};

// the statuses (CUBA_HIP_POSEREF_* of cuba_hip.h)
enum class PoseRefinementStatus { OK = 0, NOT_SELECTED, FIXED, FEW_OBSERVATIONS, SINGULAR, FEW_INLIERS };

struct PoseRefinementResult
{
	long long counts[6] = { 0, 0, 0, 0, 0, 0 };      // poses per PoseRefinementStatus
	long long count(PoseRefinementStatus s) const { return counts[static_cast<int>(s)]; }
};

// ---- pose localisation from scratch (extension: cuba::localizePoses, bundle_adjustment.hpp; the reference has no counterpart) ----
struct PoseLocalizationOptions
{
	int hypotheses = 256;                          // three-point samples per pose (1 ... 4096), a fixed count
	unsigned long long seed = 0;                   // the samples are a function of (seed, pose, hypothesis, edge) in the graph's own numbering
	double chi2Mono = 5.991, chi2Stereo = 7.815;   // the cap of an edge's term in the score and the inlier threshold (finite, > 0)
	int minInliers = 10;                           // a pose whose winner has fewer inliers (and always: fewer than 4) is FEW_INLIERS and keeps its value
	bool dryRun = false;                           // only the statuses and counts: no pose changes
};

// the statuses (CUBA_HIP_POSELOC_* of cuba_hip.h)
enum class PoseLocalizationStatus { OK = 0, NOT_SELECTED, FIXED, FEW_OBSERVATIONS, NO_SOLUTION, FEW_INLIERS };

struct PoseLocalizationResult
{
	long long counts[6] = { 0, 0, 0, 0, 0, 0 };      // poses per PoseLocalizationStatus
	long long count(PoseLocalizationStatus s) const { return counts[static_cast<int>(s)]; }
};

// short names used inside the reference's sources (types.h:242-245)
using VertexP = PoseVertex;
using VertexL = LandmarkVertex;
using Edge2D = MonoEdge;
using Edge3D = StereoEdge;

}  // namespace cuba
