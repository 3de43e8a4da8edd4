// bundle_adjustment.hpp -- the cuba::CudaBundleAdjustment interface, MI355X build.
//
// Same abstract class as /root/reference/include/cuda_bundle_adjustment.h:34-125 (every method keeps
// its name, signature and documented behaviour); the implementation behind create() is a host C++
// layer over the C ABI of include/cuba_hip.h, which runs the hot path as HIP kernels on gfx950.
//
// Behaviour kept from the reference:
//   * the optimiser never deletes vertices or edges -- the caller owns them (ref .h:30-31);
//   * poseVertex(id) / landmarkVertex(id) throw std::out_of_range for unknown ids (ref .cpp:707-715);
//   * initialize() must be called after the graph changed and before optimize();
//   * optimize() may be called repeatedly (warm start); results are written back into the vertices;
//   * chiSquared(e) is 0 for edges that were inactive (both ends fixed, or switched off: cuba::gateEdges / cuba::setEdgeActive below)
//     or unknown (ref .cpp:878-881);
//   * timeProfile() uses the reference's eight key strings (ref .cpp:545-562).
// Difference: device / numerical failures are reported by exceptions (std::runtime_error) from
// initialize()/optimize() instead of being printed and ignored (ref src/macro.h:22-27).
#pragma once

#include <array>
#include <cstddef>
#include <utility>
#include <vector>

#include "ba_types.hpp"

namespace cuba
{

class CudaBundleAdjustment
{
public:
	using Ptr = UniquePtr<CudaBundleAdjustment>;

	// Inline on purpose: the application's own view of the vertex / edge layouts (they embed Eigen types, whose size and
	// alignment depend on the Eigen the APPLICATION was compiled with) travels into the library, which refuses to start
	// when it was built against a different layout -- e.g. the library against the in-repo Eigen stand-in and the
	// application against real Eigen3, whose Quaterniond is 16-byte aligned.  Throws std::runtime_error on a mismatch.
	static Ptr create()
	{
		const size_t layout[8] = { sizeof(PoseVertex), alignof(PoseVertex), offsetof(PoseVertex, t), offsetof(PoseVertex, camera),
			sizeof(LandmarkVertex), offsetof(LandmarkVertex, fixed), sizeof(MonoEdge), sizeof(StereoEdge) };
		return createChecked(layout, 8);
	}
	static Ptr createChecked(const size_t* layout, int n);

	virtual void addPoseVertex(PoseVertex* v) = 0;
	virtual void addLandmarkVertex(LandmarkVertex* v) = 0;
	virtual void addMonocularEdge(MonoEdge* e) = 0;
	virtual void addStereoEdge(StereoEdge* e) = 0;

	virtual PoseVertex* poseVertex(int id) const = 0;
	virtual LandmarkVertex* landmarkVertex(int id) const = 0;

	virtual void removePoseVertex(PoseVertex* v) = 0;
	virtual void removeLandmarkVertex(LandmarkVertex* v) = 0;
	virtual void removeEdge(BaseEdge* e) = 0;

	virtual size_t nposes() const = 0;
	virtual size_t nlandmarks() const = 0;
	virtual size_t nedges() const = 0;

	// robust kernel for all edges of one type; default is NONE
	virtual void setRobustKernels(RobustKernelType kernelType, double delta, EdgeType edgeType) = 0;

	virtual void initialize() = 0;
	virtual void optimize(int niterations) = 0;   // Levenberg-Marquardt iterations
	virtual void clear() = 0;

	virtual const BatchStatistics& batchStatistics() const = 0;
	virtual const TimeProfile& timeProfile() const = 0;
	virtual double chiSquared(const BaseEdge* e) const = 0;

	virtual ~CudaBundleAdjustment();
};

// Extension of this library (the reference has no counterpart): optimize(niterations) of several independent objects -- ORB-SLAM's
// local-BA windows, the graphs of several agents -- as ONE device launch chain.  Every object ends exactly where its own optimize()
// would have ended (estimates in its vertices, batchStatistics(), chiSquared()), bit for bit; small graphs gain most (eight
// KITTI-07-sized graphs: 3.2 x one graph's throughput on one MI355X).  All objects must have been initialize()d.
void optimizeBatch(CudaBundleAdjustment* const* objects, int n, int niterations);

// Extension of this library (g2o's SparseOptimizer::computeMarginals; the reference has no counterpart): marginal covariances at the
// object's current estimate -- the inverse of the undamped Gauss-Newton Hessian (robust weights rho' omega, fixed vertices eliminated;
// include/cuba_hip.h, cuba_hip_compute_covariance).  Call after optimize() (or after initialize(): the graph is uploaded first).
// computeCovariances returns false when that Hessian is not positive definite; refusals (fp32 library, a factor beyond device memory)
// throw std::runtime_error.  The object's next optimize() runs exactly as if the call had not happened.
//   poseCovariance      6 x 6, column-major, in the tangent [omega, upsilon] of the pose update (left-multiplicative se3 exponential)
//   landmarkCovariance  3 x 3, column-major (only after computeCovariances(object, true))
// Both return false for a fixed vertex, a vertex the last computation did not cover, or when nothing was computed since the last
// initialize().
bool computeCovariances(CudaBundleAdjustment* object, bool landmarks);
bool poseCovariance(const CudaBundleAdjustment* object, const PoseVertex* v, double cov[36]);
bool landmarkCovariance(const CudaBundleAdjustment* object, const LandmarkVertex* v, double cov[9]);

// Covariance blocks of arbitrary vertex pairs (include/cuba_hip.h, cuba_hip_compute_covariance_pairs): any two vertices, co-visible or
// not -- the drift of the last pose against the first, loop-closure gates, pose-landmark and landmark-landmark cross terms.  A
// CovarianceVertex names a PoseVertex or a LandmarkVertex of the object; out[k] receives pair k's dim(a) x dim(b) block of the same
// inverse as computeCovariances (6 for a pose, 3 for a landmark; rows from a, columns from b, column-major with leading dimension
// dim(a), the rest zero; zero for a fixed vertex).  Self-contained (no earlier computeCovariances needed).  Returns false, out
// untouched, when the Hessian is not positive definite; a vertex that is not part of the object throws std::invalid_argument, other
// refusals (fp32 library, a factor beyond device memory) throw std::runtime_error.  The object's next optimize() is unaffected.
struct CovarianceVertex
{
	const PoseVertex* pose = nullptr;
	const LandmarkVertex* landmark = nullptr;
	CovarianceVertex(const PoseVertex* v) : pose(v) {}
	CovarianceVertex(const LandmarkVertex* v) : landmark(v) {}
};
using CovariancePair = std::pair<CovarianceVertex, CovarianceVertex>;
bool computeCrossCovariances(CudaBundleAdjustment* object, const std::vector<CovariancePair>& pairs, std::vector<std::array<double, 36>>& out);

// Extension (g2o's OptimizableGraph::Edge::setLevel / computeActiveErrors, as ORB-SLAM's local bundle adjustment and pose optimisation
// use them; the reference has no counterpart; include/cuba_hip.h, cuba_hip_gate_edges): reprojection edges are switched off and on
// WITHOUT removeEdge + initialize() -- no new topology, structure or symbolic analysis.  An edge that is switched off takes no part in
// optimize(), optimizeBatch(), the objective or the covariances, and its chiSquared() is 0.
//   gateEdges          classifies every edge of the initialize()d graph on the device at the current estimate (EdgeGate, ba_types.hpp):
//                      active iff omega |r|^2 <= chi2Mono / chi2Stereo and (positiveDepth) its point lies in front of the camera.
//                      Returns the counts; unless the mode is DRY_RUN the edges' levels are those of the classification afterwards.
//   edgeGateChiSquared the UNGATED omega |r|^2 of an edge at the last gateEdges (0 before one and for an edge it did not cover)
//   setEdgeActive      one edge's level by hand (takes effect with the next optimize / gateEdges / covariance call; no initialize() needed)
//   edgeActive         true unless the edge is switched off
//   activeObservations a landmark's edges that are part of the graph and switched on (ORB-SLAM culls points left with fewer than two)
// The levels belong to the edge objects: they survive initialize() after any change of the graph that keeps the edge, removeEdge /
// removePoseVertex / removeLandmarkVertex drop the level of the edges that leave, clear() drops all.  The ORB-SLAM flow:
//   ba->initialize(); ba->optimize(5); cuba::gateEdges(ba.get(), {}); ba->optimize(10);
// Known limit: a switched-off edge whose point lies at depth exactly 0 in its camera still evaluates to 0 * inf.
EdgeGateResult gateEdges(CudaBundleAdjustment* object, const EdgeGate& gate);
void setEdgeActive(CudaBundleAdjustment* object, const BaseEdge* edge, bool active);
bool edgeActive(const CudaBundleAdjustment* object, const BaseEdge* edge);
double edgeGateChiSquared(const CudaBundleAdjustment* object, const BaseEdge* edge);
int activeObservations(const CudaBundleAdjustment* object, const LandmarkVertex* v);

// Extension (g2o's StructureOnlySolver<3>, ORB-SLAM's CreateNewMapPoints; the reference has no counterpart; include/cuba_hip.h,
// cuba_hip_triangulate_landmarks): the free landmarks of the initialize()d graph -- or those of `subset` -- are (re-)triangulated on the
// device from their switched-on reprojection edges and the current pose estimates: a linear start, refineIterations Gauss-Newton steps
// per landmark with the poses held and the robust kernels in force, then the acceptance tests (TriangulationOptions, ba_types.hpp).  The
// landmark's current Xw is never read.  Unless dryRun is set, the accepted positions are written into the LandmarkVertex::Xw of the OK
// landmarks (and are what the next optimize() starts from); every other vertex keeps its Xw.  Landmark priors take no part.
//   triangulationStatus   a landmark's status at the last triangulateLandmarks (NOT_SELECTED before one and for a vertex it did not cover)
// New map points with any Xw at all:  ba->initialize(); cuba::triangulateLandmarks(ba.get(), {}, &newPoints); ba->optimize(10);
TriangulationResult triangulateLandmarks(CudaBundleAdjustment* object, const TriangulationOptions& options, const std::vector<LandmarkVertex*>* subset = nullptr);
TriangulationStatus triangulationStatus(const CudaBundleAdjustment* object, const LandmarkVertex* v);

// Extension (g2o's motion-only bundle adjustment with EdgeSE3ProjectXYZOnlyPose, ORB-SLAM's Optimizer::PoseOptimization; the reference has
// no counterpart; include/cuba_hip.h, cuba_hip_refine_poses): the free poses of the initialize()d graph -- or those of `subset` -- are
// refined on the device from their switched-on reprojection edges with EVERY landmark held at its current estimate: `rounds` outlier
// rounds of `iterations` Levenberg-Marquardt trials, each pose with a damping of its own, the robust kernels in force in the first
// robustRounds rounds (PoseRefinementOptions, ba_types.hpp).  Unless dryRun is set, the refined poses are written into the PoseVertex::q / t
// of the OK poses (and are what the next optimize() starts from); every other vertex keeps its value.  Pose priors, relative-pose edges,
// position, direction and range factors take no part; the edge levels (setEdgeActive) are read, never written.
//   poseRefinementStatus    a pose's status at the last refinePoses (NOT_SELECTED before one and for a vertex it did not cover)
// New keyframes from a motion-model guess:  ba->initialize(); cuba::refinePoses(ba.get(), {}, &newKeyframes); ba->optimize(10);
PoseRefinementResult refinePoses(CudaBundleAdjustment* object, const PoseRefinementOptions& options, const std::vector<PoseVertex*>* subset = nullptr);
PoseRefinementStatus poseRefinementStatus(const CudaBundleAdjustment* object, const PoseVertex* v);

// Extension (the PnP-RANSAC half of ORB-SLAM's Tracking::Relocalization; the reference has no counterpart; include/cuba_hip.h,
// cuba_hip_localize_poses): the free poses of the initialize()d graph -- or those of `subset` -- get a value on the device from their
// switched-on reprojection edges and the current landmarks ALONE, by a deterministic RANSAC of `hypotheses` three-point (P3P) samples per
// pose scored by MSAC (PoseLocalizationOptions, ba_types.hpp).  A vertex's q / t before the call is never read: it may be anything, NaN
// included.  Unless dryRun is set, the winners are written into the PoseVertex::q / t of the OK poses (and are what the next refinePoses or
// optimize() starts from); every other vertex keeps its value.  Pose factors, landmark priors and robust kernels take no part; the edge
// levels (setEdgeActive) are read, never written.
//   poseLocalizationStatus  a pose's status at the last localizePoses (NOT_SELECTED before one and for a vertex it did not cover)
// A keyframe without a guess:  ba->initialize(); cuba::localizePoses(ba.get(), {}, &lost); cuba::refinePoses(ba.get(), {}, &lost); ba->optimize(10);
PoseLocalizationResult localizePoses(CudaBundleAdjustment* object, const PoseLocalizationOptions& options, const std::vector<PoseVertex*>* subset = nullptr);
PoseLocalizationStatus poseLocalizationStatus(const CudaBundleAdjustment* object, const PoseVertex* v);

// Robust kernel of a pose factor (PosePrior, RelativePoseEdge; include/cuba_hip.h, cuba_hip_set_pose_factor_robust_kernels): with
// e = r^T Omega r the objective term becomes rho(e) and the linearisation takes rho'(e) Omega for Omega.  HUBER and TUKEY are the kernels of
// the reprojection edges; CAUCHY, rho = delta^2 log1p(e / delta^2), exists for the pose factors only -- the usual choice on loop closures,
// since its weight never reaches zero.  (RobustKernelType mirrors the reference's type and knows no Cauchy.)
enum class PoseFactorKernel { NONE = 0, HUBER = 1, TUKEY = 2, CAUCHY = 3 };

// Extension (g2o's unary pose edges; include/cuba_hip.h, cuba_hip_set_pose_priors): an SE(3) prior on one pose vertex -- prior pose (q, t),
// world -> camera like the vertex, and a symmetric 6 x 6 information matrix, column-major, in the tangent [omega, upsilon] of the pose
// update (poseCovariance's tangent: the inverse of one window's marginal is a prior of the next).  Objective term r^T Omega r with
// r = log(T Tbar^-1), or rho(r^T Omega r) when `kernel` is set (`delta` > 0 then).  The caller owns the PosePrior, as it owns edges; additions, removals and changes take effect
// at the next initialize().  removePoseVertex and clear() drop the priors of the vertex / all priors.  priorChiSquared: r^T Omega r at
// the estimate of the last optimize() (0 before one, and for a prior on a fixed vertex) -- the plain value under a kernel too.
struct PosePrior
{
	PoseVertex* vertex = nullptr;
	PoseVertex::Rotation q;
	PoseVertex::Translation t;
	std::array<double, 36> information{};
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addPosePrior(CudaBundleAdjustment* object, PosePrior* prior);
void removePosePrior(CudaBundleAdjustment* object, PosePrior* prior);
double priorChiSquared(const CudaBundleAdjustment* object, const PosePrior* prior);

// Extension (g2o's binary SE(3) edge; include/cuba_hip.h, cuba_hip_set_relative_pose_edges): a relative-pose edge between two different
// pose vertices -- odometry, IMU pre-integration, loop closures.  (q, t) is the measured relative pose T_j T_i^-1 of the world -> camera
// poses of `vertexI` and `vertexJ` (it maps camera-i coordinates to camera-j coordinates); `information` is symmetric 6 x 6, column-major,
// in the tangent [omega, upsilon] of the pose update.  Objective term r^T Omega r with r = log(T_j T_i^-1 Zbar^-1), or
// rho(r^T Omega r) when `kernel` is set (`delta` > 0 then): a false loop closure under CAUCHY or TUKEY no longer bends the trajectory.
// Ownership and lifetime as for PosePrior: the caller owns the edge; additions, removals and changes take effect at the next
// initialize(); both vertices must be part of the graph then.  removePoseVertex drops the vertex's relative-pose edges, clear() all.
// relativePoseChiSquared: r^T Omega r at the estimate of the last optimize() (0 before one, and for an edge between two fixed vertices).
struct RelativePoseEdge
{
	PoseVertex* vertexI = nullptr;
	PoseVertex* vertexJ = nullptr;
	PoseVertex::Rotation q;
	PoseVertex::Translation t;
	std::array<double, 36> information{};
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addRelativePoseEdge(CudaBundleAdjustment* object, RelativePoseEdge* edge);
void removeRelativePoseEdge(CudaBundleAdjustment* object, RelativePoseEdge* edge);
double relativePoseChiSquared(const CudaBundleAdjustment* object, const RelativePoseEdge* edge);

// Extension (g2o's unary XYZ prior edge; include/cuba_hip.h, cuba_hip_set_landmark_priors): a position prior on one landmark vertex --
// surveyed ground-control points, points of a map of finite certainty, range-sensor points, the landmark half of a previous window's
// marginal.  `position` is the prior position Xbar, `information` symmetric 3 x 3, column-major (landmarkCovariance's layout: the inverse
// of one window's marginal is a prior of the next).  Objective term r^T Omega r with r = X - Xbar, or rho(r^T Omega r) when `kernel` is
// set (`delta` > 0 then).  Ownership and lifetime as for PosePrior: the caller owns the prior; additions, removals and changes take
// effect at the next initialize(); the vertex must be part of the graph then (a landmark without an edge is not).  removeLandmarkVertex
// drops the vertex's priors, clear() all.  landmarkPriorChiSquared: r^T Omega r at the estimate of the last optimize() (0 before one, and
// for a prior on a fixed vertex) -- the plain value under a kernel too.
struct LandmarkPrior
{
	LandmarkVertex* vertex = nullptr;
	LandmarkVertex::Point3D position;
	std::array<double, 9> information{};
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addLandmarkPrior(CudaBundleAdjustment* object, LandmarkPrior* prior);
void removeLandmarkPrior(CudaBundleAdjustment* object, LandmarkPrior* prior);
double landmarkPriorChiSquared(const CudaBundleAdjustment* object, const LandmarkPrior* prior);

// Extension (include/cuba_hip.h, cuba_hip_set_position_factors): a position factor on one pose vertex -- a measured WORLD position of a
// point that rides on the camera, without an orientation: a GNSS fix of the antenna, a total-station prism, a mocap marker, a UWB
// position.  `position` is the measurement z, `leverArm` the measured point a in the camera frame (zero: the camera centre),
// `information` symmetric 3 x 3, column-major.  Objective term r^T Omega r with r = R^T (a - t) - z for the vertex's world -> camera pose
// [R | t], or rho(r^T Omega r) when `kernel` is set (`delta` > 0 then).  A PosePrior cannot say this: its translation residual depends
// on a prior rotation.  Three such factors give a graph without a fixed vertex its gauge, and a monocular one its scale.  The fp32
// library evaluates r in fp32: subtract a local origin from UTM-size coordinates first.  Ownership and lifetime as for PosePrior: the
// caller owns the factor; additions, removals and changes take effect at the next initialize(); the vertex must be part of the graph
// then.  removePoseVertex drops the vertex's factors, clear() all.  positionFactorChiSquared: r^T Omega r at the estimate of the last
// optimize() (0 before one, and for a factor on a fixed vertex) -- the plain value under a kernel too.
struct PositionFactor
{
	PoseVertex* vertex = nullptr;
	std::array<double, 3> position{};
	std::array<double, 3> leverArm{};
	std::array<double, 9> information{};
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addPositionFactor(CudaBundleAdjustment* object, PositionFactor* factor);
void removePositionFactor(CudaBundleAdjustment* object, PositionFactor* factor);
double positionFactorChiSquared(const CudaBundleAdjustment* object, const PositionFactor* factor);

// Extension (include/cuba_hip.h, cuba_hip_set_direction_factors): a direction factor on one pose vertex -- a known WORLD direction as seen
// in the camera frame: the gravity vector of an accelerometer (roll and pitch, no yaw), a magnetometer or sun-sensor bearing, the
// vanishing direction of a Manhattan world, one star of a star tracker.  `worldDirection` is d, `measurement` the same vector measured in
// the camera frame, m (neither is normalised: unit vectors, or gravity in m/s^2 against a specific-force reading), `information`
// symmetric 3 x 3, column-major; (I - m m^T) / sigma^2, of rank 2, is the usual one.  Objective term r^T Omega r with r = R d - m for the
// vertex's world -> camera rotation R, or rho(r^T Omega r) when `kernel` is set (`delta` > 0 then).  A PosePrior cannot say this: it
// needs a whole prior rotation.  Ownership and lifetime as for PosePrior: the caller owns the factor; additions, removals and changes
// take effect at the next initialize(); the vertex must be part of the graph then.  removePoseVertex drops the vertex's factors, clear()
// all.  directionFactorChiSquared: r^T Omega r at the estimate of the last optimize() (0 before one, and for a factor on a fixed vertex)
// -- the plain value under a kernel too.
struct DirectionFactor
{
	PoseVertex* vertex = nullptr;
	std::array<double, 3> worldDirection{};
	std::array<double, 3> measurement{};
	std::array<double, 9> information{};
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addDirectionFactor(CudaBundleAdjustment* object, DirectionFactor* factor);
void removeDirectionFactor(CudaBundleAdjustment* object, DirectionFactor* factor);
double directionFactorChiSquared(const CudaBundleAdjustment* object, const DirectionFactor* factor);

// Extension (include/cuba_hip.h, cuba_hip_set_range_factors): a range factor on one pose vertex -- a measured DISTANCE from a point of the
// platform to a known world point: a UWB anchor, an acoustic beacon, DME, a total station that reports slope distance only.  `anchor` is
// the world point b, `range` the measured distance (>= 0), `leverArm` the ranging antenna in the camera frame (zero: the camera centre),
// `information` the scalar 1 / sigma^2 (>= 0).  Objective term information * r^2 with r = |a - (R b + t)| - range for the vertex's
// world -> camera pose [R | t], or rho(information * r^2) when `kernel` is set (`delta` > 0 then).  One range constrains the pose to a
// sphere, which neither a PositionFactor (a 3-D fix; rank-1 information on it is a plane) nor a PosePrior can say; four non-coplanar
// anchors heard from three poses off a line give a graph without a fixed vertex its gauge, and a monocular one its scale.  With the
// antenna exactly at the anchor the direction is undefined: the factor then adds nothing to the system and keeps its chi2,
// information * range^2.  Ownership and lifetime as for PositionFactor: the caller owns the factor; additions, removals and changes take
// effect at the next initialize(); the vertex must be part of the graph then.  removePoseVertex drops the vertex's factors, clear() all.
// rangeFactorChiSquared: information * r^2 at the estimate of the last optimize() (0 before one, and for a factor on a fixed vertex) --
// the plain value under a kernel too.
struct RangeFactor
{
	PoseVertex* vertex = nullptr;
	std::array<double, 3> anchor{};
	std::array<double, 3> leverArm{};
	double range = 0;
	double information = 0;
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addRangeFactor(CudaBundleAdjustment* object, RangeFactor* factor);
void removeRangeFactor(CudaBundleAdjustment* object, RangeFactor* factor);
double rangeFactorChiSquared(const CudaBundleAdjustment* object, const RangeFactor* factor);

// Extension (include/cuba_hip.h, cuba_hip_set_pose_range_factors): a range factor BETWEEN two pose vertices -- a measured distance from
// a point riding on pose i to a point riding on pose j: the travelled distance of a wheel odometer between two keyframes (the scale of a
// monocular graph, without any orientation), peer-to-peer UWB ranging, the baseline length of a rig whose cameras are separate poses, a
// taped distance between two stations.  `leverArmI` / `leverArmJ` are the two points in their camera frames (zero: the camera centres),
// `range` the measured distance (>= 0), `information` the scalar 1 / sigma^2 (>= 0).  Objective term information * r^2 with
// r = |R_i^T (a_i - t_i) - R_j^T (a_j - t_j)| - range, or rho(information * r^2) when `kernel` is set (`delta` > 0 then).  The pair owns a
// block of the reduced matrix also where no landmark connects the two poses.  A factor with one fixed vertex acts on the free one only; one
// with two fixed vertices is ignored.  With the two points exactly on each other the direction is undefined: the factor then adds nothing to
// the system and keeps its chi2, information * range^2.  Ownership and lifetime as for RelativePoseEdge: the caller owns the factor;
// additions, removals and changes take effect at the next initialize(); both vertices must be part of the graph then.  removePoseVertex
// drops the factors touching the vertex, clear() all.  poseRangeFactorChiSquared: information * r^2 at the estimate of the last optimize()
// (0 before one, and for a factor between two fixed vertices) -- the plain value under a kernel too.
struct PoseRangeFactor
{
	PoseVertex* vertexI = nullptr;
	PoseVertex* vertexJ = nullptr;
	std::array<double, 3> leverArmI{};
	std::array<double, 3> leverArmJ{};
	double range = 0;
	double information = 0;
	PoseFactorKernel kernel = PoseFactorKernel::NONE;
	double delta = 0;
};
void addPoseRangeFactor(CudaBundleAdjustment* object, PoseRangeFactor* factor);
void removePoseRangeFactor(CudaBundleAdjustment* object, PoseRangeFactor* factor);
double poseRangeFactorChiSquared(const CudaBundleAdjustment* object, const PoseRangeFactor* factor);

}  // namespace cuba
