// factor_trace.cpp -- what the host layer (../bundle_adjustment.cpp) asks of the device library for the seven factor kinds, made
// visible without a GPU: the public API only, on the smallest graph that reaches every branch, linked against the recording stand-in
// fake_cuba_hip.cpp.  The stand-in prints every C ABI call; this program prints a marker line per step and, after it, every
// xChiSquared of every factor object it owns.  The whole output is compared with tests/golden/host_factor_calls.txt byte for byte
// (tests/test_host_factor_calls.py): the order and content of the calls are the contract a change of the host layer must keep.
#include <array>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <utility>
#include <vector>

#include <cuda_bundle_adjustment.h>

using namespace cuba;
using BA = CudaBundleAdjustment;
using V3 = Array<double, 3>;

// one name for the three public functions of every kind
static void add(BA* b, PosePrior* f) { addPosePrior(b, f); }
static void add(BA* b, RelativePoseEdge* f) { addRelativePoseEdge(b, f); }
static void add(BA* b, LandmarkPrior* f) { addLandmarkPrior(b, f); }
static void add(BA* b, PositionFactor* f) { addPositionFactor(b, f); }
static void add(BA* b, DirectionFactor* f) { addDirectionFactor(b, f); }
static void add(BA* b, RangeFactor* f) { addRangeFactor(b, f); }
static void add(BA* b, PoseRangeFactor* f) { addPoseRangeFactor(b, f); }
static void remove(BA* b, PosePrior* f) { removePosePrior(b, f); }
static void remove(BA* b, RelativePoseEdge* f) { removeRelativePoseEdge(b, f); }
static void remove(BA* b, LandmarkPrior* f) { removeLandmarkPrior(b, f); }
static void remove(BA* b, PositionFactor* f) { removePositionFactor(b, f); }
static void remove(BA* b, DirectionFactor* f) { removeDirectionFactor(b, f); }
static void remove(BA* b, RangeFactor* f) { removeRangeFactor(b, f); }
static void remove(BA* b, PoseRangeFactor* f) { removePoseRangeFactor(b, f); }
static double chi(const BA* b, const PosePrior* f) { return priorChiSquared(b, f); }
static double chi(const BA* b, const RelativePoseEdge* f) { return relativePoseChiSquared(b, f); }
static double chi(const BA* b, const LandmarkPrior* f) { return landmarkPriorChiSquared(b, f); }
static double chi(const BA* b, const PositionFactor* f) { return positionFactorChiSquared(b, f); }
static double chi(const BA* b, const DirectionFactor* f) { return directionFactorChiSquared(b, f); }
static double chi(const BA* b, const RangeFactor* f) { return rangeFactorChiSquared(b, f); }
static double chi(const BA* b, const PoseRangeFactor* f) { return poseRangeFactorChiSquared(b, f); }

template <size_t N> static std::array<double, N> ramp(double first)
{
	std::array<double, N> a;
	for (size_t i = 0; i < N; i++) a[i] = first + 0.125 * i;
	return a;
}

static PoseFactorKernel NONE = PoseFactorKernel::NONE, HUBER = PoseFactorKernel::HUBER, TUKEY = PoseFactorKernel::TUKEY, CAUCHY = PoseFactorKernel::CAUCHY;

static PosePrior posePrior(PoseVertex* v, double x, PoseFactorKernel k = NONE, double delta = 0)
{
	PosePrior f; f.vertex = v; f.q = Eigen::Quaterniond(1, x, 0, 0); f.t = V3(x, x + 1, x + 2); f.information = ramp<36>(x); f.kernel = k; f.delta = delta;
	return f;
}
static RelativePoseEdge relativePose(PoseVertex* i, PoseVertex* j, double x, PoseFactorKernel k = NONE, double delta = 0)
{
	RelativePoseEdge f; f.vertexI = i; f.vertexJ = j; f.q = Eigen::Quaterniond(1, 0, x, 0); f.t = V3(-x, x, 2 * x); f.information = ramp<36>(x); f.kernel = k; f.delta = delta;
	return f;
}
static LandmarkPrior landmarkPrior(LandmarkVertex* v, double x, PoseFactorKernel k = NONE, double delta = 0)
{
	LandmarkPrior f; f.vertex = v; f.position = V3(x, 2 * x, 3 * x); f.information = ramp<9>(x); f.kernel = k; f.delta = delta;
	return f;
}
static PositionFactor positionFactor(PoseVertex* v, double x)
{
	PositionFactor f; f.vertex = v; f.position = ramp<3>(x); f.leverArm = ramp<3>(-x); f.information = ramp<9>(x);
	return f;
}
static DirectionFactor directionFactor(PoseVertex* v, double x, PoseFactorKernel k = NONE, double delta = 0)
{
	DirectionFactor f; f.vertex = v; f.worldDirection = ramp<3>(x); f.measurement = ramp<3>(2 * x); f.information = ramp<9>(x); f.kernel = k; f.delta = delta;
	return f;
}
static RangeFactor rangeFactor(PoseVertex* v, double x, PoseFactorKernel k = NONE, double delta = 0)
{
	RangeFactor f; f.vertex = v; f.anchor = ramp<3>(x); f.leverArm = ramp<3>(-x); f.range = 10 * x; f.information = x / 4; f.kernel = k; f.delta = delta;
	return f;
}
static PoseRangeFactor poseRange(PoseVertex* i, PoseVertex* j, double x, PoseFactorKernel k = NONE, double delta = 0)
{
	PoseRangeFactor f; f.vertexI = i; f.vertexJ = j; f.leverArmI = ramp<3>(x); f.leverArmJ = ramp<3>(-x); f.range = 10 * x; f.information = x / 4; f.kernel = k; f.delta = delta;
	return f;
}

static std::vector<std::pair<const char*, std::function<double()>>> owned;      // every factor object of this program, for the chi2 listing

static void marker(const char* what)
{
	std::printf("== %s\n", what);
	for (const auto& o : owned) std::printf("chi2 %s %a\n", o.first, o.second());
}

template <class Fn> static void expectThrow(const char* what, Fn&& fn)
{
	try { fn(); std::printf("%s: no exception\n", what); }
	catch (const std::invalid_argument& e) { std::printf("%s: std::invalid_argument: %s\n", what, e.what()); }
	catch (const std::runtime_error& e) { std::printf("%s: std::runtime_error: %s\n", what, e.what()); }
	catch (const std::exception& e) { std::printf("%s: std::exception: %s\n", what, e.what()); }
}

static void solve(BA* ba, int iterations, bool init = true)
{
	if (init) ba->initialize();
	ba->optimize(iterations);
	std::printf("statistics");
	for (const auto& s : ba->batchStatistics()) std::printf(" %d:%a", s.iteration, s.chi2);
	std::printf("\n");
}

// steps 7 and 9 for one kind: what add refuses (null, no vertex, for the binary kinds one vertex or the same vertex twice), and
// remove / chi2 of an object that was never added
template <class F> static void refusals(BA* ba, const char* kind, std::vector<F> bad)
{
	expectThrow(kind, [&] { add(ba, static_cast<F*>(nullptr)); });
	for (F& f : bad)
	{
		expectThrow(kind, [&] { add(ba, &f); });
		remove(ba, &f);
		std::printf("%s never added: chi2 %a\n", kind, chi(ba, &f));
	}
}

// step 8 for one kind: a factor on a vertex that is not part of the graph is refused by the solve after the next initialize()
template <class F> static void outsideTheGraph(BA* ba, const char* kind, F f)
{
	add(ba, &f);
	expectThrow(kind, [&] { solve(ba, 1); });
	remove(ba, &f);
	solve(ba, 1, false);
	solve(ba, 1);
}

int main()
{
	CameraParams cam; cam.fx = 500; cam.fy = 510; cam.cx = 320; cam.cy = 240; cam.bf = 50;
	const Eigen::Quaterniond q0(1, 0, 0, 0);
	// solver order: free poses by id (5, 7), then the fixed one (3); pose 9 has no edges and is not part of the flattened graph
	PoseVertex p7(7, q0, V3(0, 0, 0), cam), p3(3, q0, V3(1, 0, 0), cam, true), p5(5, q0, V3(2, 0, 0), cam), p9(9, q0, V3(3, 0, 0), cam);
	LandmarkVertex l20(20, V3(0, 0, 10)), l10(10, V3(1, 0, 10), true), l30(30, V3(2, 0, 10)), l40(40, V3(3, 0, 10));
	LandmarkVertex lOut(50, V3(4, 0, 10));      // never added
	MonoEdge m1(Array<double, 2>(1, 2), 1.0, &p7, &l20), m2(Array<double, 2>(3, 4), 2.0, &p3, &l10), m3(Array<double, 2>(5, 6), 3.0, &p5, &l20),
		m4(Array<double, 2>(7, 8), 4.0, &p5, &l40);
	StereoEdge s1(Array<double, 3>(1, 2, 3), 5.0, &p3, &l20), s2(Array<double, 3>(4, 5, 6), 6.0, &p5, &l30), s3(Array<double, 3>(7, 8, 9), 7.0, &p7, &l30),
		s4(Array<double, 3>(10, 11, 12), 8.0, &p7, &l40);

	auto holder = BA::create();
	BA* ba = holder.get();
	for (auto* p : { &p7, &p3, &p5, &p9 }) ba->addPoseVertex(p);
	for (auto* l : { &l20, &l10, &l30, &l40 }) ba->addLandmarkVertex(l);
	for (auto* e : { &m1, &m2, &m3, &m4 }) ba->addMonocularEdge(e);
	for (auto* e : { &s1, &s2, &s3, &s4 }) ba->addStereoEdge(e);
	ba->setRobustKernels(RobustKernelType::HUBER, 2.5, EdgeType::MONOCULAR);

	// the position factors stay without kernels throughout
	PosePrior prA = posePrior(&p5, 1, HUBER, 1.5), prB = posePrior(&p7, 2), prC = posePrior(&p3, 3);
	RelativePoseEdge reA = relativePose(&p5, &p7, 1, CAUCHY, 2.5), reB = relativePose(&p3, &p5, 2), reC = relativePose(&p7, &p3, 3);
	LandmarkPrior lpA = landmarkPrior(&l20, 1, TUKEY, 3.5), lpB = landmarkPrior(&l30, 2), lpC = landmarkPrior(&l10, 3);
	PositionFactor poA = positionFactor(&p5, 1), poB = positionFactor(&p7, 2), poC = positionFactor(&p3, 3);
	DirectionFactor diA = directionFactor(&p5, 1, HUBER, 4.5), diB = directionFactor(&p7, 2);
	RangeFactor raA = rangeFactor(&p5, 1, CAUCHY, 5.5), raB = rangeFactor(&p7, 2), raC = rangeFactor(&p5, 3);
	PoseRangeFactor pgA = poseRange(&p5, &p7, 1, HUBER, 6.5), pgB = poseRange(&p7, &p3, 2), pgC = poseRange(&p5, &p3, 3);
#define OWN(f) owned.emplace_back(#f, [&, ba] { return chi(ba, &f); })
	OWN(prA); OWN(prB); OWN(prC); OWN(reA); OWN(reB); OWN(reC); OWN(lpA); OWN(lpB); OWN(lpC); OWN(poA); OWN(poB); OWN(poC);
	OWN(diA); OWN(diB); OWN(raA); OWN(raB); OWN(raC); OWN(pgA); OWN(pgB); OWN(pgC);
#undef OWN

	marker("step 1: two or three factors of every kind, one of each added twice");
	add(ba, &prA); add(ba, &prB); add(ba, &prB); add(ba, &prC);
	add(ba, &reA); add(ba, &reB); add(ba, &reA); add(ba, &reC);
	add(ba, &lpA); add(ba, &lpB); add(ba, &lpC); add(ba, &lpC);
	add(ba, &poA); add(ba, &poA); add(ba, &poB); add(ba, &poC);
	add(ba, &diA); add(ba, &diB); add(ba, &diB);
	add(ba, &raA); add(ba, &raB); add(ba, &raC); add(ba, &raA);
	add(ba, &pgA); add(ba, &pgB); add(ba, &pgA);
	solve(ba, 2);

	marker("step 2: optimize again, nothing changed");
	solve(ba, 1, false);

	marker("step 3: initialize and optimize, nothing changed");
	solve(ba, 1);

	marker("step 4: one factor of every kind removed");
	remove(ba, &prA); remove(ba, &reB); remove(ba, &lpA); remove(ba, &poC); remove(ba, &diA); remove(ba, &raC); remove(ba, &pgA);
	solve(ba, 1, false);      // (until the next initialize() the device holds the sets as they were, the removed factors' chi2 included)
	marker("step 4: after initialize");
	solve(ba, 1);

	marker("step 5: the last direction factor and the last range factor between poses removed");
	remove(ba, &diB); remove(ba, &pgB);
	solve(ba, 1);
	marker("step 5: once more");
	solve(ba, 1);

	marker("step 6: pose 7 and landmark 30 removed, with factors of every kind on them");
	add(ba, &diB); add(ba, &diA); add(ba, &pgA); add(ba, &pgC);
	ba->removePoseVertex(&p7);
	ba->removeLandmarkVertex(&l30);
	solve(ba, 1);

	marker("steps 7 and 9: what add refuses; remove and chi2 of factors that were never added");
	{
		PosePrior a; RelativePoseEdge b, bI, bSame; LandmarkPrior c; PositionFactor d; DirectionFactor e; RangeFactor f; PoseRangeFactor g, gI, gSame;
		bI.vertexI = &p5; bSame.vertexI = bSame.vertexJ = &p5; gI.vertexI = &p5; gSame.vertexI = gSame.vertexJ = &p5;
		refusals<PosePrior>(ba, "PosePrior", { a });
		refusals<RelativePoseEdge>(ba, "RelativePoseEdge", { b, bI, bSame });
		refusals<LandmarkPrior>(ba, "LandmarkPrior", { c });
		refusals<PositionFactor>(ba, "PositionFactor", { d });
		refusals<DirectionFactor>(ba, "DirectionFactor", { e });
		refusals<RangeFactor>(ba, "RangeFactor", { f });
		refusals<PoseRangeFactor>(ba, "PoseRangeFactor", { g, gI, gSame });
	}

	marker("step 8: factors on vertices that are not part of the graph");
	outsideTheGraph(ba, "PosePrior", posePrior(&p9, 4));
	outsideTheGraph(ba, "RelativePoseEdge", relativePose(&p5, &p9, 4));
	outsideTheGraph(ba, "RelativePoseEdge", relativePose(&p9, &p5, 5, HUBER, 1.0));
	outsideTheGraph(ba, "LandmarkPrior", landmarkPrior(&lOut, 4));
	outsideTheGraph(ba, "PositionFactor", positionFactor(&p9, 4));
	outsideTheGraph(ba, "DirectionFactor", directionFactor(&p9, 4));
	outsideTheGraph(ba, "RangeFactor", rangeFactor(&p9, 4));
	outsideTheGraph(ba, "PoseRangeFactor", poseRange(&p9, &p5, 4));
	outsideTheGraph(ba, "PoseRangeFactor", poseRange(&p5, &p9, 5, TUKEY, 2.0));

	marker("step 10: clear, then a new graph with one factor");
	ba->clear();
	PoseVertex n1(1, q0, V3(0, 1, 0), cam), n2(2, q0, V3(0, 2, 0), cam, true);
	LandmarkVertex k1(1, V3(0, 1, 10)), k2(2, V3(0, 2, 10));
	MonoEdge e1(Array<double, 2>(1, 1), 1.0, &n1, &k1), e2(Array<double, 2>(2, 2), 1.0, &n2, &k2);
	StereoEdge e3(Array<double, 3>(3, 3, 3), 1.0, &n1, &k2);
	ba->addPoseVertex(&n1); ba->addPoseVertex(&n2); ba->addLandmarkVertex(&k1); ba->addLandmarkVertex(&k2);
	ba->addMonocularEdge(&e1); ba->addMonocularEdge(&e2); ba->addStereoEdge(&e3);
	RangeFactor raN = rangeFactor(&n1, 6, HUBER, 7.5);
	add(ba, &raN);
	solve(ba, 1);
	std::printf("chi2 raN %a\n", chi(ba, &raN));
	marker("end");
	return 0;
}
