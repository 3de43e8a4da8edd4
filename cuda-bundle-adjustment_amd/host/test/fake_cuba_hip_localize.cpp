// fake_cuba_hip_localize.cpp -- the stand-in's cuba_hip_localize_poses, beside fake_cuba_hip.cpp, fake_cuba_hip_triangulate.cpp and
// fake_cuba_hip_pose_refine.cpp (which hold every other cuba_hip_* symbol that ../bundle_adjustment.cpp references) and linked into the same
// programs.  It prints the call like the others -- scalars, then the selection mask as an array or `null`, then which outputs were asked
// for -- and makes up a result in which a value attributed to the wrong pose shows: a selected pose p is OK (p % 3 == 0), FEW_INLIERS (1)
// or NO_SOLUTION (2); an OK pose's value is q = (0, 1, 0, 0), t = (1000 + p, 2000 + p, 3000 + p), every other one's is what the last
// cuba_hip_set_graph_begin was given.  Unless it is a dry run, the stand-in's estimates take the OK poses, so that a later
// cuba_hip_get_solution returns them.

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cuba_hip.h"

// (the definition of fake_cuba_hip.cpp, token for token: one type in one program)
struct cuba_hip_solver
{
	int Pt = 0, Lt = 0, E = 0;
	std::vector<double> q, t, Xw;      // what the last set_graph_begin was given
	int64_t uploads = 0;
	int nFactors[7] = { 0, 0, 0, 0, 0, 0, 0 };      // size of the set last given, per kind
};

extern "C" int cuba_hip_localize_poses(cuba_hip_solver* s, const uint8_t* select, int hypotheses, uint64_t seed, const double chi2_max[2], int min_inliers,
	int dry_run, int32_t* status, int64_t counts[CUBA_HIP_POSELOC_STATUSES], int32_t* inliers, double* cost, int32_t* winner, double* q, double* t,
	uint8_t* edge_inlier)
{
	std::printf("cuba_hip_localize_poses %d %" PRIu64 " %a %a %d %d", hypotheses, seed, chi2_max[0], chi2_max[1], min_inliers, dry_run);
	if (!select) std::printf(" | null");
	else
	{
		std::printf(" | %d", s->Pt);
		for (int p = 0; p < s->Pt; p++) std::printf(" %d", (int)select[p]);
	}
	std::printf(" | outputs %d%d%d%d%d%d%d%d", status ? 1 : 0, counts ? 1 : 0, inliers ? 1 : 0, cost ? 1 : 0, winner ? 1 : 0, q ? 1 : 0, t ? 1 : 0, edge_inlier ? 1 : 0);
	int64_t c[CUBA_HIP_POSELOC_STATUSES] = { 0, 0, 0, 0, 0, 0 };
	for (int p = 0; p < s->Pt; p++)
	{
		const int st = select && !select[p] ? CUBA_HIP_POSELOC_NOT_SELECTED : p % 3 == 0 ? CUBA_HIP_POSELOC_OK : p % 3 == 1 ? CUBA_HIP_POSELOC_FEW_INLIERS : CUBA_HIP_POSELOC_NO_SOLUTION;
		c[st]++;
		if (status) status[p] = st;
		if (inliers) inliers[p] = st == CUBA_HIP_POSELOC_NOT_SELECTED ? 0 : 10 + p;
		if (cost) cost[p] = st == CUBA_HIP_POSELOC_OK ? 0.5 + p : 0.0;
		if (winner) winner[p] = st == CUBA_HIP_POSELOC_OK ? 4 * p : -1;
		for (int k = 0; k < 4; k++)
		{
			const double x = st == CUBA_HIP_POSELOC_OK ? (k == 1 ? 1.0 : 0.0) : s->q[4 * (size_t)p + k];
			if (q) q[4 * (size_t)p + k] = x;
			if (!dry_run) s->q[4 * (size_t)p + k] = x;
		}
		for (int k = 0; k < 3; k++)
		{
			const double x = st == CUBA_HIP_POSELOC_OK ? 1000.0 * (k + 1) + p : s->t[3 * (size_t)p + k];
			if (t) t[3 * (size_t)p + k] = x;
			if (!dry_run) s->t[3 * (size_t)p + k] = x;
		}
	}
	if (edge_inlier) for (int e = 0; e < s->E; e++) edge_inlier[e] = 1;
	if (counts) for (int k = 0; k < CUBA_HIP_POSELOC_STATUSES; k++) counts[k] = c[k];
	std::printf("\n");
	return CUBA_HIP_OK;
}
