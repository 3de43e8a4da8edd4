// fake_cuba_hip_triangulate.cpp -- the stand-in's cuba_hip_triangulate_landmarks, beside fake_cuba_hip.cpp (which holds every other
// cuba_hip_* symbol that ../bundle_adjustment.cpp references) and linked into the same programs.  It prints the call like the others
// -- scalars, then the selection mask as an array or `null` -- and makes up a result in which a value attributed to the wrong landmark
// shows: a selected landmark l is OK (l % 3 == 0), CHI2 (1) or LOW_PARALLAX (2); an OK landmark's position is (100 + l, 200 + l, 300 + l),
// every other one's is what the last cuba_hip_set_graph_begin was given.  Unless it is a dry run, the stand-in's estimates take the OK
// positions, so that a later cuba_hip_get_solution returns them.

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

extern "C" int cuba_hip_triangulate_landmarks(cuba_hip_solver* s, const uint8_t* select, int refine_iterations, double min_parallax_deg,
	const double chi2_max[2], int dry_run, int32_t* status, int64_t counts[CUBA_HIP_TRI_STATUSES], double* xyz)
{
	std::printf("cuba_hip_triangulate_landmarks %d %a %a %a %d", refine_iterations, min_parallax_deg, chi2_max[0], chi2_max[1], dry_run);
	if (!select) std::printf(" | null");
	else
	{
		std::printf(" | %d", s->Lt);
		for (int l = 0; l < s->Lt; l++) std::printf(" %d", (int)select[l]);
	}
	int64_t c[CUBA_HIP_TRI_STATUSES] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	for (int l = 0; l < s->Lt; l++)
	{
		const int st = select && !select[l] ? CUBA_HIP_TRI_NOT_SELECTED : l % 3 == 0 ? CUBA_HIP_TRI_OK : l % 3 == 1 ? CUBA_HIP_TRI_CHI2 : CUBA_HIP_TRI_LOW_PARALLAX;
		c[st]++;
		if (status) status[l] = st;
		for (int k = 0; k < 3; k++)
		{
			const double x = st == CUBA_HIP_TRI_OK ? 100.0 * (k + 1) + l : s->Xw[3 * (size_t)l + k];
			if (xyz) xyz[3 * (size_t)l + k] = x;
			if (!dry_run) s->Xw[3 * (size_t)l + k] = x;
		}
	}
	if (counts) for (int k = 0; k < CUBA_HIP_TRI_STATUSES; k++) counts[k] = c[k];
	std::printf("\n");
	return CUBA_HIP_OK;
}
