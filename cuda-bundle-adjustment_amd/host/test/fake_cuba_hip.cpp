// fake_cuba_hip.cpp -- a recording stand-in for the device library: exactly the cuba_hip_* symbols that
// ../bundle_adjustment.cpp references, with no solver behind them.  Every call prints one line to stdout (the log):
// the function name, its scalar arguments, then every array argument as its length followed by its values (integers
// in decimal, doubles with %a, a null pointer as `null`).  What the host layer reads back is made up so that a value
// attributed to the wrong object shows: see cuba_hip_get_solution, cuba_hip_optimize and the *_chi_squares below.
// Linked with ../bundle_adjustment.cpp and factor_trace.cpp into one program (make factor_trace), never into a library.

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuba_hip.h"

struct cuba_hip_solver
{
	int Pt = 0, Lt = 0, E = 0;
	std::vector<double> q, t, Xw;      // what the last set_graph_begin was given
	int64_t uploads = 0;
	int nFactors[7] = { 0, 0, 0, 0, 0, 0, 0 };      // size of the set last given, per kind
};

namespace
{

// the kinds' codes in the made-up chi2 (the first two are the factor types of cuba_hip_set_pose_factor_robust_kernels)
enum { PRIOR = 0, RELATIVE_POSE = 1, LANDMARK_PRIOR = 2, POSITION = 3, DIRECTION = 4, RANGE = 5, POSE_RANGE = 6 };

void arr(const double* p, size_t n)
{
	if (!p) { std::printf(" | null"); return; }
	std::printf(" | %zu", n);
	for (size_t i = 0; i < n; i++) std::printf(" %a", p[i]);
}
template <class I> void arrInt(const I* p, size_t n)
{
	if (!p) { std::printf(" | null"); return; }
	std::printf(" | %zu", n);
	for (size_t i = 0; i < n; i++) std::printf(" %d", (int)p[i]);
}
int done() { std::printf("\n"); return CUBA_HIP_OK; }

int setFactors(cuba_hip_solver* s, int kind, int n) { s->nFactors[kind] = n; return done(); }

int chiSquares(cuba_hip_solver* s, const char* name, int kind, double* out)
{
	std::printf("%s %d", name, s->nFactors[kind]);
	for (int k = 0; k < s->nFactors[kind]; k++) out[k] = 1000.0 * kind + k + 0.5;
	return done();
}

int optimize(int niterations, double* chi2, int* n_done)
{
	for (int i = 0; i < niterations; i++) chi2[i] = 64.0 / (i + 1);
	*n_done = niterations;
	return CUBA_HIP_OK;
}

}  // namespace

extern "C" {

void* cuba_hip_host_alloc(size_t bytes) { std::printf("cuba_hip_host_alloc %zu\n", bytes); return std::malloc(bytes); }
void cuba_hip_host_free(void* p) { std::printf("cuba_hip_host_free\n"); std::free(p); }

int cuba_hip_create(int device, cuba_hip_solver** out) { std::printf("cuba_hip_create %d", device); *out = new cuba_hip_solver; return done(); }
int cuba_hip_destroy(cuba_hip_solver* s) { std::printf("cuba_hip_destroy"); delete s; return done(); }
const char* cuba_hip_last_error(const cuba_hip_solver*) { return ""; }
int cuba_hip_set_option(cuba_hip_solver*, const char* key, double value) { std::printf("cuba_hip_set_option %s %a", key, value); return done(); }
int cuba_hip_set_robust_kernel(cuba_hip_solver*, int edge_type, int kind, double delta)
{
	std::printf("cuba_hip_set_robust_kernel %d %d %a", edge_type, kind, delta);
	return done();
}
int cuba_hip_hint_unchanged(cuba_hip_solver*, int same_edges, int same_values) { std::printf("cuba_hip_hint_unchanged %d %d", same_edges, same_values); return done(); }

int cuba_hip_get_counter(cuba_hip_solver* s, const char* name, int64_t* value)
{
	*value = std::strcmp(name, "graph_uploads") == 0 ? s->uploads : 0;
	std::printf("cuba_hip_get_counter %s -> %lld", name, (long long)*value);
	return done();
}

int cuba_hip_set_graph_begin(cuba_hip_solver* s, int Pt, int Pf, int Lt, int Lf, const double* q, const double* t, const double* cam, const double* Xw,
	int E, const int32_t* edge_pose, const int32_t* edge_landmark, const uint8_t* edge_dim, const double* meas, const double* omega)
{
	std::printf("cuba_hip_set_graph_begin %d %d %d %d %d", Pt, Pf, Lt, Lf, E);
	arr(q, 4 * (size_t)Pt); arr(t, 3 * (size_t)Pt); arr(cam, 5 * (size_t)Pt); arr(Xw, 3 * (size_t)Lt);
	arrInt(edge_pose, E); arrInt(edge_landmark, E); arrInt(edge_dim, E); arr(meas, 3 * (size_t)E); arr(omega, E);
	s->Pt = Pt; s->Lt = Lt; s->E = E; s->uploads++;
	s->q.assign(q, q + 4 * (size_t)Pt); s->t.assign(t, t + 3 * (size_t)Pt); s->Xw.assign(Xw, Xw + 3 * (size_t)Lt);
	return done();
}
int cuba_hip_build_structure(cuba_hip_solver*) { std::printf("cuba_hip_build_structure"); return done(); }
int cuba_hip_set_graph_end(cuba_hip_solver*) { std::printf("cuba_hip_set_graph_end"); return done(); }

int cuba_hip_set_pose_priors(cuba_hip_solver* s, int n, const int32_t* pose, const double* q, const double* t, const double* info)
{
	std::printf("cuba_hip_set_pose_priors %d", n);
	arrInt(pose, n); arr(q, 4 * (size_t)n); arr(t, 3 * (size_t)n); arr(info, 36 * (size_t)n);
	return setFactors(s, PRIOR, n);
}
int cuba_hip_set_relative_pose_edges(cuba_hip_solver* s, int n, const int32_t* pose_i, const int32_t* pose_j, const double* q, const double* t, const double* info)
{
	std::printf("cuba_hip_set_relative_pose_edges %d", n);
	arrInt(pose_i, n); arrInt(pose_j, n); arr(q, 4 * (size_t)n); arr(t, 3 * (size_t)n); arr(info, 36 * (size_t)n);
	return setFactors(s, RELATIVE_POSE, n);
}
int cuba_hip_set_pose_factor_robust_kernels(cuba_hip_solver*, int factor_type, int n, const int32_t* kind, const double* delta)
{
	std::printf("cuba_hip_set_pose_factor_robust_kernels %d %d", factor_type, n);
	arrInt(kind, n); arr(delta, n);
	return done();
}
int cuba_hip_set_landmark_priors(cuba_hip_solver* s, int n, const int32_t* landmark, const double* xyz, const double* info, const int32_t* kind, const double* delta)
{
	std::printf("cuba_hip_set_landmark_priors %d", n);
	arrInt(landmark, n); arr(xyz, 3 * (size_t)n); arr(info, 9 * (size_t)n); arrInt(kind, n); arr(delta, n);
	return setFactors(s, LANDMARK_PRIOR, n);
}
int cuba_hip_set_position_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* position, const double* lever_arm, const double* info,
	const int32_t* kind, const double* delta)
{
	std::printf("cuba_hip_set_position_factors %d", n);
	arrInt(pose, n); arr(position, 3 * (size_t)n); arr(lever_arm, 3 * (size_t)n); arr(info, 9 * (size_t)n); arrInt(kind, n); arr(delta, n);
	return setFactors(s, POSITION, n);
}
int cuba_hip_set_direction_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* world_dir, const double* measured_dir, const double* info,
	const int32_t* kind, const double* delta)
{
	std::printf("cuba_hip_set_direction_factors %d", n);
	arrInt(pose, n); arr(world_dir, 3 * (size_t)n); arr(measured_dir, 3 * (size_t)n); arr(info, 9 * (size_t)n); arrInt(kind, n); arr(delta, n);
	return setFactors(s, DIRECTION, n);
}
int cuba_hip_set_range_factors(cuba_hip_solver* s, int n, const int32_t* pose, const double* anchor, const double* range, const double* lever_arm, const double* info,
	const int32_t* kind, const double* delta)
{
	std::printf("cuba_hip_set_range_factors %d", n);
	arrInt(pose, n); arr(anchor, 3 * (size_t)n); arr(range, n); arr(lever_arm, 3 * (size_t)n); arr(info, n); arrInt(kind, n); arr(delta, n);
	return setFactors(s, RANGE, n);
}
int cuba_hip_set_pose_range_factors(cuba_hip_solver* s, int n, const int32_t* pose_i, const int32_t* pose_j, const double* range, const double* lever_arm_i,
	const double* lever_arm_j, const double* info, const int32_t* kind, const double* delta)
{
	std::printf("cuba_hip_set_pose_range_factors %d", n);
	arrInt(pose_i, n); arrInt(pose_j, n); arr(range, n); arr(lever_arm_i, 3 * (size_t)n); arr(lever_arm_j, 3 * (size_t)n); arr(info, n); arrInt(kind, n);
	arr(delta, n);
	return setFactors(s, POSE_RANGE, n);
}

int cuba_hip_prior_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_prior_chi_squares", PRIOR, out); }
int cuba_hip_relative_pose_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_relative_pose_chi_squares", RELATIVE_POSE, out); }
int cuba_hip_landmark_prior_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_landmark_prior_chi_squares", LANDMARK_PRIOR, out); }
int cuba_hip_position_factor_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_position_factor_chi_squares", POSITION, out); }
int cuba_hip_direction_factor_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_direction_factor_chi_squares", DIRECTION, out); }
int cuba_hip_range_factor_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_range_factor_chi_squares", RANGE, out); }
int cuba_hip_pose_range_factor_chi_squares(cuba_hip_solver* s, double* out) { return chiSquares(s, "cuba_hip_pose_range_factor_chi_squares", POSE_RANGE, out); }

int cuba_hip_optimize(cuba_hip_solver*, int niterations, double* chi2_per_iter, int* n_done)
{
	std::printf("cuba_hip_optimize %d", niterations);
	optimize(niterations, chi2_per_iter, n_done);
	return done();
}
int cuba_hip_optimize_batch(cuba_hip_solver**, int n, int niterations, double* chi2_per_iter, int* n_done, int* batched_solves)
{
	std::printf("cuba_hip_optimize_batch %d %d", n, niterations);
	for (int i = 0; i < n; i++) optimize(niterations, chi2_per_iter + (size_t)i * (niterations > 1 ? niterations : 1), n_done + i);
	if (batched_solves) *batched_solves = 0;
	return done();
}

int cuba_hip_get_solution(cuba_hip_solver* s, double* q, double* t, double* Xw)
{
	std::printf("cuba_hip_get_solution");
	std::memcpy(q, s->q.data(), s->q.size() * sizeof(double));
	std::memcpy(t, s->t.data(), s->t.size() * sizeof(double));
	std::memcpy(Xw, s->Xw.data(), s->Xw.size() * sizeof(double));
	return done();
}
int cuba_hip_chi_squares_begin(cuba_hip_solver* s, double* chi2_per_edge)
{
	std::printf("cuba_hip_chi_squares_begin %d", s->E);
	for (int k = 0; k < s->E; k++) chi2_per_edge[k] = k + 0.25;
	return done();
}
int cuba_hip_chi_squares_end(cuba_hip_solver*) { std::printf("cuba_hip_chi_squares_end"); return done(); }
int cuba_hip_get_profile(cuba_hip_solver*, double seconds[CUBA_HIP_PROFILE_ITEMS])
{
	std::printf("cuba_hip_get_profile");
	for (int i = 0; i < CUBA_HIP_PROFILE_ITEMS; i++) seconds[i] = 0.0;
	return done();
}

int cuba_hip_compute_covariance(cuba_hip_solver*, double*, double*, int* not_positive_definite)
{
	std::printf("cuba_hip_compute_covariance");
	*not_positive_definite = 0;
	return done();
}
int cuba_hip_compute_covariance_pairs(cuba_hip_solver*, int n, const int32_t* kind_a, const int32_t* index_a, const int32_t* kind_b, const int32_t* index_b, double*,
	int* not_positive_definite)
{
	std::printf("cuba_hip_compute_covariance_pairs %d", n);
	arrInt(kind_a, n); arrInt(index_a, n); arrInt(kind_b, n); arrInt(index_b, n);
	*not_positive_definite = 0;
	return done();
}

// edge gating: the stand-in classifies nothing -- every edge is active, its ungated chi2 is its index
int cuba_hip_gate_edges(cuba_hip_solver* s, const double chi2_max[2], int require_positive_depth, int mode, int64_t counts[6], double* chi2_per_edge)
{
	std::printf("cuba_hip_gate_edges %a %a %d %d", chi2_max[0], chi2_max[1], require_positive_depth, mode);
	if (counts) for (int k = 0; k < 6; k++) counts[k] = k == 1 ? s->E : 0;
	if (chi2_per_edge) for (int k = 0; k < s->E; k++) chi2_per_edge[k] = k;
	return done();
}
int cuba_hip_set_edge_active(cuba_hip_solver* s, const uint8_t* active)
{
	int off = 0;
	for (int k = 0; active && k < s->E; k++) off += active[k] == 0;
	std::printf("cuba_hip_set_edge_active %s %d", active ? "mask" : "null", off);
	return done();
}
int cuba_hip_get_edge_active(cuba_hip_solver* s, uint8_t* active)
{
	std::printf("cuba_hip_get_edge_active");
	for (int k = 0; k < s->E; k++) active[k] = 1;
	return done();
}
int cuba_hip_landmark_active_edges(cuba_hip_solver*, int32_t*) { std::printf("cuba_hip_landmark_active_edges"); return done(); }

}  // extern "C"
