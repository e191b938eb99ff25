// comoving_plan.hpp -- the host's rules for the comoving radiation field (mcrat_hip_comoving_field, mcrat_hip_pool_comoving_field,
// mcrat_hip_comoving_field_bins): the argument checks and their texts, the layout of the block on the device, the rule that picks the accumulation
// path, the grid size, and the per-photon functions -- the lab cosine m, the fluid-frame cosine a, the bin -- written once here and used by the
// kernel (comoving.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them
// (tests/test_comoving_plan_cpu.py).  r_mu, the shell bin, the edge search, the edge check and the path rule are radfield_plan.hpp's and
// observe_plan.hpp's.
//
// Definitions.  A slot counts when observe_observable says so.  For a counted photon, in exactly this order, in IEEE double with
// correctly rounded `/` and sqrt and without contraction:
//     r, mu   radfield_r_mu;   cell, beta[3], g   as the radiation field obtains them (cell < 0: n_unlocated += 1, no bin)
//     bp    = (beta0*p1 + beta1*p2) + beta2*p3
//     e_lab = p0 * C_LIGHT
//     e     = (g * (p0 - bp)) * C_LIGHT                        the energy in the fluid frame [erg]
//     m     = ((p1*r0 + p2*r1) + p3*r2) / (p0 * r)             the lab cosine between the photon's direction and the radial direction
//     b2    = (beta0*beta0 + beta1*beta1) + beta2*beta2
//     a     = b2 > 0 ? ((bp / b) - b * p0) / (p0 - bp), b = sqrt(b2) : m
//             the cosine, in the fluid frame, between the photon's direction and the flow: (p' . beta_hat) / p'0 in closed form (the Lorentz factor
//             cancels).  A cell at rest has no flow direction and its frame is the lab: the radial cosine.
//     a, m clamped into [-1, 1]; a NaN stays a NaN
//     s = cell (CELLS) or ir * n_mu + imu (SHELLS, radfield_shell_bin);  ie = observe_find_bin(e_edges, n_e, e);  ia = observe_find_bin(a_edges, n_a, a)
//     bin = (s * n_e + ie) * n_a + ia;  a located photon outside any axis, or with a coordinate that is not a number: n_outside += 1, no bin
//     terms:  w,  we = w*e,  (we)*a,  ((we)*a)*a,  wl = w*e_lab,  (wl)*m,  ((wl)*m)*m
// Counts that do not hang on e or a are exact; the seven sums are added with floating-point atomics in whatever order the hardware serves them, each
// within (m + 2) * 2^-53 * sum|term| of the exact sum of the bin's m terms as the device computed them.
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "device_types.hpp"
#include "observe_plan.hpp"
#include "radfield_plan.hpp"

namespace mcrat {

// ------------------------------------------------------------------ refusals and their texts
enum ComovingMode { COMOVING_CELLS = 0, COMOVING_SHELLS = 1 };          // MCRAT_HIP_COMOVING_CELLS, MCRAT_HIP_COMOVING_SHELLS
enum ComovingRefusal {
    COMOVING_OK = 0,
    COMOVING_BAD_MODE,                // neither CELLS nor SHELLS
    COMOVING_NULL_EDGES,              // no e_edges or a_edges; SHELLS without r_edges or mu_edges
    COMOVING_NO_BINS,                 // n_e or n_a < 1; SHELLS with n_r or n_mu < 1
    COMOVING_TOO_MANY_BINS,           // n_s * n_e * n_a does not fit an int (CELLS: once the frame is known, comoving_layout)
    COMOVING_R_EDGES_NOT_FINITE,
    COMOVING_MU_EDGES_NOT_FINITE,
    COMOVING_E_EDGES_NOT_FINITE,
    COMOVING_A_EDGES_NOT_FINITE,
    COMOVING_R_EDGES_NOT_ASCENDING,
    COMOVING_MU_EDGES_NOT_ASCENDING,
    COMOVING_E_EDGES_NOT_ASCENDING,
    COMOVING_A_EDGES_NOT_ASCENDING,
    COMOVING_STAGING_TOO_LARGE,       // the edges do not fit the LDS budget
    COMOVING_BAD_PATH_SWITCH,         // MCRAT_HIP_COMOVING_PATH is neither lds nor global
    COMOVING_LDS_FORCED_ON_CELLS,     // MCRAT_HIP_COMOVING_PATH=lds with CELLS, which is always global
    COMOVING_LDS_FORCED_TOO_LARGE,    // MCRAT_HIP_COMOVING_PATH=lds with planes beyond the LDS budget
    COMOVING_HYDRO_MISMATCH           // a hydro context with other switches or on another device (the engine's check, its text here)
};
inline const char *comoving_refusal_text(ComovingRefusal why)
{
    switch (why) {
    case COMOVING_OK: return "";
    case COMOVING_BAD_MODE: return "comoving_field: mode must be MCRAT_HIP_COMOVING_CELLS or MCRAT_HIP_COMOVING_SHELLS";
    case COMOVING_NULL_EDGES: return "comoving_field: e_edges and a_edges are needed, and SHELLS needs r_edges and mu_edges";
    case COMOVING_NO_BINS: return "comoving_field: n_e and n_a, and with SHELLS n_r and n_mu, must each be at least 1";
    case COMOVING_TOO_MANY_BINS: return "comoving_field: the number of position bins * n_e * n_a overflows an int";
    case COMOVING_R_EDGES_NOT_FINITE: return "comoving_field: r_edges holds a value that is not finite";
    case COMOVING_MU_EDGES_NOT_FINITE: return "comoving_field: mu_edges holds a value that is not finite";
    case COMOVING_E_EDGES_NOT_FINITE: return "comoving_field: e_edges holds a value that is not finite";
    case COMOVING_A_EDGES_NOT_FINITE: return "comoving_field: a_edges holds a value that is not finite";
    case COMOVING_R_EDGES_NOT_ASCENDING: return "comoving_field: r_edges is not strictly ascending";
    case COMOVING_MU_EDGES_NOT_ASCENDING: return "comoving_field: mu_edges is not strictly ascending";
    case COMOVING_E_EDGES_NOT_ASCENDING: return "comoving_field: e_edges is not strictly ascending";
    case COMOVING_A_EDGES_NOT_ASCENDING: return "comoving_field: a_edges is not strictly ascending";
    case COMOVING_STAGING_TOO_LARGE: return "comoving_field: the edges do not fit the kernel's LDS budget";
    case COMOVING_BAD_PATH_SWITCH: return "comoving_field: MCRAT_HIP_COMOVING_PATH must be lds or global";
    case COMOVING_LDS_FORCED_ON_CELLS: return "comoving_field: MCRAT_HIP_COMOVING_PATH=lds, but CELLS always accumulates in global memory";
    case COMOVING_LDS_FORCED_TOO_LARGE: return "comoving_field: MCRAT_HIP_COMOVING_PATH=lds, but the planes do not fit the kernel's LDS budget";
    case COMOVING_HYDRO_MISMATCH: return "comoving_field: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY) or on another device";
    }
    return "";
}

// ------------------------------------------------------------------ the block and where it is accumulated
// One block: the radiation field's head of eight 8-byte words -- n_observable, n_unlocated, n_outside, five spare -- padded to 256 B, then the
// accumulator: eight planes of n_bins 8-byte words, plane-major, which are the planes the caller receives (no transposition); head and accumulator
// are zeroed by one memset.  Then the kernel's inputs in the order it stages them into LDS: r_edges [n_r + 1], mu_edges [n_mu + 1] (SHELLS),
// e_edges [n_e + 1], a_edges [n_a + 1].
constexpr int COMOVING_PLANES = 8;
enum ComovingPlane { CF_COUNT = 0, CF_W, CF_WE, CF_WEA, CF_WEAA, CF_WE_LAB, CF_WEM, CF_WEMM };
constexpr int COMOVING_SUMS = COMOVING_PLANES - 1;
constexpr int COMOVING_N_SCALARS = RADFIELD_N_SCALARS;       // the head's words are the radiation field's (RF_N_OBSERVABLE, RF_N_UNLOCATED, RF_N_OUTSIDE)
constexpr size_t COMOVING_ACC_OFFSET = RADFIELD_ACC_OFFSET;
constexpr int COMOVING_BLOCK = OBSERVE_BLOCK;                // threads per workgroup: one lane per slot and trip
constexpr size_t COMOVING_MATCH_BYTES = OBSERVE_MATCH_BYTES; // global path: the wavefronts' match tables (observe_plan.hpp)

// what the arguments alone decide (no frame needed): the axes, what is staged, the path
struct ComovingShape {
    int mode, n_r, n_mu, n_e, n_a;       // CELLS: n_r = n_mu = 0
    int n_shells;                        // n_r * n_mu
    int n_shell_bins;                    // n_r * n_mu * n_e * n_a (SHELLS)
    size_t staged_doubles;               // the edges
    size_t staged_bytes;                 // ... and, in LDS, the workgroup's three counters behind them
    ObservePath path;
};
struct ComovingPlan {
    ComovingShape s;
    int n_s;                             // position bins -- CELLS: the frame's cells; SHELLS: n_r * n_mu
    int n_bins;                          // n_s * n_e * n_a
    size_t acc_bytes;                    // the eight planes
    size_t zeroed_bytes;                 // head and accumulator
    size_t planes_offset;                // the planes the caller receives: the accumulator itself
    size_t staged_offset;                // the edges
    size_t total_bytes;
    size_t lds_bytes;                    // the kernel's dynamic LDS on the chosen path
    int groups_per_cu;
};

// MCRAT_HIP_COMOVING_PATH: unset or empty -- the rule decides (OBSERVE_PATH_NONE); lds, global -- that path; anything else is refused
inline ComovingRefusal comoving_path_switch(const char *env, ObservePath *forced)
{
    *forced = OBSERVE_PATH_NONE;
    if (!env || !*env) return COMOVING_OK;
    if (!strcmp(env, "lds")) *forced = OBSERVE_PATH_LDS;
    else if (!strcmp(env, "global")) *forced = OBSERVE_PATH_GLOBAL;
    else return COMOVING_BAD_PATH_SWITCH;
    return COMOVING_OK;
}

// The checks, in this order: the mode; the edge arrays (e, a; SHELLS: r, mu too); the counts; SHELLS: their product; r, mu, e, a edges finite; r, mu,
// e, a edges ascending; what must fit LDS; then the switch `env` (MCRAT_HIP_COMOVING_PATH) -- its spelling, lds with CELLS, lds with planes beyond
// the budget.  The path: LDS when the staged edges, the counters and the eight planes fit OBSERVE_LDS_BUDGET, global otherwise, unless the switch
// says which; CELLS is always global (its product is checked by comoving_layout, once the frame is known).  *shape is filled when COMOVING_OK.
inline ComovingRefusal comoving_check(int mode, int n_r, const double *r_edges, int n_mu, const double *mu_edges, int n_e, const double *e_edges, int n_a,
                                      const double *a_edges, const char *env, ComovingShape *shape)
{
    if (mode != COMOVING_CELLS && mode != COMOVING_SHELLS) return COMOVING_BAD_MODE;
    const bool shells = mode == COMOVING_SHELLS;
    ComovingShape s{};
    s.mode = mode;
    if (!e_edges || !a_edges || (shells && (!r_edges || !mu_edges))) return COMOVING_NULL_EDGES;
    if (n_e < 1 || n_a < 1 || (shells && (n_r < 1 || n_mu < 1))) return COMOVING_NO_BINS;
    const long long per_s = (long long)n_e * (long long)n_a;
    if (per_s > INT_MAX) return COMOVING_TOO_MANY_BINS;
    long long shell_bins = 0;
    if (shells) {
        const long long ns = (long long)n_r * (long long)n_mu;
        if (ns > INT_MAX || ns * per_s > INT_MAX) return COMOVING_TOO_MANY_BINS;
        shell_bins = ns * per_s;
        s.n_r = n_r; s.n_mu = n_mu; s.n_shells = (int)ns; s.n_shell_bins = (int)shell_bins;
    }
    const EdgesFault bad[4] = {shells ? edges_check(r_edges, n_r) : EDGES_OK, shells ? edges_check(mu_edges, n_mu) : EDGES_OK, edges_check(e_edges, n_e),
                               edges_check(a_edges, n_a)};          // (all four finite before any ascending)
    for (int k = 0; k < 4; ++k)
        if (bad[k] == EDGES_NOT_FINITE) return (ComovingRefusal)(COMOVING_R_EDGES_NOT_FINITE + k);
    for (int k = 0; k < 4; ++k)
        if (bad[k] == EDGES_NOT_ASCENDING) return (ComovingRefusal)(COMOVING_R_EDGES_NOT_ASCENDING + k);
    s.n_e = n_e; s.n_a = n_a;
    s.staged_doubles = (shells ? (size_t)n_r + 1 + (size_t)n_mu + 1 : 0) + (size_t)n_e + 1 + (size_t)n_a + 1;
    s.staged_bytes = 8 * s.staged_doubles + 8 * (size_t)COMOVING_N_SCALARS;
    if (s.staged_bytes > OBSERVE_LDS_BUDGET) return COMOVING_STAGING_TOO_LARGE;
    ObservePath forced;
    const ComovingRefusal why = comoving_path_switch(env, &forced);
    if (why != COMOVING_OK) return why;
    if (forced == OBSERVE_PATH_LDS && !shells) return COMOVING_LDS_FORCED_ON_CELLS;
    s.path = OBSERVE_PATH_GLOBAL;
    if (shells) {
        const AccumulateRule r = accumulate_rule(s.staged_bytes, (size_t)COMOVING_PLANES * 8 * (size_t)shell_bins, COMOVING_MATCH_BYTES, forced);
        if (forced == OBSERVE_PATH_LDS && !r.fits) return COMOVING_LDS_FORCED_TOO_LARGE;
        s.path = r.path;
    }
    *shape = s;
    return COMOVING_OK;
}

// the block of a checked shape on a frame of n_cells cells (>= 1); CELLS: n_cells * n_e * n_a beyond an int is refused here
inline ComovingRefusal comoving_layout(const ComovingShape &s, int n_cells, ComovingPlan *plan)
{
    ComovingPlan p{};
    p.s = s;
    p.n_s = s.mode == COMOVING_CELLS ? n_cells : s.n_shells;
    const long long bins = (long long)p.n_s * ((long long)s.n_e * (long long)s.n_a);      // (n_e * n_a fits an int: comoving_check)
    if (bins > INT_MAX) return COMOVING_TOO_MANY_BINS;
    p.n_bins = (int)bins;
    p.acc_bytes = (size_t)COMOVING_PLANES * 8 * (size_t)p.n_bins;
    p.zeroed_bytes = COMOVING_ACC_OFFSET + p.acc_bytes;
    p.planes_offset = COMOVING_ACC_OFFSET;
    p.staged_offset = (p.zeroed_bytes + 255) / 256 * 256;
    p.total_bytes = p.staged_offset + 8 * s.staged_doubles;
    const AccumulateRule r = accumulate_rule(s.staged_bytes, p.acc_bytes, COMOVING_MATCH_BYTES, s.path);       // (the path is decided: the LDS and the workgroups that go with it)
    p.lds_bytes = r.lds_bytes; p.groups_per_cu = r.groups_per_cu;
    *plan = p;
    return COMOVING_OK;
}

// workgroups of COMOVING_BLOCK lanes: a grid-stride loop, at most what the plan wants resident per CU
inline int comoving_grid(const ComovingPlan &p, int n_slots, int cus)
{
    return accumulate_grid(n_slots, COMOVING_BLOCK, cus, p.groups_per_cu);
}

// ------------------------------------------------------------------ one photon (host and device)
// into [-1, 1]; a NaN stays a NaN
MCRAT_RF_HD inline double comoving_clamp(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }
// the lab cosine between the photon's direction and the radial direction (r: radfield_r_mu's)
MCRAT_RF_HD inline double comoving_m(double r0, double r1, double r2, double p0, double p1, double p2, double p3, double r)
{
    return comoving_clamp(((p1 * r0 + p2 * r1) + p3 * r2) / (p0 * r));
}
MCRAT_RF_HD inline double comoving_bp(const double beta[3], double p1, double p2, double p3) { return (beta[0] * p1 + beta[1] * p2) + beta[2] * p3; }
MCRAT_RF_HD inline double comoving_e(double g, double p0, double bp) { return (g * (p0 - bp)) * C_LIGHT; }
// the fluid-frame cosine between the photon's direction and the flow; m (clamped) for a cell at rest
MCRAT_RF_HD inline double comoving_a(const double beta[3], double bp, double p0, double m)
{
    const double b2 = (beta[0] * beta[0] + beta[1] * beta[1]) + beta[2] * beta[2];
    if (!(b2 > 0)) return m;
    const double b = sqrt(b2);
    return comoving_clamp(((bp / b) - b * p0) / (p0 - bp));
}
// the bin of position bin s (cell or shell; -1: none), fluid-frame energy e and cosine a, or -1 when any lies outside (or is not a number)
MCRAT_RF_HD inline int comoving_bin(int s, const double *e_edges, int n_e, const double *a_edges, int n_a, double e, double a)
{
    if (s < 0) return -1;
    const int ie = observe_find_bin(e_edges, n_e, e), ia = observe_find_bin(a_edges, n_a, a);
    return (ie < 0 || ia < 0) ? -1 : (s * n_e + ie) * n_a + ia;
}
// the seven terms of a photon in plane order behind the count
MCRAT_RF_HD inline void comoving_terms(double w, double e, double a, double e_lab, double m, double v[COMOVING_SUMS])
{
    v[0] = w;
    v[1] = w * e; v[2] = v[1] * a; v[3] = v[2] * a;
    v[4] = w * e_lab; v[5] = v[4] * m; v[6] = v[5] * m;
}

}  // namespace mcrat
