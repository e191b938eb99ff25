// radfield_plan.hpp -- the host's rules for the radiation field on the hydro mesh (mcrat_hip_radiation_field, mcrat_hip_pool_radiation_field,
// mcrat_hip_radiation_field_bins): the argument checks and their texts, the layout of the block on the device, the rule that picks the
// accumulation path, the grid size, and the per-photon functions -- r_mu, the shell bin -- written once here and used by the kernel
// (radfield.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them (tests/test_radfield_plan_cpu.py).
//
// Definitions.  A slot counts when observe_observable says so (observe_plan.hpp).  For a counted photon, in exactly this order,
// in IEEE double with correctly rounded `/` and sqrt and without contraction:
//     r = sqrt((r0*r0 + r1*r1) + r2*r2);   mu = r2 / r
//     (a0, a1, a2) = the loop's hydro coordinates of (r0, r1, r2)
//     cell = -1 when (a0, a1, a2) fails the loop's strict domain test, else the lowest-index cell whose closed extent holds the point
//            cell < 0: n_unlocated += 1, no bin
//     beta = that cell's velocity at the azimuth of (r0, r1), as a re-location takes it
//     e_lab = p0 * C_LIGHT;   e_comv = (the time component of p boosted by beta with the cell's staged gam, kf) * C_LIGHT
//     terms:  w,  w*e_lab,  w*e_comv,  w*num_scatt,  w*temp[cell]
// CELLS: bin = cell, n_bins = the frame's cells.  SHELLS: bin = ir * n_mu + imu, ir = observe_find_bin(r_edges, n_r, r), imu =
// observe_find_bin(mu_edges, n_mu, mu); a located photon outside either range adds to n_outside and to no bin.  Counts are exact; the five sums are
// added with floating-point atomics in whatever order the hardware serves them, each within (m + 2) * 2^-53 * sum|term| of the exact sum of the
// bin's m terms as the device computed them.
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "device_types.hpp"
#include "observe_plan.hpp"

#if defined(__HIPCC__)
#define MCRAT_RF_HD __host__ __device__
#else
#define MCRAT_RF_HD
#endif

// The accumulator's layout on the global path, a build-time switch: 0 plane-major, six planes of n_bins like the observation cube (what the caller
// receives: no transposition); 1 bin-major, one 64-B record per bin -- count, W, WE_lab, WE_comv, WNS, WT, two spare words -- so that a photon's six
// adds land in one segment, transposed into planes on the way out.  Measured on the benchmark's cfg2 frame (tools/radfield_bench.py, DESIGN.md
// section 6, profiles/radfield_bench.txt).
#ifndef MCRAT_RADFIELD_BIN_MAJOR
#define MCRAT_RADFIELD_BIN_MAJOR 0
#endif

namespace mcrat {

// ------------------------------------------------------------------ refusals and their texts
enum RadfieldMode { RADFIELD_CELLS = 0, RADFIELD_SHELLS = 1 };          // MCRAT_HIP_RADFIELD_CELLS, MCRAT_HIP_RADFIELD_SHELLS
enum RadfieldRefusal {
    RADFIELD_OK = 0,
    RADFIELD_BAD_MODE,                // neither CELLS nor SHELLS
    RADFIELD_NULL_EDGES,              // SHELLS without r_edges or mu_edges
    RADFIELD_NO_BINS,                 // SHELLS with n_r or n_mu < 1
    RADFIELD_TOO_MANY_BINS,           // n_r * n_mu does not fit an int
    RADFIELD_R_EDGES_NOT_FINITE,
    RADFIELD_MU_EDGES_NOT_FINITE,
    RADFIELD_R_EDGES_NOT_ASCENDING,
    RADFIELD_MU_EDGES_NOT_ASCENDING,
    RADFIELD_STAGING_TOO_LARGE,       // the edges do not fit the LDS budget
    RADFIELD_BAD_PATH_SWITCH,         // MCRAT_HIP_RADFIELD_PATH is neither lds nor global
    RADFIELD_LDS_FORCED_ON_CELLS,     // MCRAT_HIP_RADFIELD_PATH=lds with CELLS, which is always global
    RADFIELD_LDS_FORCED_TOO_LARGE,    // MCRAT_HIP_RADFIELD_PATH=lds with planes beyond the LDS budget
    RADFIELD_HYDRO_MISMATCH           // a hydro context with other switches or on another device (the engine's check, its text here)
};
inline const char *radfield_refusal_text(RadfieldRefusal why)
{
    switch (why) {
    case RADFIELD_OK: return "";
    case RADFIELD_BAD_MODE: return "radiation_field: mode must be MCRAT_HIP_RADFIELD_CELLS or MCRAT_HIP_RADFIELD_SHELLS";
    case RADFIELD_NULL_EDGES: return "radiation_field: SHELLS needs r_edges and mu_edges";
    case RADFIELD_NO_BINS: return "radiation_field: n_r and n_mu must each be at least 1";
    case RADFIELD_TOO_MANY_BINS: return "radiation_field: n_r * n_mu overflows an int";
    case RADFIELD_R_EDGES_NOT_FINITE: return "radiation_field: r_edges holds a value that is not finite";
    case RADFIELD_MU_EDGES_NOT_FINITE: return "radiation_field: mu_edges holds a value that is not finite";
    case RADFIELD_R_EDGES_NOT_ASCENDING: return "radiation_field: r_edges is not strictly ascending";
    case RADFIELD_MU_EDGES_NOT_ASCENDING: return "radiation_field: mu_edges is not strictly ascending";
    case RADFIELD_STAGING_TOO_LARGE: return "radiation_field: the edges do not fit the kernel's LDS budget";
    case RADFIELD_BAD_PATH_SWITCH: return "radiation_field: MCRAT_HIP_RADFIELD_PATH must be lds or global";
    case RADFIELD_LDS_FORCED_ON_CELLS: return "radiation_field: MCRAT_HIP_RADFIELD_PATH=lds, but CELLS always accumulates in global memory";
    case RADFIELD_LDS_FORCED_TOO_LARGE: return "radiation_field: MCRAT_HIP_RADFIELD_PATH=lds, but the planes do not fit the kernel's LDS budget";
    case RADFIELD_HYDRO_MISMATCH: return "radiation_field: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY) or on another device";
    }
    return "";
}

// ------------------------------------------------------------------ the block and where it is accumulated
// One block: a head of eight 8-byte words -- n_observable, n_unlocated, n_outside, five spare -- padded to 256 B, then the accumulator: six planes
// of n_bins 8-byte words (plane-major) or n_bins records of eight (bin-major); head and accumulator are zeroed by one memset.  A bin-major build
// has the six planes the caller receives behind it, written by the transposition.  Then the kernel's inputs in the order it stages them into LDS:
// r_edges [n_r + 1], mu_edges [n_mu + 1] (SHELLS).
constexpr int RADFIELD_PLANES = 6;
enum RadfieldPlane { RF_COUNT = 0, RF_W, RF_WE_LAB, RF_WE_COMV, RF_WNS, RF_WT };
constexpr int RADFIELD_RECORD_WORDS = 8;         // bin-major: one 64-B record per bin
constexpr int RADFIELD_HEAD_WORDS = 8;
enum RadfieldHeadWord { RF_N_OBSERVABLE = 0, RF_N_UNLOCATED, RF_N_OUTSIDE };
constexpr int RADFIELD_N_SCALARS = 3;
constexpr size_t RADFIELD_ACC_OFFSET = 256;
constexpr bool RADFIELD_BIN_MAJOR = MCRAT_RADFIELD_BIN_MAJOR != 0;
constexpr int RADFIELD_BLOCK = OBSERVE_BLOCK;    // threads per workgroup: one lane per slot and trip
// Workgroups per CU the grid is sized for (accumulate_rule, observe_plan.hpp): two on the LDS path, as for the observation cube (every workgroup
// flushes into the same bins); eight -- 32 wavefronts -- on the global path, which is bound by the latency of the cell look-up's gathers and wants
// them in flight.
constexpr int RADFIELD_MAX_GROUPS_PER_CU = OBSERVE_MAX_GROUPS_PER_CU;
// global path: the wavefronts' match tables (observe_plan.hpp)
constexpr size_t RADFIELD_MATCH_BYTES = OBSERVE_MATCH_BYTES;

// word `plane` of bin `bin` in an accumulator of n_bins bins
MCRAT_RF_HD inline size_t radfield_word(bool bin_major, int plane, size_t bin, size_t n_bins)
{
    return bin_major ? bin * (size_t)RADFIELD_RECORD_WORDS + (size_t)plane : (size_t)plane * n_bins + bin;
}

// what the arguments alone decide (no frame needed): the shells, what is staged, the path
struct RadfieldShape {
    int mode, n_r, n_mu;                 // CELLS: n_r = n_mu = 0
    int n_shell_bins;                    // n_r * n_mu
    size_t staged_doubles;               // the edges
    size_t staged_bytes;                 // ... and, in LDS, the workgroup's three counters behind them
    ObservePath path;
};
struct RadfieldPlan {
    RadfieldShape s;
    int n_bins;                          // CELLS: the frame's cells; SHELLS: n_r * n_mu
    bool bin_major;                      // the accumulator's layout in global memory (the LDS copy is always plane-major)
    size_t acc_bytes;                    // the accumulator
    size_t zeroed_bytes;                 // head and accumulator
    size_t planes_offset;                // the six planes the caller receives: the accumulator itself, or the transposition's output
    size_t staged_offset;                // the edges
    size_t total_bytes;
    size_t lds_bytes;                    // the kernel's dynamic LDS on the chosen path
    int groups_per_cu;
};

// MCRAT_HIP_RADFIELD_PATH: unset or empty -- the rule decides (OBSERVE_PATH_NONE); lds, global -- that path; anything else is refused
inline RadfieldRefusal radfield_path_switch(const char *env, ObservePath *forced)
{
    *forced = OBSERVE_PATH_NONE;
    if (!env || !*env) return RADFIELD_OK;
    if (!strcmp(env, "lds")) *forced = OBSERVE_PATH_LDS;
    else if (!strcmp(env, "global")) *forced = OBSERVE_PATH_GLOBAL;
    else return RADFIELD_BAD_PATH_SWITCH;
    return RADFIELD_OK;
}

// The checks, in this order: the mode; SHELLS: the edge arrays, the counts, their product, r_edges finite, mu_edges finite, r_edges ascending,
// mu_edges ascending, what must fit LDS; then the switch `env` (MCRAT_HIP_RADFIELD_PATH) -- its spelling, lds with CELLS, lds with planes beyond
// the budget.  The path: LDS when the staged edges, the counters and the six planes fit OBSERVE_LDS_BUDGET, global otherwise, unless the switch says
// which; CELLS is always global.  *shape is filled when RADFIELD_OK.
inline RadfieldRefusal radfield_check(int mode, int n_r, const double *r_edges, int n_mu, const double *mu_edges, const char *env, RadfieldShape *shape)
{
    if (mode != RADFIELD_CELLS && mode != RADFIELD_SHELLS) return RADFIELD_BAD_MODE;
    RadfieldShape s{};
    s.mode = mode;
    if (mode == RADFIELD_SHELLS) {
        if (!r_edges || !mu_edges) return RADFIELD_NULL_EDGES;
        if (n_r < 1 || n_mu < 1) return RADFIELD_NO_BINS;
        const long long bins = (long long)n_r * (long long)n_mu;
        if (bins > INT_MAX) return RADFIELD_TOO_MANY_BINS;
        const EdgesFault bad_r = edges_check(r_edges, n_r), bad_mu = edges_check(mu_edges, n_mu);      // (both finite before either ascending)
        if (bad_r == EDGES_NOT_FINITE) return RADFIELD_R_EDGES_NOT_FINITE;
        if (bad_mu == EDGES_NOT_FINITE) return RADFIELD_MU_EDGES_NOT_FINITE;
        if (bad_r == EDGES_NOT_ASCENDING) return RADFIELD_R_EDGES_NOT_ASCENDING;
        if (bad_mu == EDGES_NOT_ASCENDING) return RADFIELD_MU_EDGES_NOT_ASCENDING;
        s.n_r = n_r; s.n_mu = n_mu; s.n_shell_bins = (int)bins;
        s.staged_doubles = (size_t)n_r + 1 + (size_t)n_mu + 1;
    }
    s.staged_bytes = 8 * s.staged_doubles + 8 * (size_t)RADFIELD_N_SCALARS;
    if (s.staged_bytes > OBSERVE_LDS_BUDGET) return RADFIELD_STAGING_TOO_LARGE;
    ObservePath forced;
    const RadfieldRefusal why = radfield_path_switch(env, &forced);
    if (why != RADFIELD_OK) return why;
    if (forced == OBSERVE_PATH_LDS && mode == RADFIELD_CELLS) return RADFIELD_LDS_FORCED_ON_CELLS;
    s.path = OBSERVE_PATH_GLOBAL;
    if (mode == RADFIELD_SHELLS) {
        const AccumulateRule r = accumulate_rule(s.staged_bytes, (size_t)RADFIELD_PLANES * 8 * (size_t)s.n_shell_bins, RADFIELD_MATCH_BYTES, forced);
        if (forced == OBSERVE_PATH_LDS && !r.fits) return RADFIELD_LDS_FORCED_TOO_LARGE;
        s.path = r.path;
    }
    *shape = s;
    return RADFIELD_OK;
}

// the block of a checked shape on a frame of n_cells cells (>= 1)
inline RadfieldPlan radfield_layout(const RadfieldShape &s, int n_cells, bool bin_major = RADFIELD_BIN_MAJOR)
{
    RadfieldPlan p{};
    p.s = s;
    p.n_bins = s.mode == RADFIELD_CELLS ? n_cells : s.n_shell_bins;
    p.bin_major = bin_major;
    const size_t planes = (size_t)RADFIELD_PLANES * 8 * (size_t)p.n_bins;
    p.acc_bytes = bin_major ? (size_t)RADFIELD_RECORD_WORDS * 8 * (size_t)p.n_bins : planes;
    p.zeroed_bytes = RADFIELD_ACC_OFFSET + p.acc_bytes;
    p.planes_offset = bin_major ? (p.zeroed_bytes + 255) / 256 * 256 : RADFIELD_ACC_OFFSET;
    p.staged_offset = ((bin_major ? p.planes_offset + planes : p.zeroed_bytes) + 255) / 256 * 256;
    p.total_bytes = p.staged_offset + 8 * s.staged_doubles;
    const AccumulateRule r = accumulate_rule(s.staged_bytes, planes, RADFIELD_MATCH_BYTES, s.path);       // (the path is decided: the LDS and the workgroups that go with it)
    p.lds_bytes = r.lds_bytes; p.groups_per_cu = r.groups_per_cu;
    return p;
}

// workgroups of RADFIELD_BLOCK lanes: a grid-stride loop, at most what the plan wants resident per CU
inline int radfield_grid(const RadfieldPlan &p, int n_slots, int cus)
{
    return accumulate_grid(n_slots, RADFIELD_BLOCK, cus, p.groups_per_cu);
}

// ------------------------------------------------------------------ one photon (host and device)
MCRAT_RF_HD inline void radfield_r_mu(double r0, double r1, double r2, double &r, double &mu)
{
    r = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
    mu = r2 / r;
}
// SHELLS: the bin of (r, mu), or -1 when either lies outside its range (or is not a number)
MCRAT_RF_HD inline int radfield_shell_bin(const double *r_edges, int n_r, const double *mu_edges, int n_mu, double r, double mu)
{
    const int ir = observe_find_bin(r_edges, n_r, r), imu = observe_find_bin(mu_edges, n_mu, mu);
    return (ir < 0 || imu < 0) ? -1 : ir * n_mu + imu;
}
MCRAT_RF_HD inline double radfield_e_lab(double p0) { return p0 * C_LIGHT; }

}  // namespace mcrat
