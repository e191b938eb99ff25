// sky_plan.hpp -- the host's rules for a mock observation from any direction on the sky, with images (mcrat_hip_observe_sky,
// mcrat_hip_pool_observe_sky): the argument checks and their texts, the layout of the block on the device, the rule that picks the accumulation
// path, the largest grid, the hash of the global path's match table, and the per-photon functions -- accepted, t_det, xy, bin -- written once here
// and used by the kernel (sky.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them
// (tests/test_sky_plan_cpu.py).
//
// Definitions.  A slot counts when observe_observable says so (observe_plan.hpp).  Observer o has a unit vector n towards
// the observer, an acceptance cosine cos_acc and, with image axes, two unit vectors ex, ey that span the sky plane.  In exactly this order, in IEEE
// double with a correctly rounded `/` and without contraction:
//     accepted:  ((p1 * n0 + p2 * n1) + p3 * n2) >= p0 * cos_acc          (cones may overlap; a photon counts for every observer that accepts it)
//     e = observe_energy(p0)
//     t_det = time_now - (((r0 * n0 + r1 * n1) + r2 * n2) / C_LIGHT)
//     X = (r0 * ex0 + r1 * ex1) + r2 * ex2;   Y = (r0 * ey0 + r1 * ey1) + r2 * ey2        [cm]
// Bin k of an axis holds  edges[k] <= x < edges[k + 1]  (observe_find_bin).  The axes are time, energy and, optionally, X and Y; the cube is
// [n_obs][n_t][n_e][n_y][n_x], x fastest.  n_x == 0 && n_y == 0: no image axes -- X and Y are not computed, ex and ey are not read.  An accepted
// photon outside any axis, or with a coordinate that is not a number, is in no bin and adds to n_outside[o].  Counts are exact; the six sums per bin
// are added with floating-point atomics in whatever order the hardware serves them, each within (m + 2) * 2^-53 * sum|term| of the exact sum of the
// bin's m terms.
//
// The Stokes frame.  Q and U are summed as the photons store them, as mcrat_hip_observe does.  MCRaT defines a photon's Stokes frame from its own
// direction and the polar axis (mcrat_scattering.c, findXY); for photons inside a narrow cone about n those frames coincide to first order in the
// cone's half-angle, at any azimuth, so the sums are the observer's Q and U to that order.  The natural sky axes of an observer at (theta, phi) are
//     ey = phi_hat = (-sin phi, cos phi, 0),   ex = theta_hat = (cos theta cos phi, cos theta sin phi, -sin theta),   ex x ey = n.
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "device_types.hpp"
#include "observe_plan.hpp"

#if defined(__HIPCC__)
#define MCRAT_SKY_HD __host__ __device__
#else
#define MCRAT_SKY_HD
#endif

// The global path's match table, a build-time switch: 0 (the default) the wavefront finds the lanes that share a bin through a one-byte table in LDS
// before it adds (bin_accumulate.hpp, match_alone); 1 no table, every lane goes through the rounds (add_shared_bins).  tools/sky_bench.py measures
// both on an image (profiles/sky_observe.txt).
#ifndef MCRAT_SKY_NO_MATCH
#define MCRAT_SKY_NO_MATCH 0
#endif

namespace mcrat {

// ------------------------------------------------------------------ refusals and their texts
enum SkyRefusal {
    SKY_OK = 0,
    SKY_NO_BINS,                     // n_obs, n_t or n_e < 1
    SKY_IMAGE_AXES_MISMATCH,         // n_x and n_y neither both 0 nor both >= 1
    SKY_TOO_MANY_BINS,               // n_obs * n_t * n_e * n_y * n_x does not fit an int
    SKY_DIRECTION_NOT_FINITE,
    SKY_DIRECTION_NOT_UNIT,          // |n.n - 1| > SKY_UNIT_TOLERANCE
    SKY_BAD_CONE,                    // cos_acc not finite or outside [-1, 1]
    SKY_AXES_NULL,                   // image axes without ex or ey
    SKY_AXES_NOT_FINITE,
    SKY_AXES_NOT_UNIT,
    SKY_AXES_NOT_ORTHOGONAL,         // |ex.n|, |ey.n| or |ex.ey| > SKY_UNIT_TOLERANCE
    SKY_T_EDGES_NOT_FINITE,
    SKY_T_EDGES_NOT_ASCENDING,
    SKY_E_EDGES_NOT_FINITE,
    SKY_E_EDGES_NOT_ASCENDING,
    SKY_X_EDGES_NOT_FINITE,
    SKY_X_EDGES_NOT_ASCENDING,
    SKY_Y_EDGES_NOT_FINITE,
    SKY_Y_EDGES_NOT_ASCENDING,
    SKY_STAGING_TOO_LARGE,           // the edges and the observers' vectors do not fit the LDS budget
    SKY_BAD_PATH_SWITCH,             // MCRAT_HIP_SKY_PATH is neither lds nor global
    SKY_LDS_FORCED_TOO_LARGE         // MCRAT_HIP_SKY_PATH=lds with a cube beyond the LDS budget
};
inline const char *sky_refusal_text(SkyRefusal why)
{
    switch (why) {
    case SKY_OK: return "";
    case SKY_NO_BINS: return "observe_sky: n_obs, n_t and n_e must each be at least 1";
    case SKY_IMAGE_AXES_MISMATCH: return "observe_sky: n_x and n_y must both be 0 (no image axes) or both at least 1";
    case SKY_TOO_MANY_BINS: return "observe_sky: n_obs * n_t * n_e * n_y * n_x overflows an int";
    case SKY_DIRECTION_NOT_FINITE: return "observe_sky: an observer's direction holds a value that is not finite";
    case SKY_DIRECTION_NOT_UNIT: return "observe_sky: an observer's direction is not a unit vector (to 1e-12)";
    case SKY_BAD_CONE: return "observe_sky: cos_acc must be a number in [-1, 1]";
    case SKY_AXES_NULL: return "observe_sky: image axes need the sky-plane vectors x0 .. x2 and y0 .. y2";
    case SKY_AXES_NOT_FINITE: return "observe_sky: a sky-plane vector holds a value that is not finite";
    case SKY_AXES_NOT_UNIT: return "observe_sky: a sky-plane vector is not a unit vector (to 1e-12)";
    case SKY_AXES_NOT_ORTHOGONAL: return "observe_sky: the sky-plane vectors and the direction are not orthogonal (to 1e-12)";
    case SKY_T_EDGES_NOT_FINITE: return "observe_sky: t_edges holds a value that is not finite";
    case SKY_T_EDGES_NOT_ASCENDING: return "observe_sky: t_edges is not strictly ascending";
    case SKY_E_EDGES_NOT_FINITE: return "observe_sky: e_edges holds a value that is not finite";
    case SKY_E_EDGES_NOT_ASCENDING: return "observe_sky: e_edges is not strictly ascending";
    case SKY_X_EDGES_NOT_FINITE: return "observe_sky: x_edges holds a value that is not finite";
    case SKY_X_EDGES_NOT_ASCENDING: return "observe_sky: x_edges is not strictly ascending";
    case SKY_Y_EDGES_NOT_FINITE: return "observe_sky: y_edges holds a value that is not finite";
    case SKY_Y_EDGES_NOT_ASCENDING: return "observe_sky: y_edges is not strictly ascending";
    case SKY_STAGING_TOO_LARGE: return "observe_sky: the edges and the observers' vectors do not fit the kernel's LDS budget";
    case SKY_BAD_PATH_SWITCH: return "observe_sky: MCRAT_HIP_SKY_PATH must be lds or global";
    case SKY_LDS_FORCED_TOO_LARGE: return "observe_sky: MCRAT_HIP_SKY_PATH=lds, but the cube does not fit the kernel's LDS budget";
    }
    return "";
}

// A condition on the inputs, not a rounding allowance: vectors built from cos and sin in double miss 1 and 0 by a few 1e-16.
constexpr double SKY_UNIT_TOLERANCE = 1e-12;

// ------------------------------------------------------------------ the block and where it is accumulated
// One block: seven planes of 8 bytes per bin -- OBSERVE_PLANES: count (integer), W, WE, I, Q, U, V -- each [n_obs][n_t][n_e][n_y][n_x], followed by
// the per-observer counters n_accepted[n_obs], n_outside[n_obs]; cube and counters are zeroed by one memset.  Behind them the kernel's inputs, in
// the order it stages them into LDS: n0, n1, n2, cos_acc [n_obs each]; with image axes x0, x1, x2, y0, y1, y2 [n_obs each]; t_edges [n_t + 1],
// e_edges [n_e + 1]; with image axes x_edges [n_x + 1], y_edges [n_y + 1].  Then the lists' clocks [n_clocks].
constexpr int SKY_BLOCK = 256;                   // threads per workgroup: one lane per slot and trip
// The grid: a grid-stride loop over at most this many workgroups (eight per CU on the 256 CUs of an MI355X), whatever the device reports.
constexpr int SKY_MAX_GRID = 2048;
// global path: the wavefronts' match tables (observe_plan.hpp), unless the build does without them
static_assert(SKY_BLOCK == OBSERVE_BLOCK, "the match tables are sized for the workgroup");
constexpr int SKY_MATCH_BITS = OBSERVE_MATCH_BITS;
constexpr size_t SKY_MATCH_BYTES = MCRAT_SKY_NO_MATCH ? 0 : OBSERVE_MATCH_BYTES;
MCRAT_SKY_HD inline unsigned sky_match_hash(int bin) { return observe_match_hash(bin); }

// the caller's arguments as the checks read them (host pointers)
struct SkyArgs {
    int n_obs;
    const double *n0, *n1, *n2, *cos_acc;        // [n_obs]
    const double *x0, *x1, *x2, *y0, *y1, *y2;   // [n_obs], image axes only
    int n_t; const double *t_edges;
    int n_e; const double *e_edges;
    int n_x; const double *x_edges;
    int n_y; const double *y_edges;
};
struct SkyPlan {
    int n_obs, n_t, n_e, n_x, n_y;       // as given: n_x == n_y == 0 without image axes
    bool image;
    int n_bins;                          // n_obs * n_t * n_e * max(n_y, 1) * max(n_x, 1)
    size_t cube_bytes;                   // the seven planes
    size_t out_bytes;                    // ... and the per-observer counters: what is zeroed, and what the kernel adds into
    size_t staged_doubles;               // vectors, cosines and edges
    size_t staged_bytes;                 // ... and, in LDS, the workgroup's per-observer counters behind them
    size_t lds_bytes;                    // the kernel's dynamic LDS on the chosen path: behind the staged part the cube (LDS) or the match tables (global)
    int groups_per_cu;                   // workgroups the grid is sized for per CU: two on the LDS path, up to eight on the global path
    ObservePath path;
};
// x fastest, then y, energy, time, observer; n_y and n_x as 1 without image axes (iy = ix = 0)
MCRAT_SKY_HD inline size_t sky_bin_index(int o, int it, int ie, int iy, int ix, int n_t, int n_e, int n_y, int n_x)
{
    return ((((size_t)o * (size_t)n_t + (size_t)it) * (size_t)n_e + (size_t)ie) * (size_t)n_y + (size_t)iy) * (size_t)n_x + (size_t)ix;
}

inline SkyRefusal sky_edges_check(const double *edges, int n, SkyRefusal not_finite, SkyRefusal not_ascending)
{
    return edges_refusal(edges, n, SKY_OK, not_finite, not_ascending);
}
inline bool sky_finite3(const double *a, const double *b, const double *c, int o) { return isfinite(a[o]) && isfinite(b[o]) && isfinite(c[o]); }
inline double sky_dot(const double *a0, const double *a1, const double *a2, const double *b0, const double *b1, const double *b2, int o)
{
    return (a0[o] * b0[o] + a1[o] * b1[o]) + a2[o] * b2[o];
}
inline bool sky_unit(const double *a, const double *b, const double *c, int o) { return !(fabs(sky_dot(a, b, c, a, b, c, o) - 1.0) > SKY_UNIT_TOLERANCE); }

// The checks of the arguments alone, in this order: the counts; the image axes' counts; the product; the directions finite, then unit; the cones;
// with image axes the sky-plane vectors -- there, finite, unit, orthogonal --; the edges of t, e, x, y -- each finite, then ascending.  *n_bins is
// filled when SKY_OK.  Also what the escape-weighted observation checks of its observers (escape_plan.hpp).
inline SkyRefusal sky_args_check(const SkyArgs &a, int *n_bins)
{
    if (a.n_obs < 1 || a.n_t < 1 || a.n_e < 1) return SKY_NO_BINS;
    if (!((a.n_x == 0 && a.n_y == 0) || (a.n_x >= 1 && a.n_y >= 1))) return SKY_IMAGE_AXES_MISMATCH;
    const bool image = a.n_x >= 1;
    const int counts[5] = {a.n_obs, a.n_t, a.n_e, image ? a.n_y : 1, image ? a.n_x : 1};
    long long bins = 1;
    for (int k = 0; k < 5; ++k) {
        bins *= (long long)counts[k];                    // (at most (2^31 - 1)^2 < 2^63 before the test)
        if (bins > INT_MAX) return SKY_TOO_MANY_BINS;
    }
    for (int o = 0; o < a.n_obs; ++o)
        if (!sky_finite3(a.n0, a.n1, a.n2, o)) return SKY_DIRECTION_NOT_FINITE;
    for (int o = 0; o < a.n_obs; ++o)
        if (!sky_unit(a.n0, a.n1, a.n2, o)) return SKY_DIRECTION_NOT_UNIT;
    for (int o = 0; o < a.n_obs; ++o)
        if (!(a.cos_acc[o] >= -1.0 && a.cos_acc[o] <= 1.0)) return SKY_BAD_CONE;
    if (image) {
        if (!a.x0 || !a.x1 || !a.x2 || !a.y0 || !a.y1 || !a.y2) return SKY_AXES_NULL;
        for (int o = 0; o < a.n_obs; ++o)
            if (!sky_finite3(a.x0, a.x1, a.x2, o) || !sky_finite3(a.y0, a.y1, a.y2, o)) return SKY_AXES_NOT_FINITE;
        for (int o = 0; o < a.n_obs; ++o)
            if (!sky_unit(a.x0, a.x1, a.x2, o) || !sky_unit(a.y0, a.y1, a.y2, o)) return SKY_AXES_NOT_UNIT;
        for (int o = 0; o < a.n_obs; ++o)
            if (fabs(sky_dot(a.x0, a.x1, a.x2, a.n0, a.n1, a.n2, o)) > SKY_UNIT_TOLERANCE || fabs(sky_dot(a.y0, a.y1, a.y2, a.n0, a.n1, a.n2, o)) > SKY_UNIT_TOLERANCE ||
                fabs(sky_dot(a.x0, a.x1, a.x2, a.y0, a.y1, a.y2, o)) > SKY_UNIT_TOLERANCE)
                return SKY_AXES_NOT_ORTHOGONAL;
    }
    SkyRefusal why = sky_edges_check(a.t_edges, a.n_t, SKY_T_EDGES_NOT_FINITE, SKY_T_EDGES_NOT_ASCENDING);
    if (why == SKY_OK) why = sky_edges_check(a.e_edges, a.n_e, SKY_E_EDGES_NOT_FINITE, SKY_E_EDGES_NOT_ASCENDING);
    if (why == SKY_OK && image) why = sky_edges_check(a.x_edges, a.n_x, SKY_X_EDGES_NOT_FINITE, SKY_X_EDGES_NOT_ASCENDING);
    if (why == SKY_OK && image) why = sky_edges_check(a.y_edges, a.n_y, SKY_Y_EDGES_NOT_FINITE, SKY_Y_EDGES_NOT_ASCENDING);
    if (why != SKY_OK) return why;
    *n_bins = (int)bins;
    return SKY_OK;
}

// The checks, in this order: the arguments' (sky_args_check); what must fit LDS; then the switch `env` (MCRAT_HIP_SKY_PATH) -- its spelling, lds
// with a cube beyond the budget.  The path, the LDS and the workgroups per CU are accumulate_rule's (observe_plan.hpp).  *plan is filled when SKY_OK.
inline SkyRefusal sky_plan(const SkyArgs &a, const char *env, SkyPlan *plan)
{
    int bins = 0;
    const SkyRefusal why = sky_args_check(a, &bins);
    if (why != SKY_OK) return why;
    const bool image = a.n_x >= 1;
    SkyPlan p{};
    p.n_obs = a.n_obs; p.n_t = a.n_t; p.n_e = a.n_e; p.n_x = a.n_x; p.n_y = a.n_y; p.image = image; p.n_bins = bins;
    p.cube_bytes = (size_t)OBSERVE_PLANES * 8 * (size_t)p.n_bins;
    p.out_bytes = p.cube_bytes + (size_t)2 * 8 * (size_t)a.n_obs;
    p.staged_doubles = (size_t)(image ? 10 : 4) * a.n_obs + (size_t)a.n_t + 1 + (size_t)a.n_e + 1 + (image ? (size_t)a.n_x + 1 + (size_t)a.n_y + 1 : 0);
    p.staged_bytes = 8 * p.staged_doubles + (size_t)2 * 8 * (size_t)a.n_obs;
    if (p.staged_bytes + SKY_MATCH_BYTES > OBSERVE_LDS_BUDGET) return SKY_STAGING_TOO_LARGE;       // (so that the global path always has room for its tables)
    ObservePath forced;
    if (observe_path_switch(env, &forced) != OBSERVE_OK) return SKY_BAD_PATH_SWITCH;
    const AccumulateRule r = accumulate_rule(p.staged_bytes, p.cube_bytes, SKY_MATCH_BYTES, forced);
    if (forced == OBSERVE_PATH_LDS && !r.fits) return SKY_LDS_FORCED_TOO_LARGE;
    p.path = r.path; p.lds_bytes = r.lds_bytes; p.groups_per_cu = r.groups_per_cu;
    *plan = p;
    return SKY_OK;
}

// workgroups of SKY_BLOCK lanes: a grid-stride loop, at most what the plan wants resident per CU and never more than SKY_MAX_GRID
inline int sky_grid(const SkyPlan &p, int n_slots, int cus)
{
    return accumulate_grid(n_slots, SKY_BLOCK, cus, p.groups_per_cu, SKY_MAX_GRID);
}

// ------------------------------------------------------------------ one photon (host and device)
MCRAT_SKY_HD inline bool sky_accepted(double p0, double p1, double p2, double p3, double n0, double n1, double n2, double cos_acc)
{
    return ((p1 * n0 + p2 * n1) + p3 * n2) >= p0 * cos_acc;
}
MCRAT_SKY_HD inline double sky_t_det(double time_now, double r0, double r1, double r2, double n0, double n1, double n2)
{
    return time_now - (((r0 * n0 + r1 * n1) + r2 * n2) / C_LIGHT);
}
MCRAT_SKY_HD inline void sky_xy(double r0, double r1, double r2, double ex0, double ex1, double ex2, double ey0, double ey1, double ey2, double &X, double &Y)
{
    X = (r0 * ex0 + r1 * ex1) + r2 * ex2;
    Y = (r0 * ey0 + r1 * ey1) + r2 * ey2;
}
// the bin of observer o's photon at (t, e) and, with image axes, (X, Y); -1 when any coordinate lies outside its axis or is not a number.
// Without image axes (n_x == n_y == 0) x_edges, y_edges, X and Y are not looked at.
MCRAT_SKY_HD inline int sky_bin(int o, const double *t_edges, int n_t, double t, const double *e_edges, int n_e, double e, const double *x_edges, int n_x, double X,
                                const double *y_edges, int n_y, double Y)
{
    const int it = observe_find_bin(t_edges, n_t, t), ie = observe_find_bin(e_edges, n_e, e);
    if (it < 0 || ie < 0) return -1;
    if (n_x == 0) return (int)sky_bin_index(o, it, ie, 0, 0, n_t, n_e, 1, 1);
    const int ix = observe_find_bin(x_edges, n_x, X), iy = observe_find_bin(y_edges, n_y, Y);
    if (ix < 0 || iy < 0) return -1;
    return (int)sky_bin_index(o, it, ie, iy, ix, n_t, n_e, n_y, n_x);      // < n_bins, an int (sky_plan)
}

}  // namespace mcrat
