// escape_plan.hpp -- the host's rules for an escape-weighted sky observation (mcrat_hip_observe_escaping, mcrat_hip_pool_observe_escaping): the
// refusals and their texts, the layout of the block on the device, the rule that picks the accumulation path, the grids, and the per-photon
// function escape_bin, written once here and used by the kernel (escape.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that
// a CPU test can drive them (tests/test_escape_plan_cpu.py).  The observers' checks are sky_plan.hpp's, the march's sightline_plan.hpp's: called,
// not restated.
//
// Definitions.  A slot counts when observe_observable says so.  Observer o accepts a photon by sky_accepted; its e, t_det and
// (X, Y) are sky_plan.hpp's.  A slot that at least one observer accepts is marched once, from (r0, r1, r2) along (p0 .. p3) through one frozen
// staged frame, exactly as sightline_plan.hpp defines a sightline: it ends in tau and a status.  For every observer that accepts it: OPAQUE adds
// to n_opaque[o], STEP_CAP and OFF_TABLE add to n_unresolved[o]; LEFT_MESH -- tau is the optical depth to the edge of the frame -- goes to bin
// (o, itau, it, ie[, iy, ix]), every axis decided by observe_find_bin, or, outside any axis or with a coordinate (tau included) that is not a number,
// adds to n_outside[o].  A photon that starts outside the frame has tau = 0 exactly and belongs to the bin that holds 0.
// Per bin nine planes of 8 bytes: count, W, WE, I, Q, U, V as observe_sky has them, WX = sum w * x and WEX = sum (w * e) * x with x = exp(-tau).
//
// What exp(-tau) means: for a photon at x moving along p_hat through ONE frozen frame it is the probability that its current flight leaves the frame
// without another scattering.  The accepted photons move within the cone about n, so sum w * exp(-tau) per (observer, time, energy[, pixel]) is the
// expected signal already streaming towards that observer, and the tau axis shows from which depth it comes.  This is NOT a peel-off estimator
// towards n: the direction is the photon's own.
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "device_types.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "sightline_plan.hpp"

namespace mcrat {

// ------------------------------------------------------------------ refusals and their texts
// In the order they are checked.  The observers' refusals keep sky_plan.hpp's numbers (1 .. SKY_Y_EDGES_NOT_ASCENDING), the march's
// sightline_plan.hpp's behind ESCAPE_MARCH: their texts are those headers' with this product's prefix.
enum EscapeRefusal {
    ESCAPE_OK = 0,
    // 1 .. 18: SkyRefusal, SKY_NO_BINS .. SKY_Y_EDGES_NOT_ASCENDING
    ESCAPE_NO_TAU_BINS = 32,         // n_tau < 1
    ESCAPE_TOO_MANY_BINS,            // n_obs * n_tau * n_t * n_e * n_y * n_x does not fit an int
    ESCAPE_TAU_EDGES_NOT_FINITE,
    ESCAPE_TAU_EDGES_NOT_ASCENDING,
    ESCAPE_MARCH = 48,               // + SightlineRefusal: SIGHTLINE_BAD_STEP_FRAC .. SIGHTLINE_BAD_TAU_STOP
    ESCAPE_STAGING_TOO_LARGE = 64,   // the edges and the observers' vectors do not fit the LDS budget
    ESCAPE_BAD_PATH_SWITCH,          // MCRAT_HIP_ESCAPE_PATH is neither lds nor global
    ESCAPE_LDS_FORCED_TOO_LARGE,     // MCRAT_HIP_ESCAPE_PATH=lds with a cube beyond the LDS budget
    ESCAPE_HYDRO_MISMATCH            // the frame's context has other switches or another device (the engine's check)
};
inline EscapeRefusal escape_from_sky(SkyRefusal why) { return (EscapeRefusal)(int)why; }
inline EscapeRefusal escape_from_march(SightlineRefusal why) { return why == SIGHTLINE_OK ? ESCAPE_OK : (EscapeRefusal)((int)ESCAPE_MARCH + (int)why); }
constexpr size_t ESCAPE_TEXT_BYTES = 256;
// -> buf: the refusal's text, every one prefixed "observe_escaping: "
inline const char *escape_refusal_text(EscapeRefusal why, char (&buf)[ESCAPE_TEXT_BYTES])
{
    const char *own = nullptr, *theirs = nullptr;
    switch ((int)why) {
    case ESCAPE_OK: own = ""; break;
    case ESCAPE_NO_TAU_BINS: own = "observe_escaping: n_tau must be at least 1"; break;
    case ESCAPE_TOO_MANY_BINS: own = "observe_escaping: n_obs * n_tau * n_t * n_e * n_y * n_x overflows an int"; break;
    case ESCAPE_TAU_EDGES_NOT_FINITE: own = "observe_escaping: tau_edges holds a value that is not finite"; break;
    case ESCAPE_TAU_EDGES_NOT_ASCENDING: own = "observe_escaping: tau_edges is not strictly ascending"; break;
    case ESCAPE_STAGING_TOO_LARGE: own = "observe_escaping: the edges and the observers' vectors do not fit the kernel's LDS budget"; break;
    case ESCAPE_BAD_PATH_SWITCH: own = "observe_escaping: MCRAT_HIP_ESCAPE_PATH must be lds or global"; break;
    case ESCAPE_LDS_FORCED_TOO_LARGE: own = "observe_escaping: MCRAT_HIP_ESCAPE_PATH=lds, but the cube does not fit the kernel's LDS budget"; break;
    case ESCAPE_HYDRO_MISMATCH:
        own = "observe_escaping: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY, TAU_CALCULATION) or on another device";
        break;
    default:
        if ((int)why >= 1 && (int)why <= (int)SKY_Y_EDGES_NOT_ASCENDING) theirs = sky_refusal_text((SkyRefusal)(int)why);
        else if ((int)why > (int)ESCAPE_MARCH && (int)why <= (int)ESCAPE_MARCH + (int)SIGHTLINE_BAD_TAU_STOP)
            theirs = sightline_refusal_text((SightlineRefusal)((int)why - (int)ESCAPE_MARCH));
        else own = "";
    }
    if (own) {
        snprintf(buf, sizeof buf, "%s", own);
    } else {
        const char *colon = strchr(theirs, ':');                 // "observe_sky: ..." / "sightline: ...": the text behind the other product's prefix
        snprintf(buf, sizeof buf, "observe_escaping:%s", colon ? colon + 1 : theirs);
    }
    return buf;
}

// ------------------------------------------------------------------ the block and where it is accumulated
// One block.  First what one memset zeroes and what is read back -- the planes and counters the caller asks for, and the head --: nine planes of 8
// bytes per bin -- ESCAPE_PLANES: count (integer), W, WE, I, Q, U, V, WX, WEX -- each [n_obs][n_tau][n_t][n_e][n_y][n_x], x fastest; the per-observer counters n_accepted, n_outside, n_opaque, n_unresolved [n_obs
// each]; the head of eight 8-byte words -- n_status[5] (word 0, SKIPPED, stays 0: a slot nobody accepts is not marched), n_selected (the compacted
// list's length, which the kernels read from here), n_observable, one spare.  Behind them the binning kernel's inputs in the order it stages them
// into LDS: sky_plan.hpp's -- n0, n1, n2, cos_acc [n_obs each]; with image axes x0 .. x2, y0 .. y2 [n_obs each]; t_edges, e_edges; with image axes
// x_edges, y_edges -- then tau_edges [n_tau + 1].  Then the lists' clocks [n_clocks].  Then the compacted list, sized for every slot: tau [n_slots]
// doubles, index [n_slots] and status [n_slots] ints.
constexpr int ESCAPE_PLANES = 9;
enum EscapePlane { ESC_COUNT = 0, ESC_W, ESC_WE, ESC_I, ESC_Q, ESC_U, ESC_V, ESC_WX, ESC_WEX };
constexpr int ESCAPE_COUNTERS = 4;               // per observer: accepted, outside, opaque, unresolved
constexpr int ESCAPE_HEAD_WORDS = 8;
constexpr int ESCAPE_SELECTED_WORD = 5, ESCAPE_OBSERVABLE_WORD = 6;
constexpr int ESCAPE_BLOCK = 256;                // threads per workgroup of all three kernels
static_assert(ESCAPE_BLOCK == OBSERVE_BLOCK && ESCAPE_BLOCK == SIGHTLINE_BLOCK, "the match tables are sized for the workgroup");
constexpr int ESCAPE_MAX_GRID = SKY_MAX_GRID;    // select and bin: grid-stride loops over at most this many workgroups
// The march: one lane per list entry up to this many workgroups (16.7 million entries), a stride beyond.  The list's length is known on the device
// only, so the grid covers every slot; a workgroup beyond the list reads the length and ends, and the device hands its place to the next -- the
// same way the sightline kernel's plain form, its measured default, fills the places of rays that ended.
constexpr int ESCAPE_MARCH_MAX_GRID = 65536;
constexpr size_t ESCAPE_MATCH_BYTES = OBSERVE_MATCH_BYTES;

struct EscapePlan {
    int n_obs, n_tau, n_t, n_e, n_x, n_y;    // as given: n_x == n_y == 0 without image axes
    bool image;
    int n_bins;                          // n_obs * n_tau * n_t * n_e * max(n_y, 1) * max(n_x, 1)
    SightlineParams march;               // surface_level is not read
    size_t cube_bytes;                   // the nine planes
    size_t counters_offset, head_offset; // bytes from the block's start
    size_t out_bytes;                    // planes, counters and head: what is zeroed, and what is read back from
    size_t staged_doubles;               // vectors, cosines and edges
    size_t staged_bytes;                 // ... and, in LDS, the workgroup's four counters per observer behind them
    size_t lds_bytes;                    // the binning kernel's dynamic LDS on the chosen path: behind the staged part the cube (LDS) or the match tables (global)
    size_t select_lds_bytes;             // the selecting kernel's: n0, n1, n2, cos_acc
    int groups_per_cu;                   // workgroups the binning grid is sized for per CU
    ObservePath path;
};
// where the parts behind out_bytes lie for n_slots slots and n_clocks clocks (0: one clock for all); total: the block's size
struct EscapeLayout { size_t staged_offset, clocks_offset, tau_offset, index_offset, status_offset, total_bytes; };
inline EscapeLayout escape_layout(const EscapePlan &p, int n_slots, int n_clocks)
{
    EscapeLayout l{};
    l.staged_offset = p.out_bytes;
    l.clocks_offset = l.staged_offset + 8 * p.staged_doubles;
    l.tau_offset = l.clocks_offset + 8 * (size_t)n_clocks;
    l.index_offset = l.tau_offset + 8 * (size_t)n_slots;
    l.status_offset = l.index_offset + 4 * (size_t)n_slots;
    l.total_bytes = l.status_offset + 4 * (size_t)n_slots;
    return l;
}

// x fastest, then y, energy, time, optical depth, observer; n_y and n_x as 1 without image axes (iy = ix = 0)
MCRAT_SKY_HD inline size_t escape_bin_index(int o, int itau, int it, int ie, int iy, int ix, int n_tau, int n_t, int n_e, int n_y, int n_x)
{
    return sky_bin_index(o * n_tau + itau, it, ie, iy, ix, n_t, n_e, n_y, n_x);
}

// the caller's arguments as the checks read them (host pointers)
struct EscapeArgs {
    SkyArgs sky;
    int n_tau; const double *tau_edges;
    SightlineParams march;
};

// The checks, in this order: the observers' in sky_plan.hpp's order (sky_args_check); n_tau; the product of all counts; tau_edges finite, then
// ascending; the march's four parameters in sightline_plan.hpp's order; what must fit LDS; then the switch `env` (MCRAT_HIP_ESCAPE_PATH) -- its
// spelling, lds with a cube beyond the budget.  The path, the LDS and the workgroups per CU are accumulate_rule's.  *plan is filled when ESCAPE_OK.
inline EscapeRefusal escape_plan(const EscapeArgs &a, const char *env, EscapePlan *plan)
{
    int per_tau = 0;
    const SkyRefusal sky = sky_args_check(a.sky, &per_tau);
    if (sky != SKY_OK) return escape_from_sky(sky);
    if (a.n_tau < 1) return ESCAPE_NO_TAU_BINS;
    const long long bins = (long long)per_tau * (long long)a.n_tau;
    if (bins > INT_MAX) return ESCAPE_TOO_MANY_BINS;
    const EscapeRefusal edges = edges_refusal(a.tau_edges, a.n_tau, ESCAPE_OK, ESCAPE_TAU_EDGES_NOT_FINITE, ESCAPE_TAU_EDGES_NOT_ASCENDING);
    if (edges != ESCAPE_OK) return edges;
    const EscapeRefusal march = escape_from_march(sightline_march_check(a.march));
    if (march != ESCAPE_OK) return march;
    const SkyArgs &s = a.sky;
    EscapePlan p{};
    p.n_obs = s.n_obs; p.n_tau = a.n_tau; p.n_t = s.n_t; p.n_e = s.n_e; p.n_x = s.n_x; p.n_y = s.n_y; p.image = s.n_x >= 1; p.n_bins = (int)bins;
    p.march = a.march;
    p.cube_bytes = (size_t)ESCAPE_PLANES * 8 * (size_t)p.n_bins;
    p.counters_offset = p.cube_bytes;
    p.head_offset = p.counters_offset + (size_t)ESCAPE_COUNTERS * 8 * (size_t)s.n_obs;
    p.out_bytes = p.head_offset + (size_t)ESCAPE_HEAD_WORDS * 8;
    p.staged_doubles = (size_t)(p.image ? 10 : 4) * s.n_obs + (size_t)s.n_t + 1 + (size_t)s.n_e + 1 + (p.image ? (size_t)s.n_x + 1 + (size_t)s.n_y + 1 : 0) +
                       (size_t)a.n_tau + 1;
    p.staged_bytes = 8 * p.staged_doubles + (size_t)ESCAPE_COUNTERS * 8 * (size_t)s.n_obs;
    p.select_lds_bytes = (size_t)4 * 8 * (size_t)s.n_obs;
    if (p.staged_bytes + ESCAPE_MATCH_BYTES > OBSERVE_LDS_BUDGET) return ESCAPE_STAGING_TOO_LARGE;       // (so that the global path always has room for its tables)
    ObservePath forced;
    if (observe_path_switch(env, &forced) != OBSERVE_OK) return ESCAPE_BAD_PATH_SWITCH;
    const AccumulateRule r = accumulate_rule(p.staged_bytes, p.cube_bytes, ESCAPE_MATCH_BYTES, forced);
    if (forced == OBSERVE_PATH_LDS && !r.fits) return ESCAPE_LDS_FORCED_TOO_LARGE;
    p.path = r.path; p.lds_bytes = r.lds_bytes; p.groups_per_cu = r.groups_per_cu;
    *plan = p;
    return ESCAPE_OK;
}

// select: workgroups of ESCAPE_BLOCK lanes in a grid-stride loop over the slots, up to eight per CU
inline int escape_select_grid(int n_slots, int cus) { return accumulate_grid(n_slots, ESCAPE_BLOCK, cus, OBSERVE_MAX_GROUPS_PER_CU, ESCAPE_MAX_GRID); }
// march: one lane per list entry; the list is no longer than the slots
inline int escape_march_grid(int n_slots)
{
    const long long want = ((long long)n_slots + ESCAPE_BLOCK - 1) / ESCAPE_BLOCK;
    return (int)(want < ESCAPE_MARCH_MAX_GRID ? want : ESCAPE_MARCH_MAX_GRID);
}
// bin: a grid-stride loop over the list, at most what the plan wants resident per CU
inline int escape_bin_grid(const EscapePlan &p, int n_slots, int cus) { return accumulate_grid(n_slots, ESCAPE_BLOCK, cus, p.groups_per_cu, ESCAPE_MAX_GRID); }

// ------------------------------------------------------------------ one photon (host and device)
// The bin of observer o's LEFT_MESH photon at optical depth tau, (t, e) and, with image axes, (X, Y); -1 when any coordinate lies outside its axis or
// is not a number.  The axes behind tau are sky_bin's: the photon's bin within one observer's part of a sky cube.
MCRAT_SKY_HD inline int escape_bin(int o, const double *tau_edges, int n_tau, double tau, const double *t_edges, int n_t, double t, const double *e_edges, int n_e,
                                   double e, const double *x_edges, int n_x, double X, const double *y_edges, int n_y, double Y)
{
    const int itau = observe_find_bin(tau_edges, n_tau, tau);
    if (itau < 0) return -1;
    return sky_bin(o * n_tau + itau, t_edges, n_t, t, e_edges, n_e, e, x_edges, n_x, X, y_edges, n_y, Y);      // < n_bins, an int (escape_plan)
}
// what a photon's flight is weighted with: the probability that it leaves the frame without another scattering
MCRAT_SKY_HD inline double escape_weight(double tau) { return exp(-tau); }

}  // namespace mcrat
