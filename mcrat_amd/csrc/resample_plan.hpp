// resample_plan.hpp -- the host's rules for a sky observation with a resampling axis and a choice of Stokes frame (mcrat_hip_observe_sky_resampled,
// mcrat_hip_pool_observe_sky_resampled): the refusals and their texts, the layout of the block on the device, the multiplicity functions and their
// threshold table, the Stokes rotation, the bin index with the replica axis, the rule that picks the accumulation path, and the grid -- written once
// here and used by the kernel (resample.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them
// (tests/test_resample_plan_cpu.py).  The observers' checks, the per-photon rules and the bin within one (observer, replica) are sky_plan.hpp's:
// called, not restated.
//
// Definitions.  Which slots count, acceptance, e, t_det, (X, Y), the bin rule, n_accepted and n_outside are
// mcrat_hip_observe_sky's.  The cube is [n_obs][n_rep][n_t][n_e][n_y][n_x], x fastest: the replica axis sits where the escape cube's tau axis sits.
// An accepted, binned photon adds to replica rho  k  to count and  (double)k * term  to each of the six sums, term exactly observe_sky's: w, w * e,
// w * s0, w * s1', w * s2', w * s3 (s1', s2': the stored s1, s2, or those carried into the observer's frame, below).
//
// Multiplicity.  k = k(photon identity, rho) does not depend on the observer.  A photon's identity is (rank, slot): rank the list's index in its
// pool (view_rank for a view, slot / rank_stride in a pool call, 0 for a stand-alone context), slot the index within the list -- a view and its pool
// give a photon the same k.  All draws come from  keyed_block(seed, slot | (uint64_t)rank << 32, block, RNG_RESAMPLE, mode)  (rng.hpp):
//     NONE        n_rep == 1, k = 1
//     JACKKNIFE   n_rep = G >= 2 disjoint groups: block 0,  g = ((uint64_t)w[0] * G) >> 32,  k = [rho == g]
//     BOOTSTRAP   n_rep = B + 1 >= 2: rho = 0 is the sample itself, k = 1; for rho >= 1, j = rho - 1, the block is j >> 2, the word w[j & 3] and
//                 k = #{m : word >= T_m},  T_m = floor(2^32 * sum_{i <= m} e^-1 / i!),  m = 0 .. 11: a Poisson(1) draw cut at 12, with a truncation
//                 bias below 2^-31.
// Integer arithmetic throughout: every count is exactly reproducible on the host.
//
// The Stokes frame.  AS_STORED: Q and U are summed as the photons store them, as observe_sky does.  SKY_PLANE: for every accepted (photon,
// observer) pair (Q, U) = (s1, s2) are carried from the photon's frame to the observer's by the reference's own rule -- findPhi followed by
// mullerMatrixRotation (mcrat_scattering.c), rotate_stokes_between in physics.hpp, old -> new -- in a form that stays well conditioned near zero
// angle.  With p = (p1, p2, p3), p_hat = p / |p|:
//     y_ph ~ p x z_hat = (p2, -p1, 0),   x_ph = y_ph x p_hat           the photon's frame (findXY against z_hat)
//     y_new ~ ey - (ey . p_hat) p_hat                                   the observer's ey carried into the plane perpendicular to p
//     d ~ y_ph . y_new,   s ~ x_ph . y_new,   normalised jointly:  h = sqrt(d^2 + s^2),  c = d / h,  sigma = s / h
//     c2 = c^2 - sigma^2,  s2 = -2 sigma c,   Q' = Q c2 - U s2,   U' = Q s2 + U c2;   I and V are unchanged.
// y_ph . p = x_ph . p = 0, so y_new's second term drops out of both products and, up to one common positive factor,
//     d = p2 * ey0 - p1 * ey1,    s = (rho2 * ey2 - p3 * (p1 * ey0 + p2 * ey1)) / |p|,    rho2 = p1^2 + p2^2.
// This equals the reference's c2 = 2 d^2 - 1, s2 = -sign(x . y') 2 d sqrt(1 - d^2) without the cancellation at d -> +-1.  When h is 0 or not finite
// (p parallel to z_hat, or to ey) the pair's Q and U are added as stored and n_frame_undefined[o] counts it.  The exact order of the IEEE operations
// (+ - * / sqrt, correctly rounded, -ffp-contract=off) is resample_rotation's below: the terms are bit-identical in the kernel, in g++ and in NumPy.
// The sense of U: a photon at azimuth phi_p infinitesimally off the axis, with stored (Q, U) = (1, 0), seen by the on-axis observer with ex = x_hat,
// ey = y_hat, contributes (cos 2 phi_p, -sin 2 phi_p).  It is MCRaT's sense of U.
#pragma once
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "device_types.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "rng.hpp"

namespace mcrat {

enum ResampleMode { RESAMPLE_NONE = 0, RESAMPLE_JACKKNIFE = 1, RESAMPLE_BOOTSTRAP = 2 };
enum StokesFrame { STOKES_AS_STORED = 0, STOKES_SKY_PLANE = 1 };
// path numbers as mcrat_hip_observe_sky_resampled_path reports them: 1 and 2 mean what they mean for every other binned sum
enum ResamplePath { RESAMPLE_PATH_NONE = 0, RESAMPLE_PATH_LDS = 1, RESAMPLE_PATH_GLOBAL = 2, RESAMPLE_PATH_SLICED = 3 };

// ------------------------------------------------------------------ refusals and their texts
// In the order they are checked.  The observers' refusals keep sky_plan.hpp's numbers (1 .. SKY_Y_EDGES_NOT_ASCENDING); their texts are that
// header's with this product's prefix.
enum ResampleRefusal {
    RESAMPLE_OK = 0,
    // 1 .. 18: SkyRefusal, SKY_NO_BINS .. SKY_Y_EDGES_NOT_ASCENDING
    RESAMPLE_BAD_MODE = 32,
    RESAMPLE_BAD_FRAME,
    RESAMPLE_N_REP_NOT_ONE,          // NONE with n_rep != 1
    RESAMPLE_N_REP_TOO_SMALL,        // JACKKNIFE or BOOTSTRAP with n_rep < 2
    RESAMPLE_TOO_MANY_BINS,          // n_obs * n_rep * n_t * n_e * n_y * n_x does not fit an int
    RESAMPLE_AXES_NULL,              // SKY_PLANE without ex or ey
    RESAMPLE_AXES_NOT_FINITE,
    RESAMPLE_AXES_NOT_UNIT,
    RESAMPLE_AXES_NOT_ORTHOGONAL,
    RESAMPLE_STAGING_TOO_LARGE,
    RESAMPLE_BAD_PATH_SWITCH,        // MCRAT_HIP_RESAMPLE_PATH is none of lds, sliced, global
    RESAMPLE_LDS_FORCED_TOO_LARGE,   // lds forced with a cube beyond the LDS budget
    RESAMPLE_SLICED_FORCED_TOO_LARGE // sliced forced with one replica's sub-cube beyond the LDS budget
};
inline ResampleRefusal resample_from_sky(SkyRefusal why) { return (ResampleRefusal)(int)why; }
constexpr size_t RESAMPLE_TEXT_BYTES = 256;
// -> buf: the refusal's text, every one prefixed "observe_sky_resampled: "
inline const char *resample_refusal_text(ResampleRefusal why, char (&buf)[RESAMPLE_TEXT_BYTES])
{
    const char *own = nullptr, *theirs = nullptr;
    switch ((int)why) {
    case RESAMPLE_OK: own = ""; break;
    case RESAMPLE_BAD_MODE: own = "observe_sky_resampled: mode must be MCRAT_HIP_RESAMPLE_NONE, _JACKKNIFE or _BOOTSTRAP"; break;
    case RESAMPLE_BAD_FRAME: own = "observe_sky_resampled: stokes_frame must be MCRAT_HIP_STOKES_AS_STORED or _SKY_PLANE"; break;
    case RESAMPLE_N_REP_NOT_ONE: own = "observe_sky_resampled: n_rep must be 1 with MCRAT_HIP_RESAMPLE_NONE"; break;
    case RESAMPLE_N_REP_TOO_SMALL: own = "observe_sky_resampled: n_rep must be at least 2 (jackknife groups, or the sample and one bootstrap replica)"; break;
    case RESAMPLE_TOO_MANY_BINS: own = "observe_sky_resampled: n_obs * n_rep * n_t * n_e * n_y * n_x overflows an int"; break;
    case RESAMPLE_AXES_NULL: own = "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE needs the sky-plane vectors x0 .. x2 and y0 .. y2"; break;
    case RESAMPLE_AXES_NOT_FINITE: own = "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE: a sky-plane vector holds a value that is not finite"; break;
    case RESAMPLE_AXES_NOT_UNIT: own = "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE: a sky-plane vector is not a unit vector (to 1e-12)"; break;
    case RESAMPLE_AXES_NOT_ORTHOGONAL: own = "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE: the sky-plane vectors and the direction are not orthogonal (to 1e-12)"; break;
    case RESAMPLE_STAGING_TOO_LARGE: own = "observe_sky_resampled: the edges and the observers' vectors do not fit the kernel's LDS budget"; break;
    case RESAMPLE_BAD_PATH_SWITCH: own = "observe_sky_resampled: MCRAT_HIP_RESAMPLE_PATH must be lds, sliced or global"; break;
    case RESAMPLE_LDS_FORCED_TOO_LARGE: own = "observe_sky_resampled: MCRAT_HIP_RESAMPLE_PATH=lds, but the cube does not fit the kernel's LDS budget"; break;
    case RESAMPLE_SLICED_FORCED_TOO_LARGE:
        own = "observe_sky_resampled: MCRAT_HIP_RESAMPLE_PATH=sliced, but one replica's part of the cube does not fit the kernel's LDS budget";
        break;
    default:
        if ((int)why >= 1 && (int)why <= (int)SKY_Y_EDGES_NOT_ASCENDING) theirs = sky_refusal_text((SkyRefusal)(int)why);
        else own = "";
    }
    if (own) {
        snprintf(buf, sizeof buf, "%s", own);
    } else {
        const char *colon = strchr(theirs, ':');                 // "observe_sky: ...": the text behind the other product's prefix
        snprintf(buf, sizeof buf, "observe_sky_resampled:%s", colon ? colon + 1 : theirs);
    }
    return buf;
}

// ------------------------------------------------------------------ multiplicities (host and device)
// T_m = floor(2^32 * sum_{i <= m} e^-1 / i!), m = 0 .. 11, computed with 50 decimal digits (tests/test_resample_checker_cpu.py recomputes them)
constexpr int RESAMPLE_POISSON_MAX = 12;
// k = #{m : word >= T_m}: a Poisson(1) draw from one uniform 32-bit word, at most RESAMPLE_POISSON_MAX.  The table is written out as comparisons so
// that the thresholds are literals of the instruction stream on the device and no table lives in memory.
MCRAT_SKY_HD inline unsigned resample_poisson(uint32_t word)
{
    return (unsigned)(word >= 1580030168u) + (unsigned)(word >= 3160060337u) + (unsigned)(word >= 3950075421u) + (unsigned)(word >= 4213413783u) +
           (unsigned)(word >= 4279248373u) + (unsigned)(word >= 4292415291u) + (unsigned)(word >= 4294609777u) + (unsigned)(word >= 4294923276u) +
           (unsigned)(word >= 4294962463u) + (unsigned)(word >= 4294966817u) + (unsigned)(word >= 4294967252u) + (unsigned)(word >= 4294967292u);
}
MCRAT_SKY_HD inline uint64_t resample_identity(uint32_t rank, uint32_t slot) { return (uint64_t)slot | (uint64_t)rank << 32; }
MCRAT_SKY_HD inline Philox4 resample_block(uint64_t seed, uint32_t rank, uint32_t slot, uint32_t block, int mode)
{
    return keyed_block(seed, resample_identity(rank, slot), block, RNG_RESAMPLE, (uint32_t)mode);
}
// the jackknife group of a photon, 0 .. G - 1
MCRAT_SKY_HD inline int resample_group(uint64_t seed, uint32_t rank, uint32_t slot, int G)
{
    return (int)(((uint64_t)resample_block(seed, rank, slot, 0u, RESAMPLE_JACKKNIFE).w[0] * (uint64_t)(uint32_t)G) >> 32);
}
// the bootstrap multiplicity of a photon in entry rho >= 1, from the block that holds its word (block == (rho - 1) >> 2)
// (the word by selects: an index that varies keeps the block in registers on the device only when it is no address)
MCRAT_SKY_HD inline unsigned resample_bootstrap_k(const Philox4 &block, int rho)
{
    const int j = (rho - 1) & 3;
    return resample_poisson(j == 0 ? block.w[0] : (j == 1 ? block.w[1] : (j == 2 ? block.w[2] : block.w[3])));
}
// k(photon, rho) in any mode: the definition, one replica at a time (the kernel draws a bootstrap block once for its four replicas)
MCRAT_SKY_HD inline unsigned resample_multiplicity(int mode, uint64_t seed, uint32_t rank, uint32_t slot, int n_rep, int rho)
{
    if (mode == RESAMPLE_JACKKNIFE) return resample_group(seed, rank, slot, n_rep) == rho ? 1u : 0u;
    if (mode == RESAMPLE_BOOTSTRAP && rho >= 1) return resample_bootstrap_k(resample_block(seed, rank, slot, (uint32_t)(rho - 1) >> 2, RESAMPLE_BOOTSTRAP), rho);
    return 1u;
}

// ------------------------------------------------------------------ the Stokes rotation (host and device)
// (Q, U) of a photon moving along (p1, p2, p3) from its own frame into that of an observer whose sky-plane vector is ey; the operations in exactly
// this order.  -> false: the frame is undefined (h is 0 or not finite), Q and U are left as stored.
MCRAT_SKY_HD inline bool resample_rotation(double p1, double p2, double p3, double ey0, double ey1, double ey2, double &Q, double &U)
{
    const double rho2 = p1 * p1 + p2 * p2;
    const double pn = sqrt(rho2 + p3 * p3);
    const double d = p2 * ey0 - p1 * ey1;
    const double s = (rho2 * ey2 - p3 * (p1 * ey0 + p2 * ey1)) / pn;
    const double h = sqrt(d * d + s * s);
    if (!(h > 0.0) || !(h <= DBL_MAX)) return false;
    const double c = d / h, sg = s / h;
    const double c2 = c * c - sg * sg;
    const double s2 = (-2.0 * sg) * c;
    const double q = Q * c2 - U * s2;
    const double u = Q * s2 + U * c2;
    Q = q; U = u;
    return true;
}

// ------------------------------------------------------------------ the block and where it is accumulated
// One block.  First what one memset zeroes: seven planes of 8 bytes per bin -- OBSERVE_PLANES: count (integer), W, WE, I, Q, U, V -- each
// [n_obs][n_rep][n_t][n_e][n_y][n_x]; the per-observer counters n_accepted, n_outside, n_frame_undefined [n_obs each].  Behind them the kernel's
// inputs in the order it stages them into LDS: n0, n1, n2, cos_acc [n_obs each]; with image axes or SKY_PLANE x0 .. x2, y0 .. y2 [n_obs each];
// t_edges, e_edges; with image axes x_edges, y_edges.  Then the lists' clocks [n_clocks].
constexpr int RESAMPLE_COUNTERS = 3;             // per observer: accepted, outside, frame undefined
constexpr int RESAMPLE_BLOCK = 256;              // threads per workgroup: one lane per slot and trip
static_assert(RESAMPLE_BLOCK == OBSERVE_BLOCK, "the match tables are sized for the workgroup");
constexpr int RESAMPLE_MAX_GRID = SKY_MAX_GRID;  // workgroups along x: a grid-stride loop over the slots
constexpr int RESAMPLE_MAX_GRID_Y = 65535;       // ... and along y, over the slices: a stride beyond
constexpr size_t RESAMPLE_MATCH_BYTES = OBSERVE_MATCH_BYTES;
// Sliced or global, where one replica's sub-cube fits LDS and the whole cube does not.  Every slice's workgroups walk all slots once more (flags,
// type and weight, then the hash) and skip the replicas of the other slices; the global path reads the slots once and pays a round of atomics in HBM
// per (photon, replica) that adds.  Measured on the benchmark pool (cfg2, 10^6 photons as 1025 lists, 900 000 accepted; tools/resample_bench.py,
// DESIGN.md section 6, profiles/resample_observe.txt), kernel times:
//     JACKKNIFE, 1 x 32 x 32, one group per slice     8 slices   193 us sliced   328 us global
//                                                     32 slices   673 us          271 us
//                                                    128 slices  2760 us          305 us
//                                                    512 slices 10974 us          291 us
//     JACKKNIFE, 1 x 1 x 1 x 36 x 36 pixels          16 slices   442 us          282 us
//     BOOTSTRAP, 1 x 8 x 16, 201 entries, 19 slices of 11        1818 us        22993 us
// A jackknife photon adds to one replica, so the global path costs the same ~300 us whatever G while the sliced path costs 21 - 24 us per slice: they
// meet at 12 - 14 slices, and the rule is sliced up to RESAMPLE_JACKKNIFE_MAX_SLICES.  A bootstrap photon adds to two replicas in three, so the
// global path pays ~114 us per replica; a slice costs its walk plus ~7 us per replica it holds, a quarter of that even with one replica per slice:
// sliced whenever one replica fits (measured at 19 slices of 11; one replica per slice is this estimate, not a measurement).
constexpr int RESAMPLE_JACKKNIFE_MAX_SLICES = 12;

struct ResampleArgs {
    SkyArgs sky;
    int mode, n_rep, stokes_frame;
};
struct ResamplePlan {
    int n_obs, n_rep, n_t, n_e, n_x, n_y;   // as given: n_x == n_y == 0 without image axes
    int mode, frame;
    bool image, axes;                    // axes: ex and ey are staged (image axes, or SKY_PLANE)
    int per_rep;                         // bins of one (observer, replica): n_t * n_e * max(n_y, 1) * max(n_x, 1)
    int n_bins;                          // n_obs * n_rep * per_rep
    size_t cube_bytes;                   // the seven planes
    size_t out_bytes;                    // ... and the per-observer counters: what is zeroed
    size_t staged_doubles;               // vectors, cosines and edges
    size_t staged_bytes;                 // ... and, in LDS, the workgroup's three counters per observer behind them
    size_t replica_bytes;                // the seven planes of one replica of every observer: the unit a slice is made of
    int slice_reps, n_slices;            // LDS and sliced: replicas per slice (the last may hold fewer) and slices; global: n_rep and 1
    size_t lds_bytes;                    // the kernel's dynamic LDS: behind the staged part the slice's sub-cube (LDS, sliced) or the match tables (global)
    int groups_per_cu;
    ResamplePath path;
};
struct ResampleLayout { size_t counters_offset, staged_offset, clocks_offset, total_bytes; };
inline ResampleLayout resample_layout(const ResamplePlan &p, int n_clocks)
{
    ResampleLayout l{};
    l.counters_offset = p.cube_bytes;
    l.staged_offset = p.out_bytes;
    l.clocks_offset = l.staged_offset + 8 * p.staged_doubles;
    l.total_bytes = l.clocks_offset + 8 * (size_t)n_clocks;
    return l;
}

// x fastest, then y, energy, time, replica, observer; n_y and n_x as 1 without image axes (iy = ix = 0)
MCRAT_SKY_HD inline size_t resample_bin_index(int o, int rho, int it, int ie, int iy, int ix, int n_rep, int n_t, int n_e, int n_y, int n_x)
{
    return sky_bin_index(o * n_rep + rho, it, ie, iy, ix, n_t, n_e, n_y, n_x);
}
// The bin of observer o's photon in replica 0: sky_bin with the observers n_rep apart; replica rho's bin is per_rep * rho further.  -1: in no bin.
MCRAT_SKY_HD inline int resample_bin0(int o, int n_rep, const double *t_edges, int n_t, double t, const double *e_edges, int n_e, double e, const double *x_edges, int n_x,
                                      double X, const double *y_edges, int n_y, double Y)
{
    return sky_bin(o * n_rep, t_edges, n_t, t, e_edges, n_e, e, x_edges, n_x, X, y_edges, n_y, Y);       // < n_bins, an int (resample_plan)
}

// MCRAT_HIP_RESAMPLE_PATH: unset or empty -- the rule decides; lds, sliced, global -- that path; anything else is refused (-> false)
inline bool resample_path_switch(const char *env, ResamplePath *forced)
{
    *forced = RESAMPLE_PATH_NONE;
    if (!env || !*env) return true;
    if (!strcmp(env, "lds")) *forced = RESAMPLE_PATH_LDS;
    else if (!strcmp(env, "sliced")) *forced = RESAMPLE_PATH_SLICED;
    else if (!strcmp(env, "global")) *forced = RESAMPLE_PATH_GLOBAL;
    else return false;
    return true;
}

// The checks, in this order: the observers' in sky_plan.hpp's order (sky_args_check); mode; stokes_frame; n_rep; the product of all counts; with
// SKY_PLANE and without image axes the sky-plane vectors -- there, finite, unit, orthogonal: sky_args_check's own, asked through a one-pixel
// image --; what must fit LDS; then the switch `env` (MCRAT_HIP_RESAMPLE_PATH) -- its spelling, a forced path that does not fit.  The path: LDS when
// the whole cube fits the budget behind the staged part (accumulate_rule); else, when one replica's sub-cube fits, the replica axis is cut into the
// largest slices that fit and the path is sliced -- for JACKKNIFE only up to RESAMPLE_JACKKNIFE_MAX_SLICES slices --; else global.  *plan is filled when RESAMPLE_OK.
inline ResampleRefusal resample_plan(const ResampleArgs &a, const char *env, ResamplePlan *plan)
{
    int sky_bins = 0;                            // one replica of every observer
    const SkyRefusal sky = sky_args_check(a.sky, &sky_bins);
    if (sky != SKY_OK) return resample_from_sky(sky);
    if (a.mode != RESAMPLE_NONE && a.mode != RESAMPLE_JACKKNIFE && a.mode != RESAMPLE_BOOTSTRAP) return RESAMPLE_BAD_MODE;
    if (a.stokes_frame != STOKES_AS_STORED && a.stokes_frame != STOKES_SKY_PLANE) return RESAMPLE_BAD_FRAME;
    if (a.mode == RESAMPLE_NONE && a.n_rep != 1) return RESAMPLE_N_REP_NOT_ONE;
    if (a.mode != RESAMPLE_NONE && a.n_rep < 2) return RESAMPLE_N_REP_TOO_SMALL;
    const long long bins = (long long)sky_bins * (long long)a.n_rep;
    if (bins > INT_MAX) return RESAMPLE_TOO_MANY_BINS;
    const SkyArgs &s = a.sky;
    const bool image = s.n_x >= 1;
    if (a.stokes_frame == STOKES_SKY_PLANE && !image) {
        if (!s.x0 || !s.x1 || !s.x2 || !s.y0 || !s.y1 || !s.y2) return RESAMPLE_AXES_NULL;
        const double unit_edges[2] = {0.0, 1.0};
        SkyArgs pixel = s;
        pixel.n_x = pixel.n_y = 1; pixel.x_edges = pixel.y_edges = unit_edges;
        int unused = 0;
        switch (sky_args_check(pixel, &unused)) {
        case SKY_AXES_NOT_FINITE: return RESAMPLE_AXES_NOT_FINITE;
        case SKY_AXES_NOT_UNIT: return RESAMPLE_AXES_NOT_UNIT;
        case SKY_AXES_NOT_ORTHOGONAL: return RESAMPLE_AXES_NOT_ORTHOGONAL;
        default: break;
        }
    }
    ResamplePlan p{};
    p.n_obs = s.n_obs; p.n_rep = a.n_rep; p.n_t = s.n_t; p.n_e = s.n_e; p.n_x = s.n_x; p.n_y = s.n_y; p.mode = a.mode; p.frame = a.stokes_frame;
    p.image = image; p.axes = image || a.stokes_frame == STOKES_SKY_PLANE;
    p.per_rep = sky_bins / s.n_obs; p.n_bins = (int)bins;
    p.cube_bytes = (size_t)OBSERVE_PLANES * 8 * (size_t)p.n_bins;
    p.out_bytes = p.cube_bytes + (size_t)RESAMPLE_COUNTERS * 8 * (size_t)s.n_obs;
    p.staged_doubles = (size_t)(p.axes ? 10 : 4) * s.n_obs + (size_t)s.n_t + 1 + (size_t)s.n_e + 1 + (image ? (size_t)s.n_x + 1 + (size_t)s.n_y + 1 : 0);
    p.staged_bytes = 8 * p.staged_doubles + (size_t)RESAMPLE_COUNTERS * 8 * (size_t)s.n_obs;
    if (p.staged_bytes + RESAMPLE_MATCH_BYTES > OBSERVE_LDS_BUDGET) return RESAMPLE_STAGING_TOO_LARGE;   // (so that the global path always has room for its tables)
    ResamplePath forced;
    if (!resample_path_switch(env, &forced)) return RESAMPLE_BAD_PATH_SWITCH;
    p.replica_bytes = (size_t)OBSERVE_PLANES * 8 * (size_t)sky_bins;
    const AccumulateRule whole = accumulate_rule(p.staged_bytes, p.cube_bytes, RESAMPLE_MATCH_BYTES, OBSERVE_PATH_NONE);
    const size_t room = OBSERVE_LDS_BUDGET - p.staged_bytes;
    const bool one_fits = p.replica_bytes <= room;
    if (forced == RESAMPLE_PATH_LDS && !whole.fits) return RESAMPLE_LDS_FORCED_TOO_LARGE;
    if (forced == RESAMPLE_PATH_SLICED && !one_fits) return RESAMPLE_SLICED_FORCED_TOO_LARGE;
    int reps = 0, slices = 0;
    if (one_fits) {
        const size_t most = room / p.replica_bytes;
        reps = most < (size_t)a.n_rep ? (int)most : a.n_rep;
        slices = (a.n_rep + reps - 1) / reps;
    }
    ResamplePath path = forced;
    if (path == RESAMPLE_PATH_NONE)
        path = whole.fits ? RESAMPLE_PATH_LDS
                          : (one_fits && (a.mode == RESAMPLE_BOOTSTRAP || slices <= RESAMPLE_JACKKNIFE_MAX_SLICES) ? RESAMPLE_PATH_SLICED : RESAMPLE_PATH_GLOBAL);
    p.path = path;
    if (path == RESAMPLE_PATH_GLOBAL) {
        const AccumulateRule g = accumulate_rule(p.staged_bytes, p.cube_bytes, RESAMPLE_MATCH_BYTES, OBSERVE_PATH_GLOBAL);
        p.slice_reps = a.n_rep; p.n_slices = 1; p.lds_bytes = g.lds_bytes; p.groups_per_cu = g.groups_per_cu;
    } else {
        p.slice_reps = reps; p.n_slices = slices;
        p.lds_bytes = p.staged_bytes + (size_t)reps * p.replica_bytes;
        p.groups_per_cu = OBSERVE_LDS_GROUPS_PER_CU;
    }
    *plan = p;
    return RESAMPLE_OK;
}

// The grid.  x: workgroups of RESAMPLE_BLOCK lanes in a grid-stride loop over the slots; y: one row of them per slice (beyond RESAMPLE_MAX_GRID_Y
// slices a row takes several in turn).  With slices the workgroups a CU should hold (groups_per_cu) are shared among them, so that all slices stream
// side by side and each walks the slots with fewer workgroups.  The launch itself is one-dimensional, x * y workgroups: workgroup b is number
// b % x of row b / x (launch.hpp, ResampleDev).
struct ResampleGrid { int x, y; };
inline ResampleGrid resample_grid(const ResamplePlan &p, int n_slots, int cus)
{
    ResampleGrid g{};
    g.y = p.n_slices < RESAMPLE_MAX_GRID_Y ? p.n_slices : RESAMPLE_MAX_GRID_Y;
    g.x = accumulate_grid(n_slots, RESAMPLE_BLOCK, cus, p.groups_per_cu, RESAMPLE_MAX_GRID);
    if (g.y > 1 && g.x > 1) {
        const int share = (g.x + g.y - 1) / g.y;
        g.x = share > 1 ? share : 1;
    }
    return g;
}

}  // namespace mcrat
