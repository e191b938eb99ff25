// observe_plan.hpp -- the host's rules for a mock observation (mcrat_hip_observe, mcrat_hip_pool_observe): the argument checks and their texts, the
// layout of the cube on the device, the rule that picks the accumulation path, and the three per-photon functions -- accepted, t_det, find_bin --
// written once here and used by the kernel (observe.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can
// drive them (tests/test_observe_plan_cpu.py).
//
// Definitions.  The polar axis is r2 / p3.  A slot is observable when it has FLAG_VALID, weight != 0 and a type that is
// neither 'p' (pool photon) nor 'N' (null photon).  Observer o accepts a photon when  p3 <= p0 * cos_lo[o] && p3 > p0 * cos_hi[o]  (a cone given by
// two cosines, cos_lo > cos_hi; cones may overlap).  Its energy is  e = p0 * C_LIGHT  [erg], its detection time
//     t_det = time_now - ((r2 * cos_obs[o] + sqrt(r0 * r0 + r1 * r1) * sin_obs[o]) / C_LIGHT)
// and bin k of an axis holds  edges[k] <= x < edges[k + 1], found by comparisons alone.  Every expression is written in exactly this order and the
// build keeps -ffp-contract=off, so what decides a bin is bit-identical here, in the kernel and in NumPy: counts are exact.  The six sums per bin
// (W, WE, I, Q, U, V) are added with floating-point atomics in whatever order the hardware serves them: they differ in the last bits from run to
// run, each within  (m + 2) * 2^-53 * sum|term|  of the exact sum of the bin's m terms.
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "device_types.hpp"

#if defined(__HIPCC__)
#define MCRAT_OBS_HD __host__ __device__
#else
#define MCRAT_OBS_HD
#endif

namespace mcrat {

// ------------------------------------------------------------------ refusals and their texts
enum ObserveRefusal {
    OBSERVE_OK = 0,
    OBSERVE_NO_BINS,                 // n_obs, n_t or n_e < 1
    OBSERVE_TOO_MANY_BINS,           // n_obs * n_t * n_e does not fit an int
    OBSERVE_BAD_CONE,                // cos_lo <= cos_hi (or not a number)
    OBSERVE_T_EDGES_NOT_FINITE,
    OBSERVE_T_EDGES_NOT_ASCENDING,
    OBSERVE_E_EDGES_NOT_FINITE,
    OBSERVE_E_EDGES_NOT_ASCENDING,
    OBSERVE_STAGING_TOO_LARGE,       // the edges and the observers' cosines do not fit the LDS budget
    OBSERVE_BAD_PATH_SWITCH,         // MCRAT_HIP_OBSERVE_PATH is neither lds nor global
    OBSERVE_LDS_FORCED_TOO_LARGE     // MCRAT_HIP_OBSERVE_PATH=lds with a cube beyond the LDS budget
};
inline const char *observe_refusal_text(ObserveRefusal why)
{
    switch (why) {
    case OBSERVE_OK: return "";
    case OBSERVE_NO_BINS: return "observe: n_obs, n_t and n_e must each be at least 1";
    case OBSERVE_TOO_MANY_BINS: return "observe: n_obs * n_t * n_e overflows an int";
    case OBSERVE_BAD_CONE: return "observe: an observer's cone needs cos_lo > cos_hi";
    case OBSERVE_T_EDGES_NOT_FINITE: return "observe: t_edges holds a value that is not finite";
    case OBSERVE_T_EDGES_NOT_ASCENDING: return "observe: t_edges is not strictly ascending";
    case OBSERVE_E_EDGES_NOT_FINITE: return "observe: e_edges holds a value that is not finite";
    case OBSERVE_E_EDGES_NOT_ASCENDING: return "observe: e_edges is not strictly ascending";
    case OBSERVE_STAGING_TOO_LARGE: return "observe: the edges and the observers' cosines do not fit the kernel's LDS budget";
    case OBSERVE_BAD_PATH_SWITCH: return "observe: MCRAT_HIP_OBSERVE_PATH must be lds or global";
    case OBSERVE_LDS_FORCED_TOO_LARGE: return "observe: MCRAT_HIP_OBSERVE_PATH=lds, but the cube does not fit the kernel's LDS budget";
    }
    return "";
}

// ------------------------------------------------------------------ the cube and where it is accumulated
// Seven planes of 8 bytes per bin -- count (integer), W, WE, I, Q, U, V -- each [n_obs][n_t][n_e], observer-major then time then energy, followed by
// the per-observer counters n_accepted[n_obs], n_outside[n_obs]: one block, zeroed by one memset.  Behind it the kernel's inputs, in the order it
// stages them into LDS: cos_obs, sin_obs, cos_lo, cos_hi [n_obs each], t_edges [n_t + 1], e_edges [n_e + 1]; then the lists' clocks [n_clocks].
constexpr int OBSERVE_PLANES = 7;
enum ObservePlane { OBS_COUNT = 0, OBS_W, OBS_WE, OBS_I, OBS_Q, OBS_U, OBS_V };
// A workgroup's LDS: 160 KiB per CU on gfx950, so half of it still lets two workgroups share a CU -- one streams while the other flushes.
constexpr size_t OBSERVE_LDS_PER_CU = 160 * 1024;
constexpr size_t OBSERVE_LDS_BUDGET = OBSERVE_LDS_PER_CU / 2;
// Workgroups of 256 threads the grid is sized for, per CU: eight fill a CU's 32 wavefront slots.
constexpr int OBSERVE_MAX_GROUPS_PER_CU = 8;
constexpr int OBSERVE_LDS_GROUPS_PER_CU = 2;
enum ObservePath { OBSERVE_PATH_NONE = 0, OBSERVE_PATH_LDS = 1, OBSERVE_PATH_GLOBAL = 2 };
constexpr int OBSERVE_BLOCK = 256;               // threads per workgroup of every binned-sum kernel: one lane per slot and trip
// global path of observe_sky and radiation_field: a wavefront's table of 2048 one-byte lane numbers that tells which of its lanes share a bin
// (bin_accumulate.hpp, match_alone), one table per wavefront of the workgroup, and the entry a bin goes to
constexpr int OBSERVE_MATCH_BITS = 11;
constexpr size_t OBSERVE_MATCH_BYTES = (size_t)(OBSERVE_BLOCK / 64) << OBSERVE_MATCH_BITS;
MCRAT_OBS_HD inline unsigned observe_match_hash(int bin) { return ((unsigned)bin * 2654435761u) >> (32 - OBSERVE_MATCH_BITS); }

struct ObservePlan {
    int n_obs, n_t, n_e, n_bins;         // n_bins = n_obs * n_t * n_e
    size_t cube_bytes;                   // the seven planes
    size_t out_bytes;                    // ... and the per-observer counters: what is zeroed, and what the kernel adds into
    size_t staged_doubles;               // cosines and edges
    size_t staged_bytes;                 // ... and, in LDS, the workgroup's per-observer counters behind them
    size_t lds_bytes;                    // the kernel's dynamic LDS on the chosen path
    int groups_per_cu;                   // workgroups the grid is sized for per CU: two on the LDS path, up to eight on the global path
    ObservePath path;
};
MCRAT_OBS_HD inline size_t observe_bin(int o, int it, int ie, int n_t, int n_e) { return ((size_t)o * (size_t)n_t + (size_t)it) * (size_t)n_e + (size_t)ie; }

// MCRAT_HIP_OBSERVE_PATH: unset or empty -- the rule decides (OBSERVE_PATH_NONE); lds, global -- that path; anything else is refused
inline ObserveRefusal observe_path_switch(const char *env, ObservePath *forced)
{
    *forced = OBSERVE_PATH_NONE;
    if (!env || !*env) return OBSERVE_OK;
    if (!strcmp(env, "lds")) *forced = OBSERVE_PATH_LDS;
    else if (!strcmp(env, "global")) *forced = OBSERVE_PATH_GLOBAL;
    else return OBSERVE_BAD_PATH_SWITCH;
    return OBSERVE_OK;
}

// An axis' edges[0 .. n]: all finite, then strictly ascending -- which of the two failed; every product maps that to its own refusal.
enum EdgesFault { EDGES_OK = 0, EDGES_NOT_FINITE, EDGES_NOT_ASCENDING };
inline EdgesFault edges_check(const double *edges, int n)
{
    for (int k = 0; k <= n; ++k)
        if (!isfinite(edges[k])) return EDGES_NOT_FINITE;
    for (int k = 0; k < n; ++k)
        if (!(edges[k] < edges[k + 1])) return EDGES_NOT_ASCENDING;
    return EDGES_OK;
}
template <class Refusal>
inline Refusal edges_refusal(const double *edges, int n, Refusal ok, Refusal not_finite, Refusal not_ascending)
{
    const EdgesFault f = edges_check(edges, n);
    return f == EDGES_OK ? ok : (f == EDGES_NOT_FINITE ? not_finite : not_ascending);
}

// Where a binned sum is accumulated (observe, observe_sky, radiation_field): in the workgroup's LDS when the staged inputs with the counters behind
// them (staged_bytes) and the whole accumulator (acc_bytes) fit the budget, in global memory otherwise, unless `forced` says which -- forced LDS
// without `fits` is the caller's to refuse.  lds_bytes: behind the staged part the accumulator (LDS) or the wavefronts' match tables (global;
// match_bytes, 0 for a kernel without them).  groups_per_cu, LDS path: two, whatever would fit.  Every workgroup flushes its bins to the same
// addresses and the memory side serves the atomics of one address one after the other, so more workgroups cost more at the flush than they win
// streaming (1 x 1 x 64 on 10^6 photons: 88.6 us with eight per CU against 31.8 us with two).  Global path: as many as share a
// CU's LDS, at most eight.
struct AccumulateRule {
    bool fits;
    ObservePath path;
    size_t lds_bytes;
    int groups_per_cu;
};
inline AccumulateRule accumulate_rule(size_t staged_bytes, size_t acc_bytes, size_t match_bytes, ObservePath forced)
{
    AccumulateRule r{};
    r.fits = staged_bytes + acc_bytes <= OBSERVE_LDS_BUDGET;
    r.path = forced != OBSERVE_PATH_NONE ? forced : (r.fits ? OBSERVE_PATH_LDS : OBSERVE_PATH_GLOBAL);
    r.lds_bytes = staged_bytes + (r.path == OBSERVE_PATH_LDS ? acc_bytes : match_bytes);
    const size_t share = OBSERVE_LDS_PER_CU / r.lds_bytes;       // (0 < lds_bytes; within the budget: 2 or more)
    r.groups_per_cu = r.path == OBSERVE_PATH_LDS ? OBSERVE_LDS_GROUPS_PER_CU
                                                 : (share < (size_t)OBSERVE_MAX_GROUPS_PER_CU ? (int)share : OBSERVE_MAX_GROUPS_PER_CU);
    return r;
}

// workgroups of `block` lanes for a grid-stride loop over n items: what covers them, at most groups_per_cu per CU and never more than hard_max (> 0)
inline int accumulate_grid(long long n, int block, int cus, int groups_per_cu, int hard_max = 0)
{
    const long long want = (n + block - 1) / block;
    long long cap = (long long)(cus > 0 ? cus : 256) * groups_per_cu;
    if (hard_max > 0 && cap > hard_max) cap = hard_max;
    return (int)(want < cap ? want : cap);
}

// The checks, in this order: the counts, their product, the cones, the time edges, the energy edges, what must fit LDS; then the path -- LDS when
// the staged inputs, the counters and the whole cube fit the budget, global otherwise, unless `forced` says which.  *plan is filled when OBSERVE_OK.
inline ObserveRefusal observe_plan(int n_obs, const double *cos_lo, const double *cos_hi, int n_t, const double *t_edges, int n_e, const double *e_edges,
                                   ObservePath forced, ObservePlan *plan)
{
    if (n_obs < 1 || n_t < 1 || n_e < 1) return OBSERVE_NO_BINS;
    const long long per_obs = (long long)n_t * (long long)n_e;
    if (per_obs > INT_MAX || per_obs * (long long)n_obs > INT_MAX) return OBSERVE_TOO_MANY_BINS;
    for (int o = 0; o < n_obs; ++o)
        if (!(cos_lo[o] > cos_hi[o])) return OBSERVE_BAD_CONE;
    ObserveRefusal why = edges_refusal(t_edges, n_t, OBSERVE_OK, OBSERVE_T_EDGES_NOT_FINITE, OBSERVE_T_EDGES_NOT_ASCENDING);
    if (why == OBSERVE_OK) why = edges_refusal(e_edges, n_e, OBSERVE_OK, OBSERVE_E_EDGES_NOT_FINITE, OBSERVE_E_EDGES_NOT_ASCENDING);
    if (why != OBSERVE_OK) return why;
    ObservePlan p{};
    p.n_obs = n_obs; p.n_t = n_t; p.n_e = n_e; p.n_bins = (int)(per_obs * n_obs);
    p.cube_bytes = (size_t)OBSERVE_PLANES * 8 * (size_t)p.n_bins;
    p.out_bytes = p.cube_bytes + (size_t)2 * 8 * (size_t)n_obs;
    p.staged_doubles = (size_t)4 * n_obs + (size_t)n_t + 1 + (size_t)n_e + 1;
    p.staged_bytes = 8 * p.staged_doubles + (size_t)2 * 8 * (size_t)n_obs;
    if (p.staged_bytes > OBSERVE_LDS_BUDGET) return OBSERVE_STAGING_TOO_LARGE;
    const AccumulateRule r = accumulate_rule(p.staged_bytes, p.cube_bytes, 0, forced);
    if (forced == OBSERVE_PATH_LDS && !r.fits) return OBSERVE_LDS_FORCED_TOO_LARGE;
    p.path = r.path; p.lds_bytes = r.lds_bytes; p.groups_per_cu = r.groups_per_cu;
    *plan = p;
    return OBSERVE_OK;
}

// ------------------------------------------------------------------ one photon (host and device)
MCRAT_OBS_HD inline bool observe_observable(unsigned flags, char type, double weight)
{
    return (flags & FLAG_VALID) != 0 && weight != 0 && type != 'p' && type != 'N';
}
MCRAT_OBS_HD inline bool observe_accepted(double p0, double p3, double cos_lo, double cos_hi)
{
    return p3 <= p0 * cos_lo && p3 > p0 * cos_hi;
}
MCRAT_OBS_HD inline double observe_energy(double p0) { return p0 * C_LIGHT; }
MCRAT_OBS_HD inline double observe_t_det(double time_now, double r0, double r1, double r2, double cos_obs, double sin_obs)
{
    return time_now - ((r2 * cos_obs + sqrt(r0 * r0 + r1 * r1) * sin_obs) / C_LIGHT);
}
// the bin k of edges[0 .. n] with edges[k] <= x < edges[k + 1], or -1 (x outside, or not a number): comparisons only
MCRAT_OBS_HD inline int observe_find_bin(const double *edges, int n, double x)
{
    if (!(x >= edges[0]) || !(x < edges[n])) return -1;
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (x >= edges[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace mcrat
