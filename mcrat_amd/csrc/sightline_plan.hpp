// sightline_plan.hpp -- the host's rules for line-of-sight optical depths (mcrat_hip_sightline_rays, mcrat_hip_sightline_photons,
// mcrat_hip_pool_sightline_photons): the argument checks and their texts, the status values, the layout of the output block on the device, the
// rule that sizes the grid, and the per-ray functions -- direction, step length, midpoint, advance, surface predicate -- written once here and
// called by the kernel (sightline.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them
// (tests/test_sightline_plan_cpu.py).
//
// Definitions.  A sightline is the straight ray from x_0 = (r0, r1, r2) along the unit vector of a photon 4-momentum
// (p0, p1, p2, p3) through ONE frozen staged hydro frame, the fluid piecewise constant per cell and sampled at step midpoints:
//     ipn = 1 / sqrt((p1*p1 + p2*p2) + p3*p3);   n = (p1*ipn, p2*ipn, p3*ipn);   tau = 0;  path = 0;  k = 0
//     loop:  k == max_steps                                      -> STEP_CAP
//            rho = sqrt((x*x + y*y) + z*z);  h = step_frac * rho;  if (!(h > h_min)) h = h_min
//            m = (x + (0.5*h)*n_x, y + (0.5*h)*n_y, z + (0.5*h)*n_z)
//            m outside the domain (the loop's strict test), or in no cell   -> LEFT_MESH
//            kappa [1/cm] of the lowest-index cell that holds m, at the azimuth of m; TABLE: look-up off the table -> OFF_TABLE
//            tau += kappa*h;  path += h;  x += h*n_x;  y += h*n_y;  z += h*n_z;  k += 1
//            tau >= tau_stop                                     -> OPAQUE
// Every expression is written in exactly this order, `/` and sqrt are the correctly rounded ones and the build keeps -ffp-contract=off, so the
// positions -- and with them steps, path and every decision that does not hang on tau -- are bit-identical here, in the kernel and in NumPy.
// Surface (surface_level >= 0): for a ray that LEFT_MESH with total T and partial sums S_k (tau after k counted steps, S_0 = 0), surface_step is
// the smallest k with (T - S_k) <= surface_level and surface_r = x_k.  The march is deterministic, so a second march reproduces S_k bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "device_types.hpp"

#if defined(__HIPCC__)
#define MCRAT_SL_HD __host__ __device__
#else
#define MCRAT_SL_HD
#endif

namespace mcrat {

// ------------------------------------------------------------------ refusals and their texts
enum SightlineRefusal {
    SIGHTLINE_OK = 0,
    SIGHTLINE_NO_RAYS,               // n <= 0
    SIGHTLINE_BAD_STEP_FRAC,         // negative or not finite
    SIGHTLINE_BAD_H_MIN,             // not finite or <= 0
    SIGHTLINE_BAD_MAX_STEPS,         // outside 1 .. 2^20
    SIGHTLINE_BAD_TAU_STOP,          // NaN or <= 0 (+inf: never opaque)
    SIGHTLINE_BAD_SURFACE_LEVEL,     // NaN or +inf (negative: no surface)
    SIGHTLINE_BAD_REFILL_SWITCH      // MCRAT_HIP_SIGHTLINE_REFILL is neither 0 nor 1
};
inline const char *sightline_refusal_text(SightlineRefusal why)
{
    switch (why) {
    case SIGHTLINE_OK: return "";
    case SIGHTLINE_NO_RAYS: return "sightline: n must be at least 1";
    case SIGHTLINE_BAD_STEP_FRAC: return "sightline: step_frac must be finite and not negative";
    case SIGHTLINE_BAD_H_MIN: return "sightline: h_min must be finite and positive";
    case SIGHTLINE_BAD_MAX_STEPS: return "sightline: max_steps must lie between 1 and 1048576";
    case SIGHTLINE_BAD_TAU_STOP: return "sightline: tau_stop must be positive (+inf: never opaque)";
    case SIGHTLINE_BAD_SURFACE_LEVEL: return "sightline: surface_level must be a number below +inf (negative: no surface)";
    case SIGHTLINE_BAD_REFILL_SWITCH: return "sightline: MCRAT_HIP_SIGHTLINE_REFILL must be 0 or 1";
    }
    return "";
}

// ------------------------------------------------------------------ how a ray ended
enum SightlineStatus {
    SIGHTLINE_SKIPPED = 0,           // a resident slot that is not observable (observe_plan.hpp, observe_observable): nothing was marched
    SIGHTLINE_LEFT_MESH = 1,         // a midpoint outside the domain or in no cell: tau is the optical depth to the edge of the frame
    SIGHTLINE_OPAQUE = 2,            // tau >= tau_stop
    SIGHTLINE_STEP_CAP = 3,          // max_steps steps were counted
    SIGHTLINE_OFF_TABLE = 4          // TABLE: a look-up the reference would integrate afresh; tau up to there
};
constexpr int SIGHTLINE_N_STATUS = 5;
constexpr int SIGHTLINE_MAX_STEPS = 1 << 20;

struct SightlineParams {
    double step_frac, h_min;
    int max_steps;
    double tau_stop, surface_level;
};

// ------------------------------------------------------------------ the output block and the grid
// One block, zeroed by one memset: the five status counts and the refill form's global ray counter (eight 8-byte words), then five planes of n
// doubles -- tau, path, surface_r0, surface_r1, surface_r2 -- then three planes of n ints -- steps, status, surface_step.  Behind it, for caller
// rays, the seven input planes r0, r1, r2, p0, p1, p2, p3 of n doubles each.
constexpr int SIGHTLINE_BLOCK = 256;             // threads per workgroup: one lane per ray
constexpr int SIGHTLINE_HEAD_WORDS = 8;          // n_status[5], the ray counter, two spare
constexpr int SIGHTLINE_COUNTER_WORD = 5;
constexpr int SIGHTLINE_F8_PLANES = 5, SIGHTLINE_I4_PLANES = 3, SIGHTLINE_RAY_PLANES = 7;
enum SightlineF8Plane { SL_TAU = 0, SL_PATH, SL_SURFACE_R0, SL_SURFACE_R1, SL_SURFACE_R2 };
enum SightlineI4Plane { SL_STEPS = 0, SL_STATUS, SL_SURFACE_STEP };
// Workgroups per CU the refill form's grid is sized for: four of 256 threads are the sixteen wavefronts a CU holds at up to 128 VGPRs.
constexpr int SIGHTLINE_GROUPS_PER_CU = 4;
// The refill form's split: three quarters of the rays, in whole wavefronts, are dealt to the workgroups as ranges of their own (claimed through
// an LDS counter); the last quarter is claimed from one global counter by whoever runs dry first.
constexpr int SIGHTLINE_OWN_NUM = 3, SIGHTLINE_OWN_DEN = 4;

struct SightlinePlan {
    int n;
    SightlineParams p;
    bool refill;                         // lanes whose ray has ended take the next unclaimed ray
    size_t f8_offset, i4_offset;         // bytes from the block's start to the first double plane and the first int plane
    size_t out_bytes;                    // head and the eight output planes: what is zeroed and read back
    size_t ray_offset, ray_bytes;        // the caller's rays behind it (sightline_rays only)
};
MCRAT_SL_HD inline size_t sightline_f8_plane(const SightlinePlan &pl, int plane) { return pl.f8_offset + sizeof(double) * (size_t)plane * (size_t)pl.n; }
MCRAT_SL_HD inline size_t sightline_i4_plane(const SightlinePlan &pl, int plane) { return pl.i4_offset + sizeof(int) * (size_t)plane * (size_t)pl.n; }

// MCRAT_HIP_SIGHTLINE_REFILL: unset or empty -- the default form (-1); 0 the plain form, 1 lane refill; anything else is refused
inline SightlineRefusal sightline_refill_switch(const char *env, int *forced)
{
    *forced = -1;
    if (!env || !*env) return SIGHTLINE_OK;
    if (!strcmp(env, "0")) *forced = 0;
    else if (!strcmp(env, "1")) *forced = 1;
    else return SIGHTLINE_BAD_REFILL_SWITCH;
    return SIGHTLINE_OK;
}
// The default form.  Measured on the benchmark's cfg2 frame and on a dense jet with tau_stop = 20 (DESIGN.md section 6,
// profiles/sightline_forms.txt): refill becomes the default only where it wins on both by more than the run-to-run spread.
constexpr bool SIGHTLINE_REFILL_DEFAULT = false;

// The four parameters of the march itself, in this order: step_frac, h_min, max_steps, tau_stop (surface_level is not looked at).  Also what the
// escape-weighted observation checks of its march (escape_plan.hpp).
inline SightlineRefusal sightline_march_check(const SightlineParams &p)
{
    if (!isfinite(p.step_frac) || p.step_frac < 0) return SIGHTLINE_BAD_STEP_FRAC;
    if (!isfinite(p.h_min) || !(p.h_min > 0)) return SIGHTLINE_BAD_H_MIN;
    if (p.max_steps < 1 || p.max_steps > SIGHTLINE_MAX_STEPS) return SIGHTLINE_BAD_MAX_STEPS;
    if (!(p.tau_stop > 0)) return SIGHTLINE_BAD_TAU_STOP;
    return SIGHTLINE_OK;
}

// The checks, in this order: n, step_frac, h_min, max_steps, tau_stop, surface_level; then the switch.  *plan is filled when SIGHTLINE_OK.
inline SightlineRefusal sightline_plan(int n, const SightlineParams &p, int forced_refill, SightlinePlan *plan)
{
    if (n <= 0) return SIGHTLINE_NO_RAYS;
    const SightlineRefusal march = sightline_march_check(p);
    if (march != SIGHTLINE_OK) return march;
    if (!(p.surface_level < INFINITY)) return SIGHTLINE_BAD_SURFACE_LEVEL;
    SightlinePlan pl{};
    pl.n = n; pl.p = p;
    pl.refill = forced_refill < 0 ? SIGHTLINE_REFILL_DEFAULT : forced_refill != 0;
    pl.f8_offset = sizeof(unsigned long long) * SIGHTLINE_HEAD_WORDS;
    pl.i4_offset = pl.f8_offset + sizeof(double) * (size_t)SIGHTLINE_F8_PLANES * (size_t)n;
    pl.out_bytes = pl.i4_offset + sizeof(int) * (size_t)SIGHTLINE_I4_PLANES * (size_t)n;
    pl.ray_offset = (pl.out_bytes + 255) / 256 * 256;
    pl.ray_bytes = sizeof(double) * (size_t)SIGHTLINE_RAY_PLANES * (size_t)n;
    *plan = pl;
    return SIGHTLINE_OK;
}

// workgroups of SIGHTLINE_BLOCK lanes: one lane per ray in the plain form; in the refill form at most what the device holds at once
inline int sightline_grid(const SightlinePlan &pl, int cus)
{
    const long long want = ((long long)pl.n + SIGHTLINE_BLOCK - 1) / SIGHTLINE_BLOCK;
    if (!pl.refill) return (int)want;
    const long long cap = (long long)(cus > 0 ? cus : 256) * SIGHTLINE_GROUPS_PER_CU;
    return (int)(want < cap ? want : cap);
}
// refill form: rays per workgroup's own range, a multiple of 64; the ranges of `groups` workgroups lie first, the shared rest behind them
MCRAT_SL_HD inline int sightline_own_rays(int n, int groups)
{
    const long long own = (long long)n * SIGHTLINE_OWN_NUM / SIGHTLINE_OWN_DEN / groups;
    return (int)(own / 64 * 64);
}

// ------------------------------------------------------------------ one ray (host and device)
MCRAT_SL_HD inline void sightline_direction(double p1, double p2, double p3, double &nx, double &ny, double &nz)
{
    const double ipn = 1.0 / sqrt((p1 * p1 + p2 * p2) + p3 * p3);
    nx = p1 * ipn; ny = p2 * ipn; nz = p3 * ipn;
}
MCRAT_SL_HD inline double sightline_step_length(double x, double y, double z, double step_frac, double h_min)
{
    const double rho = sqrt((x * x + y * y) + z * z);
    double h = step_frac * rho;
    if (!(h > h_min)) h = h_min;
    return h;
}
MCRAT_SL_HD inline void sightline_midpoint(double x, double y, double z, double h, double nx, double ny, double nz, double &mx, double &my, double &mz)
{
    const double half = 0.5 * h;
    mx = x + half * nx; my = y + half * ny; mz = z + half * nz;
}
MCRAT_SL_HD inline void sightline_advance(double &x, double &y, double &z, double h, double nx, double ny, double nz)
{
    x += h * nx; y += h * ny; z += h * nz;
}
// from x_k on, at most `level` of optical depth is left to the edge of the frame (total: the ray's tau; partial: S_k)
MCRAT_SL_HD inline bool sightline_surface_reached(double total, double partial, double level) { return (total - partial) <= level; }

}  // namespace mcrat
