// sightline.hip -- line-of-sight optical depths and photospheres on the device (mcrat_hip_sightline_rays, mcrat_hip_sightline_photons,
// mcrat_hip_pool_sightline_photons): every ray marched straight through the staged frame with the per-ray rules of sightline_plan.hpp and the
// loop's own cell look-up and optical depth (physics.hpp).  One lane per ray, 256-thread workgroups.  A step is two dependent gathers -- the
// bucket's record (16 B), then one bucket-list entry (128 B), which holds everything the step needs from the cell (TABLE adds the cell's
// temperature) -- and some forty f64 operations between them: the kernel is bound by the latency of those gathers.  There is no same-cell
// shortcut: a frame may keep covered coarse cells, and "still inside the entry I hold" does not prove "lowest-index containing cell".
//
// A lane is a small state machine: idle, marching (phase 1), or marching a second time to find the surface (phase 2: the march is deterministic,
// so the partial sums S_k come out bit for bit, and the ray's total T is known by then).  Both phases share one step body, sightline_step
// (sightline_march.hpp), which the escape-weighted observation's march calls too.
// Two forms of handing rays to lanes, same outputs per ray:
//   plain    lane i of the grid takes ray i; a wavefront idles on its longest ray.
//   refill   a lane whose ray has ended takes the next unclaimed ray: from its workgroup's own range first (an LDS counter), then from one global
//            counter that serves the last quarter of the rays to whoever runs dry.  One atomic per wavefront and claim, nobody waits for anybody.
// The per-status counts are kept in LDS and leave the workgroup as one integer atomic per status.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "physics.hpp"
#include "sightline_plan.hpp"
#include "sightline_march.hpp"

namespace mcrat {

namespace {

template <bool FROM_COLUMNS>
__device__ __forceinline__ void ray_origin(const PhotonDev &ph, const SightlineDev &a, int i, double &x, double &y, double &z)
{
    if constexpr (FROM_COLUMNS) {
        x = ph.r0[i]; y = ph.r1[i]; z = ph.r2[i];
    } else {
        const size_t n = (size_t)a.n;
        x = a.ray[i]; y = a.ray[n + i]; z = a.ray[2 * n + i];
    }
}
template <bool FROM_COLUMNS>
__device__ __forceinline__ void ray_momentum(const PhotonDev &ph, const SightlineDev &a, int i, double p[4])
{
    if constexpr (FROM_COLUMNS) {
        p[0] = ph.p0[i]; p[1] = ph.p1[i]; p[2] = ph.p2[i]; p[3] = ph.p3[i];
    } else {
        const size_t n = (size_t)a.n;
        p[0] = a.ray[3 * n + i]; p[1] = a.ray[4 * n + i]; p[2] = a.ray[5 * n + i]; p[3] = a.ray[6 * n + i];
    }
}

__device__ __forceinline__ void write_surface(const SightlineDev &a, int i, int step, double x, double y, double z)
{
    const size_t n = (size_t)a.n;
    a.i4[SL_SURFACE_STEP * n + i] = step;
    a.f8[SL_SURFACE_R0 * n + i] = x; a.f8[SL_SURFACE_R1 * n + i] = y; a.f8[SL_SURFACE_R2 * n + i] = z;
}
__device__ __forceinline__ void write_march(const SightlineDev &a, int i, double tau, double path, int steps, int status)
{
    const size_t n = (size_t)a.n;
    a.f8[SL_TAU * n + i] = tau; a.f8[SL_PATH * n + i] = path;
    a.i4[SL_STEPS * n + i] = steps; a.i4[SL_STATUS * n + i] = status;
}

template <int DIMS, int GEOM, bool TABLE, bool FROM_COLUMNS>
__global__ __launch_bounds__(SIGHTLINE_BLOCK) void sightline_kernel(PhotonDev ph, HydroDev hy, SightlineDev a)
{
    __shared__ unsigned s_count[SIGHTLINE_N_STATUS];
    __shared__ unsigned s_next;
    const int tid = threadIdx.x, lane = tid & 63;
    // refill form: this workgroup's own range, and where the shared rest begins
    const unsigned own_lo = blockIdx.x * (unsigned)a.own_rays, own_hi = own_lo + (unsigned)a.own_rays;      // (<= n < 2^31)
    const unsigned shared_lo = gridDim.x * (unsigned)a.own_rays, n = (unsigned)a.n;
    if (tid < SIGHTLINE_N_STATUS) s_count[tid] = 0u;
    if (tid == 0) s_next = own_lo;
    __syncthreads();

    const double nan = __builtin_nan("");
    int ray = -1, phase = 0, k = 0, k_total = 0;         // ray < 0: the lane is idle
    double x = 0, y = 0, z = 0, nx = 0, ny = 0, nz = 0, tau = 0, path = 0, tau_total = 0;
    double p[4] = {0, 0, 0, 0};
    bool dry = false, own_dry = a.own_rays == 0;         // (both the same in every lane of a wavefront) no unclaimed ray is left: anywhere, in the own range

    for (;;) {
        if (!dry) {
            const unsigned long long idle = __ballot(ray < 0);
            if (idle) {
                int got = -1;
                if (!a.refill) {
                    const unsigned i = blockIdx.x * (unsigned)SIGHTLINE_BLOCK + (unsigned)tid;
                    if (i < n) got = (int)i;
                    dry = true;
                } else {
                    const unsigned long long below = (1ull << lane) - 1ull;
                    if (!own_dry) {
                        const int leader = __ffsll((long long)idle) - 1;
                        const unsigned want = (unsigned)__popcll(idle);
                        unsigned base = 0;
                        if (lane == leader) base = atomicAdd(&s_next, want);
                        base = __shfl(base, leader, 64);
                        const unsigned i = base + (unsigned)__popcll(idle & below);
                        if (ray < 0 && i < own_hi) got = (int)i;
                        own_dry = base + want >= own_hi;
                    }
                    const unsigned long long unserved = __ballot(ray < 0 && got < 0);
                    if (unserved) {
                        const int leader = __ffsll((long long)unserved) - 1;
                        const unsigned long long want = (unsigned long long)__popcll(unserved);
                        unsigned long long base = 0;
                        if (lane == leader) base = atomicAdd(&a.head[SIGHTLINE_COUNTER_WORD], want);
                        base = __shfl(base, leader, 64);
                        const unsigned long long i = (unsigned long long)shared_lo + base + (unsigned long long)__popcll(unserved & below);
                        if (ray < 0 && got < 0 && i < (unsigned long long)n) got = (int)i;
                        dry = (unsigned long long)shared_lo + base + want >= (unsigned long long)n;
                    }
                }
                if (got >= 0) {
                    bool march = true;
                    if constexpr (FROM_COLUMNS) march = observe_observable(ph.flags[got], ph.type[got], ph.weight[got]);
                    if (march) {
                        ray = got; phase = 1; k = 0; tau = 0; path = 0;
                        ray_origin<FROM_COLUMNS>(ph, a, got, x, y, z);
                        ray_momentum<FROM_COLUMNS>(ph, a, got, p);
                        sightline_direction(p[1], p[2], p[3], nx, ny, nz);
                    } else {
                        write_march(a, got, 0.0, 0.0, 0, SIGHTLINE_SKIPPED);
                        write_surface(a, got, -1, nan, nan, nan);
                        atomicAdd(&s_count[SIGHTLINE_SKIPPED], 1u);
                    }
                }
            }
        }
        if (dry && !__ballot(ray >= 0)) break;            // (a wavefront whose claim brought only skipped slots claims again)
        if (ray >= 0) {
            int status = -1;                                  // >= 0: phase 1 ends here with this status
            bool surface_done = false;                        // phase 2 ends here
            if (phase == 1) {
                if (k == a.max_steps) status = SIGHTLINE_STEP_CAP;
            } else if (sightline_surface_reached(tau_total, tau, a.surface_level)) {
                write_surface(a, ray, k, x, y, z);
                surface_done = true;
            } else if (k == k_total) {                        // (a total that is not a number: no k satisfies the predicate)
                write_surface(a, ray, -1, nan, nan, nan);
                surface_done = true;
            }
            if (status < 0 && !surface_done) {
                status = sightline_step<DIMS, GEOM, TABLE>(hy, p, a.step_frac, a.h_min, nx, ny, nz, x, y, z, tau, path);
                if (status < 0) {                             // the step was counted
                    k += 1;
                    if (phase == 1 && tau >= a.tau_stop) status = SIGHTLINE_OPAQUE;
                }
                if (phase == 2 && status >= 0) {              // (cannot happen: phase 2 repeats steps that phase 1 has counted)
                    write_surface(a, ray, -1, nan, nan, nan);
                    surface_done = true;
                }
            }
            if (phase == 1 && status >= 0) {
                write_march(a, ray, tau, path, k, status);
                atomicAdd(&s_count[status], 1u);
                if (a.surface_level >= 0 && status == SIGHTLINE_LEFT_MESH) {
                    phase = 2; tau_total = tau; k_total = k;
                    k = 0; tau = 0; path = 0;
                    ray_origin<FROM_COLUMNS>(ph, a, ray, x, y, z);
                } else {
                    write_surface(a, ray, -1, nan, nan, nan);
                    ray = -1;
                }
            } else if (surface_done) {
                ray = -1;
            }
        }
    }
    __syncthreads();
    if (tid < SIGHTLINE_N_STATUS && s_count[tid]) atomicAdd(&a.head[tid], (unsigned long long)s_count[tid]);
}

template <int DIMS, int GEOM>
hipError_t launch_pair(bool table, const PhotonDev &ph, const HydroDev &hy, const SightlineDev &a, int blocks, hipStream_t stream)
{
    const dim3 grid(blocks), block(SIGHTLINE_BLOCK);
    const bool columns = a.ray == nullptr;
    if (table) {
        if (columns) hipLaunchKernelGGL((sightline_kernel<DIMS, GEOM, true, true>), grid, block, 0, stream, ph, hy, a);
        else hipLaunchKernelGGL((sightline_kernel<DIMS, GEOM, true, false>), grid, block, 0, stream, ph, hy, a);
    } else {
        if (columns) hipLaunchKernelGGL((sightline_kernel<DIMS, GEOM, false, true>), grid, block, 0, stream, ph, hy, a);
        else hipLaunchKernelGGL((sightline_kernel<DIMS, GEOM, false, false>), grid, block, 0, stream, ph, hy, a);
    }
    return hipGetLastError();
}

}  // namespace

// The nine (DIMENSIONS, geometry) pairs the engine accepts (engine.hip, geometry_supported), as functions.hip switches over them; a.ray == nullptr:
// the rays are the photon columns.  The caller has zeroed the block's head and sized the grid (sightline_plan.hpp, sightline_grid).
hipError_t launch_sightline(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const SightlineDev &a, int blocks, hipStream_t stream)
{
    if (a.n <= 0 || blocks <= 0) return hipErrorInvalidValue;
    const bool table = kc.table != 0;
    switch (kc.dimensions * 4 + kc.geometry) {
    case DIM_TWO * 4 + GEOM_CARTESIAN: return launch_pair<DIM_TWO, GEOM_CARTESIAN>(table, ph, hy, a, blocks, stream);
    case DIM_TWO * 4 + GEOM_CYLINDRICAL: return launch_pair<DIM_TWO, GEOM_CYLINDRICAL>(table, ph, hy, a, blocks, stream);
    case DIM_TWO * 4 + GEOM_SPHERICAL: return launch_pair<DIM_TWO, GEOM_SPHERICAL>(table, ph, hy, a, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CARTESIAN: return launch_pair<DIM_TWO_POINT_FIVE, GEOM_CARTESIAN>(table, ph, hy, a, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CYLINDRICAL: return launch_pair<DIM_TWO_POINT_FIVE, GEOM_CYLINDRICAL>(table, ph, hy, a, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_SPHERICAL: return launch_pair<DIM_TWO_POINT_FIVE, GEOM_SPHERICAL>(table, ph, hy, a, blocks, stream);
    case DIM_THREE * 4 + GEOM_CARTESIAN: return launch_pair<DIM_THREE, GEOM_CARTESIAN>(table, ph, hy, a, blocks, stream);
    case DIM_THREE * 4 + GEOM_SPHERICAL: return launch_pair<DIM_THREE, GEOM_SPHERICAL>(table, ph, hy, a, blocks, stream);
    case DIM_THREE * 4 + GEOM_POLAR: return launch_pair<DIM_THREE, GEOM_POLAR>(table, ph, hy, a, blocks, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mcrat
