// escape.hip -- escape-weighted sky observations (mcrat_hip_observe_escaping, mcrat_hip_pool_observe_escaping): the resident photons that an
// observer accepts, marched to the edge of the staged frame and binned by observer, optical depth, detection time, energy and, optionally, their
// position on the observer's sky plane, the escape-weighted sums beside the raw ones.  The rules are escape_plan.hpp's, sky_plan.hpp's and
// sightline_plan.hpp's.  Three kernels on one stream, nothing on the host between them:
//   escape_select_kernel   streams the slots once -- flags, type, weight, p0 .. p3, 46 bytes coalesced; the observers' directions and cosines staged in
//                          LDS -- and gives every slot that is observable and accepted by any observer a place in a compacted list of slot
//                          numbers: a wavefront ballot, one atomic per wavefront on a device counter.  The list's order is unspecified; it only
//                          reorders sums.  Counts n_observable.
//   escape_march_kernel    one lane per list entry, the length read from the device counter: the march of sightline.hip, its step written once in
//                          sightline_march.hpp, so tau is that kernel's tau bit for bit.  The list is what makes the wavefronts dense in marching
//                          lanes: with a narrow cone most slots are nobody's, and a lane per slot would idle beside the few that march.  Lanes are
//                          not refilled within a wavefront (sightline.hip's plain form, its measured default): a workgroup that has ended gives
//                          its place to the next.  Writes tau and status per entry and the five n_status counters.
//   escape_bin_kernel      one lane per list entry in a grid-stride loop: gathers the photon by its slot number, goes through the observers one by
//                          one, applies escape_bin and adds the count and N sums -- W, WE, (Stokes on: I, Q, U, V,) WX, WEX -- with
//                          bin_accumulate.hpp's forms.  Photons are 3-D Cartesian whatever the run's DIMENSIONS and GEOMETRY, so only the march is
//                          instantiated per geometry: 1 + 18 + 8 kernels, not 144.
// Two accumulation paths, picked by the plan from the cube's size, as in sky.hip: LDS -- the workgroup's private copy of the cube, flushed once --
// and global -- hardware atomics into HBM after the wavefront has found out which of its lanes share a bin (match_alone, add_shared_bins).
// match_alone's rule holds: the list's length comes from the device counter, which every lane reads alike, so every lane of a workgroup makes the
// same trips over the list and over the observers.
// Every loop is bounded by the slot count, the observers, max_steps or the 64 lanes of a wavefront; no workgroup waits on another.
// Counts are exact.  The sums depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run; each stays
// within (m + 2) * 2^-53 * sum|term| of the exact sum of the bin's m terms.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "sightline_plan.hpp"
#include "escape_plan.hpp"
#include "physics.hpp"
#include "sightline_march.hpp"
#include "bin_accumulate.hpp"

namespace mcrat {

namespace {

// ------------------------------------------------------------------ 1. the slots that any observer accepts
__global__ __launch_bounds__(ESCAPE_BLOCK) void escape_select_kernel(PhotonDev ph, EscapeDev a)
{
    extern __shared__ double s_mem[];                 // n0, n1, n2, cos_acc [n_obs each]: the head of the staged inputs
    const int tid = threadIdx.x, lane = tid & 63, no = a.n_obs;
    for (int k = tid; k < 4 * no; k += ESCAPE_BLOCK) s_mem[k] = a.staged[k];
    __syncthreads();
    const double *s_n0 = s_mem, *s_n1 = s_n0 + no, *s_n2 = s_n1 + no, *s_cos_acc = s_n2 + no;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long observable = 0;                // this wavefront's count, the same in every lane
    const unsigned n = (unsigned)a.n_slots, stride = gridDim.x * ESCAPE_BLOCK;
    for (unsigned base = blockIdx.x * ESCAPE_BLOCK; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap)
        const unsigned i = base + tid;
        bool live = i < n;
        if (live) live = observe_observable(ph.flags[i], ph.type[i], ph.weight[i]);
        bool any = false;
        if (live) {
            const double p0 = ph.p0[i], p1 = ph.p1[i], p2 = ph.p2[i], p3 = ph.p3[i];
            for (int o = 0; o < no && !any; ++o) any = sky_accepted(p0, p1, p2, p3, s_n0[o], s_n1[o], s_n2[o], s_cos_acc[o]);
        }
        observable += (unsigned long long)__popcll(__ballot(live));
        const unsigned long long chosen = __ballot(any);
        if (chosen) {
            const int leader = __ffsll((long long)chosen) - 1;
            unsigned long long first = 0;
            if (lane == leader) first = atomicAdd(&a.head[ESCAPE_SELECTED_WORD], (unsigned long long)__popcll(chosen));
            first = __shfl(first, leader, 64);
            if (any) a.index[first + (unsigned long long)__popcll(chosen & below)] = (int)i;      // (at most n_slots places are ever given out)
        }
    }
    if (lane == 0 && observable) add_u64(&a.head[ESCAPE_OBSERVABLE_WORD], observable);
}

// ------------------------------------------------------------------ 2. their optical depths to the edge of the frame
template <int DIMS, int GEOM, bool TABLE>
__global__ __launch_bounds__(ESCAPE_BLOCK) void escape_march_kernel(PhotonDev ph, HydroDev hy, EscapeDev a)
{
    __shared__ unsigned s_count[SIGHTLINE_N_STATUS];
    const int tid = threadIdx.x;
    if (tid < SIGHTLINE_N_STATUS) s_count[tid] = 0u;
    __syncthreads();
    const unsigned m = (unsigned)a.head[ESCAPE_SELECTED_WORD];                            // (<= n_slots < 2^31; the selecting kernel has ended)
    const unsigned stride = gridDim.x * ESCAPE_BLOCK;                                     // (<= 2^24)
    for (unsigned long long j = blockIdx.x * (unsigned)ESCAPE_BLOCK + (unsigned)tid; j < m; j += stride) {
        const int i = a.index[j];
        double x = ph.r0[i], y = ph.r1[i], z = ph.r2[i], nx, ny, nz, tau = 0, path = 0;
        const double p[4] = {ph.p0[i], ph.p1[i], ph.p2[i], ph.p3[i]};
        sightline_direction(p[1], p[2], p[3], nx, ny, nz);
        int k = 0, status = -1;
        while (status < 0) {                                                              // (at most max_steps counted steps)
            if (k == a.max_steps) {
                status = SIGHTLINE_STEP_CAP;
            } else {
                status = sightline_step<DIMS, GEOM, TABLE>(hy, p, a.step_frac, a.h_min, nx, ny, nz, x, y, z, tau, path);
                if (status < 0) {
                    k += 1;
                    if (tau >= a.tau_stop) status = SIGHTLINE_OPAQUE;
                }
            }
        }
        a.tau[j] = tau;
        a.status[j] = status;
        atomicAdd(&s_count[status], 1u);
    }
    __syncthreads();
    if (tid < SIGHTLINE_N_STATUS && s_count[tid]) add_u64(&a.head[tid], (unsigned long long)s_count[tid]);
}

template <int DIMS, int GEOM>
hipError_t launch_march(bool table, const PhotonDev &ph, const HydroDev &hy, const EscapeDev &a, int blocks, hipStream_t stream)
{
    const dim3 grid(blocks), block(ESCAPE_BLOCK);
    if (table) hipLaunchKernelGGL((escape_march_kernel<DIMS, GEOM, true>), grid, block, 0, stream, ph, hy, a);
    else hipLaunchKernelGGL((escape_march_kernel<DIMS, GEOM, false>), grid, block, 0, stream, ph, hy, a);
    return hipGetLastError();
}

// the nine (DIMENSIONS, geometry) pairs the engine accepts, as launch_sightline switches over them
hipError_t launch_march_for(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const EscapeDev &a, int blocks, hipStream_t stream)
{
    const bool table = kc.table != 0;
    switch (kc.dimensions * 4 + kc.geometry) {
    case DIM_TWO * 4 + GEOM_CARTESIAN: return launch_march<DIM_TWO, GEOM_CARTESIAN>(table, ph, hy, a, blocks, stream);
    case DIM_TWO * 4 + GEOM_CYLINDRICAL: return launch_march<DIM_TWO, GEOM_CYLINDRICAL>(table, ph, hy, a, blocks, stream);
    case DIM_TWO * 4 + GEOM_SPHERICAL: return launch_march<DIM_TWO, GEOM_SPHERICAL>(table, ph, hy, a, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CARTESIAN: return launch_march<DIM_TWO_POINT_FIVE, GEOM_CARTESIAN>(table, ph, hy, a, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CYLINDRICAL: return launch_march<DIM_TWO_POINT_FIVE, GEOM_CYLINDRICAL>(table, ph, hy, a, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_SPHERICAL: return launch_march<DIM_TWO_POINT_FIVE, GEOM_SPHERICAL>(table, ph, hy, a, blocks, stream);
    case DIM_THREE * 4 + GEOM_CARTESIAN: return launch_march<DIM_THREE, GEOM_CARTESIAN>(table, ph, hy, a, blocks, stream);
    case DIM_THREE * 4 + GEOM_SPHERICAL: return launch_march<DIM_THREE, GEOM_SPHERICAL>(table, ph, hy, a, blocks, stream);
    case DIM_THREE * 4 + GEOM_POLAR: return launch_march<DIM_THREE, GEOM_POLAR>(table, ph, hy, a, blocks, stream);
    default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------ 3. the list into the cube
// The kernel's words per bin in its own order -- count, W, WE, (STOKES: I, Q, U, V,) WX, WEX -- onto the block's nine planes: with Stokes off the four
// planes in the middle are never touched and stay zero.  The planes' bases are worked out once (PlaneBases).
template <bool STOKES>
struct EscapeAt {
    PlaneBases<ESCAPE_PLANES> base;
    __device__ __forceinline__ EscapeAt(double *acc, size_t nb) : base(acc, nb) {}
    __device__ __forceinline__ double *operator()(int k, size_t bin) const { return base((STOKES || k <= ESC_WE) ? k : k + (ESC_WX - ESC_I), bin); }
};

template <bool LDS_CUBE, bool STOKES, bool IMAGE>
__global__ __launch_bounds__(ESCAPE_BLOCK) void escape_bin_kernel(PhotonDev ph, EscapeDev a)
{
    extern __shared__ double s_mem[];
    constexpr int N = STOKES ? 8 : 4, BLOCK = ESCAPE_BLOCK;
    const int tid = threadIdx.x, lane = tid & 63, no = a.n_obs;
    // the staged layout (escape_plan.hpp): sky_plan.hpp's, then tau_edges
    const double *s_n0 = s_mem, *s_n1 = s_n0 + no, *s_n2 = s_n1 + no, *s_cos_acc = s_n2 + no;
    const double *s_x0 = s_cos_acc + no, *s_x1 = s_x0 + no, *s_x2 = s_x1 + no, *s_y0 = s_x2 + no, *s_y1 = s_y0 + no, *s_y2 = s_y1 + no;      // (IMAGE)
    const double *s_t_edges = s_cos_acc + no + (IMAGE ? 6 * no : 0), *s_e_edges = s_t_edges + (a.n_t + 1);
    const double *s_x_edges = s_e_edges + (a.n_e + 1), *s_y_edges = s_x_edges + (a.n_x + 1);                                             // (IMAGE)
    const double *s_tau_edges = s_e_edges + (a.n_e + 1) + (IMAGE ? a.n_x + a.n_y + 2 : 0);
    const int n_x = IMAGE ? a.n_x : 0, n_y = IMAGE ? a.n_y : 0;
    const int n_staged = (IMAGE ? 10 : 4) * no + a.n_t + a.n_e + 2 + (IMAGE ? a.n_x + a.n_y + 2 : 0) + a.n_tau + 1;
    unsigned long long *s_counters = reinterpret_cast<unsigned long long *>(s_mem + n_staged);      // accepted, outside, opaque, unresolved: [n_obs] each
    double *s_cube = reinterpret_cast<double *>(s_counters + ESCAPE_COUNTERS * no);
    for (int k = tid; k < n_staged; k += BLOCK) s_mem[k] = a.staged[k];
    for (int k = tid; k < ESCAPE_COUNTERS * no; k += BLOCK) s_counters[k] = 0ull;
    const size_t nb = (size_t)a.n_bins;
    const PlaneMajor at_lds{s_cube, nb};                                                  // the workgroup's copy: N + 1 planes in the kernel's order
    const EscapeAt<STOKES> at(a.cube, nb);
    if constexpr (LDS_CUBE)
        for (size_t k = tid; k < (size_t)(N + 1) * nb; k += BLOCK) s_cube[k] = 0.0;       // (+0.0 and the integer 0 are the same bits)
    __syncthreads();
    unsigned char *s_match = nullptr;
    if constexpr (!LDS_CUBE) s_match = reinterpret_cast<unsigned char *>(s_cube) + ((size_t)(tid >> 6) << OBSERVE_MATCH_BITS);      // this wavefront's table

    const unsigned m = (unsigned)a.head[ESCAPE_SELECTED_WORD], stride = gridDim.x * BLOCK;      // (m <= n_slots < 2^31, the same in every lane)
    for (unsigned base = blockIdx.x * BLOCK; base < m; base += stride) {                  // (stride <= 2^19: no wrap; the same trips for every lane of the workgroup)
        const unsigned j = base + tid;
        const bool live = j < m;
        double w = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, clock = a.time_now, tau = 0;
        double p0 = 0, p1 = 0, p2 = 0, p3 = 0, r0 = 0, r1 = 0, r2 = 0;
        int status = SIGHTLINE_SKIPPED;
        if (live) {
            const unsigned i = (unsigned)a.index[j];
            w = ph.weight[i];
            p0 = ph.p0[i]; p1 = ph.p1[i]; p2 = ph.p2[i]; p3 = ph.p3[i]; r0 = ph.r0[i]; r1 = ph.r1[i]; r2 = ph.r2[i];
            if constexpr (STOKES) { s0 = ph.s0[i]; s1 = ph.s1[i]; s2 = ph.s2[i]; s3 = ph.s3[i]; }
            if (a.clocks) clock = a.clocks[i / (unsigned)a.slots_per_clock];
            tau = a.tau[j];
            status = a.status[j];
        }
        const double e = observe_energy(p0), x = escape_weight(tau);                      // exp(-tau), once per photon
        double v[N];
        v[0] = w; v[1] = w * e;
        if constexpr (STOKES) { v[2] = w * s0; v[3] = w * s1; v[4] = w * s2; v[5] = w * s3; }
        v[N - 2] = w * x; v[N - 1] = (w * e) * x;
        for (int o = 0; o < no; ++o) {                                                    // (the same trips for every lane of the workgroup)
            const double n0 = s_n0[o], n1 = s_n1[o], n2 = s_n2[o];
            const bool accepted = live && sky_accepted(p0, p1, p2, p3, n0, n1, n2, s_cos_acc[o]);
            const bool left = accepted && status == SIGHTLINE_LEFT_MESH;
            int bin = -1;
            if (left) {
                double X = 0, Y = 0;
                if constexpr (IMAGE) sky_xy(r0, r1, r2, s_x0[o], s_x1[o], s_x2[o], s_y0[o], s_y1[o], s_y2[o], X, Y);
                bin = escape_bin(o, s_tau_edges, a.n_tau, tau, s_t_edges, a.n_t, sky_t_det(clock, r0, r1, r2, n0, n1, n2), s_e_edges, a.n_e, e, s_x_edges, n_x, X,
                                 s_y_edges, n_y, Y);                                      // < n_bins, an int (escape_plan)
            }
            const unsigned long long m_accepted = __ballot(accepted), m_outside = __ballot(left && bin < 0),
                                     m_opaque = __ballot(accepted && status == SIGHTLINE_OPAQUE),
                                     m_unresolved = __ballot(accepted && (status == SIGHTLINE_STEP_CAP || status == SIGHTLINE_OFF_TABLE));
            if (lane == 0) {
                if (m_accepted) add_u64(&s_counters[o], (unsigned long long)__popcll(m_accepted));
                if (m_outside) add_u64(&s_counters[no + o], (unsigned long long)__popcll(m_outside));
                if (m_opaque) add_u64(&s_counters[2 * no + o], (unsigned long long)__popcll(m_opaque));
                if (m_unresolved) add_u64(&s_counters[3 * no + o], (unsigned long long)__popcll(m_unresolved));
            }
            const bool has = bin >= 0;
            if constexpr (LDS_CUBE) {
                if (has) add_bin<N>(at_lds, bin, 1ull, v);
            } else {
                const bool alone = match_alone(s_match, lane, bin, has);
                if (alone) add_bin<N>(at, bin, 1ull, v);
                add_shared_bins<N>(at, lane, alone ? -1 : bin, v);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < ESCAPE_COUNTERS * no; k += BLOCK)
        if (s_counters[k]) add_u64(&a.counters[k], s_counters[k]);
    if constexpr (LDS_CUBE) flush_lds_bins<N, BLOCK>(s_cube, nb, at, tid);
}

template <bool LDS_CUBE, bool STOKES, bool IMAGE>
hipError_t launch_bin_one(const PhotonDev &ph, const EscapeDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return launch_with_lds(&escape_bin_kernel<LDS_CUBE, STOKES, IMAGE>, blocks, ESCAPE_BLOCK, lds_bytes, OBSERVE_LDS_BUDGET, stream, ph, a);
}

template <bool LDS_CUBE, bool STOKES>
hipError_t launch_bin_image(const PhotonDev &ph, const EscapeDev &a, bool image, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return image ? launch_bin_one<LDS_CUBE, STOKES, true>(ph, a, blocks, lds_bytes, stream) : launch_bin_one<LDS_CUBE, STOKES, false>(ph, a, blocks, lds_bytes, stream);
}

hipError_t launch_bin(const PhotonDev &ph, const EscapeDev &a, const EscapePlan &plan, bool stokes, int blocks, hipStream_t stream)
{
    if (plan.path == OBSERVE_PATH_LDS)
        return stokes ? launch_bin_image<true, true>(ph, a, plan.image, blocks, plan.lds_bytes, stream)
                      : launch_bin_image<true, false>(ph, a, plan.image, blocks, plan.lds_bytes, stream);
    return stokes ? launch_bin_image<false, true>(ph, a, plan.image, blocks, plan.lds_bytes, stream)
                  : launch_bin_image<false, false>(ph, a, plan.image, blocks, plan.lds_bytes, stream);
}

}  // namespace

// The caller has zeroed the planes, the counters and the head, copied the staged inputs and the clocks behind them (escape_plan.hpp) and sized the
// three grids (escape_select_grid, escape_march_grid, escape_bin_grid).
hipError_t launch_escape(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const EscapeDev &a, const EscapePlan &plan, bool stokes,
                         int select_blocks, int march_blocks, int bin_blocks, hipStream_t stream)
{
    if (a.n_slots <= 0) return hipSuccess;
    if (select_blocks <= 0 || select_blocks > ESCAPE_MAX_GRID || bin_blocks <= 0 || bin_blocks > ESCAPE_MAX_GRID || march_blocks <= 0 ||
        march_blocks > ESCAPE_MARCH_MAX_GRID)
        return hipErrorInvalidValue;
    if (a.n_bins != plan.n_bins || plan.lds_bytes > OBSERVE_LDS_BUDGET || plan.select_lds_bytes > OBSERVE_LDS_BUDGET) return hipErrorInvalidValue;
    if (a.n_obs != plan.n_obs || a.n_tau != plan.n_tau || a.n_t != plan.n_t || a.n_e != plan.n_e || a.n_x != plan.n_x || a.n_y != plan.n_y) return hipErrorInvalidValue;
    hipError_t e = launch_with_lds(&escape_select_kernel, select_blocks, ESCAPE_BLOCK, plan.select_lds_bytes, OBSERVE_LDS_BUDGET, stream, ph, a);
    if (e != hipSuccess) return e;
    if ((e = launch_march_for(kc, ph, hy, a, march_blocks, stream)) != hipSuccess) return e;
    return launch_bin(ph, a, plan, stokes, bin_blocks, stream);
}

}  // namespace mcrat
