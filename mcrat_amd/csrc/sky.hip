// sky.hip -- mock observations from any direction on the sky, with images: the resident photons binned by observer, detection time, energy and,
// optionally, their position on the observer's sky plane (mcrat_hip_observe_sky, mcrat_hip_pool_observe_sky).  One lane per slot, a grid-stride
// loop, with the per-photon rules of sky_plan.hpp.  Photons are 3-D Cartesian whatever the run's DIMENSIONS and GEOMETRY: one kernel for all of
// them.  A counted slot reads flags, type, weight, p0 .. p3, r0 .. r2 and, with Stokes on, s0 .. s3 -- 66 to 98 bytes, coalesced -- and then goes
// through the observers one by one.  The observers' vectors and the edges are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan from the cube's size (observe.hip's and radfield.hip's forms):
//   LDS      light curves, spectra and small images: the workgroup owns a private copy of the whole cube in LDS, adds into it with LDS atomics and
//            flushes the bins it touched to HBM once, when it has run out of slots.
//   global   images: hardware f64 atomic adds that return nothing, and an integer atomic for the count, straight into the cube in HBM.  A
//            wavefront's 64 photons may sit in 64 different pixels or all in the one pixel of the jet's core, so the wavefront first finds out which of
//            its lanes share a bin: every lane writes its number into a one-byte table in LDS at a hash of its bin and reads back who won the entry; a
//            lane that lost to a lane of the same bin marks the entry.  A lane that won an unmarked entry has a bin of its own and adds what it
//            holds.  The rest -- lanes of shared bins, and the few that lost an entry to another bin -- go through rounds, one per distinct bin: the
//            group is summed over the wavefront and its first lane adds for all.  -DMCRAT_SKY_NO_MATCH=1 builds the path without the table: every
//            lane goes through the rounds.
// Every loop is bounded by the slot count, the observers or the 64 lanes of a wavefront; no workgroup waits on another.
// Counts are exact.  The six sums per bin depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run; each
// stays within (m + 2) * 2^-53 * sum|term| of the exact sum of the bin's m terms.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"

namespace mcrat {

namespace {

// no-return hardware adds: ds_add_f64 / global_atomic_add_f64 and their 64-bit integer kin
__device__ __forceinline__ void add_f64(double *p, double v) { (void)unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void add_u64(unsigned long long *p, unsigned long long v) { (void)atomicAdd(p, v); }

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one bin's seven adds (five with Stokes off: those planes stay zero)
template <bool STOKES>
__device__ __forceinline__ void add_bin(double *cube, size_t nb, int bin, unsigned long long m, double w, double we, double wi, double wq, double wu, double wv)
{
    add_u64(reinterpret_cast<unsigned long long *>(cube) + bin, m);
    add_f64(&cube[OBS_W * nb + bin], w); add_f64(&cube[OBS_WE * nb + bin], we);
    if constexpr (STOKES) {
        add_f64(&cube[OBS_I * nb + bin], wi); add_f64(&cube[OBS_Q * nb + bin], wq);
        add_f64(&cube[OBS_U * nb + bin], wu); add_f64(&cube[OBS_V * nb + bin], wv);
    }
}

template <bool LDS_CUBE, bool STOKES, bool IMAGE>
__global__ __launch_bounds__(SKY_BLOCK) void sky_kernel(PhotonDev ph, SkyDev a)
{
    extern __shared__ double s_mem[];
    // LDS: the staged inputs in the block's order, the workgroup's per-observer counters, then its copy of the cube (LDS path) or the wavefronts'
    // match tables (global path)
    const int no = a.n_obs;
    const double *s_n0 = s_mem, *s_n1 = s_n0 + no, *s_n2 = s_n1 + no, *s_cos_acc = s_n2 + no;
    const double *s_vec_end = s_cos_acc + no + (IMAGE ? 6 * no : 0);
    const double *s_x0 = s_cos_acc + no, *s_x1 = s_x0 + no, *s_x2 = s_x1 + no, *s_y0 = s_x2 + no, *s_y1 = s_y0 + no, *s_y2 = s_y1 + no;      // (IMAGE)
    const double *s_t_edges = s_vec_end, *s_e_edges = s_t_edges + (a.n_t + 1);
    const double *s_x_edges = s_e_edges + (a.n_e + 1), *s_y_edges = s_x_edges + (a.n_x + 1);                                               // (IMAGE)
    const int n_staged = (IMAGE ? 10 : 4) * no + a.n_t + a.n_e + 2 + (IMAGE ? a.n_x + a.n_y + 2 : 0);
    unsigned long long *s_accepted = reinterpret_cast<unsigned long long *>(s_mem + n_staged), *s_outside = s_accepted + no;
    double *s_cube = reinterpret_cast<double *>(s_outside + no);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < n_staged; k += SKY_BLOCK) s_mem[k] = a.staged[k];
    for (int k = tid; k < 2 * no; k += SKY_BLOCK) s_accepted[k] = 0ull;
    const size_t nb = (size_t)a.n_bins;
    if constexpr (LDS_CUBE)
        for (size_t k = tid; k < (size_t)OBSERVE_PLANES * nb; k += SKY_BLOCK) s_cube[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
    __syncthreads();
#if !MCRAT_SKY_NO_MATCH
    unsigned char *const s_match = reinterpret_cast<unsigned char *>(s_cube) + ((size_t)(tid >> 6) << SKY_MATCH_BITS);      // (global path) this wavefront's table
#endif

    const unsigned n = (unsigned)a.n_slots, stride = gridDim.x * SKY_BLOCK;
    for (unsigned base = blockIdx.x * SKY_BLOCK; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap; the same trips for every lane of the workgroup)
        const unsigned i = base + tid;
        bool live = i < n;
        double w = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0, r0 = 0, r1 = 0, r2 = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, clock = a.time_now;
        if (live) {
            w = ph.weight[i];
            live = observe_observable(ph.flags[i], ph.type[i], w);
        }
        if (live) {
            p0 = ph.p0[i]; p1 = ph.p1[i]; p2 = ph.p2[i]; p3 = ph.p3[i]; r0 = ph.r0[i]; r1 = ph.r1[i]; r2 = ph.r2[i];
            if constexpr (STOKES) { s0 = ph.s0[i]; s1 = ph.s1[i]; s2 = ph.s2[i]; s3 = ph.s3[i]; }
            if (a.clocks) clock = a.clocks[i / (unsigned)a.slots_per_clock];
        }
        const double e = observe_energy(p0);
        const double we = w * e, wi = w * s0, wq = w * s1, wu = w * s2, wv = w * s3;
        for (int o = 0; o < no; ++o) {                                                // (the same trips for every lane of the workgroup)
            const double n0 = s_n0[o], n1 = s_n1[o], n2 = s_n2[o];
            const bool accepted = live && sky_accepted(p0, p1, p2, p3, n0, n1, n2, s_cos_acc[o]);
            int bin = -1;
            if (accepted) {
                double X = 0, Y = 0;
                if constexpr (IMAGE) sky_xy(r0, r1, r2, s_x0[o], s_x1[o], s_x2[o], s_y0[o], s_y1[o], s_y2[o], X, Y);
                bin = sky_bin(o, s_t_edges, a.n_t, sky_t_det(clock, r0, r1, r2, n0, n1, n2), s_e_edges, a.n_e, e, s_x_edges, IMAGE ? a.n_x : 0, X, s_y_edges,
                              IMAGE ? a.n_y : 0, Y);                                  // < n_bins, an int (sky_plan)
            }
            const unsigned long long m_accepted = __ballot(accepted), m_outside = __ballot(accepted && bin < 0);
            if (lane == 0) {
                if (m_accepted) add_u64(&s_accepted[o], (unsigned long long)__popcll(m_accepted));
                if (m_outside) add_u64(&s_outside[o], (unsigned long long)__popcll(m_outside));
            }
            const bool has = bin >= 0;
            if constexpr (LDS_CUBE) {
                if (has) add_bin<STOKES>(s_cube, nb, bin, 1ull, w, we, wi, wq, wu, wv);
            } else {
#if MCRAT_SKY_NO_MATCH
                const bool alone = false;
#else
                // which lanes share a bin: the table entry at a hash of the bin goes to one of the lanes that want it
                const unsigned h = sky_match_hash(bin);
                if (has) s_match[h] = (unsigned char)lane;
                __syncthreads();
                const int owner = has ? (int)s_match[h] : lane;
                const int owner_bin = __shfl(bin, owner, 64);
                __syncthreads();
                if (has && owner != lane && owner_bin == bin) s_match[h] = 64;      // the owner has company
                __syncthreads();
                const bool alone = has && owner == lane && s_match[h] == (unsigned char)lane;
                if (alone) add_bin<STOKES>(a.cube, nb, bin, 1ull, w, we, wi, wq, wu, wv);
#endif
                // the rest, group by group of the lanes that share a bin (the others contribute +0.0, which changes no sum): at most 64 rounds
                unsigned long long todo = __ballot(has && !alone);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int lb = __shfl(bin, leader, 64);
                    const bool mine = !alone && bin == lb;
                    const unsigned long long group = __ballot(mine);
                    todo &= ~group;
                    const int m = __popcll(group);
                    double gw = w, gwe = we, gwi = wi, gwq = wq, gwu = wu, gwv = wv;
                    if (m > 1) {
                        gw = wave_sum(mine ? w : 0.0); gwe = wave_sum(mine ? we : 0.0);
                        if constexpr (STOKES) {
                            gwi = wave_sum(mine ? wi : 0.0); gwq = wave_sum(mine ? wq : 0.0);
                            gwu = wave_sum(mine ? wu : 0.0); gwv = wave_sum(mine ? wv : 0.0);
                        }
                    }
                    if (lane == leader) add_bin<STOKES>(a.cube, nb, lb, (unsigned long long)m, gw, gwe, gwi, gwq, gwu, gwv);
                }
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < no; k += SKY_BLOCK) {
        if (s_accepted[k]) add_u64(&a.n_accepted[k], s_accepted[k]);
        if (s_outside[k]) add_u64(&a.n_outside[k], s_outside[k]);
    }
    if constexpr (LDS_CUBE) {
        const unsigned long long *const s_count = reinterpret_cast<const unsigned long long *>(s_cube);
        for (size_t b = tid; b < nb; b += SKY_BLOCK) {
            const unsigned long long m = s_count[b];
            if (!m) continue;
            add_bin<STOKES>(a.cube, nb, (int)b, m, s_cube[OBS_W * nb + b], s_cube[OBS_WE * nb + b], s_cube[OBS_I * nb + b], s_cube[OBS_Q * nb + b],
                            s_cube[OBS_U * nb + b], s_cube[OBS_V * nb + b]);
        }
    }
}

template <bool LDS_CUBE, bool STOKES, bool IMAGE>
hipError_t launch_one(const PhotonDev &ph, const SkyDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    if (lds_bytes > 64 * 1024) {               // more than the default 64 KB of dynamic LDS has to be asked for (per device: asked every time)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&sky_kernel<LDS_CUBE, STOKES, IMAGE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)OBSERVE_LDS_BUDGET);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((sky_kernel<LDS_CUBE, STOKES, IMAGE>), dim3(blocks), dim3(SKY_BLOCK), lds_bytes, stream, ph, a);
    return hipGetLastError();
}

template <bool LDS_CUBE, bool STOKES>
hipError_t launch_image(const PhotonDev &ph, const SkyDev &a, bool image, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return image ? launch_one<LDS_CUBE, STOKES, true>(ph, a, blocks, lds_bytes, stream) : launch_one<LDS_CUBE, STOKES, false>(ph, a, blocks, lds_bytes, stream);
}

}  // namespace

// The caller has zeroed the cube and the counters, copied the staged inputs and the clocks behind them (sky_plan.hpp) and sized the grid (sky_grid).
hipError_t launch_sky(const PhotonDev &ph, const SkyDev &a, const SkyPlan &plan, bool stokes, int blocks, hipStream_t stream)
{
    if (a.n_slots <= 0) return hipSuccess;
    if (blocks <= 0 || blocks > SKY_MAX_GRID || a.n_bins != plan.n_bins || plan.lds_bytes > OBSERVE_LDS_BUDGET) return hipErrorInvalidValue;
    if (a.n_obs != plan.n_obs || a.n_t != plan.n_t || a.n_e != plan.n_e || a.n_x != plan.n_x || a.n_y != plan.n_y) return hipErrorInvalidValue;
    if (plan.path == OBSERVE_PATH_LDS)
        return stokes ? launch_image<true, true>(ph, a, plan.image, blocks, plan.lds_bytes, stream) : launch_image<true, false>(ph, a, plan.image, blocks, plan.lds_bytes, stream);
    return stokes ? launch_image<false, true>(ph, a, plan.image, blocks, plan.lds_bytes, stream) : launch_image<false, false>(ph, a, plan.image, blocks, plan.lds_bytes, stream);
}

}  // namespace mcrat
