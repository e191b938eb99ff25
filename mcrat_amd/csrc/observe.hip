// observe.hip -- mock observations on the device: the resident photons binned by observer, detection time and energy (mcrat_hip_observe,
// mcrat_hip_pool_observe).  One streaming pass over flags, type, weight, p0, p3, r0, r1, r2 and, with Stokes on, s0 .. s3 -- 50 to 82 bytes per
// slot, coalesced -- with the per-photon rules of observe_plan.hpp.  The edges and the observers' cosines are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan from the cube's size:
//   LDS      the workgroup owns a private copy of the whole cube in LDS, adds into it with LDS atomics and flushes the bins it touched to HBM once,
//            when it has run out of slots.
//   global   the cube is too large for that: hardware f64 atomic adds that return nothing go straight to the HBM cube, and an integer atomic for
//            the count.  The lanes of a wavefront that hit the same bin are summed first and one lane adds for all of them (a light-curve peak puts
//            most of a wavefront into one bin).
// Counts are exact.  The six sums per bin depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run; each
// stays within (m + 2) * 2^-53 * sum|term| of the exact sum of the bin's m terms (the worst case of any summation order).
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"

namespace mcrat {

namespace {

constexpr int OBSERVE_BLOCK = 256;

// no-return hardware adds: ds_add_f64 / global_atomic_add_f64 and their 64-bit integer kin
__device__ __forceinline__ void add_f64(double *p, double v) { (void)unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void add_u64(unsigned long long *p, unsigned long long v) { (void)atomicAdd(p, v); }

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool LDS_CUBE, bool STOKES>
__global__ __launch_bounds__(OBSERVE_BLOCK) void observe_kernel(PhotonDev ph, ObserveDev a)
{
    extern __shared__ double s_mem[];
    // LDS: the staged inputs, the workgroup's per-observer counters, then (LDS path) its copy of the cube
    double *s_cos_obs = s_mem, *s_sin_obs = s_cos_obs + a.n_obs, *s_cos_lo = s_sin_obs + a.n_obs, *s_cos_hi = s_cos_lo + a.n_obs;
    double *s_t_edges = s_cos_hi + a.n_obs, *s_e_edges = s_t_edges + (a.n_t + 1);
    unsigned long long *s_accepted = reinterpret_cast<unsigned long long *>(s_e_edges + (a.n_e + 1)), *s_outside = s_accepted + a.n_obs;
    double *s_cube = reinterpret_cast<double *>(s_outside + a.n_obs);
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_staged = 4 * a.n_obs + a.n_t + a.n_e + 2;
    for (int k = tid; k < n_staged; k += OBSERVE_BLOCK) s_mem[k] = a.staged[k];
    for (int k = tid; k < 2 * a.n_obs; k += OBSERVE_BLOCK) s_accepted[k] = 0ull;
    if constexpr (LDS_CUBE)
        for (size_t k = tid; k < (size_t)OBSERVE_PLANES * (size_t)a.n_bins; k += OBSERVE_BLOCK) s_cube[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
    __syncthreads();

    double *const cube = LDS_CUBE ? s_cube : a.cube;
    unsigned long long *const count = reinterpret_cast<unsigned long long *>(cube);
    const size_t nb = (size_t)a.n_bins;
    const unsigned n = (unsigned)a.n_slots, stride = gridDim.x * OBSERVE_BLOCK;
    for (unsigned base = blockIdx.x * OBSERVE_BLOCK; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap)
        const unsigned i = base + tid;
        bool live = i < n;
        double w = 0, p0 = 0, p3 = 0, r0 = 0, r1 = 0, r2 = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, clock = a.time_now;
        if (live) {
            w = ph.weight[i];
            live = observe_observable(ph.flags[i], ph.type[i], w);
        }
        if (live) {
            p0 = ph.p0[i]; p3 = ph.p3[i]; r0 = ph.r0[i]; r1 = ph.r1[i]; r2 = ph.r2[i];
            if constexpr (STOKES) { s0 = ph.s0[i]; s1 = ph.s1[i]; s2 = ph.s2[i]; s3 = ph.s3[i]; }
            if (a.clocks) clock = a.clocks[i / (unsigned)a.slots_per_clock];
        }
        const double e = observe_energy(p0);
        const double we = w * e, wi = w * s0, wq = w * s1, wu = w * s2, wv = w * s3;
        for (int o = 0; o < a.n_obs; ++o) {
            const bool accepted = live && observe_accepted(p0, p3, s_cos_lo[o], s_cos_hi[o]);
            int bin = -1;
            if (accepted) {
                const int it = observe_find_bin(s_t_edges, a.n_t, observe_t_det(clock, r0, r1, r2, s_cos_obs[o], s_sin_obs[o]));
                const int ie = observe_find_bin(s_e_edges, a.n_e, e);
                if (it >= 0 && ie >= 0) bin = (int)observe_bin(o, it, ie, a.n_t, a.n_e);      // < n_bins, an int (observe_plan)
            }
            const unsigned long long m_accepted = __ballot(accepted), m_outside = __ballot(accepted && bin < 0);
            if (lane == 0) {
                if (m_accepted) add_u64(&s_accepted[o], (unsigned long long)__popcll(m_accepted));
                if (m_outside) add_u64(&s_outside[o], (unsigned long long)__popcll(m_outside));
            }
            if constexpr (LDS_CUBE) {
                if (bin >= 0) {
                    add_u64(&count[bin], 1ull);
                    add_f64(&cube[OBS_W * nb + bin], w); add_f64(&cube[OBS_WE * nb + bin], we);
                    if constexpr (STOKES) {
                        add_f64(&cube[OBS_I * nb + bin], wi); add_f64(&cube[OBS_Q * nb + bin], wq);
                        add_f64(&cube[OBS_U * nb + bin], wu); add_f64(&cube[OBS_V * nb + bin], wv);
                    }
                }
            } else {
                // the lanes of this wavefront, group by group of those that share a bin: a lane on its own adds what it holds, a group is summed
                // over the wavefront (the others contribute +0.0, which changes no sum) and its first lane adds for all
                unsigned long long todo = __ballot(bin >= 0);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int lb = __shfl(bin, leader, 64);
                    const bool mine = bin == lb;
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
                    if (lane == leader) {
                        add_u64(&count[lb], (unsigned long long)m);
                        add_f64(&cube[OBS_W * nb + lb], gw); add_f64(&cube[OBS_WE * nb + lb], gwe);
                        if constexpr (STOKES) {
                            add_f64(&cube[OBS_I * nb + lb], gwi); add_f64(&cube[OBS_Q * nb + lb], gwq);
                            add_f64(&cube[OBS_U * nb + lb], gwu); add_f64(&cube[OBS_V * nb + lb], gwv);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < a.n_obs; k += OBSERVE_BLOCK) {
        if (s_accepted[k]) add_u64(&a.n_accepted[k], s_accepted[k]);
        if (s_outside[k]) add_u64(&a.n_outside[k], s_outside[k]);
    }
    if constexpr (LDS_CUBE) {
        unsigned long long *const g_count = reinterpret_cast<unsigned long long *>(a.cube);
        for (size_t b = tid; b < nb; b += OBSERVE_BLOCK) {
            const unsigned long long m = count[b];
            if (!m) continue;
            add_u64(&g_count[b], m);
            add_f64(&a.cube[OBS_W * nb + b], s_cube[OBS_W * nb + b]); add_f64(&a.cube[OBS_WE * nb + b], s_cube[OBS_WE * nb + b]);
            if constexpr (STOKES) {
                add_f64(&a.cube[OBS_I * nb + b], s_cube[OBS_I * nb + b]); add_f64(&a.cube[OBS_Q * nb + b], s_cube[OBS_Q * nb + b]);
                add_f64(&a.cube[OBS_U * nb + b], s_cube[OBS_U * nb + b]); add_f64(&a.cube[OBS_V * nb + b], s_cube[OBS_V * nb + b]);
            }
        }
    }
}

template <bool LDS_CUBE, bool STOKES>
hipError_t launch_one(const PhotonDev &ph, const ObserveDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    if (lds_bytes > 64 * 1024) {               // more than the default 64 KB of dynamic LDS has to be asked for (per device: asked every time)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&observe_kernel<LDS_CUBE, STOKES>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)OBSERVE_LDS_BUDGET);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((observe_kernel<LDS_CUBE, STOKES>), dim3(blocks), dim3(OBSERVE_BLOCK), lds_bytes, stream, ph, a);
    return hipGetLastError();
}

}  // namespace

// Workgroups: the pass is a grid-stride loop, so that a workgroup stages its LDS once for many slots.  Per CU as many as the plan says
// (observe_plan.hpp): two on the LDS path, each flushing once -- more were measured slower, the flushes of all workgroups meet at the same
// addresses --, eight -- 32 wavefronts -- on the global path, which keeps only the staged inputs in LDS and needs the atomics' queues fed.
hipError_t launch_observe(const PhotonDev &ph, const ObserveDev &a, const ObservePlan &plan, bool stokes, int cus, hipStream_t stream)
{
    if (a.n_slots <= 0) return hipSuccess;
    if (plan.lds_bytes > OBSERVE_LDS_BUDGET) return hipErrorInvalidValue;
    const bool lds = plan.path == OBSERVE_PATH_LDS;
    const long long want = ((long long)a.n_slots + OBSERVE_BLOCK - 1) / OBSERVE_BLOCK, cap = (long long)(cus > 0 ? cus : 256) * plan.groups_per_cu;
    const int blocks = (int)(want < cap ? want : cap);
    if (lds) return stokes ? launch_one<true, true>(ph, a, blocks, plan.lds_bytes, stream) : launch_one<true, false>(ph, a, blocks, plan.lds_bytes, stream);
    return stokes ? launch_one<false, true>(ph, a, blocks, plan.lds_bytes, stream) : launch_one<false, false>(ph, a, blocks, plan.lds_bytes, stream);
}

}  // namespace mcrat
