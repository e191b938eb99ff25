// observe.hip -- mock observations on the device: the resident photons binned by observer, detection time and energy (mcrat_hip_observe,
// mcrat_hip_pool_observe).  One streaming pass over flags, type, weight, p0, p3, r0, r1, r2 and, with Stokes on, s0 .. s3 -- 50 to 82 bytes per
// slot, coalesced -- with the per-photon rules of observe_plan.hpp.  The edges and the observers' cosines are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan from the cube's size; the pass and both paths' forms are bin_accumulate.hpp's (cube_pass):
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
#include "bin_accumulate.hpp"

namespace mcrat {

namespace {

// cube_pass's rule: the staged layout -- cos_obs, sin_obs, cos_lo, cos_hi [n_obs each], t_edges, e_edges -- and observe_plan.hpp's per-photon rules
struct ObserveRule {
    using Dev = ObserveDev;
    static constexpr int BLOCK = OBSERVE_BLOCK;
    static constexpr bool MATCH = false;
    const double *s_cos_obs, *s_sin_obs, *s_cos_lo, *s_cos_hi, *s_t_edges, *s_e_edges;
    int n_t, n_e, n_staged;
    struct Photon { double p0, p3, r0, r1, r2; };
    struct Observer {};
    __device__ __forceinline__ ObserveRule(const ObserveDev &a, const double *s_mem)
        : s_cos_obs(s_mem), s_sin_obs(s_cos_obs + a.n_obs), s_cos_lo(s_sin_obs + a.n_obs), s_cos_hi(s_cos_lo + a.n_obs), s_t_edges(s_cos_hi + a.n_obs),
          s_e_edges(s_t_edges + (a.n_t + 1)), n_t(a.n_t), n_e(a.n_e), n_staged(4 * a.n_obs + a.n_t + a.n_e + 2) {}
    __device__ __forceinline__ void load(const PhotonDev &ph, unsigned i, Photon &q) const
    {
        q.p0 = ph.p0[i]; q.p3 = ph.p3[i]; q.r0 = ph.r0[i]; q.r1 = ph.r1[i]; q.r2 = ph.r2[i];
    }
    __device__ __forceinline__ Observer observer(int) const { return {}; }
    __device__ __forceinline__ bool accepted(const Photon &q, Observer, int o) const { return observe_accepted(q.p0, q.p3, s_cos_lo[o], s_cos_hi[o]); }
    __device__ __forceinline__ int bin(const Photon &q, Observer, double clock, double e, int o) const
    {
        const int it = observe_find_bin(s_t_edges, n_t, observe_t_det(clock, q.r0, q.r1, q.r2, s_cos_obs[o], s_sin_obs[o]));
        const int ie = observe_find_bin(s_e_edges, n_e, e);
        return (it >= 0 && ie >= 0) ? (int)observe_bin(o, it, ie, n_t, n_e) : -1;      // < n_bins, an int (observe_plan)
    }
};

template <bool LDS_CUBE, bool STOKES>
__global__ __launch_bounds__(OBSERVE_BLOCK) void observe_kernel(PhotonDev ph, ObserveDev a)
{
    extern __shared__ double s_mem[];
    cube_pass<LDS_CUBE, STOKES, ObserveRule>(ph, a, s_mem);
}

template <bool LDS_CUBE, bool STOKES>
hipError_t launch_one(const PhotonDev &ph, const ObserveDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return launch_with_lds(&observe_kernel<LDS_CUBE, STOKES>, blocks, OBSERVE_BLOCK, lds_bytes, OBSERVE_LDS_BUDGET, stream, ph, a);
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
    const int blocks = accumulate_grid(a.n_slots, OBSERVE_BLOCK, cus, plan.groups_per_cu);
    if (lds) return stokes ? launch_one<true, true>(ph, a, blocks, plan.lds_bytes, stream) : launch_one<true, false>(ph, a, blocks, plan.lds_bytes, stream);
    return stokes ? launch_one<false, true>(ph, a, blocks, plan.lds_bytes, stream) : launch_one<false, false>(ph, a, blocks, plan.lds_bytes, stream);
}

}  // namespace mcrat
