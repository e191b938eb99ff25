// sky.hip -- mock observations from any direction on the sky, with images: the resident photons binned by observer, detection time, energy and,
// optionally, their position on the observer's sky plane (mcrat_hip_observe_sky, mcrat_hip_pool_observe_sky).  One lane per slot, a grid-stride
// loop, with the per-photon rules of sky_plan.hpp.  Photons are 3-D Cartesian whatever the run's DIMENSIONS and GEOMETRY: one kernel for all of
// them.  A counted slot reads flags, type, weight, p0 .. p3, r0 .. r2 and, with Stokes on, s0 .. s3 -- 66 to 98 bytes, coalesced -- and then goes
// through the observers one by one.  The observers' vectors and the edges are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan from the cube's size; the pass and both paths' forms are bin_accumulate.hpp's (cube_pass):
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
#include "bin_accumulate.hpp"

namespace mcrat {

namespace {

// cube_pass's rule: the staged layout -- n0, n1, n2, cos_acc [n_obs each]; (IMAGE) x0 .. x2, y0 .. y2 [n_obs each]; t_edges, e_edges; (IMAGE)
// x_edges, y_edges -- and sky_plan.hpp's per-photon rules
template <bool IMAGE>
struct SkyRule {
    using Dev = SkyDev;
    static constexpr int BLOCK = SKY_BLOCK;
    static constexpr bool MATCH = !MCRAT_SKY_NO_MATCH;
    const double *s_n0, *s_n1, *s_n2, *s_cos_acc, *s_x0, *s_x1, *s_x2, *s_y0, *s_y1, *s_y2, *s_t_edges, *s_e_edges, *s_x_edges, *s_y_edges;
    int n_t, n_e, n_x, n_y, n_staged;
    struct Photon { double p0, p1, p2, p3, r0, r1, r2; };
    struct Observer { double n0, n1, n2; };          // the direction towards the observer
    __device__ __forceinline__ SkyRule(const SkyDev &a, const double *s_mem)
        : s_n0(s_mem), s_n1(s_n0 + a.n_obs), s_n2(s_n1 + a.n_obs), s_cos_acc(s_n2 + a.n_obs), s_x0(s_cos_acc + a.n_obs), s_x1(s_x0 + a.n_obs),
          s_x2(s_x1 + a.n_obs), s_y0(s_x2 + a.n_obs), s_y1(s_y0 + a.n_obs), s_y2(s_y1 + a.n_obs),                                             // (IMAGE)
          s_t_edges(s_cos_acc + a.n_obs + (IMAGE ? 6 * a.n_obs : 0)), s_e_edges(s_t_edges + (a.n_t + 1)), s_x_edges(s_e_edges + (a.n_e + 1)),
          s_y_edges(s_x_edges + (a.n_x + 1)),                                                                                                  // (IMAGE)
          n_t(a.n_t), n_e(a.n_e), n_x(IMAGE ? a.n_x : 0), n_y(IMAGE ? a.n_y : 0),
          n_staged((IMAGE ? 10 : 4) * a.n_obs + a.n_t + a.n_e + 2 + (IMAGE ? a.n_x + a.n_y + 2 : 0)) {}
    __device__ __forceinline__ void load(const PhotonDev &ph, unsigned i, Photon &q) const
    {
        q.p0 = ph.p0[i]; q.p1 = ph.p1[i]; q.p2 = ph.p2[i]; q.p3 = ph.p3[i]; q.r0 = ph.r0[i]; q.r1 = ph.r1[i]; q.r2 = ph.r2[i];
    }
    __device__ __forceinline__ Observer observer(int o) const { return {s_n0[o], s_n1[o], s_n2[o]}; }
    __device__ __forceinline__ bool accepted(const Photon &q, const Observer &ob, int o) const
    {
        return sky_accepted(q.p0, q.p1, q.p2, q.p3, ob.n0, ob.n1, ob.n2, s_cos_acc[o]);
    }
    __device__ __forceinline__ int bin(const Photon &q, const Observer &ob, double clock, double e, int o) const
    {
        double X = 0, Y = 0;
        if constexpr (IMAGE) sky_xy(q.r0, q.r1, q.r2, s_x0[o], s_x1[o], s_x2[o], s_y0[o], s_y1[o], s_y2[o], X, Y);
        return sky_bin(o, s_t_edges, n_t, sky_t_det(clock, q.r0, q.r1, q.r2, ob.n0, ob.n1, ob.n2), s_e_edges, n_e, e, s_x_edges, n_x, X, s_y_edges, n_y,
                       Y);                                                            // < n_bins, an int (sky_plan)
    }
};

template <bool LDS_CUBE, bool STOKES, bool IMAGE>
__global__ __launch_bounds__(SKY_BLOCK) void sky_kernel(PhotonDev ph, SkyDev a)
{
    extern __shared__ double s_mem[];
    cube_pass<LDS_CUBE, STOKES, SkyRule<IMAGE>>(ph, a, s_mem);
}

template <bool LDS_CUBE, bool STOKES, bool IMAGE>
hipError_t launch_one(const PhotonDev &ph, const SkyDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return launch_with_lds(&sky_kernel<LDS_CUBE, STOKES, IMAGE>, blocks, SKY_BLOCK, lds_bytes, OBSERVE_LDS_BUDGET, stream, ph, a);
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
