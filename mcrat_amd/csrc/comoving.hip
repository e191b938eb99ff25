// comoving.hip -- the comoving radiation field: the resident photons located in the staged frame, boosted into their cell's frame and binned by
// position (hydro cell or (radius, polar cosine) shell), fluid-frame energy and fluid-frame direction cosine about the flow, eight planes per bin
// (mcrat_hip_comoving_field, mcrat_hip_pool_comoving_field).  One lane per slot, a grid-stride loop, with the per-photon rules of comoving_plan.hpp
// and radfield_plan.hpp and the loop's own cell look-up, azimuth and boost (physics.hpp): what radfield_kernel does per photon, plus one division
// and one square root for the two cosines and two edge searches.  The edges of all four axes are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan; the forms of both are bin_accumulate.hpp's, as the radiation field uses them:
//   LDS      SHELLS whose eight planes fit: the workgroup owns a private copy in LDS, adds into it with LDS atomics and flushes the bins it touched
//            once, when it has run out of slots (flush_lds_bins).
//   global   CELLS, and SHELLS beyond LDS: hardware atomics straight into the accumulator in HBM, the lanes with a bin of their own at once
//            (match_alone), the rest in rounds (add_shared_bins).
// The accumulator is plane-major: the planes the caller receives.
// Counts are exact for the device's own e and a.  The seven sums per bin depend on the order in which the atomics are served: they are NOT
// bit-reproducible from run to run.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "physics.hpp"
#include "radfield_plan.hpp"
#include "comoving_plan.hpp"
#include "bin_accumulate.hpp"

namespace mcrat {

namespace {

template <int DIMS, int GEOM, bool SHELLS, bool LDS_PLANES>
__global__ __launch_bounds__(COMOVING_BLOCK) void comoving_kernel(PhotonDev ph, HydroDev hy, ComovingDev a)
{
    extern __shared__ double s_mem[];
    // LDS: the staged edges, the workgroup's three counters, then its copy of the planes (LDS path) or the wavefronts' match tables (global path)
    const int n_shell_edges = SHELLS ? a.n_r + a.n_mu + 2 : 0;
    const int n_staged = n_shell_edges + a.n_e + a.n_a + 2;
    const double *s_r_edges = s_mem, *s_mu_edges = s_mem + (a.n_r + 1);
    const double *s_e_edges = s_mem + n_shell_edges, *s_a_edges = s_e_edges + (a.n_e + 1);
    unsigned long long *s_scalar = reinterpret_cast<unsigned long long *>(s_mem + n_staged);
    double *s_planes = reinterpret_cast<double *>(s_scalar + COMOVING_N_SCALARS);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < n_staged; k += COMOVING_BLOCK) s_mem[k] = a.staged[k];
    if (tid < COMOVING_N_SCALARS) s_scalar[tid] = 0ull;
    const size_t nb = (size_t)a.n_bins;
    const PlaneMajor at_lds{s_planes, nb}, at_flush{a.acc, nb};
    if constexpr (LDS_PLANES)
        for (size_t k = tid; k < (size_t)COMOVING_PLANES * nb; k += COMOVING_BLOCK) s_planes[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
    __syncthreads();
    unsigned char *const s_match = reinterpret_cast<unsigned char *>(s_planes) + ((size_t)(tid >> 6) << OBSERVE_MATCH_BITS);      // (global path) this wavefront's table

    const unsigned n = (unsigned)a.n_slots, stride = gridDim.x * COMOVING_BLOCK;
    for (unsigned base = blockIdx.x * COMOVING_BLOCK; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap; the same trips for every lane of the workgroup)
        const unsigned i = base + tid;
        bool live = i < n;
        double w = 0;
        if (live) {
            w = ph.weight[i];
            live = observe_observable(ph.flags[i], ph.type[i], w);
        }
        int cell = -1, bin = -1;
        double v[COMOVING_SUMS] = {0, 0, 0, 0, 0, 0, 0};
        if (live) {
            const double r0 = ph.r0[i], r1 = ph.r1[i], r2 = ph.r2[i];
            const double p0 = ph.p0[i], p1 = ph.p1[i], p2 = ph.p2[i], p3 = ph.p3[i];
            double a0, a1, a2;
            phys::hydro_coords<DIMS, GEOM>(r0, r1, r2, a0, a1, a2);
            FatCell hit;
            hit.cell = -1;
            if (phys::in_domain<DIMS>(hy, a0, a1, a2))
                phys::find_in_bucket<DIMS>(hy, phys::grid_bucket_of<DIMS>(hy.grid, a0, a1, a2), a0, a1, a2, hit);
            cell = hit.cell;
            if (cell >= hy.M) cell = -1;                      // (cannot happen: the look-up names cells of hy; nothing may be added past the accumulator)
            if (cell >= 0) {
                double cphi, sphi, beta[3], r, mu;
                phys::relocation_azimuth<DIMS, GEOM>(r0, r1, a0, cphi, sphi);
                phys::beta_from_record<DIMS>(hit.a, hit.b, hit.c, cphi, sphi, beta);
                const double bp = comoving_bp(beta, p1, p2, p3);
                const double e = comoving_e(hit.gam, p0, bp);          // (boost_with's time component)
                radfield_r_mu(r0, r1, r2, r, mu);
                const double m = comoving_m(r0, r1, r2, p0, p1, p2, p3, r);
                const double ac = comoving_a(beta, bp, p0, m);
                comoving_terms(w, e, ac, radfield_e_lab(p0), m, v);
                int s = cell;                                 // < hy.M == n_s
                if constexpr (SHELLS) s = radfield_shell_bin(s_r_edges, a.n_r, s_mu_edges, a.n_mu, r, mu);
                bin = comoving_bin(s, s_e_edges, a.n_e, s_a_edges, a.n_a, e, ac);      // < n_bins, an int (comoving_check, comoving_layout)
            }
        }
        const unsigned long long m_live = __ballot(live), m_unlocated = __ballot(live && cell < 0), m_outside = __ballot(cell >= 0 && bin < 0);
        if (lane == 0) {
            if (m_live) add_u64(&s_scalar[RF_N_OBSERVABLE], (unsigned long long)__popcll(m_live));
            if (m_unlocated) add_u64(&s_scalar[RF_N_UNLOCATED], (unsigned long long)__popcll(m_unlocated));
            if (m_outside) add_u64(&s_scalar[RF_N_OUTSIDE], (unsigned long long)__popcll(m_outside));
        }
        const bool has = bin >= 0;
        if constexpr (LDS_PLANES) {
            if (has) add_bin<COMOVING_SUMS>(at_lds, bin, 1ull, v);
        } else {
            const PlaneBases<COMOVING_PLANES> at(a.acc, nb);          // (the same for every trip: worked out once)
            const bool alone = match_alone(s_match, lane, bin, has);  // (barriers inside: every lane, every trip; an idle lane has nothing)
            if (alone) add_bin<COMOVING_SUMS>(at, bin, 1ull, v);
            add_shared_bins<COMOVING_SUMS>(at, lane, alone ? -1 : bin, v);
        }
    }
    __syncthreads();
    if (tid < COMOVING_N_SCALARS && s_scalar[tid]) add_u64(&a.head[tid], s_scalar[tid]);
    if constexpr (LDS_PLANES) flush_lds_bins<COMOVING_SUMS, COMOVING_BLOCK>(s_planes, nb, at_flush, tid);
}

template <int DIMS, int GEOM, bool SHELLS, bool LDS_PLANES>
hipError_t launch_one(const PhotonDev &ph, const HydroDev &hy, const ComovingDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return launch_with_lds(&comoving_kernel<DIMS, GEOM, SHELLS, LDS_PLANES>, blocks, COMOVING_BLOCK, lds_bytes, lds_bytes, stream, ph, hy, a);
}

template <int DIMS, int GEOM>
hipError_t launch_pair(const PhotonDev &ph, const HydroDev &hy, const ComovingDev &a, const ComovingPlan &plan, int blocks, hipStream_t stream)
{
    if (plan.s.mode == COMOVING_CELLS) return launch_one<DIMS, GEOM, false, false>(ph, hy, a, blocks, plan.lds_bytes, stream);
    if (plan.s.path == OBSERVE_PATH_LDS) return launch_one<DIMS, GEOM, true, true>(ph, hy, a, blocks, plan.lds_bytes, stream);
    return launch_one<DIMS, GEOM, true, false>(ph, hy, a, blocks, plan.lds_bytes, stream);
}

}  // namespace

// The nine (DIMENSIONS, geometry) pairs the engine accepts, as launch_radfield switches over them.  The caller has zeroed the block's head and
// accumulator, copied the edges behind them and sized the grid (comoving_plan.hpp, comoving_grid); hy is the frame the photons are located in.
hipError_t launch_comoving(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const ComovingDev &a, const ComovingPlan &plan, int blocks,
                           hipStream_t stream)
{
    if (a.n_slots <= 0 || blocks <= 0 || a.n_bins <= 0 || a.n_bins != plan.n_bins || a.n_e != plan.s.n_e || a.n_a != plan.s.n_a) return hipErrorInvalidValue;
    if (plan.s.mode == COMOVING_CELLS && (plan.s.path != OBSERVE_PATH_GLOBAL || plan.n_s != hy.M)) return hipErrorInvalidValue;
    if (plan.s.mode == COMOVING_SHELLS && (a.n_r != plan.s.n_r || a.n_mu != plan.s.n_mu || plan.n_s != plan.s.n_shells)) return hipErrorInvalidValue;
    if ((long long)plan.n_s * plan.s.n_e * plan.s.n_a != (long long)plan.n_bins) return hipErrorInvalidValue;
    if (plan.lds_bytes > OBSERVE_LDS_PER_CU) return hipErrorInvalidValue;
    switch (kc.dimensions * 4 + kc.geometry) {
    case DIM_TWO * 4 + GEOM_CARTESIAN: return launch_pair<DIM_TWO, GEOM_CARTESIAN>(ph, hy, a, plan, blocks, stream);
    case DIM_TWO * 4 + GEOM_CYLINDRICAL: return launch_pair<DIM_TWO, GEOM_CYLINDRICAL>(ph, hy, a, plan, blocks, stream);
    case DIM_TWO * 4 + GEOM_SPHERICAL: return launch_pair<DIM_TWO, GEOM_SPHERICAL>(ph, hy, a, plan, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CARTESIAN: return launch_pair<DIM_TWO_POINT_FIVE, GEOM_CARTESIAN>(ph, hy, a, plan, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CYLINDRICAL: return launch_pair<DIM_TWO_POINT_FIVE, GEOM_CYLINDRICAL>(ph, hy, a, plan, blocks, stream);
    case DIM_TWO_POINT_FIVE * 4 + GEOM_SPHERICAL: return launch_pair<DIM_TWO_POINT_FIVE, GEOM_SPHERICAL>(ph, hy, a, plan, blocks, stream);
    case DIM_THREE * 4 + GEOM_CARTESIAN: return launch_pair<DIM_THREE, GEOM_CARTESIAN>(ph, hy, a, plan, blocks, stream);
    case DIM_THREE * 4 + GEOM_SPHERICAL: return launch_pair<DIM_THREE, GEOM_SPHERICAL>(ph, hy, a, plan, blocks, stream);
    case DIM_THREE * 4 + GEOM_POLAR: return launch_pair<DIM_THREE, GEOM_POLAR>(ph, hy, a, plan, blocks, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mcrat
