// radfield.hip -- the radiation field on the hydro mesh: the resident photons located in the staged frame and their moments summed per hydro cell
// or per (radius, polar cosine) shell (mcrat_hip_radiation_field, mcrat_hip_pool_radiation_field).  One lane per slot, a grid-stride loop, with the
// per-photon rules of radfield_plan.hpp and the loop's own cell look-up, azimuth and boost (physics.hpp).  A counted photon reads flags, type,
// weight, r0 .. r2, p0 .. p3 and num_scatt -- 74 bytes, coalesced --, then two dependent gathers for its cell (the covered-octant entry and the cell's
// record, or the bucket's record and one list entry) and one for the cell's temperature: the pass is bound by the latency of those gathers, as a
// sightline step is.  The edges of SHELLS are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan; the forms of both are bin_accumulate.hpp's:
//   LDS      SHELLS whose six planes fit: the workgroup owns a private copy in LDS, adds into it with LDS atomics and flushes the bins it touched
//            once, when it has run out of slots (flush_lds_bins).
//   global   CELLS, and SHELLS beyond LDS: hardware f64 atomic adds that return nothing, and an integer atomic for the count, straight into the
//            accumulator in HBM.  A wavefront's 64 photons may sit in 64 different cells or all in one cell of the jet core.  So the wavefront first
//            finds out which of its lanes share a bin: every lane writes its number into a one-byte table in LDS at a hash of its bin and reads back
//            who won the entry; a lane that lost to a lane of the same bin marks the entry.  A lane that won an unmarked entry has a bin of its own
//            and adds what it holds, all such lanes in the same six instructions (match_alone).  Only the rest -- lanes of shared bins, and the few
//            that lost an entry to another bin -- go through the rounds (add_shared_bins): one per distinct bin, the group summed over the wavefront,
//            its first lane adding for all.  Spread photons take no round at all, a wavefront inside one cell takes one.
// The accumulator in HBM is plane-major or bin-major (radfield_plan.hpp, MCRAT_RADFIELD_BIN_MAJOR); a bin-major one is transposed into the planes
// the caller receives by radfield_transpose_kernel.
// Counts are exact.  The five sums per bin depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "physics.hpp"
#include "radfield_plan.hpp"
#include "bin_accumulate.hpp"

namespace mcrat {

namespace {

constexpr int RF_SUMS = RADFIELD_PLANES - 1;      // W, WE_lab, WE_comv, WNS, WT behind the count

// the accumulator's address rule in HBM: plane- or bin-major (radfield_plan.hpp)
struct RadfieldWord {
    double *acc;
    size_t nb;
    __device__ __forceinline__ double *operator()(int plane, size_t bin) const { return acc + radfield_word(RADFIELD_BIN_MAJOR, plane, bin, nb); }
};

template <int DIMS, int GEOM, bool SHELLS, bool LDS_PLANES>
__global__ __launch_bounds__(RADFIELD_BLOCK) void radfield_kernel(PhotonDev ph, HydroDev hy, RadfieldDev a)
{
    extern __shared__ double s_mem[];
    // LDS: the staged edges, the workgroup's three counters, then its copy of the planes (LDS path) or the wavefronts' match tables (global path)
    const int n_staged = SHELLS ? a.n_r + a.n_mu + 2 : 0;
    double *s_r_edges = s_mem, *s_mu_edges = s_mem + (a.n_r + 1);
    unsigned long long *s_scalar = reinterpret_cast<unsigned long long *>(s_mem + n_staged);
    double *s_planes = reinterpret_cast<double *>(s_scalar + RADFIELD_N_SCALARS);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < n_staged; k += RADFIELD_BLOCK) s_mem[k] = a.staged[k];
    if (tid < RADFIELD_N_SCALARS) s_scalar[tid] = 0ull;
    const size_t nb = (size_t)a.n_bins;
    const PlaneMajor at_lds{s_planes, nb};
    const RadfieldWord at{a.acc, nb};
    if constexpr (LDS_PLANES)
        for (size_t k = tid; k < (size_t)RADFIELD_PLANES * nb; k += RADFIELD_BLOCK) s_planes[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
    __syncthreads();
    unsigned char *const s_match = reinterpret_cast<unsigned char *>(s_planes) + ((size_t)(tid >> 6) << OBSERVE_MATCH_BITS);      // (global path) this wavefront's table

    const unsigned n = (unsigned)a.n_slots, stride = gridDim.x * RADFIELD_BLOCK;
    for (unsigned base = blockIdx.x * RADFIELD_BLOCK; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap; the same trips for every lane of the workgroup)
        const unsigned i = base + tid;
        bool live = i < n;
        double w = 0;
        if (live) {
            w = ph.weight[i];
            live = observe_observable(ph.flags[i], ph.type[i], w);
        }
        int cell = -1, bin = -1;
        double v[RF_SUMS] = {0, 0, 0, 0, 0};              // w, w * e_lab, w * e_comv, w * num_scatt, w * temp
        if (live) {
            const double r0 = ph.r0[i], r1 = ph.r1[i], r2 = ph.r2[i];
            const double p[4] = {ph.p0[i], ph.p1[i], ph.p2[i], ph.p3[i]};
            const double ns = ph.num_scatt[i];
            double a0, a1, a2;
            phys::hydro_coords<DIMS, GEOM>(r0, r1, r2, a0, a1, a2);
            FatCell hit;
            hit.cell = -1;
            if (phys::in_domain<DIMS>(hy, a0, a1, a2))
                phys::find_in_bucket<DIMS>(hy, phys::grid_bucket_of<DIMS>(hy.grid, a0, a1, a2), a0, a1, a2, hit);
            cell = hit.cell;
            if (cell >= hy.M) cell = -1;                      // (cannot happen: the look-up names cells of hy; nothing may be added past the accumulator)
            if (cell >= 0) {
                double cphi, sphi, beta[3], comv[4];
                phys::relocation_azimuth<DIMS, GEOM>(r0, r1, a0, cphi, sphi);
                phys::beta_from_record<DIMS>(hit.a, hit.b, hit.c, cphi, sphi, beta);
                phys::boost_with<false>(beta, hit.gam, phys::kf_of_gamma(hit.gam), p, comv);
                v[1] = w * radfield_e_lab(p[0]);
                v[2] = w * (comv[0] * C_LIGHT);
                v[3] = w * ns;
                v[4] = w * hy.temp[cell];
                if constexpr (SHELLS) {
                    double r, mu;
                    radfield_r_mu(r0, r1, r2, r, mu);
                    bin = radfield_shell_bin(s_r_edges, a.n_r, s_mu_edges, a.n_mu, r, mu);      // < n_bins, an int (radfield_check)
                } else {
                    bin = cell;                               // < hy.M == n_bins
                }
            }
        }
        const unsigned long long m_live = __ballot(live), m_unlocated = __ballot(live && cell < 0), m_outside = __ballot(cell >= 0 && bin < 0);
        if (lane == 0) {
            if (m_live) add_u64(&s_scalar[RF_N_OBSERVABLE], (unsigned long long)__popcll(m_live));
            if (m_unlocated) add_u64(&s_scalar[RF_N_UNLOCATED], (unsigned long long)__popcll(m_unlocated));
            if (m_outside) add_u64(&s_scalar[RF_N_OUTSIDE], (unsigned long long)__popcll(m_outside));
        }
        v[0] = w;
        const bool has = bin >= 0;
        if constexpr (LDS_PLANES) {
            if (has) add_bin<RF_SUMS>(at_lds, bin, 1ull, v);
        } else {
            const bool alone = match_alone(s_match, lane, bin, has);
            if (alone) add_bin<RF_SUMS>(at, bin, 1ull, v);
            add_shared_bins<RF_SUMS>(at, lane, alone ? -1 : bin, v);
        }
    }
    __syncthreads();
    if (tid < RADFIELD_N_SCALARS && s_scalar[tid]) add_u64(&a.head[tid], s_scalar[tid]);
    if constexpr (LDS_PLANES) flush_lds_bins<RF_SUMS, RADFIELD_BLOCK>(s_planes, nb, at, tid);
}

// a bin-major accumulator into the six planes the caller receives: one lane per bin, the stores coalesced per plane
__global__ __launch_bounds__(RADFIELD_BLOCK) void radfield_transpose_kernel(const double *records, double *planes, int n_bins)
{
    const size_t nb = (size_t)n_bins;
    for (size_t b = (size_t)blockIdx.x * RADFIELD_BLOCK + threadIdx.x; b < nb; b += (size_t)gridDim.x * RADFIELD_BLOCK)
#pragma unroll
        for (int k = 0; k < RADFIELD_PLANES; ++k) planes[(size_t)k * nb + b] = records[b * RADFIELD_RECORD_WORDS + k];
}

template <int DIMS, int GEOM, bool SHELLS, bool LDS_PLANES>
hipError_t launch_one(const PhotonDev &ph, const HydroDev &hy, const RadfieldDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return launch_with_lds(&radfield_kernel<DIMS, GEOM, SHELLS, LDS_PLANES>, blocks, RADFIELD_BLOCK, lds_bytes, lds_bytes, stream, ph, hy, a);
}

template <int DIMS, int GEOM>
hipError_t launch_pair(const PhotonDev &ph, const HydroDev &hy, const RadfieldDev &a, const RadfieldPlan &plan, int blocks, hipStream_t stream)
{
    if (plan.s.mode == RADFIELD_CELLS) return launch_one<DIMS, GEOM, false, false>(ph, hy, a, blocks, plan.lds_bytes, stream);
    if (plan.s.path == OBSERVE_PATH_LDS) return launch_one<DIMS, GEOM, true, true>(ph, hy, a, blocks, plan.lds_bytes, stream);
    return launch_one<DIMS, GEOM, true, false>(ph, hy, a, blocks, plan.lds_bytes, stream);
}

}  // namespace

// The nine (DIMENSIONS, geometry) pairs the engine accepts, as launch_sightline switches over them.  The caller has zeroed the block's head and
// accumulator, copied the edges behind them and sized the grid (radfield_plan.hpp, radfield_grid); hy is the frame the photons are located in.
hipError_t launch_radfield(const KernelConfig &kc, const PhotonDev &ph, const HydroDev &hy, const RadfieldDev &a, const RadfieldPlan &plan, int blocks,
                           hipStream_t stream)
{
    if (a.n_slots <= 0 || blocks <= 0 || a.n_bins != plan.n_bins) return hipErrorInvalidValue;
    if (plan.s.mode == RADFIELD_CELLS && (plan.s.path != OBSERVE_PATH_GLOBAL || a.n_bins != hy.M)) return hipErrorInvalidValue;
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

hipError_t launch_radfield_transpose(const double *records, double *planes, int n_bins, int cus, hipStream_t stream)
{
    if (n_bins <= 0) return hipErrorInvalidValue;
    const int blocks = accumulate_grid(n_bins, RADFIELD_BLOCK, cus, RADFIELD_MAX_GROUPS_PER_CU);
    hipLaunchKernelGGL(radfield_transpose_kernel, dim3((unsigned)blocks), dim3(RADFIELD_BLOCK), 0, stream, records, planes, n_bins);
    return hipGetLastError();
}

}  // namespace mcrat
