// radfield.hip -- the radiation field on the hydro mesh: the resident photons located in the staged frame and their moments summed per hydro cell
// or per (radius, polar cosine) shell (mcrat_hip_radiation_field, mcrat_hip_pool_radiation_field).  One lane per slot, a grid-stride loop, with the
// per-photon rules of radfield_plan.hpp and the loop's own cell look-up, azimuth and boost (physics.hpp).  A counted photon reads flags, type,
// weight, r0 .. r2, p0 .. p3 and num_scatt -- 74 bytes, coalesced --, then two dependent gathers for its cell (the covered-octant entry and the cell's
// record, or the bucket's record and one list entry) and one for the cell's temperature: the pass is bound by the latency of those gathers, as a
// sightline step is.  The edges of SHELLS are staged into LDS once per workgroup.
//
// Two accumulation paths, picked by the plan:
//   LDS      SHELLS whose six planes fit: the workgroup owns a private copy in LDS, adds into it with LDS atomics and flushes the bins it touched
//            once, when it has run out of slots (observe.hip's form).
//   global   CELLS, and SHELLS beyond LDS: hardware f64 atomic adds that return nothing, and an integer atomic for the count, straight into the
//            accumulator in HBM.  A wavefront's 64 photons may sit in 64 different cells or all in one cell of the jet core.  So the wavefront first
//            finds out which of its lanes share a bin: every lane writes its number into a one-byte table in LDS at a hash of its bin and reads back
//            who won the entry; a lane that lost to a lane of the same bin marks the entry.  A lane that won an unmarked entry has a bin of its own
//            and adds what it holds, all such lanes in the same six instructions.  Only the rest -- lanes of shared bins, and the few that lost an
//            entry to another bin -- go through observe.hip's rounds: one per distinct bin, the group summed over the wavefront, its first lane
//            adding for all.  Spread photons take no round at all, a wavefront inside one cell takes one.
// The accumulator in HBM is plane-major or bin-major (radfield_plan.hpp, MCRAT_RADFIELD_BIN_MAJOR); a bin-major one is transposed into the planes
// the caller receives by radfield_transpose_kernel.
// Counts are exact.  The five sums per bin depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "physics.hpp"
#include "radfield_plan.hpp"

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

// one bin's six adds
template <bool BIN_MAJOR>
__device__ __forceinline__ void add_bin(double *acc, size_t nb, int bin, unsigned long long m, double w, double we_lab, double we_comv, double wns, double wt)
{
    add_u64(reinterpret_cast<unsigned long long *>(acc) + radfield_word(BIN_MAJOR, RF_COUNT, (size_t)bin, nb), m);
    add_f64(acc + radfield_word(BIN_MAJOR, RF_W, (size_t)bin, nb), w);
    add_f64(acc + radfield_word(BIN_MAJOR, RF_WE_LAB, (size_t)bin, nb), we_lab);
    add_f64(acc + radfield_word(BIN_MAJOR, RF_WE_COMV, (size_t)bin, nb), we_comv);
    add_f64(acc + radfield_word(BIN_MAJOR, RF_WNS, (size_t)bin, nb), wns);
    add_f64(acc + radfield_word(BIN_MAJOR, RF_WT, (size_t)bin, nb), wt);
}

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
    if constexpr (LDS_PLANES)
        for (size_t k = tid; k < (size_t)RADFIELD_PLANES * nb; k += RADFIELD_BLOCK) s_planes[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
    __syncthreads();
    unsigned char *const s_match = reinterpret_cast<unsigned char *>(s_planes) + ((size_t)(tid >> 6) << RADFIELD_MATCH_BITS);      // (global path) this wavefront's table

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
        double we_lab = 0, we_comv = 0, wns = 0, wt = 0;
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
                we_lab = w * radfield_e_lab(p[0]);
                we_comv = w * (comv[0] * C_LIGHT);
                wns = w * ns;
                wt = w * hy.temp[cell];
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
        const bool has = bin >= 0;
        if constexpr (LDS_PLANES) {
            if (has) add_bin<false>(s_planes, nb, bin, 1ull, w, we_lab, we_comv, wns, wt);
        } else {
            // which lanes share a bin: the table entry at a hash of the bin goes to one of the lanes that want it
            const unsigned h = ((unsigned)bin * 2654435761u) >> (32 - RADFIELD_MATCH_BITS);
            if (has) s_match[h] = (unsigned char)lane;
            __syncthreads();
            const int owner = has ? (int)s_match[h] : lane;
            const int owner_bin = __shfl(bin, owner, 64);
            __syncthreads();
            if (has && owner != lane && owner_bin == bin) s_match[h] = 64;      // the owner has company
            __syncthreads();
            const bool alone = has && owner == lane && s_match[h] == (unsigned char)lane;
            if (alone) add_bin<RADFIELD_BIN_MAJOR>(a.acc, nb, bin, 1ull, w, we_lab, we_comv, wns, wt);
            // the rest, group by group of the lanes that share a bin (the others contribute +0.0, which changes no sum)
            unsigned long long todo = __ballot(has && !alone);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int lb = __shfl(bin, leader, 64);
                const bool mine = !alone && bin == lb;
                const unsigned long long group = __ballot(mine);
                todo &= ~group;
                const int m = __popcll(group);
                double gw = w, gl = we_lab, gc = we_comv, gn = wns, gt = wt;
                if (m > 1) {
                    gw = wave_sum(mine ? w : 0.0); gl = wave_sum(mine ? we_lab : 0.0); gc = wave_sum(mine ? we_comv : 0.0);
                    gn = wave_sum(mine ? wns : 0.0); gt = wave_sum(mine ? wt : 0.0);
                }
                if (lane == leader) add_bin<RADFIELD_BIN_MAJOR>(a.acc, nb, lb, (unsigned long long)m, gw, gl, gc, gn, gt);
            }
        }
    }
    __syncthreads();
    if (tid < RADFIELD_N_SCALARS && s_scalar[tid]) add_u64(&a.head[tid], s_scalar[tid]);
    if constexpr (LDS_PLANES) {
        const unsigned long long *const s_count = reinterpret_cast<const unsigned long long *>(s_planes);
        for (size_t b = tid; b < nb; b += RADFIELD_BLOCK) {
            const unsigned long long m = s_count[b];
            if (!m) continue;
            add_bin<RADFIELD_BIN_MAJOR>(a.acc, nb, (int)b, m, s_planes[RF_W * nb + b], s_planes[RF_WE_LAB * nb + b], s_planes[RF_WE_COMV * nb + b],
                                        s_planes[RF_WNS * nb + b], s_planes[RF_WT * nb + b]);
        }
    }
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
    if (lds_bytes > 64 * 1024) {               // more than the default 64 KB of dynamic LDS has to be asked for (per device: asked every time)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&radfield_kernel<DIMS, GEOM, SHELLS, LDS_PLANES>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((radfield_kernel<DIMS, GEOM, SHELLS, LDS_PLANES>), dim3(blocks), dim3(RADFIELD_BLOCK), lds_bytes, stream, ph, hy, a);
    return hipGetLastError();
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
    const long long want = ((long long)n_bins + RADFIELD_BLOCK - 1) / RADFIELD_BLOCK, cap = (long long)(cus > 0 ? cus : 256) * RADFIELD_MAX_GROUPS_PER_CU;
    hipLaunchKernelGGL(radfield_transpose_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(RADFIELD_BLOCK), 0, stream, records, planes, n_bins);
    return hipGetLastError();
}

}  // namespace mcrat
