// resample.hip -- sky observations with a resampling axis and a choice of Stokes frame (mcrat_hip_observe_sky_resampled,
// mcrat_hip_pool_observe_sky_resampled): observe_sky's pass -- one lane per slot in a grid-stride loop, every counted slot through the observers one
// by one, with the per-photon rules of sky_plan.hpp -- and behind the observer a replica axis: an accepted, binned photon adds k times its terms to
// replica rho, k = k(photon identity, rho) from a keyed Philox block (resample_plan.hpp).  With SKY_PLANE the photon's Q and U are first carried into
// the observer's frame (resample_rotation); AS_STORED is instantiated without it and pays nothing for it.
//
// Three accumulation paths, picked by the plan; the forms are bin_accumulate.hpp's:
//   LDS      the whole cube fits: the workgroup owns a private copy in LDS, adds into it with LDS atomics and flushes the bins it touched once.
//   sliced   one replica's sub-cube fits, the cube does not (a bootstrap cube is B times a sky cube): the replica axis is cut into slices of
//            slice_reps replicas.  A workgroup owns one slice's sub-cube [n_obs][slice_reps][...] in LDS, walks ALL slots and adds only the replicas
//            of its slice: a jackknife photon whose group lies elsewhere is dropped right after the hash, before its momentum, position and Stokes
//            columns are read; a bootstrap photon draws only the Philox blocks of the slice's replicas.  One flush at the end, to the slice's place
//            in the cube.  The per-observer counters are added by the workgroups of slice 0 alone.  LDS is this path with one slice.
//   global   one replica's sub-cube does not fit: atomics straight into the cube in HBM, the replica inside the bin index.  NONE and JACKKNIFE
//            have one bin per (photon, observer): the match table and the rounds exactly as sky_kernel's global path.  BOOTSTRAP goes through the
//            replicas one by one, each a round of the match table; the lanes that share a bin are summed over the wavefront with their
//            multiplicities (add_shared_multiples, below: add_shared_bins with the count summed instead of counted).
// Every loop is bounded by the slot count, the observers, the replicas or the 64 lanes of a wavefront; no workgroup waits on another.
// Counts are exact.  The six sums per bin depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run; each
// stays within (m + 2) * 2^-53 * sum|term| of the exact sum of the bin's m terms k * term.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "resample_plan.hpp"
#include "bin_accumulate.hpp"

namespace mcrat {

namespace {

__device__ __forceinline__ unsigned wave_sum_u(unsigned v)
{
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}

// add_shared_bins for lanes that hold k photons each (v: k times the terms): the group's multiplicities are summed like its values.  At most 64 rounds.
template <int N, class At>
__device__ __forceinline__ void add_shared_multiples(const At &at, int lane, int bin, unsigned k, const double (&v)[N])
{
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(bin, leader, 64);
        const bool mine = bin == lb;
        const unsigned long long group = __ballot(mine);
        todo &= ~group;
        unsigned m = k;
        double g[N];
#pragma unroll
        for (int j = 0; j < N; ++j) g[j] = v[j];
        if (__popcll(group) > 1) {
            m = wave_sum_u(mine ? k : 0u);
#pragma unroll
            for (int j = 0; j < N; ++j) g[j] = wave_sum(mine ? v[j] : 0.0);
        }
        if (lane == leader) add_bin<N>(at, lb, (unsigned long long)m, g);
    }
}

// where a bin of a slice's sub-cube [n_obs][slice_reps][per_rep] lies in the cube [n_obs][n_rep][per_rep]: the flush's address rule
struct SliceAt {
    double *cube;
    size_t nb;
    int slice_bins, n_rep, rep_lo, per_rep;      // slice_bins = slice_reps * per_rep
    __device__ __forceinline__ double *operator()(int plane, size_t bin) const
    {
        const int o = (int)bin / slice_bins, rest = (int)bin - o * slice_bins;          // rest = (rho - rep_lo) * per_rep + the bin within the replica
        return cube + ((size_t)plane * nb + ((size_t)(o * n_rep + rep_lo) * (size_t)per_rep + (size_t)rest));
    }
};

template <bool LDS_CUBE, bool STOKES, bool SKY_PLANE, bool IMAGE>
__global__ __launch_bounds__(RESAMPLE_BLOCK) void resample_kernel(PhotonDev ph, ResampleDev a)
{
    extern __shared__ double s_mem[];
    constexpr int BLOCK = RESAMPLE_BLOCK, N = STOKES ? 6 : 2;
    static_assert(!SKY_PLANE || STOKES, "nothing to rotate with Stokes off");
    const int no = a.n_obs, n_t = a.n_t, n_e = a.n_e, n_x = IMAGE ? a.n_x : 0, n_y = IMAGE ? a.n_y : 0;
    // the staged layout (resample_plan.hpp)
    const double *s_n0 = s_mem, *s_n1 = s_n0 + no, *s_n2 = s_n1 + no, *s_cos_acc = s_n2 + no;
    const double *s_x0 = s_cos_acc + no, *s_x1 = s_x0 + no, *s_x2 = s_x1 + no, *s_y0 = s_x2 + no, *s_y1 = s_y0 + no, *s_y2 = s_y1 + no;      // (axes)
    const double *s_t_edges = s_cos_acc + no + (a.axes ? 6 * no : 0), *s_e_edges = s_t_edges + (n_t + 1);
    const double *s_x_edges = s_e_edges + (n_e + 1), *s_y_edges = s_x_edges + (n_x + 1);                                                        // (IMAGE)
    const int n_staged = (a.axes ? 10 : 4) * no + n_t + n_e + 2 + (IMAGE ? n_x + n_y + 2 : 0);
    unsigned long long *s_accepted = reinterpret_cast<unsigned long long *>(s_mem + n_staged), *s_outside = s_accepted + no, *s_undefined = s_outside + no;
    double *s_cube = reinterpret_cast<double *>(s_undefined + no);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < n_staged; k += BLOCK) s_mem[k] = a.staged[k];

    const int mode = a.mode, n_rep = a.n_rep, per_rep = a.per_rep;
    const int reps = LDS_CUBE ? a.slice_reps : n_rep;                    // the replicas of the accumulator this workgroup adds into
    const size_t nb = (size_t)a.n_bins, nb_lds = (size_t)no * (size_t)reps * (size_t)per_rep;
    const PlaneMajor at_lds{s_cube, nb_lds};
    unsigned char *s_match = nullptr;
    if constexpr (!LDS_CUBE) s_match = reinterpret_cast<unsigned char *>(s_cube) + ((size_t)(tid >> 6) << OBSERVE_MATCH_BITS);      // this wavefront's table
    const unsigned n = (unsigned)a.n_slots, gx = (unsigned)a.grid_x, stride = gx * BLOCK, first = (blockIdx.x % gx) * BLOCK;

    for (int slice = (int)(blockIdx.x / gx); slice < a.n_slices; slice += a.grid_y) {      // (the global path has one slice)
        const int rep_lo = LDS_CUBE ? slice * reps : 0, rep_hi = rep_lo + reps < n_rep ? rep_lo + reps : n_rep;
        const bool counts = slice == 0;                                  // the per-observer counters: once per photon, not once per slice
        for (int k = tid; k < RESAMPLE_COUNTERS * no; k += BLOCK) s_accepted[k] = 0ull;
        if constexpr (LDS_CUBE)
            for (size_t k = tid; k < (size_t)OBSERVE_PLANES * nb_lds; k += BLOCK) s_cube[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
        __syncthreads();

        for (unsigned base = first; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap; the same trips for every lane of the workgroup)
            const unsigned i = base + tid;
            bool live = i < n;
            double w = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, clock = a.time_now;
            double p0 = 0, p1 = 0, p2 = 0, p3 = 0, r0 = 0, r1 = 0, r2 = 0;
            if (live) {
                w = ph.weight[i];
                live = observe_observable(ph.flags[i], ph.type[i], w);
            }
            uint32_t rank = (uint32_t)a.rank_base, slot = i;             // the photon's identity: what its draws are keyed with
            if (mode != RESAMPLE_NONE && a.rank_stride > 0) { rank += i / (unsigned)a.rank_stride; slot = i % (unsigned)a.rank_stride; }
            int group = 0;                                               // JACKKNIFE: the one replica this photon adds to
            if (mode == RESAMPLE_JACKKNIFE && live) {
                group = resample_group(a.seed, rank, slot, n_rep);
                if (!counts && (group < rep_lo || group >= rep_hi)) live = false;        // another slice's photon: nothing more is read of it
            }
            if (live) {
                p0 = ph.p0[i]; p1 = ph.p1[i]; p2 = ph.p2[i]; p3 = ph.p3[i]; r0 = ph.r0[i]; r1 = ph.r1[i]; r2 = ph.r2[i];
                if constexpr (STOKES) { s0 = ph.s0[i]; s1 = ph.s1[i]; s2 = ph.s2[i]; s3 = ph.s3[i]; }
                if (a.clocks) clock = a.clocks[i / (unsigned)a.slots_per_clock];
            }
            const double e = observe_energy(p0);
            double v[N];
            v[0] = w; v[1] = w * e;
            if constexpr (STOKES) { v[2] = w * s0; v[3] = w * s1; v[4] = w * s2; v[5] = w * s3; }
            for (int o = 0; o < no; ++o) {                                   // (the same trips for every lane of the workgroup)
                const double n0 = s_n0[o], n1 = s_n1[o], n2 = s_n2[o];
                const bool accepted = live && sky_accepted(p0, p1, p2, p3, n0, n1, n2, s_cos_acc[o]);
                int bin = -1;                                                // replica rep_lo's bin in the accumulator
                bool undefined = false;
                if (accepted) {
                    double X = 0, Y = 0;
                    if constexpr (IMAGE) sky_xy(r0, r1, r2, s_x0[o], s_x1[o], s_x2[o], s_y0[o], s_y1[o], s_y2[o], X, Y);
                    bin = resample_bin0(o, reps, s_t_edges, n_t, sky_t_det(clock, r0, r1, r2, n0, n1, n2), s_e_edges, n_e, e, s_x_edges, n_x, X, s_y_edges,
                                        n_y, Y);                             // < no * reps * per_rep - (reps - 1) * per_rep (the plan)
                    if constexpr (SKY_PLANE) {
                        double q = s1, u = s2;
                        undefined = !resample_rotation(p1, p2, p3, s_y0[o], s_y1[o], s_y2[o], q, u);
                        v[3] = w * q; v[4] = w * u;
                    }
                }
                if (counts) {
                    const unsigned long long m_accepted = __ballot(accepted), m_outside = __ballot(accepted && bin < 0), m_undefined = __ballot(undefined);
                    if (lane == 0) {
                        if (m_accepted) add_u64(&s_accepted[o], (unsigned long long)__popcll(m_accepted));
                        if (m_outside) add_u64(&s_outside[o], (unsigned long long)__popcll(m_outside));
                        if (m_undefined) add_u64(&s_undefined[o], (unsigned long long)__popcll(m_undefined));
                    }
                }
                if (mode == RESAMPLE_JACKKNIFE && bin >= 0) bin = (group >= rep_lo && group < rep_hi) ? bin + (group - rep_lo) * per_rep : -1;
                if (mode != RESAMPLE_BOOTSTRAP) {                            // one bin per (photon, observer), k = 1
                    if constexpr (LDS_CUBE) {
                        if (bin >= 0) add_bin<N>(at_lds, bin, 1ull, v);
                    } else {
                        const PlaneBases<N + 1> at(a.cube, nb);
                        const bool alone = match_alone(s_match, lane, bin, bin >= 0);
                        if (alone) add_bin<N>(at, bin, 1ull, v);
                        add_shared_bins<N>(at, lane, alone ? -1 : bin, v);
                    }
                } else {                                                     // the sample itself, then a Poisson(1) multiple per replica
                    Philox4 draw{};
                    for (int rho = rep_lo; rho < rep_hi; ++rho) {            // (the same trips for every lane of the workgroup)
                        unsigned k = 1u;
                        if (rho >= 1) {
                            if (bin >= 0 && (rho == rep_lo || ((rho - 1) & 3) == 0)) draw = resample_block(a.seed, rank, slot, (uint32_t)(rho - 1) >> 2, RESAMPLE_BOOTSTRAP);
                            k = resample_bootstrap_k(draw, rho);
                        }
                        const int b = (bin >= 0 && k > 0u) ? bin + (rho - rep_lo) * per_rep : -1;
                        double kv[N];
#pragma unroll
                        for (int j = 0; j < N; ++j) kv[j] = (double)k * v[j];
                        if constexpr (LDS_CUBE) {
                            if (b >= 0) add_bin<N>(at_lds, b, (unsigned long long)k, kv);
                        } else {
                            const PlaneBases<N + 1> at(a.cube, nb);
                            const bool alone = match_alone(s_match, lane, b, b >= 0);
                            if (alone) add_bin<N>(at, b, (unsigned long long)k, kv);
                            add_shared_multiples<N>(at, lane, alone ? -1 : b, k, kv);
                        }
                    }
                }
                if constexpr (SKY_PLANE) { v[3] = w * s1; v[4] = w * s2; }   // the next observer starts from the stored pair
            }
        }
        __syncthreads();
        if (counts)
            for (int k = tid; k < no; k += BLOCK) {
                if (s_accepted[k]) add_u64(&a.n_accepted[k], s_accepted[k]);
                if (s_outside[k]) add_u64(&a.n_outside[k], s_outside[k]);
                if (s_undefined[k]) add_u64(&a.n_undefined[k], s_undefined[k]);
            }
        if constexpr (LDS_CUBE) {
            if (a.n_slices == 1) flush_lds_bins<N, BLOCK>(s_cube, nb_lds, PlaneMajor{a.cube, nb}, tid);
            else flush_lds_bins<N, BLOCK>(s_cube, nb_lds, SliceAt{a.cube, nb, reps * per_rep, n_rep, rep_lo, per_rep}, tid);
            __syncthreads();                                                 // the next slice zeroes what this one has flushed
        }
    }
}

template <bool LDS_CUBE, bool STOKES, bool SKY_PLANE, bool IMAGE>
hipError_t launch_one(const PhotonDev &ph, const ResampleDev &a, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return launch_with_lds(&resample_kernel<LDS_CUBE, STOKES, SKY_PLANE, IMAGE>, blocks, RESAMPLE_BLOCK, lds_bytes, OBSERVE_LDS_BUDGET, stream, ph, a);
}

template <bool LDS_CUBE, bool STOKES, bool SKY_PLANE>
hipError_t launch_image(const PhotonDev &ph, const ResampleDev &a, bool image, int blocks, size_t lds_bytes, hipStream_t stream)
{
    return image ? launch_one<LDS_CUBE, STOKES, SKY_PLANE, true>(ph, a, blocks, lds_bytes, stream)
                 : launch_one<LDS_CUBE, STOKES, SKY_PLANE, false>(ph, a, blocks, lds_bytes, stream);
}

template <bool LDS_CUBE>
hipError_t launch_frame(const PhotonDev &ph, const ResampleDev &a, bool stokes, bool sky_plane, bool image, int blocks, size_t lds_bytes, hipStream_t stream)
{
    if (!stokes) return launch_image<LDS_CUBE, false, false>(ph, a, image, blocks, lds_bytes, stream);      // nothing to rotate: the planes stay zero
    return sky_plane ? launch_image<LDS_CUBE, true, true>(ph, a, image, blocks, lds_bytes, stream)
                     : launch_image<LDS_CUBE, true, false>(ph, a, image, blocks, lds_bytes, stream);
}

}  // namespace

// The caller has zeroed the cube and the counters, copied the staged inputs and the clocks behind them (resample_plan.hpp) and sized the grid
// (resample_grid).
hipError_t launch_resample(const PhotonDev &ph, const ResampleDev &a, const ResamplePlan &plan, bool stokes, int blocks_x, int blocks_y, hipStream_t stream)
{
    if (a.n_slots <= 0) return hipSuccess;
    if (blocks_x <= 0 || blocks_x > RESAMPLE_MAX_GRID || blocks_y <= 0 || blocks_y > RESAMPLE_MAX_GRID_Y || blocks_y > plan.n_slices) return hipErrorInvalidValue;
    if ((long long)blocks_x * blocks_y > INT_MAX || a.grid_x != blocks_x || a.grid_y != blocks_y) return hipErrorInvalidValue;
    if (a.n_bins != plan.n_bins || plan.lds_bytes > OBSERVE_LDS_BUDGET || a.per_rep != plan.per_rep || a.n_rep != plan.n_rep) return hipErrorInvalidValue;
    if (a.n_obs != plan.n_obs || a.n_t != plan.n_t || a.n_e != plan.n_e || a.n_x != plan.n_x || a.n_y != plan.n_y) return hipErrorInvalidValue;
    if (a.slice_reps != plan.slice_reps || a.n_slices != plan.n_slices || a.mode != plan.mode || (a.axes != 0) != plan.axes) return hipErrorInvalidValue;
    if ((long long)plan.n_obs * plan.n_rep * plan.per_rep != plan.n_bins) return hipErrorInvalidValue;
    const bool lds = plan.path != RESAMPLE_PATH_GLOBAL, sky_plane = plan.frame == STOKES_SKY_PLANE;
    if (lds && plan.staged_bytes + (size_t)plan.slice_reps * plan.replica_bytes != plan.lds_bytes) return hipErrorInvalidValue;
    if (!lds && (plan.n_slices != 1 || plan.slice_reps != plan.n_rep)) return hipErrorInvalidValue;
    const int blocks = blocks_x * blocks_y;
    return lds ? launch_frame<true>(ph, a, stokes, sky_plane, plan.image, blocks, plan.lds_bytes, stream)
               : launch_frame<false>(ph, a, stokes, sky_plane, plan.image, blocks, plan.lds_bytes, stream);
}

}  // namespace mcrat
