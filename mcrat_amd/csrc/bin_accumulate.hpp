// bin_accumulate.hpp -- how the binned-sum kernels add: device code, included by observe.hip, sky.hip, radfield.hip, comoving.hip and escape.hip and by nothing else.  A bin is
// a 64-bit integer count (plane 0) and N double sums (planes 1 .. N); where word `plane` of bin `bin` lies is the caller's address rule `at(plane,
// bin)`, bound to its accumulator -- plane-major for the observation cube, the comoving field and every LDS copy (PlaneMajor, PlaneBases), plane- or
// bin-major for the radiation field (radfield_word).  A lane's N values travel as double[N], N a template parameter and every loop over it unrolled: they stay in
// registers.
//
// The forms, once each:
//   add_bin            one bin's N + 1 adds: hardware atomics that return nothing, the count first, then the sums in plane order
//   match_alone        global path: which lanes of a wavefront have a bin to themselves, through the wavefront's one-byte table in LDS
//   add_shared_bins    global path: the other lanes in rounds, one per distinct bin -- the group summed over the wavefront, its first lane adds for all
//   flush_lds_bins     LDS path: the bins the workgroup touched, from its private copy to HBM
//   launch_with_lds    a launch that asks for more than the default 64 KB of dynamic LDS when it needs them
//   cube_pass          the whole pass of observe_kernel and sky_kernel over the slots and the observers, the per-photon rules supplied by a rule type
//                      (escape_bin_kernel's pass runs over a compacted list with tau and status per entry and nine planes: its own loop, these forms)
// Barriers: match_alone holds three __syncthreads().  It must be called by every lane of the workgroup the same number of times -- from loops whose
// trip counts are uniform per workgroup, with `has` false for a lane that has nothing to add.
// Counts are exact.  The sums depend on the order in which the atomics are served: they are NOT bit-reproducible from run to run; each stays within
// (m + 2) * 2^-53 * sum|term| of the exact sum of the bin's m terms (the worst case of any summation order).
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "observe_plan.hpp"

namespace mcrat {

// no-return hardware adds: ds_add_f64 / global_atomic_add_f64 and their 64-bit integer kin
__device__ __forceinline__ void add_f64(double *p, double v) { (void)unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void add_u64(unsigned long long *p, unsigned long long v) { (void)atomicAdd(p, v); }

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the observation cube's address rule, and that of every LDS copy: planes of n_bins words
struct PlaneMajor {
    double *acc;
    size_t nb;
    __device__ __forceinline__ double *operator()(int plane, size_t bin) const { return acc + ((size_t)plane * nb + bin); }
};
// ... and the same rule for the global path's adds into HBM, with the planes' bases worked out once: they are the same for every lane and stay in
// scalar registers, and a bin's adds take their addresses from them one by one.  (With PlaneMajor the compiler turns a bin's addresses into a
// chain, each the one before plus nb, and the adds of a round wait for one another's address arithmetic: 1 % of a pass that lives in the rounds.
// The LDS copies and the flush keep PlaneMajor: seven more bases there cost scalar registers and, in one kernel, a wave of occupancy.)
template <int PLANES>
struct PlaneBases {
    double *plane[PLANES];
    __device__ __forceinline__ PlaneBases(double *acc, size_t nb)
    {
#pragma unroll
        for (int k = 0; k < PLANES; ++k) plane[k] = acc + (size_t)k * nb;
    }
    __device__ __forceinline__ double *operator()(int k, size_t bin) const { return plane[k] + bin; }
};

// one bin's N + 1 adds: m photons and their N sums
template <int N, class At>
__device__ __forceinline__ void add_bin(const At &at, int bin, unsigned long long m, const double (&v)[N])
{
    add_u64(reinterpret_cast<unsigned long long *>(at(0, (size_t)bin)), m);
#pragma unroll
    for (int k = 0; k < N; ++k) add_f64(at(k + 1, (size_t)bin), v[k]);
}

// Which lanes share a bin: the table entry at a hash of the bin goes to one of the lanes that want it; a lane that lost to a lane of the same bin marks
// the entry.  -> this lane won an unmarked entry: it has a bin of its own.  s_match: this wavefront's OBSERVE_MATCH_BITS table.
__device__ __forceinline__ bool match_alone(unsigned char *s_match, int lane, int bin, bool has)
{
    const unsigned h = observe_match_hash(bin);
    if (has) s_match[h] = (unsigned char)lane;
    __syncthreads();
    const int owner = has ? (int)s_match[h] : lane;
    const int owner_bin = __shfl(bin, owner, 64);
    __syncthreads();
    if (has && owner != lane && owner_bin == bin) s_match[h] = 64;      // the owner has company
    __syncthreads();
    return has && owner == lane && s_match[h] == (unsigned char)lane;
}

// The lanes of this wavefront that have a bin (bin >= 0; -1: nothing to add, or added already), group by group of those that share one: a lane on its
// own adds what it holds, a group is summed over the wavefront (the others contribute +0.0, which changes no sum) and its first lane adds for all.
// At most 64 rounds.
template <int N, class At>
__device__ __forceinline__ void add_shared_bins(const At &at, int lane, int bin, const double (&v)[N])
{
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(bin, leader, 64);
        const bool mine = bin == lb;
        const unsigned long long group = __ballot(mine);
        todo &= ~group;
        const int m = __popcll(group);
        double g[N];
#pragma unroll
        for (int k = 0; k < N; ++k) g[k] = v[k];
        if (m > 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) g[k] = wave_sum(mine ? v[k] : 0.0);
        }
        if (lane == leader) add_bin<N>(at, lb, (unsigned long long)m, g);
    }
}

// The workgroup's plane-major copy in LDS into the accumulator in HBM: the bins that were touched, BLOCK lanes side by side.
template <int N, int BLOCK, class At>
__device__ __forceinline__ void flush_lds_bins(const double *s_planes, size_t nb, const At &at, int tid)
{
    const unsigned long long *const s_count = reinterpret_cast<const unsigned long long *>(s_planes);
    for (size_t b = tid; b < nb; b += BLOCK) {
        const unsigned long long m = s_count[b];
        if (!m) continue;
        double v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = s_planes[(size_t)(k + 1) * nb + b];
        add_bin<N>(at, (int)b, m, v);
    }
}

// attr_bytes: what the kernel is allowed when lds_bytes is beyond the default 64 KB of dynamic LDS (per device: asked every time)
template <class... Params, class... Args>
hipError_t launch_with_lds(void (*kernel)(Params...), int blocks, int block, size_t lds_bytes, size_t attr_bytes, hipStream_t stream, const Args &...args)
{
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(block), lds_bytes, stream, args...);
    return hipGetLastError();
}

// The pass of observe_kernel and sky_kernel: one lane per slot in a grid-stride loop, every counted slot through the observers one by one, into the
// seven-plane cube (OBSERVE_PLANES: count, W, WE, I, Q, U, V; with Stokes off the last four stay zero).  s_mem, the workgroup's dynamic LDS: the
// staged inputs in the block's order, its per-observer counters, then its copy of the cube (LDS path) or the wavefronts' match tables.
// Rule supplies what differs (observe_plan.hpp's and sky_plan.hpp's per-photon rules stay there):
//   Dev, BLOCK, MATCH         the kernel's argument struct, its workgroup size, whether the global path uses the match table
//   Rule(a, s_mem), n_staged  the staged layout
//   Photon, load(ph, i, q)    what a counted slot reads beside weight and Stokes vector; a slot that is not counted keeps zeros
//   Observer, observer(o)     what of observer o both rules below read: fetched once per observer, by every lane
//   accepted(q, ob, o)        observer o accepts the photon
//   bin(q, ob, clock, e, o)   its bin in the cube, or -1
template <bool LDS_CUBE, bool STOKES, class Rule>
__device__ __forceinline__ void cube_pass(const PhotonDev &ph, const typename Rule::Dev &a, double *s_mem)
{
    constexpr int BLOCK = Rule::BLOCK, N = STOKES ? 6 : 2;
    const Rule rule(a, s_mem);
    const int no = a.n_obs, n_staged = rule.n_staged;
    unsigned long long *s_accepted = reinterpret_cast<unsigned long long *>(s_mem + n_staged), *s_outside = s_accepted + no;
    double *s_cube = reinterpret_cast<double *>(s_outside + no);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < n_staged; k += BLOCK) s_mem[k] = a.staged[k];
    for (int k = tid; k < 2 * no; k += BLOCK) s_accepted[k] = 0ull;
    const size_t nb = (size_t)a.n_bins;
    const PlaneMajor at_lds{s_cube, nb}, at_flush{a.cube, nb};
    if constexpr (LDS_CUBE)
        for (size_t k = tid; k < (size_t)OBSERVE_PLANES * nb; k += BLOCK) s_cube[k] = 0.0;      // (+0.0 and the integer 0 are the same bits)
    __syncthreads();
    unsigned char *s_match = nullptr;
    if constexpr (!LDS_CUBE && Rule::MATCH)                                       // this wavefront's table
        s_match = reinterpret_cast<unsigned char *>(s_cube) + ((size_t)(tid >> 6) << OBSERVE_MATCH_BITS);

    const unsigned n = (unsigned)a.n_slots, stride = gridDim.x * BLOCK;
    for (unsigned base = blockIdx.x * BLOCK; base < n; base += stride) {          // (n < 2^31 and stride <= 2^19: no wrap; the same trips for every lane of the workgroup)
        const unsigned i = base + tid;
        bool live = i < n;
        double w = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, clock = a.time_now;
        typename Rule::Photon q{};
        if (live) {
            w = ph.weight[i];
            live = observe_observable(ph.flags[i], ph.type[i], w);
        }
        if (live) {
            rule.load(ph, i, q);
            if constexpr (STOKES) { s0 = ph.s0[i]; s1 = ph.s1[i]; s2 = ph.s2[i]; s3 = ph.s3[i]; }
            if (a.clocks) clock = a.clocks[i / (unsigned)a.slots_per_clock];
        }
        const double e = observe_energy(q.p0);
        double v[N];
        v[0] = w; v[1] = w * e;
        if constexpr (STOKES) { v[2] = w * s0; v[3] = w * s1; v[4] = w * s2; v[5] = w * s3; }
        for (int o = 0; o < no; ++o) {                                                // (the same trips for every lane of the workgroup)
            const typename Rule::Observer ob = rule.observer(o);
            const bool accepted = live && rule.accepted(q, ob, o);
            int bin = -1;
            if (accepted) bin = rule.bin(q, ob, clock, e, o);                         // < n_bins, an int (the plan)
            const unsigned long long m_accepted = __ballot(accepted), m_outside = __ballot(accepted && bin < 0);
            if (lane == 0) {
                if (m_accepted) add_u64(&s_accepted[o], (unsigned long long)__popcll(m_accepted));
                if (m_outside) add_u64(&s_outside[o], (unsigned long long)__popcll(m_outside));
            }
            const bool has = bin >= 0;
            if constexpr (LDS_CUBE) {
                if (has) add_bin<N>(at_lds, bin, 1ull, v);
            } else {
                const PlaneBases<N + 1> at(a.cube, nb);                           // (the same for every trip: worked out once)
                bool alone = false;
                if constexpr (Rule::MATCH) {
                    alone = match_alone(s_match, lane, bin, has);
                    if (alone) add_bin<N>(at, bin, 1ull, v);
                }
                add_shared_bins<N>(at, lane, alone ? -1 : bin, v);
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < no; k += BLOCK) {
        if (s_accepted[k]) add_u64(&a.n_accepted[k], s_accepted[k]);
        if (s_outside[k]) add_u64(&a.n_outside[k], s_outside[k]);
    }
    if constexpr (LDS_CUBE) flush_lds_bins<N, BLOCK>(s_cube, nb, at_flush, tid);
}

}  // namespace mcrat
