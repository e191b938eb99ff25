// events.hip -- detected-photon event lists (mcrat_hip_observe_events, mcrat_hip_pool_observe_events): the accepted (photon, observer) pairs inside
// a window of detection time and energy, one row each, in a fully specified order (events_plan.hpp).  The kernels of one call, all on one stream,
// none of them waiting for the host:
//   count    one wavefront per chunk of slots (events_chunk_slots), one lane per slot and trip, every counted slot through the observers one by
//            one with the per-pair rules of sky_plan.hpp.  Ballots give the chunk's events per observer -- count[o][chunk] -- and the per-observer
//            counters; the OR of the event keys and of their complements goes to the head with integer atomics (any order gives the same bits).
//   scan     one workgroup: the exclusive prefix sum of the table in (observer, chunk) order.  It is every chunk's first row per observer, and at
//            the observers' boundaries it is offsets.
//   write    the count kernel's walk once more.  An event's row is  first row of its chunk + events of the chunk's earlier trips + lanes below
//            it in the ballot: no atomic decides a position.  BY_PHOTON writes the row's columns (emit_row); BY_TIME writes (key(t), row) and
//            the row's slot.
//   sort     BY_TIME: a stable LSD radix sort of the pairs, EVENTS_DIGIT_BITS bits a pass, three kernels a pass -- a histogram per tile of
//            EVENTS_SORT_TILE pairs, the scan over (digit, tile), and a scatter that ranks a tile's pairs in order: a strip of EVENTS_BLOCK pairs
//            at a time, within a wavefront by ballot matching (the lanes with my digit below me), across wavefronts and strips through per-digit
//            counts in LDS.  The passes of a key digit read the masks first and return when the digit is the same in all keys.
//   gather   BY_TIME: sorted position j takes the row of pair j: its slot, its observer from offsets, its columns by emit_row.
// Every loop is bounded by the slot count, the rows, the observers, the digits or the 64 lanes of a wavefront; no workgroup waits on another.
// Every value in a row is one of the documented IEEE expressions, and the order does not depend on timing: the list is bit-reproducible.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "resample_plan.hpp"
#include "events_plan.hpp"

namespace mcrat {

namespace {

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, mask, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask, 64);
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int delta)
{
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, delta, 64), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), delta, 64);
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// one slot as the count and write kernels read it
struct Slot {
    bool live;
    double p0, p1, p2, p3, r0, r1, r2, clock, e;
};
__device__ __forceinline__ Slot load_slot(const PhotonDev &ph, const EventsDev &a, unsigned i, bool in_range)
{
    Slot s{};
    s.live = in_range;
    s.clock = a.time_now;
    if (s.live) s.live = observe_observable(ph.flags[i], ph.type[i], ph.weight[i]);
    if (s.live) {
        s.p0 = ph.p0[i]; s.p1 = ph.p1[i]; s.p2 = ph.p2[i]; s.p3 = ph.p3[i]; s.r0 = ph.r0[i]; s.r1 = ph.r1[i]; s.r2 = ph.r2[i];
        if (a.clocks) s.clock = a.clocks[i / (unsigned)a.slots_per_clock];
    }
    s.e = observe_energy(s.p0);
    return s;
}
// whether observer o accepts the slot, and then its detection time and whether the pair lies in the window
__device__ __forceinline__ bool pair_accepted(const Slot &s, const EventsDev &a, int o, double &t, bool &inside)
{
    const int no = a.n_obs;
    const double n0 = a.staged[o], n1 = a.staged[no + o], n2 = a.staged[2 * no + o];
    const bool accepted = s.live && sky_accepted(s.p0, s.p1, s.p2, s.p3, n0, n1, n2, a.staged[3 * no + o]);
    t = 0.0; inside = false;
    if (accepted) {
        t = sky_t_det(s.clock, s.r0, s.r1, s.r2, n0, n1, n2);
        inside = events_in_window(t, s.e, a.t_lo, a.t_hi, a.e_lo, a.e_hi);
    }
    return accepted;
}

// ------------------------------------------------------------------ count
// UNDEFINED: the call carries Q and U into the observers' frames, so the pairs whose frame is undefined are counted
template <bool UNDEFINED>
__global__ __launch_bounds__(EVENTS_BLOCK) void events_count_kernel(PhotonDev ph, EventsDev a)
{
    extern __shared__ unsigned s_count[];                            // [EVENTS_WAVES][4][n_obs]: events, accepted, outside, undefined of this wavefront
    const int no = a.n_obs, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned *mine = s_count + (size_t)wave * 4 * no, *s_events = mine, *s_accepted = mine + no, *s_outside = mine + 2 * no, *s_undefined = mine + 3 * no;
    for (int k = lane; k < 4 * no; k += EVENTS_WAVE) mine[k] = 0u;
    __syncthreads();
    const long long chunk = (long long)blockIdx.x * EVENTS_WAVES + wave;
    const bool mine_exists = chunk < (long long)a.n_chunks;              // (the same for every lane of the wavefront)
    unsigned long long k_or = 0ull, k_nand = 0ull;
    if (mine_exists) {
        const unsigned first = (unsigned)chunk * (unsigned)a.chunk_slots, n = (unsigned)a.n_slots;
        const unsigned end = n - first < (unsigned)a.chunk_slots ? n : first + (unsigned)a.chunk_slots;       // (first < n < 2^31)
        for (unsigned base = first; base < end; base += EVENTS_WAVE) {
            const unsigned i = base + lane;
            const Slot s = load_slot(ph, a, i, i < end);
            if (!__any(s.live)) continue;
            for (int o = 0; o < no; ++o) {                               // (the same trips for every lane)
                double t;
                bool inside;
                const bool accepted = pair_accepted(s, a, o, t, inside);
                bool undefined = false;
                if (UNDEFINED && accepted) {
                    double q = 0.0, u = 0.0;
                    undefined = !resample_rotation(s.p1, s.p2, s.p3, a.staged[7 * no + o], a.staged[8 * no + o], a.staged[9 * no + o], q, u);
                }
                if (inside) {
                    const unsigned long long key = events_key(t);
                    k_or |= key; k_nand |= ~key;
                }
                const unsigned long long m_accepted = __ballot(accepted);
                if (!m_accepted) continue;
                const unsigned long long m_inside = __ballot(inside), m_undefined = __ballot(undefined);
                if (lane == 0) {                                         // this wavefront's own words: no other touches them before the barrier
                    s_accepted[o] += (unsigned)__popcll(m_accepted);
                    s_events[o] += (unsigned)__popcll(m_inside);
                    s_outside[o] += (unsigned)__popcll(m_accepted & ~m_inside);
                    s_undefined[o] += (unsigned)__popcll(m_undefined);
                }
            }
        }
    }
    __syncthreads();
    if (!mine_exists) return;
    for (int o = lane; o < no; o += EVENTS_WAVE) {
        a.table[(size_t)o * (size_t)a.n_chunks + (size_t)chunk] = (unsigned long long)s_events[o];
        if (s_accepted[o]) atomicAdd(&a.n_accepted[o], (unsigned long long)s_accepted[o]);
        if (s_outside[o]) atomicAdd(&a.n_outside[o], (unsigned long long)s_outside[o]);
        if (s_undefined[o]) atomicAdd(&a.n_undefined[o], (unsigned long long)s_undefined[o]);
    }
    for (int off = 32; off > 0; off >>= 1) { k_or |= shfl_xor_u64(k_or, off); k_nand |= shfl_xor_u64(k_nand, off); }
    if (lane == 0 && (k_or | k_nand)) { atomicOr(a.key_or, k_or); atomicOr(a.key_nand, k_nand); }
}

// ------------------------------------------------------------------ the sort's gate
// What every kernel behind the write kernel asks first: the rows there are -- none when the list is empty or does not fit --, whether this pass
// runs, and the buffer it reads.  observer: a digit of the observer index (always runs); digit < 0: no pass, the buffer that holds the sorted pairs.
__device__ __forceinline__ bool sort_gate(const EventsDev &a, int observer, int digit, unsigned &n, int &src)
{
    const unsigned long long total = a.offsets[a.n_obs];
    if (total == 0ull || total > (unsigned long long)a.capacity) return false;
    n = (unsigned)total;
    const unsigned long long k_or = *a.key_or, k_and = ~*a.key_nand;
    if (digit < 0) { src = events_source_buffer(k_or, k_and, EVENTS_KEY_PASSES + events_observer_passes(a.n_obs)); return true; }
    if (!observer && !events_digit_active(k_or, k_and, digit)) return false;
    src = events_source_buffer(k_or, k_and, observer ? EVENTS_KEY_PASSES + digit : digit);
    return true;
}
__device__ __forceinline__ unsigned pair_digit(const EventsDev &a, int observer, int digit, unsigned long long key, unsigned row)
{
    if (!observer) return (unsigned)(key >> (digit * EVENTS_DIGIT_BITS)) & (unsigned)(EVENTS_DIGITS - 1);
    return ((unsigned)events_row_observer(a.offsets, a.n_obs, (unsigned long long)row) >> (digit * EVENTS_DIGIT_BITS)) & (unsigned)(EVENTS_DIGITS - 1);
}

// ------------------------------------------------------------------ scan
// The exclusive prefix sum of table[0 .. m) in place, by one workgroup: EVENTS_SCAN_ITEMS consecutive entries per thread and step, the step's total
// carried on.  With offsets: entry o * per_segment's prefix is offsets[o], the total offsets[n_segments] (the count table).  Without: a pass of the
// sort, gated like its other kernels.
template <class T>
__global__ __launch_bounds__(EVENTS_SCAN_BLOCK) void events_scan_kernel(T *table, size_t m, EventsDev a, int per_segment, bool for_offsets, int observer, int digit)
{
    __shared__ unsigned long long s_wave[EVENTS_SCAN_BLOCK / EVENTS_WAVE];
    constexpr int WAVES = EVENTS_SCAN_BLOCK / EVENTS_WAVE, ITEMS = EVENTS_SCAN_ITEMS;
    if (!for_offsets) {
        unsigned n; int src;
        if (!sort_gate(a, observer, digit, n, src)) return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long carry = 0ull;
    for (size_t base = 0; base < m; base += (size_t)EVENTS_SCAN_BLOCK * ITEMS) {       // (the same trips for every thread)
        const size_t at = base + (size_t)tid * ITEMS;
        unsigned long long v[ITEMS], sum = 0ull;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) { v[k] = at + k < m ? (unsigned long long)table[at + k] : 0ull; sum += v[k]; }
        unsigned long long incl = sum;
        for (int d = 1; d < EVENTS_WAVE; d <<= 1) {
            const unsigned long long up = shfl_up_u64(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == EVENTS_WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        unsigned long long before = 0ull, total = 0ull;
        for (int w = 0; w < WAVES; ++w) { const unsigned long long ws = s_wave[w]; if (w < wave) before += ws; total += ws; }
        unsigned long long run = carry + before + (incl - sum);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (at + k < m) {
                table[at + k] = (T)run;
                if (for_offsets && (at + k) % (size_t)per_segment == 0) a.offsets[(at + k) / (size_t)per_segment] = run;
            }
            run += v[k];
        }
        carry += total;
        __syncthreads();
    }
    if (for_offsets && tid == 0) a.offsets[a.n_obs] = carry;
}

// ------------------------------------------------------------------ a row
// Row `row` of the list: slot i of c->ph as observer o detects it.  The expressions are the definitions' (sky_plan.hpp, resample_plan.hpp).
template <bool STOKES>
__device__ __forceinline__ void emit_row(const PhotonDev &ph, const EventsDev &a, unsigned i, int o, unsigned row)
{
    const int no = a.n_obs;
    const double p0 = ph.p0[i], p1 = ph.p1[i], p2 = ph.p2[i], p3 = ph.p3[i], r0 = ph.r0[i], r1 = ph.r1[i], r2 = ph.r2[i];
    const double clock = a.clocks ? a.clocks[i / (unsigned)a.slots_per_clock] : a.time_now;
    unsigned rank = (unsigned)a.rank_base, slot = i;
    if (a.rank_stride > 0) { rank += i / (unsigned)a.rank_stride; slot = i % (unsigned)a.rank_stride; }
    a.rank[row] = (int)rank;
    a.slot[row] = (int)slot;
    a.t[row] = sky_t_det(clock, r0, r1, r2, a.staged[o], a.staged[no + o], a.staged[2 * no + o]);
    a.e[row] = observe_energy(p0);
    a.w[row] = ph.weight[i];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if constexpr (STOKES) {
        s0 = ph.s0[i]; s1 = ph.s1[i]; s2 = ph.s2[i]; s3 = ph.s3[i];
        if (a.sky_plane) (void)resample_rotation(p1, p2, p3, a.staged[7 * no + o], a.staged[8 * no + o], a.staged[9 * no + o], s1, s2);     // (undefined: as stored)
    }
    a.s0[row] = s0; a.s1[row] = s1; a.s2[row] = s2; a.s3[row] = s3;
    a.num_scatt[row] = ph.num_scatt[i];
    if (a.axes) {
        double X, Y;
        sky_xy(r0, r1, r2, a.staged[4 * no + o], a.staged[5 * no + o], a.staged[6 * no + o], a.staged[7 * no + o], a.staged[8 * no + o], a.staged[9 * no + o], X, Y);
        a.X[row] = X; a.Y[row] = Y;
    }
    a.type[row] = ph.type[i];
}

// ------------------------------------------------------------------ write
template <bool STOKES>
__global__ __launch_bounds__(EVENTS_BLOCK) void events_write_kernel(PhotonDev ph, EventsDev a)
{
    extern __shared__ unsigned s_count[];                            // [EVENTS_WAVES][n_obs]: this wavefront's events so far, per observer
    const int no = a.n_obs, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned *s_run = s_count + (size_t)wave * no;
    for (int k = lane; k < no; k += EVENTS_WAVE) s_run[k] = 0u;
    __syncthreads();
    const long long chunk = (long long)blockIdx.x * EVENTS_WAVES + wave;
    if (chunk >= (long long)a.n_chunks) return;                      // (no barrier behind this line)
    const unsigned first = (unsigned)chunk * (unsigned)a.chunk_slots, n = (unsigned)a.n_slots;
    const unsigned end = n - first < (unsigned)a.chunk_slots ? n : first + (unsigned)a.chunk_slots;
    const unsigned long long capacity = (unsigned long long)a.capacity;
    for (unsigned base = first; base < end; base += EVENTS_WAVE) {
        const unsigned i = base + lane;
        const Slot s = load_slot(ph, a, i, i < end);
        if (!__any(s.live)) continue;
        for (int o = 0; o < no; ++o) {
            double t;
            bool inside;
            (void)pair_accepted(s, a, o, t, inside);
            const unsigned long long m_inside = __ballot(inside);
            if (!m_inside) continue;
            // lane 0 alone reads and writes the running count; the others get it through a register
            unsigned run = 0u;
            if (lane == 0) { run = s_run[o]; s_run[o] = run + (unsigned)__popcll(m_inside); }
            run = (unsigned)__shfl((int)run, 0, 64);
            const unsigned long long row = a.table[(size_t)o * (size_t)a.n_chunks + (size_t)chunk] + run + (unsigned long long)__popcll(m_inside & lanes_below(lane));
            if (inside && row < capacity) {
                if (a.order == EVENTS_BY_TIME) {
                    a.keys[0][row] = events_key(t);
                    a.index[0][row] = (unsigned)row;
                    a.source[row] = i;
                } else {
                    emit_row<STOKES>(ph, a, i, o, (unsigned)row);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ sort: histogram, scatter
__global__ __launch_bounds__(EVENTS_BLOCK) void events_hist_kernel(EventsDev a, int observer, int digit)
{
    __shared__ unsigned s_hist[EVENTS_DIGITS];
    unsigned n; int src;
    if (!sort_gate(a, observer, digit, n, src)) return;              // (the same for every thread of the grid)
    const int tid = threadIdx.x;
    s_hist[tid] = 0u;
    __syncthreads();
    const unsigned long long *keys = a.keys[src];
    const unsigned *index = a.index[src];
    const unsigned first = blockIdx.x * (unsigned)EVENTS_SORT_TILE;
    for (int strip = 0; strip < EVENTS_SORT_TILE / EVENTS_BLOCK; ++strip) {
        const unsigned r = first + (unsigned)(strip * EVENTS_BLOCK + tid);
        if (r < n) atomicAdd(&s_hist[pair_digit(a, observer, digit, keys[r], index[r])], 1u);      // a count: any order gives the same
    }
    __syncthreads();
    a.sort_table[(size_t)tid * (size_t)a.n_tiles + blockIdx.x] = s_hist[tid];
}

__global__ __launch_bounds__(EVENTS_BLOCK) void events_scatter_kernel(EventsDev a, int observer, int digit)
{
    __shared__ unsigned s_base[EVENTS_DIGITS];                       // where the tile's next pair with this digit goes
    __shared__ unsigned s_wave[EVENTS_WAVES][EVENTS_DIGITS];         // the strip's pairs with this digit, per wavefront
    unsigned n; int src;
    if (!sort_gate(a, observer, digit, n, src)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_base[tid] = a.sort_table[(size_t)tid * (size_t)a.n_tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < EVENTS_WAVES; ++w) s_wave[w][tid] = 0u;
    __syncthreads();
    const unsigned long long *keys = a.keys[src];
    const unsigned *index = a.index[src];
    unsigned long long *keys_out = a.keys[src ^ 1];
    unsigned *index_out = a.index[src ^ 1];
    const unsigned first = blockIdx.x * (unsigned)EVENTS_SORT_TILE;
    for (int strip = 0; strip < EVENTS_SORT_TILE / EVENTS_BLOCK; ++strip) {     // (the same trips for every thread: the barriers)
        const unsigned r = first + (unsigned)(strip * EVENTS_BLOCK + tid);
        const bool valid = r < n;
        unsigned long long key = 0ull;
        unsigned row = 0u, d = 0u;
        if (valid) { key = keys[r]; row = index[r]; d = pair_digit(a, observer, digit, key, row); }
        unsigned long long peers = __ballot(valid);                  // -> the lanes of this wavefront that hold my digit
#pragma unroll
        for (int b = 0; b < EVENTS_DIGIT_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        const unsigned below = (unsigned)__popcll(peers & lanes_below(lane));
        if (valid && below == 0u) s_wave[wave][d] = (unsigned)__popcll(peers);     // one lane per digit present writes
        __syncthreads();
        if (valid) {
            unsigned at = s_base[d] + below;
            for (int w = 0; w < wave; ++w) at += s_wave[w][d];
            if (at < (unsigned)a.capacity) { keys_out[at] = key; index_out[at] = row; }      // (at < n by construction)
        }
        __syncthreads();
        unsigned sum = 0u;
#pragma unroll
        for (int w = 0; w < EVENTS_WAVES; ++w) { sum += s_wave[w][tid]; s_wave[w][tid] = 0u; }
        s_base[tid] += sum;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ gather
template <bool STOKES>
__global__ __launch_bounds__(EVENTS_BLOCK) void events_gather_kernel(PhotonDev ph, EventsDev a)
{
    unsigned n; int src;
    if (!sort_gate(a, 0, -1, n, src)) return;
    const unsigned j = blockIdx.x * (unsigned)EVENTS_BLOCK + threadIdx.x;
    if (j >= n) return;
    const unsigned row = a.index[src][j];
    if (row >= n) return;                                            // (never: the pairs are a permutation of the rows)
    const unsigned i = a.source[row];
    if (i >= (unsigned)a.n_slots) return;                            // (never)
    emit_row<STOKES>(ph, a, i, events_row_observer(a.offsets, a.n_obs, (unsigned long long)row), j);
}

}  // namespace

// The caller has zeroed the head and copied the staged observers and the clocks (events_plan.hpp).
hipError_t launch_events(const PhotonDev &ph, const EventsDev &a, const EventsPlan &plan, bool stokes, hipStream_t stream)
{
    if (a.n_slots <= 0) return hipSuccess;                           // offsets and counters stay zero
    if (a.n_obs != plan.n_obs || a.n_obs < 1 || a.n_obs > EVENTS_MAX_OBS || a.capacity != plan.capacity || a.capacity < 0) return hipErrorInvalidValue;
    if (a.chunk_slots != events_chunk_slots(a.n_slots) || a.n_chunks != events_n_chunks(a.n_slots) || a.order != plan.order) return hipErrorInvalidValue;
    if ((a.axes != 0) != plan.axes || (a.sky_plane != 0) != (plan.frame == STOKES_SKY_PLANE) || (a.sky_plane && !a.axes)) return hipErrorInvalidValue;
    if (a.order == EVENTS_BY_TIME && a.n_tiles != events_sort_tiles(a.capacity)) return hipErrorInvalidValue;
    const int groups = (a.n_chunks + EVENTS_WAVES - 1) / EVENTS_WAVES;
    const size_t count_lds = sizeof(unsigned) * 4 * EVENTS_WAVES * (size_t)a.n_obs, write_lds = sizeof(unsigned) * EVENTS_WAVES * (size_t)a.n_obs;
    if (stokes && a.sky_plane) hipLaunchKernelGGL(events_count_kernel<true>, dim3(groups), dim3(EVENTS_BLOCK), count_lds, stream, ph, a);
    else hipLaunchKernelGGL(events_count_kernel<false>, dim3(groups), dim3(EVENTS_BLOCK), count_lds, stream, ph, a);
    hipLaunchKernelGGL(events_scan_kernel<unsigned long long>, dim3(1), dim3(EVENTS_SCAN_BLOCK), 0, stream, a.table, (size_t)a.n_obs * (size_t)a.n_chunks, a,
                       a.n_chunks, true, 0, 0);
    if (stokes) hipLaunchKernelGGL(events_write_kernel<true>, dim3(groups), dim3(EVENTS_BLOCK), write_lds, stream, ph, a);
    else hipLaunchKernelGGL(events_write_kernel<false>, dim3(groups), dim3(EVENTS_BLOCK), write_lds, stream, ph, a);
    if (a.order == EVENTS_BY_TIME && a.n_tiles > 0) {
        EventsPass list[EVENTS_MAX_PASSES];
        const int passes = events_launch_list(a.n_obs, list);
        for (int k = 0; k < passes; ++k) {
            hipLaunchKernelGGL(events_hist_kernel, dim3(a.n_tiles), dim3(EVENTS_BLOCK), 0, stream, a, list[k].observer, list[k].digit);
            hipLaunchKernelGGL(events_scan_kernel<unsigned>, dim3(1), dim3(EVENTS_SCAN_BLOCK), 0, stream, a.sort_table, (size_t)EVENTS_DIGITS * (size_t)a.n_tiles, a,
                               1, false, list[k].observer, list[k].digit);
            hipLaunchKernelGGL(events_scatter_kernel, dim3(a.n_tiles), dim3(EVENTS_BLOCK), 0, stream, a, list[k].observer, list[k].digit);
        }
        const int gather_groups = a.n_tiles * (EVENTS_SORT_TILE / EVENTS_BLOCK);
        if (stokes) hipLaunchKernelGGL(events_gather_kernel<true>, dim3(gather_groups), dim3(EVENTS_BLOCK), 0, stream, ph, a);
        else hipLaunchKernelGGL(events_gather_kernel<false>, dim3(gather_groups), dim3(EVENTS_BLOCK), 0, stream, ph, a);
    }
    return hipGetLastError();
}

}  // namespace mcrat
