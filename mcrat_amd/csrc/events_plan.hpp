// events_plan.hpp -- the host's rules for a detected-photon event list (mcrat_hip_observe_events, mcrat_hip_pool_observe_events): the refusals and
// their texts, the order-preserving key of a detection time, the layout of the block on the device, the chunks of the compaction, and the passes of
// the sort -- written once here and used by the kernels (events.hip).  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU
// test can drive them (tests/test_events_plan_cpu.py).  The observers' checks and the per-pair rules are sky_plan.hpp's, the Stokes rotation is
// resample_plan.hpp's: called, not restated.
//
// Definitions.  Which slots count, acceptance, e, t_det and (X, Y) are mcrat_hip_observe_sky's.  An accepted (photon,
// observer) pair is an event when  t_lo <= t_det < t_hi  and  e_lo <= e < e_hi, by comparisons only (a NaN coordinate is outside); every other
// accepted pair adds to n_outside[o]:  n_events[o] + n_outside[o] == n_accepted[o].  One row per event.  Observer o's rows are
// [offsets[o], offsets[o + 1]); within an observer they are ordered by (rank, slot) -- BY_PHOTON -- or by (key(t), rank, slot) -- BY_TIME --, key the
// map below.  A photon's identity (rank, slot) is observe_sky_resampled's.  The order is fully specified and every value in a row is one of the
// documented IEEE expressions, so the whole list is bit-reproducible.
//
// How the list is made (events.hip).  The slots are cut into fixed contiguous chunks (events_chunk_slots), one wavefront each.  A count kernel
// streams the slots once and fills count[o][chunk], the per-observer counters and the OR and the AND of all event keys; one scan over the table in
// (observer, chunk) order gives offsets and every chunk's first row per observer; a write kernel walks the chunks again and places each event by
// ballots and prefix popcounts.  BY_PHOTON writes the rows there.  BY_TIME writes (key, row) pairs and the row's slot, sorts the pairs with a stable
// LSD radix sort -- EVENTS_DIGIT_BITS bits a pass over key(t), least significant first, then over the observer index -- and one gather writes the rows
// in their final order.  A key digit in which OR and AND agree is the same in every key: its pass would change nothing and is skipped, by the
// kernels themselves, from the masks in device memory.
#pragma once
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "device_types.hpp"
#include "observe_plan.hpp"
#include "sky_plan.hpp"
#include "resample_plan.hpp"

namespace mcrat {

enum EventsOrder { EVENTS_BY_PHOTON = 0, EVENTS_BY_TIME = 1 };

// ------------------------------------------------------------------ refusals and their texts
// In the order they are checked.  The observers' refusals keep sky_plan.hpp's numbers (SKY_NO_BINS .. SKY_BAD_CONE); their texts are that header's
// with this product's prefix.
enum EventsRefusal {
    EVENTS_OK = 0,
    // 1 .. 6: SkyRefusal, SKY_NO_BINS .. SKY_BAD_CONE
    EVENTS_BAD_ORDER = 32,
    EVENTS_BAD_FRAME,
    EVENTS_AXES_NOT_FINITE,
    EVENTS_AXES_NOT_UNIT,
    EVENTS_AXES_NOT_ORTHOGONAL,
    EVENTS_FRAME_NEEDS_AXES,         // SKY_PLANE without ex and ey
    EVENTS_XY_NEED_AXES,             // an X or Y column asked for without ex and ey
    EVENTS_WINDOW_NAN,
    EVENTS_WINDOW_EMPTY,             // lo >= hi
    EVENTS_CAPACITY_NEGATIVE,
    EVENTS_CAPACITY_TOO_LARGE,       // rows are indexed with an int
    EVENTS_TOO_MANY_OBSERVERS
};
constexpr size_t EVENTS_TEXT_BYTES = 256;
// -> buf: the refusal's text, every one prefixed "observe_events: "
inline const char *events_refusal_text(EventsRefusal why, char (&buf)[EVENTS_TEXT_BYTES])
{
    const char *own = nullptr, *theirs = nullptr;
    switch ((int)why) {
    case EVENTS_OK: own = ""; break;
    case EVENTS_BAD_ORDER: own = "observe_events: order must be MCRAT_HIP_EVENTS_BY_PHOTON or _BY_TIME"; break;
    case EVENTS_BAD_FRAME: own = "observe_events: stokes_frame must be MCRAT_HIP_STOKES_AS_STORED or _SKY_PLANE"; break;
    case EVENTS_AXES_NOT_FINITE: own = "observe_events: a sky-plane vector holds a value that is not finite"; break;
    case EVENTS_AXES_NOT_UNIT: own = "observe_events: a sky-plane vector is not a unit vector (to 1e-12)"; break;
    case EVENTS_AXES_NOT_ORTHOGONAL: own = "observe_events: the sky-plane vectors and the direction are not orthogonal (to 1e-12)"; break;
    case EVENTS_FRAME_NEEDS_AXES: own = "observe_events: MCRAT_HIP_STOKES_SKY_PLANE needs the sky-plane vectors x0 .. x2 and y0 .. y2"; break;
    case EVENTS_XY_NEED_AXES: own = "observe_events: the X and Y columns need the sky-plane vectors x0 .. x2 and y0 .. y2"; break;
    case EVENTS_WINDOW_NAN: own = "observe_events: a bound of the window is not a number"; break;
    case EVENTS_WINDOW_EMPTY: own = "observe_events: the window needs t_lo < t_hi and e_lo < e_hi"; break;
    case EVENTS_CAPACITY_NEGATIVE: own = "observe_events: capacity must not be negative"; break;
    case EVENTS_CAPACITY_TOO_LARGE: own = "observe_events: capacity is beyond what an int row index can hold"; break;
    case EVENTS_TOO_MANY_OBSERVERS: own = "observe_events: more observers than the kernels keep counters for (512)"; break;
    default:
        if ((int)why >= 1 && (int)why <= (int)SKY_BAD_CONE) theirs = sky_refusal_text((SkyRefusal)(int)why);
        else own = "";
    }
    if (own) {
        snprintf(buf, sizeof buf, "%s", own);
    } else {
        const char *colon = strchr(theirs, ':');                 // "observe_sky: ...": the text behind the other product's prefix
        snprintf(buf, sizeof buf, "observe_events:%s", colon ? colon + 1 : theirs);
    }
    return buf;
}

// ------------------------------------------------------------------ the key of a detection time (host and device)
// The usual order-preserving map of a double's bits to an unsigned integer: with the sign bit set all bits are inverted, otherwise the sign bit is
// set.  a < b  <=>  key(a) < key(b) for all numbers, infinities included; -0.0 sorts before +0.0.  A NaN never reaches a row (the window).
MCRAT_SKY_HD inline uint64_t events_key(double t)
{
    uint64_t bits;
    memcpy(&bits, &t, sizeof bits);
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// ------------------------------------------------------------------ chunks, tiles and passes
constexpr int EVENTS_MAX_OBS = 512;              // per-wavefront counters in LDS: 16 of 4 bytes per observer, 32 KB at the most
constexpr int EVENTS_BLOCK = 256;                // threads per workgroup of the count, write, sort and gather kernels
constexpr int EVENTS_WAVE = 64;
constexpr int EVENTS_WAVES = EVENTS_BLOCK / EVENTS_WAVE;
constexpr int EVENTS_COUNTERS = 3;               // per observer: accepted, outside, frame undefined (n_events comes from offsets)
// A chunk is what one wavefront compacts: EVENTS_WAVE slots a trip, at least EVENTS_MIN_TRIPS trips, and as many more as keep the chunks of the
// largest list below EVENTS_MAX_CHUNKS (the count table is n_obs * n_chunks words).
constexpr int EVENTS_MIN_TRIPS = 8;
constexpr int EVENTS_MAX_CHUNKS = 65536;
inline int events_chunk_slots(int n_slots)
{
    const long long per_trip = (long long)EVENTS_WAVE * EVENTS_MAX_CHUNKS;
    long long trips = ((long long)(n_slots > 0 ? n_slots : 0) + per_trip - 1) / per_trip;
    if (trips < EVENTS_MIN_TRIPS) trips = EVENTS_MIN_TRIPS;
    return (int)(trips * EVENTS_WAVE);           // (n_slots < 2^31: at most 512 trips)
}
inline int events_n_chunks(int n_slots)
{
    if (n_slots <= 0) return 0;
    const int chunk = events_chunk_slots(n_slots);
    return (int)(((long long)n_slots + chunk - 1) / chunk);
}
// The sort: EVENTS_DIGIT_BITS bits a pass; one workgroup ranks EVENTS_SORT_TILE consecutive pairs a pass, EVENTS_BLOCK at a time (a strip), each
// wavefront by ballot matching, the wavefronts and strips in order through LDS.  The scan: one workgroup of EVENTS_SCAN_BLOCK threads,
// EVENTS_SCAN_ITEMS consecutive entries per thread and step.
constexpr int EVENTS_DIGIT_BITS = 8;
constexpr int EVENTS_DIGITS = 1 << EVENTS_DIGIT_BITS;
constexpr int EVENTS_KEY_PASSES = 64 / EVENTS_DIGIT_BITS;
constexpr int EVENTS_SORT_TILE = 2048;
constexpr int EVENTS_SCAN_BLOCK = 1024;
constexpr int EVENTS_SCAN_ITEMS = 4;
static_assert(EVENTS_SORT_TILE % EVENTS_BLOCK == 0 && EVENTS_DIGITS == EVENTS_BLOCK, "a strip per trip, a thread per digit");
inline int events_sort_tiles(long long capacity) { return (int)((capacity + EVENTS_SORT_TILE - 1) / EVENTS_SORT_TILE); }

// digits of the observer index behind the key's: none for one observer
MCRAT_SKY_HD inline int events_observer_passes(int n_obs)
{
    int passes = 0;
    for (unsigned most = (unsigned)(n_obs > 0 ? n_obs - 1 : 0); most; most >>= EVENTS_DIGIT_BITS) ++passes;
    return passes;
}
// whether the key's digit d (0: least significant) differs between any two keys, from the OR and the AND of all keys
MCRAT_SKY_HD inline bool events_digit_active(uint64_t key_or, uint64_t key_and, int d)
{
    return (((key_or ^ key_and) >> (d * EVENTS_DIGIT_BITS)) & (uint64_t)(EVENTS_DIGITS - 1)) != 0;
}
// The pairs ping-pong between two buffers, and a skipped pass moves nothing: a pass reads buffer (passes run before it) & 1.  `pass` counts the key's
// digits first (0 .. EVENTS_KEY_PASSES - 1), then the observer's; an observer pass always runs.  pass == all of them: where the sorted pairs are.
MCRAT_SKY_HD inline int events_source_buffer(uint64_t key_or, uint64_t key_and, int pass)
{
    int run = 0;
    for (int d = 0; d < EVENTS_KEY_PASSES && d < pass; ++d) run += events_digit_active(key_or, key_and, d) ? 1 : 0;
    if (pass > EVENTS_KEY_PASSES) run += pass - EVENTS_KEY_PASSES;
    return run & 1;
}
// One pass as the host launches it: every key digit is launched -- the kernels decide -- and the observer's digits behind them.
struct EventsPass { int observer; int digit; };      // observer: 0 a digit of key(t), 1 a digit of the observer index
constexpr int EVENTS_MAX_PASSES = EVENTS_KEY_PASSES + 2;     // (n_obs <= EVENTS_MAX_OBS: two observer digits at the most)
inline int events_launch_list(int n_obs, EventsPass (&list)[EVENTS_MAX_PASSES])
{
    int n = 0;
    for (int d = 0; d < EVENTS_KEY_PASSES; ++d) list[n++] = EventsPass{0, d};
    for (int j = 0; j < events_observer_passes(n_obs) && n < EVENTS_MAX_PASSES; ++j) list[n++] = EventsPass{1, j};
    return n;
}
// ... and the passes that run for given masks (what the kernels decide, for the tests and the benchmark): -> their number, the passes in `list`
inline int events_pass_list(uint64_t key_or, uint64_t key_and, int n_obs, EventsPass (&list)[EVENTS_MAX_PASSES])
{
    EventsPass all[EVENTS_MAX_PASSES];
    const int launched = events_launch_list(n_obs, all);
    int n = 0;
    for (int k = 0; k < launched; ++k)
        if (all[k].observer || events_digit_active(key_or, key_and, all[k].digit)) list[n++] = all[k];
    return n;
}

// ------------------------------------------------------------------ the arguments, the plan and the block
// the caller's arguments as the checks read them (host pointers)
struct EventsArgs {
    int n_obs;
    const double *n0, *n1, *n2, *cos_acc;        // [n_obs]
    const double *x0, *x1, *x2, *y0, *y1, *y2;   // [n_obs]: all six or they are not read
    double t_lo, t_hi, e_lo, e_hi;
    int order, stokes_frame;
    long long capacity;
    bool want_xy;                                // an X or Y column is asked for
};
struct EventsPlan {
    int n_obs, order, frame;
    bool axes;                                   // ex and ey are staged; X and Y are produced
    int capacity;
    size_t head_words;                           // 8-byte words one memset zeroes: the counters, offsets and the two masks
    size_t staged_doubles;                       // n0, n1, n2, cos_acc [n_obs each]; (axes) x0 .. x2, y0 .. y2 [n_obs each]
};
// The head: n_accepted, n_outside, n_frame_undefined [n_obs each]; offsets [n_obs + 1] (offsets[n_obs] is n_total); the OR of all event keys; the
// OR of all inverted event keys (so that zero is the neutral start of both: AND = ~that).
inline size_t events_head_offsets_word(const EventsPlan &p) { return (size_t)EVENTS_COUNTERS * (size_t)p.n_obs; }
inline size_t events_head_or_word(const EventsPlan &p) { return events_head_offsets_word(p) + (size_t)p.n_obs + 1; }
// The block: head; staged observers; the lists' clocks [n_clocks]; the count table, 8 bytes per (observer, chunk), observer-major; the row columns
// for `capacity` rows -- rank, slot (int), t, e, w, s0 .. s3, num_scatt and with axes X, Y (double), type (char) --; and for BY_TIME the sort's
// table, 4 bytes per (digit, tile), digit-major, the slot behind each unsorted row (4 bytes), and two buffers each of keys (8) and row indices (4).
// Every part starts on a multiple of EVENTS_ALIGN bytes.
constexpr size_t EVENTS_ALIGN = 256;
constexpr int EVENTS_F8_COLUMNS = 10;            // t, e, w, s0, s1, s2, s3, num_scatt, X, Y: the last two with axes only
struct EventsLayout {
    size_t staged_offset, clocks_offset, table_offset;
    size_t rank_offset, slot_offset, f8_offset, type_offset;         // column k of the doubles at f8_offset + k * f8_pitch
    size_t f8_pitch;
    size_t sort_table_offset, source_offset, keys_offset, index_offset;   // buffer b of the keys at keys_offset + b * keys_pitch; likewise the indices
    size_t keys_pitch, index_pitch;
    size_t total_bytes;
};
inline size_t events_align(size_t x) { return (x + EVENTS_ALIGN - 1) / EVENTS_ALIGN * EVENTS_ALIGN; }
inline EventsLayout events_layout(const EventsPlan &p, int n_slots, int n_clocks)
{
    EventsLayout l{};
    const size_t cap = (size_t)p.capacity;
    size_t at = events_align(8 * p.head_words);
    l.staged_offset = at; at = events_align(at + 8 * p.staged_doubles);
    l.clocks_offset = at; at = events_align(at + 8 * (size_t)n_clocks);
    l.table_offset = at; at = events_align(at + 8 * (size_t)p.n_obs * (size_t)events_n_chunks(n_slots));
    l.rank_offset = at; at = events_align(at + 4 * cap);
    l.slot_offset = at; at = events_align(at + 4 * cap);
    l.f8_pitch = events_align(8 * cap);
    l.f8_offset = at; at += l.f8_pitch * (size_t)(p.axes ? EVENTS_F8_COLUMNS : EVENTS_F8_COLUMNS - 2);
    l.type_offset = at; at = events_align(at + cap);
    if (p.order == EVENTS_BY_TIME) {
        l.sort_table_offset = at; at = events_align(at + 4 * (size_t)EVENTS_DIGITS * (size_t)events_sort_tiles(p.capacity));
        l.source_offset = at; at = events_align(at + 4 * cap);
        l.keys_pitch = events_align(8 * cap);
        l.keys_offset = at; at += 2 * l.keys_pitch;
        l.index_pitch = events_align(4 * cap);
        l.index_offset = at; at += 2 * l.index_pitch;
    }
    l.total_bytes = at;
    return l;
}

// The checks, in this order: the observers' -- sky_args_check's own up to the cones, asked through one bin of time and of energy --; order;
// stokes_frame; with all six of x0 .. y2 given the sky-plane vectors finite, unit, orthogonal -- sky_args_check's again, asked through a one-pixel
// image --; SKY_PLANE without them; an X or Y column without them; the window -- a bound that is not a number, then lo >= hi, time before energy --;
// the capacity negative, then beyond an int; more observers than the kernels keep counters for.  *plan is filled when EVENTS_OK.
inline EventsRefusal events_plan(const EventsArgs &a, EventsPlan *plan)
{
    const double unit_edges[2] = {0.0, 1.0};
    SkyArgs s{};
    s.n_obs = a.n_obs; s.n0 = a.n0; s.n1 = a.n1; s.n2 = a.n2; s.cos_acc = a.cos_acc;
    s.n_t = 1; s.t_edges = unit_edges; s.n_e = 1; s.e_edges = unit_edges;
    int unused = 0;
    const SkyRefusal sky = sky_args_check(s, &unused);
    if (sky != SKY_OK) return (EventsRefusal)(int)sky;           // (one of SKY_NO_BINS .. SKY_BAD_CONE: nothing else can fail with these edges)
    if (a.order != EVENTS_BY_PHOTON && a.order != EVENTS_BY_TIME) return EVENTS_BAD_ORDER;
    if (a.stokes_frame != STOKES_AS_STORED && a.stokes_frame != STOKES_SKY_PLANE) return EVENTS_BAD_FRAME;
    const bool axes = a.x0 && a.x1 && a.x2 && a.y0 && a.y1 && a.y2;
    if (axes) {
        SkyArgs pixel = s;
        pixel.x0 = a.x0; pixel.x1 = a.x1; pixel.x2 = a.x2; pixel.y0 = a.y0; pixel.y1 = a.y1; pixel.y2 = a.y2;
        pixel.n_x = pixel.n_y = 1; pixel.x_edges = pixel.y_edges = unit_edges;
        switch (sky_args_check(pixel, &unused)) {
        case SKY_AXES_NOT_FINITE: return EVENTS_AXES_NOT_FINITE;
        case SKY_AXES_NOT_UNIT: return EVENTS_AXES_NOT_UNIT;
        case SKY_AXES_NOT_ORTHOGONAL: return EVENTS_AXES_NOT_ORTHOGONAL;
        default: break;
        }
    }
    if (a.stokes_frame == STOKES_SKY_PLANE && !axes) return EVENTS_FRAME_NEEDS_AXES;
    if (a.want_xy && !axes) return EVENTS_XY_NEED_AXES;
    if (a.t_lo != a.t_lo || a.t_hi != a.t_hi || a.e_lo != a.e_lo || a.e_hi != a.e_hi) return EVENTS_WINDOW_NAN;
    if (!(a.t_lo < a.t_hi) || !(a.e_lo < a.e_hi)) return EVENTS_WINDOW_EMPTY;
    if (a.capacity < 0) return EVENTS_CAPACITY_NEGATIVE;
    if (a.capacity > (long long)INT_MAX) return EVENTS_CAPACITY_TOO_LARGE;
    if (a.n_obs > EVENTS_MAX_OBS) return EVENTS_TOO_MANY_OBSERVERS;
    EventsPlan p{};
    p.n_obs = a.n_obs; p.order = a.order; p.frame = a.stokes_frame; p.axes = axes; p.capacity = (int)a.capacity;
    p.head_words = (size_t)EVENTS_COUNTERS * (size_t)a.n_obs + (size_t)a.n_obs + 1 + 2;
    p.staged_doubles = (size_t)(axes ? 10 : 4) * (size_t)a.n_obs;
    *plan = p;
    return EVENTS_OK;
}

// the window, by comparisons only: a coordinate that is not a number is outside
MCRAT_SKY_HD inline bool events_in_window(double t, double e, double t_lo, double t_hi, double e_lo, double e_hi)
{
    return t >= t_lo && t < t_hi && e >= e_lo && e < e_hi;
}
// the observer of row `row`: the o with offsets[o] <= row < offsets[o + 1] (empty segments are stepped over); row < offsets[n_obs]
MCRAT_SKY_HD inline int events_row_observer(const unsigned long long *offsets, int n_obs, unsigned long long row)
{
    int lo = 0, hi = n_obs;                      // offsets[lo] <= row < offsets[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= row) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace mcrat
