// frame_queue.hpp -- the frame queue: what its kernel and the host share (the queue's kernel argument, its items and records), and the host's planning
// of a queue launch (the staging block's layout, the order the items are taken in, what a launch that ended leaves to do).  The planning functions
// are plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them (tests/test_queue_plan_cpu.py).
#pragma once
#include <stddef.h>
#include <string.h>
#include "device_types.hpp"

#if defined(__HIPCC__)
#define MCRAT_FQ_HD __host__ __device__
#else
#define MCRAT_FQ_HD
#endif

namespace mcrat {

// The frame queue (round 4): ONE launch takes every list through SEVERAL hydro frames.  The reference's ranks are asynchronous processes, each in
// its own frame loop (mcrat.c:457-479, :566-934); a launch per hydro frame makes them wait for each other at every frame's end.  A queue launch has
// as many persistent workgroups as the device holds; each draws (frame, list) items from the queue of the XCD it runs on until that is empty, the k-th
// draw on an XCD getting the k-th open item of that XCD's lists in frame-major order (`order`, `ticket`): a list that is through frame f starts f + 1 as
// soon as a workgroup is free, while other lists are still in f.  The item of a list whose previous frame is still running waits for it (frames_done;
// that item was drawn earlier, by a workgroup that is running and depends on nothing later, so this cannot deadlock).  Every list sees exactly the frames it would have seen one launch at a time: the same seeds, clocks, passes and photons
// (tests/test_gpu_frame_queue.py).
struct FrameItem {                   // list r in frame f: item f * n_ranks + r
    unsigned long long seed;         // the list's seed of this frame (gsl_rng_get, mcrat.c:701)
    double time_now;                 // its clock at the start of the frame ...
    double remaining_time;           // ... and the time left in it (mcrat.c:757), unless the clock is chained (below)
    double frame_end;                // (scatt_frame + increment_scatt_frame) / fps: a chained list gets frame_end - its own time_now, the host's expression
    int open;                        // the list takes part in this frame (a rank joins at its injection frame, mcrat.c:566-700)
    int hydro;                       // which staged hydro frame of the launch it propagates through
};
// What a (frame, list) item leaves for the host: the members of LoopState that mcrat_hip_frame_stats shows (engine.hip, state_to_stats) and `done` -- not
// the pending segments, the shortlist's estimates or the diagnostic stamps, which only the kernel reads (a stalled list resumes from states[rank], a full
// LoopState).  One lane stores it when the item's frame ends, complete or at the launch's pass limit, and when a frame has no time left.
// VALIDITY.  The records' buffer is never cleared, so a record means something only for an item the kernel is KNOWN to have written in this call, and the
// host decides that from frames_done[list] alone (read back with the records): with d = frames_done & ~FRAME_STALLED, the list's open items of frames
// < d are complete and their records written; with FRAME_STALLED set, so is the record of frame d (iterations > 0, done == 0: the frame goes on with
// open = 2); every later item of the list gave up or was never drawn, wrote nothing, and its record holds whatever an earlier call left there.
struct alignas(32) FrameRecord {
    double remaining_time, time_now;
    long long iterations;
    int done;
    int last_scattered_index;
    double last_time_step, last_scattered_temp;
    long long frame_scatt_cnt, n_relocated;
    long long not_found, kn_rejections, rescans, slot_steps;
    MCRAT_FQ_HD void from_state(const LoopState &s)
    {
        remaining_time = s.remaining_time; time_now = s.time_now; iterations = s.iterations; done = s.done; last_scattered_index = s.last_scattered_index;
        last_time_step = s.last_time_step; last_scattered_temp = s.last_scattered_temp; frame_scatt_cnt = s.frame_scatt_cnt; n_relocated = s.n_relocated;
        not_found = s.not_found; kn_rejections = s.kn_rejections; rescans = s.rescans; slot_steps = s.slot_steps;
    }
};
static_assert(sizeof(FrameRecord) <= 128, "the frame record stays compact: at most half a LoopState");
struct FrameQueueDev {
    int n_frames;                  // 0: no queue -- one workgroup per list, one frame, as before
    int restore;                     // every frame starts from the context's snapshot (mcrat_hip_snapshot_photons; benchmarks: the same work every frame)
    int chain_clock;                 // a list's clock carries over from its previous frame of this launch (time_now of the LoopState it left)
    int pad;
    unsigned *ticket;                // [FRAME_QUEUE_XCDS * FRAME_TICKET_STRIDE] per XCD: workgroups that have started there
    const int *order;                // [open items] per XCD (order_off[x] .. order_off[x + 1]) its lists' items in the order they are taken: frame-major
    int order_off[9];
    unsigned *frames_done;           // [n_ranks] f + 1 once item (f, r) is complete; FRAME_STALLED | f: frame f ran into the launch's pass limit
    const FrameItem *items;          // [n_frames * n_ranks]
    const HydroDev *hydro;           // [n_hydro] the staged hydro frames of the launch (FrameItem::hydro indexes it); read through the constant address space
    FrameRecord *records;            // [n_frames * n_ranks] what every frame ended with (see FrameRecord for which of them may be read)
    long long snap_delta;            // bytes from a column of the live lists to its copy in the snapshot (restore)
    long long capture_delta, capture_stride;   // != 0: at the end of frame f < n_frames - 1 the list's columns are copied to live + capture_delta + f * capture_stride
};
constexpr unsigned FRAME_STALLED = 0x80000000u;
constexpr int FRAME_QUEUE_XCDS = 8, FRAME_TICKET_STRIDE = 16;     // (a ticket per XCD, each on a 64-B line of its own)

// ------------------------------------------------------------------ the host's planning of a queue launch

// The queue's block, device memory with a pinned mirror laid out alike: [order N | items N | hydro frames | list descriptions R] are only uploaded,
// [ticket | frames_done R] go both ways, [records N] only come back -- so one launch is ONE copy up (`up`) and ONE copy down (`down`).
struct FrameQueueLayout {
    struct Range { size_t off, bytes; };
    size_t off_items, off_hydro, off_desc, off_ticket, off_done, off_rec, bytes;    // (order: offset 0)
    Range up;                        // [0, off_rec): what the host writes before a launch
    Range down;                      // [off_ticket, bytes): what a launch leaves
    Range words;                     // [off_ticket, off_rec): ticket and frames_done, all that starts a call cleared (and all that comes back when the
                                     // kernel stores the records into the pinned block itself)
    static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
    FrameQueueLayout(int R, int F, size_t n_hydro)
    {
        const size_t N = (size_t)R * (size_t)F;
        off_items = align_up(sizeof(int) * N, 64);
        off_hydro = align_up(off_items + sizeof(FrameItem) * N, 256);
        off_desc = align_up(off_hydro + sizeof(HydroDev) * n_hydro, 64);
        off_ticket = align_up(off_desc + sizeof(RankDesc) * (size_t)R, 256);
        off_done = off_ticket + sizeof(unsigned) * FRAME_QUEUE_XCDS * FRAME_TICKET_STRIDE;
        off_rec = align_up(off_done + sizeof(unsigned) * (size_t)R, 256);
        bytes = off_rec + sizeof(FrameRecord) * N;
        up = Range{0, off_rec};
        down = Range{off_ticket, bytes - off_ticket};
        words = Range{off_ticket, off_rec - off_ticket};
    }
    template <class T> static T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }
    // the block's members from its base: the pinned mirror's or the device block's
    int *order(void *b) const { return at<int>(b, 0); }
    FrameItem *items(void *b) const { return at<FrameItem>(b, off_items); }
    HydroDev *hydro(void *b) const { return at<HydroDev>(b, off_hydro); }
    RankDesc *desc(void *b) const { return at<RankDesc>(b, off_desc); }
    unsigned *ticket(void *b) const { return at<unsigned>(b, off_ticket); }
    unsigned *frames_done(void *b) const { return at<unsigned>(b, off_done); }
    FrameRecord *records(void *b) const { return at<FrameRecord>(b, off_rec); }
};

// Which XCD a list belongs to: list r to XCD r % 8, where one launch per frame puts it too: a list never changes L2.  (Measured against contiguous
// eighths of the lists -- neighbouring lists hold photons of neighbouring cells, so an XCD's L2 would have an eighth of the cells to hold: 0.567
// against 0.52 ms per frame on the benchmark frame, the eighths differ in optical depth and the launch ends with the slowest XCD.)
inline int frame_list_class(int r) { return r % FRAME_QUEUE_XCDS; }

// The open items in the order they are taken: per XCD the items of its lists -- the lists of class k are in the queue of XCD xcd_of_class[k], the
// identity unless an XCD turned out to start no workgroups -- frame-major.  Fills order and order_off[0 .. 8] (order_off[8]: the open items) and
// returns the longest queue's length: as the hardware deals workgroups round-robin over the XCDs, a launch needs eight times that many to have one
// workgroup per item (frame_queue_groups).  The first launch of a call and a relaunch use it alike.
inline int frame_queue_order(const FrameItem *items, int R, int F, const int *xcd_of_class, int *order, int *order_off)
{
    int count[FRAME_QUEUE_XCDS] = {0}, fill[FRAME_QUEUE_XCDS], n_open = 0, longest = 0;
    for (int f = 0; f < F; ++f)
        for (int r = 0; r < R; ++r)
            if (items[(size_t)f * R + r].open) count[xcd_of_class[frame_list_class(r)]] += 1;
    for (int x = 0; x < FRAME_QUEUE_XCDS; ++x) {
        order_off[x] = fill[x] = n_open;
        n_open += count[x];
        if (count[x] > longest) longest = count[x];
    }
    order_off[FRAME_QUEUE_XCDS] = n_open;
    for (int f = 0; f < F; ++f)
        for (int r = 0; r < R; ++r)
            if (items[(size_t)f * R + r].open) order[fill[xcd_of_class[frame_list_class(r)]]++] = f * R + r;
    return longest;
}
inline int frame_queue_groups(int longest_queue) { return FRAME_QUEUE_XCDS * longest_queue; }

// What a launch that has ended leaves to do, from what it wrote (frames_done, tickets, records: the pinned mirror's) and the plan (first[r], last[r]:
// list r's first and last open frame, -1: it takes no part).
//   FRAME_QUEUE_DONE     every list is through its last frame.
//   FRAME_QUEUE_GO_ON    lists ran into the launch's pass limit (and their later frames' workgroups gave up): the block is ready for the next launch.
//                        frames_done has lost its FRAME_STALLED flags, stalled[r] is the frame of list r that a launch of this call left at its pass
//                        limit (-1: none; it stays that until frames_done has moved past it), the tickets are cleared, finished frames have left the
//                        queue (open = 0), a frame in progress goes on from its LoopState (open = 2) and the rest as planned -- with chain_clock, the
//                        next frame of a list whose previous one has left the queue gets the clock it would have read there.  Only records this call is
//                        known to have written are read (FrameRecord): the stalled frame's, and those of frames that are through.
//                        A device whose workgroups report fewer XCDs than eight (another partition mode): the classes whose queue nobody drew from
//                        move to XCDs that exist (xcd_of_class, for the next frame_queue_order).
//   FRAME_QUEUE_NO_DRAW  no workgroup drew an item: an error.
enum FrameQueueNext { FRAME_QUEUE_DONE = 0, FRAME_QUEUE_GO_ON = 1, FRAME_QUEUE_NO_DRAW = 2 };
inline FrameQueueNext frame_queue_after_launch(unsigned *frames_done, unsigned *tickets, const FrameRecord *records, FrameItem *items, int R,
                                               const int *first, const int *last, bool chain_clock, int *stalled, int *xcd_of_class)
{
    bool all = true;
    for (int r = 0; r < R; ++r) {
        // (the frame that ran into the pass limit = the frames before it are through)
        if (frames_done[r] & FRAME_STALLED) { frames_done[r] &= ~FRAME_STALLED; stalled[r] = (int)frames_done[r]; }
        all = all && (first[r] < 0 || (int)frames_done[r] == last[r] + 1);
    }
    if (all) return FRAME_QUEUE_DONE;
    int alive[FRAME_QUEUE_XCDS], n_alive = 0;
    for (int x = 0; x < FRAME_QUEUE_XCDS; ++x)
        if (tickets[(size_t)x * FRAME_TICKET_STRIDE] > 0) alive[n_alive++] = x;
    if (n_alive == 0) return FRAME_QUEUE_NO_DRAW;
    for (int k = 0; k < FRAME_QUEUE_XCDS; ++k)
        if (tickets[(size_t)xcd_of_class[k] * FRAME_TICKET_STRIDE] == 0) xcd_of_class[k] = alive[k % n_alive];
    memset(tickets, 0, sizeof(unsigned) * FRAME_QUEUE_XCDS * FRAME_TICKET_STRIDE);
    for (int r = 0; r < R; ++r) {
        if (first[r] < 0) continue;
        const int nf = (int)frames_done[r] > first[r] ? (int)frames_done[r] : first[r];     // the first frame that is not complete
        for (int f = first[r]; f <= last[r]; ++f) {
            FrameItem &it = items[(size_t)f * R + r];
            if (f < nf) { it.open = 0; continue; }
            if (f > nf) continue;
            const FrameRecord &rec = records[(size_t)f * R + r];
            if (stalled[r] == nf && rec.iterations > 0 && !rec.done) it.open = 2;
            else if (chain_clock && f > first[r]) {                            // (its previous frame has left the queue: the clock it would have read there)
                it.time_now = records[(size_t)(f - 1) * R + r].time_now;
                it.remaining_time = it.frame_end - it.time_now;
            }
        }
    }
    return FRAME_QUEUE_GO_ON;
}

}  // namespace mcrat
