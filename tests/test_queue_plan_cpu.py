"""The frame queue's host planning (mcrat_amd/csrc/frame_queue.hpp) on the CPU: the staging block's layout, the order the open items are taken in, and
what the host does with what a launch left -- the relaunch after a pass limit, and the queues of XCDs that drew nothing, which no GPU test reaches on
a device that reports all eight XCDs.  The functions are plain C++: a small driver is compiled with g++ and what it prints is compared with the rules
of frame_queue.hpp's comments, restated here."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XCDS, TICKET_STRIDE, STALLED = 8, 16, 0x80000000

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "frame_queue.hpp"
using namespace mcrat;

static void ints(const char *key, const int *v, size_t n) { printf("%s:", key); for (size_t i = 0; i < n; ++i) printf(" %d", v[i]); printf("\n"); }
static void items_out(const char *tag, const std::vector<FrameItem> &it)
{
    printf("%s_open:", tag); for (const FrameItem &i : it) printf(" %d", i.open); printf("\n");
    printf("%s_time_now:", tag); for (const FrameItem &i : it) printf(" %.17g", i.time_now); printf("\n");
    printf("%s_remaining:", tag); for (const FrameItem &i : it) printf(" %.17g", i.remaining_time); printf("\n");
}
static void order_out(const char *tag, const std::vector<FrameItem> &it, int R, int F, const int *xcd_of_class)
{
    std::vector<int> order(it.size() + 1, -7);             // (one word more than any order needs: it must stay as it is)
    int off[FRAME_QUEUE_XCDS + 1];
    const int longest = frame_queue_order(it.data(), R, F, xcd_of_class, order.data(), off);
    char key[64];
    snprintf(key, sizeof key, "%s_order", tag); ints(key, order.data(), order.size());
    snprintf(key, sizeof key, "%s_order_off", tag); ints(key, off, FRAME_QUEUE_XCDS + 1);
    printf("%s_longest: %d\n%s_groups: %d\n", tag, longest, tag, frame_queue_groups(longest));
}
static FrameItem item(int f, int r, int open)
{
    FrameItem it;
    it.seed = 1000u * f + r; it.time_now = 10.0 * f + 0.125 * r; it.remaining_time = 0.5 + 0.25 * f; it.frame_end = 10.0 * (f + 1) + 0.375; it.open = open; it.hydro = 0;
    return it;
}
static FrameRecord stale()
{
    FrameRecord rec;
    memset(&rec, 0xff, sizeof rec);
    rec.remaining_time = rec.time_now = std::nan(""); rec.iterations = 1ll << 60; rec.done = 0;
    return rec;
}

static void order_case()
{
    const int R = 19, F = 3;
    std::vector<FrameItem> it;
    for (int f = 0; f < F; ++f)
        for (int r = 0; r < R; ++r) it.push_back(item(f, r, !(f == 0 && r == 4) && !(r == 11 && f != 1)));
    int ident[FRAME_QUEUE_XCDS];
    for (int k = 0; k < FRAME_QUEUE_XCDS; ++k) ident[k] = k;
    order_out("order", it, R, F, ident);
}

// lists: 0 through all three frames; 1 stalled in frame 1 after some passes; 2 stalled in frame 1 before its first pass; 3 never started;
// 4 through frame 0, its frame 1 gave up waiting or was never drawn
static void relaunch_case(int chain)
{
    const int R = 5, F = 3;
    std::vector<FrameItem> it;
    for (int f = 0; f < F; ++f)
        for (int r = 0; r < R; ++r) it.push_back(item(f, r, 1));
    std::vector<FrameRecord> rec((size_t)R * F, stale());
    auto valid = [&](int f, int r, long long iterations, int done) {
        FrameRecord &x = rec[(size_t)f * R + r];
        memset(&x, 0, sizeof x);
        x.time_now = 100.0 + 10.0 * f + 0.0625 * r; x.remaining_time = 0.0; x.iterations = iterations; x.done = done;
    };
    for (int f = 0; f < 3; ++f) valid(f, 0, 7, 1);
    valid(0, 1, 7, 1); valid(1, 1, 5, 0);
    valid(0, 2, 7, 1); valid(1, 2, 0, 0);
    valid(0, 4, 7, 1);
    unsigned done[R] = {3u, FRAME_STALLED | 1u, FRAME_STALLED | 1u, 0u, 1u};
    unsigned tickets[FRAME_QUEUE_XCDS * FRAME_TICKET_STRIDE];
    for (unsigned &t : tickets) t = 3;
    int first[R] = {0, 0, 0, 0, 0}, last[R] = {2, 2, 2, 2, 2}, stalled[R] = {-1, -1, -1, -1, -1}, xcd[FRAME_QUEUE_XCDS];
    for (int k = 0; k < FRAME_QUEUE_XCDS; ++k) xcd[k] = k;
    const int next = frame_queue_after_launch(done, tickets, rec.data(), it.data(), R, first, last, chain != 0, stalled, xcd);
    const char *tag = chain ? "chain" : "plain";
    char key[64];
    printf("%s_next: %d\n", tag, next);
    snprintf(key, sizeof key, "%s_done", tag); ints(key, reinterpret_cast<const int *>(done), R);
    snprintf(key, sizeof key, "%s_stalled", tag); ints(key, stalled, R);
    snprintf(key, sizeof key, "%s_xcd", tag); ints(key, xcd, FRAME_QUEUE_XCDS);
    int ticket_sum = 0;
    for (unsigned t : tickets) ticket_sum += (int)t;
    printf("%s_ticket_sum: %d\n", tag, ticket_sum);
    items_out(tag, it);
}

static void dead_case()
{
    const int R = 19, F = 3;
    std::vector<FrameItem> it;
    for (int f = 0; f < F; ++f)
        for (int r = 0; r < R; ++r) it.push_back(item(f, r, 1));
    std::vector<FrameRecord> rec((size_t)R * F, stale());
    std::vector<unsigned> done((size_t)R, 0u);
    std::vector<int> first((size_t)R, 0), last((size_t)R, F - 1), stalled((size_t)R, -1);
    for (int r = 0; r < R; ++r)
        if (r % FRAME_QUEUE_XCDS < 4) {                      // the lists of the XCDs that exist are through
            done[r] = F;
            for (int f = 0; f < F; ++f) { FrameRecord &x = rec[(size_t)f * R + r]; memset(&x, 0, sizeof x); x.iterations = 3; x.done = 1; }
        }
    unsigned tickets[FRAME_QUEUE_XCDS * FRAME_TICKET_STRIDE] = {0};
    for (int x = 0; x < 4; ++x) tickets[x * FRAME_TICKET_STRIDE] = 40;
    int xcd[FRAME_QUEUE_XCDS];
    for (int k = 0; k < FRAME_QUEUE_XCDS; ++k) xcd[k] = k;
    printf("dead_next: %d\n", (int)frame_queue_after_launch(done.data(), tickets, rec.data(), it.data(), R, first.data(), last.data(), false, stalled.data(), xcd));
    ints("dead_xcd", xcd, FRAME_QUEUE_XCDS);
    items_out("dead", it);
    order_out("dead", it, R, F, xcd);
    // no ticket was drawn at all
    std::vector<FrameItem> it2 = it;
    std::vector<unsigned> done2((size_t)R, 0u);
    unsigned none[FRAME_QUEUE_XCDS * FRAME_TICKET_STRIDE] = {0};
    for (int k = 0; k < FRAME_QUEUE_XCDS; ++k) xcd[k] = k;
    printf("nodraw_next: %d\n", (int)frame_queue_after_launch(done2.data(), none, rec.data(), it2.data(), R, first.data(), last.data(), false, stalled.data(), xcd));
}

static void layout_case()
{
    printf("sizes: %zu %zu %zu %zu\n", sizeof(FrameItem), sizeof(HydroDev), sizeof(RankDesc), sizeof(FrameRecord));
    const int shapes[3][3] = {{1, 1, 1}, {19, 3, 2}, {1025, 20, 1}};
    for (const auto &s : shapes) {
        const FrameQueueLayout l(s[0], s[1], (size_t)s[2]);
        std::vector<char> block(l.bytes);
        char *b = block.data();
        printf("layout_%d_%d_%d: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", s[0], s[1], s[2], l.off_items, l.off_hydro, l.off_desc, l.off_ticket, l.off_done,
               l.off_rec, l.bytes, l.up.off, l.up.bytes, l.down.off, l.down.bytes, l.words.off, l.words.bytes);
        printf("access_%d_%d_%d: %td %td %td %td %td %td %td\n", s[0], s[1], s[2], (char *)l.order(b) - b, (char *)l.items(b) - b, (char *)l.hydro(b) - b,
               (char *)l.desc(b) - b, (char *)l.ticket(b) - b, (char *)l.frames_done(b) - b, (char *)l.records(b) - b);
    }
}

int main()
{
    order_case();
    relaunch_case(1);
    relaunch_case(0);
    dead_case();
    layout_case();
    return 0;
}
'''


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """what the driver printed: {key: [numbers]}"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the planning functions' driver")
    d = tmp_path_factory.mktemp("queue_plan")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    res = {}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        res[key] = [float(v) if any(ch in v for ch in ".naife") else int(v) for v in vals.split()]
    return res


def item(f, r):
    """the driver's item (f, r): time_now, remaining_time, frame_end"""
    return 10.0 * f + 0.125 * r, 0.5 + 0.25 * f, 10.0 * (f + 1) + 0.375


def expected_queues(open_, R, F, xcd_of_class):
    """per XCD, its lists' open items frame-major: list r is of class r % 8, in the queue of XCD xcd_of_class[r % 8]"""
    return [[f * R + r for f in range(F) for r in range(R) if open_[f * R + r] and xcd_of_class[r % XCDS] == x] for x in range(XCDS)]


def check_order(out, tag, open_, R, F, xcd_of_class):
    queues = expected_queues(open_, R, F, xcd_of_class)
    n_open = sum(1 for o in open_ if o)
    off, order = out[tag + "_order_off"], out[tag + "_order"]
    assert off[0] == 0 and off[XCDS] == n_open
    for x in range(XCDS):
        assert order[off[x]:off[x + 1]] == queues[x], x
    assert sorted(order[:n_open]) == [t for t in range(R * F) if open_[t]]          # every open item exactly once
    assert order[n_open:] == [-7] * (len(order) - n_open)                            # and nothing behind them
    longest = max(len(q) for q in queues)
    assert out[tag + "_longest"] == [longest] and out[tag + "_groups"] == [XCDS * longest]
    return queues


def test_order_per_xcd_frame_major(out):
    R, F = 19, 3
    open_ = [int(not (f == 0 and r == 4) and not (r == 11 and f != 1)) for f in range(F) for r in range(R)]
    assert sum(open_) == R * F - 1 - 2
    queues = check_order(out, "order", open_, R, F, list(range(XCDS)))
    assert all(t % R % XCDS == x for x in range(XCDS) for t in queues[x])
    assert queues[3] == [3, 19 + 3, 19 + 11, 38 + 3]                  # lists 3 and 11 (11 in frame 1 only); list 19 would be the next of this class
    assert queues[4] == [12, 19 + 4, 19 + 12, 38 + 4, 38 + 12]        # list 4 closed in frame 0


@pytest.mark.parametrize("chain", [True, False])
def test_relaunch_after_a_pass_limit(out, chain):
    tag = "chain" if chain else "plain"
    R, F = 5, 3
    assert out[tag + "_next"] == [1]                                  # FRAME_QUEUE_GO_ON
    assert out[tag + "_done"] == [3, 1, 1, 0, 1]                      # the flags are stripped: the frames before the stalled one are through
    assert out[tag + "_stalled"] == [-1, 1, 1, -1, -1]
    assert out[tag + "_xcd"] == list(range(XCDS)) and out[tag + "_ticket_sum"] == [0]
    # finished frames close; the frame in progress goes on (2) only where its record says it has begun; everything else as planned
    want_open = {0: [0, 0, 0], 1: [0, 2, 1], 2: [0, 1, 1], 3: [1, 1, 1], 4: [0, 1, 1]}
    open_ = out[tag + "_open"]
    for r in range(R):
        assert [open_[f * R + r] for f in range(F)] == want_open[r], r
    assert open_.count(2) == 1
    # the clocks: with chain_clock the next frame of a list whose previous frame has left the queue reads that frame's record (lists 2 and 4: frame 1
    # from the record of frame 0, 100 + 0.0625 r) and gets frame_end - time_now; a frame that goes on (list 1) and a first frame (list 3) keep theirs
    for f in range(F):
        for r in range(R):
            t_now, t_rem, t_end = item(f, r)
            if chain and f == 1 and r in (2, 4):
                t_now = 100.0 + 0.0625 * r
                t_rem = t_end - t_now
            assert out[tag + "_time_now"][f * R + r] == t_now, (f, r)
            assert out[tag + "_remaining"][f * R + r] == t_rem, (f, r)
    # nothing of a record beyond frames_done (NaN clocks, 2^60 iterations) shows up
    assert not any(math.isnan(v) for v in out[tag + "_time_now"] + out[tag + "_remaining"])


def test_dead_queues_move_to_xcds_that_exist(out):
    R, F = 19, 3
    assert out["dead_next"] == [1]
    alive = [0, 1, 2, 3]
    xcd = [k if k < 4 else alive[k % 4] for k in range(XCDS)]
    assert out["dead_xcd"] == xcd == [0, 1, 2, 3, 0, 1, 2, 3]
    open_ = [int(r % XCDS >= 4) for f in range(F) for r in range(R)]                 # the lists of XCDs 0..3 are through, the others never started
    assert out["dead_open"] == open_
    queues = check_order(out, "dead", open_, R, F, xcd)
    off = out["dead_order_off"]
    assert all(off[x] == off[x + 1] == sum(open_) for x in range(4, XCDS))           # the dead XCDs' ranges are empty
    assert all(len(queues[x]) > 0 and all(t % R % XCDS == x + 4 for t in queues[x]) for x in range(4))
    assert out["nodraw_next"] == [2]                                                 # FRAME_QUEUE_NO_DRAW


@pytest.mark.parametrize("shape", [(1, 1, 1), (19, 3, 2), (1025, 20, 1)])
def test_block_layout(out, shape):
    R, F, H = shape
    N = R * F
    s_item, s_hydro, s_desc, s_rec = out["sizes"]
    off_items, off_hydro, off_desc, off_ticket, off_done, off_rec, nbytes, up_off, up_bytes, down_off, down_bytes, words_off, words_bytes = out["layout_%d_%d_%d" % shape]
    assert off_items % 64 == 0 and off_hydro % 256 == 0 and off_desc % 64 == 0 and off_ticket % 256 == 0 and off_rec % 256 == 0 and off_done % 64 == 0
    # [order | items | hydro frames | descriptions | ticket | frames_done | records], none overlapping the next, each start the first aligned one
    parts = [(0, 4 * N, 1), (off_items, s_item * N, 64), (off_hydro, s_hydro * H, 256), (off_desc, s_desc * R, 64), (off_ticket, 4 * XCDS * TICKET_STRIDE, 256),
             (off_done, 4 * R, 1), (off_rec, s_rec * N, 256)]
    end = 0
    for off, size, align in parts:
        assert off == -(-end // align) * align, (off, end, align)
        end = off + size
    assert nbytes == end
    assert (up_off, up_bytes) == (0, off_rec)                                        # one copy up: [0, off_rec)
    assert (down_off, down_off + down_bytes) == (off_ticket, nbytes)                 # one copy down: [off_ticket, bytes)
    assert (words_off, words_off + words_bytes) == (off_ticket, off_rec)
    assert out["access_%d_%d_%d" % shape] == [0, off_items, off_hydro, off_desc, off_ticket, off_done, off_rec]
