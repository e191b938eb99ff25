"""The host's rules for a detected-photon event list (mcrat_amd/csrc/events_plan.hpp) on the CPU: every refusal with its text and in its order, the
block's layout for two capacities and both orders, the chunks of the compaction around a chunk's size, the key of a detection time against the
NumPy restatement (tests/events_checker.py), and the passes of the sort for hand-written OR and AND masks.  Plain C++: a small driver is compiled
with g++ and what it prints is compared.  The same driver is built a second time with -fsanitize=address,undefined as a stand-alone program and
run once.  (The pattern of tests/test_resample_plan_cpu.py.)"""
import shutil
import subprocess

import numpy as np
import pytest

from tests import events_checker as E
from tests import test_sky_plan_cpu as P
from tests.test_sky_plan_cpu import INF, NAN, X, Y, Z, TILT

BY_PHOTON, BY_TIME = 0, 1
AS_STORED, SKY_PLANE = 0, 1
OK = 0
(BAD_ORDER, BAD_FRAME, AXES_NOT_FINITE, AXES_NOT_UNIT, AXES_NOT_ORTHOGONAL, FRAME_NEEDS_AXES, XY_NEED_AXES, WINDOW_NAN, WINDOW_EMPTY, CAPACITY_NEGATIVE,
 CAPACITY_TOO_LARGE, TOO_MANY_OBSERVERS) = range(32, 44)
# the constants the GPU tests import: what one wavefront compacts at least, what one workgroup ranks per pass, the digit, the most observers
MAX_OBS, BLOCK, WAVE, MIN_TRIPS, MAX_CHUNKS, DIGIT_BITS, SORT_TILE, SCAN_BLOCK, SCAN_ITEMS, ALIGN = 512, 256, 64, 8, 65536, 8, 2048, 1024, 4, 256
CHUNK = WAVE * MIN_TRIPS
KEY_PASSES = 64 // DIGIT_BITS
PREFIX = "observe_events:"

TEXTS = {k: PREFIX + t[len("observe_sky:"):] for k, t in P.TEXTS.items() if k in (P.NO_BINS, P.DIR_NOT_FINITE, P.DIR_NOT_UNIT, P.BAD_CONE)}
TEXTS.update({
    BAD_ORDER: "observe_events: order must be MCRAT_HIP_EVENTS_BY_PHOTON or _BY_TIME",
    BAD_FRAME: "observe_events: stokes_frame must be MCRAT_HIP_STOKES_AS_STORED or _SKY_PLANE",
    AXES_NOT_FINITE: "observe_events: a sky-plane vector holds a value that is not finite",
    AXES_NOT_UNIT: "observe_events: a sky-plane vector is not a unit vector (to 1e-12)",
    AXES_NOT_ORTHOGONAL: "observe_events: the sky-plane vectors and the direction are not orthogonal (to 1e-12)",
    FRAME_NEEDS_AXES: "observe_events: MCRAT_HIP_STOKES_SKY_PLANE needs the sky-plane vectors x0 .. x2 and y0 .. y2",
    XY_NEED_AXES: "observe_events: the X and Y columns need the sky-plane vectors x0 .. x2 and y0 .. y2",
    WINDOW_NAN: "observe_events: a bound of the window is not a number",
    WINDOW_EMPTY: "observe_events: the window needs t_lo < t_hi and e_lo < e_hi",
    CAPACITY_NEGATIVE: "observe_events: capacity must not be negative",
    CAPACITY_TOO_LARGE: "observe_events: capacity is beyond what an int row index can hold",
    TOO_MANY_OBSERVERS: "observe_events: more observers than the kernels keep counters for (512)",
})


def plan(n_obs=1, n=(Z,), cos_acc=(0.5,), ex=(X,), ey=(Y,), window=(-INF, INF, 0.0, INF), order=BY_TIME, frame=AS_STORED, capacity=1000, want_xy=False):
    return dict(n_obs=n_obs, n=n, cos_acc=cos_acc, ex=ex, ey=ey, window=window, order=order, frame=frame, capacity=capacity, want_xy=want_xy)


def bare(**kw):
    """no sky-plane vectors"""
    return plan(ex=None, ey=None, **kw)


def many(n_obs, **kw):
    return bare(n_obs=n_obs, n=(Z,) * n_obs, cos_acc=(0.5,) * n_obs, **kw)


PLANS = {
    "axes": plan(),
    "bare": bare(),
    "by_photon": bare(order=BY_PHOTON),
    "sky_plane": plan(frame=SKY_PLANE, want_xy=True),
    "counting": bare(capacity=0),
    "largest": bare(capacity=2 ** 31 - 1),
    "finite_window": bare(window=(100.0, 360.0, 1e-9, 1e-4)),
    "half_open": bare(window=(-INF, 0.0, 5e-324, 1.0)),
    "three": plan(n_obs=3, n=(Z, X, Y), cos_acc=(1.0, -1.0, 0.0), ex=(X, Y, Z), ey=(Y, Z, X), capacity=4097),
    "most_observers": many(MAX_OBS),
    "only_ex_is_no_axes": plan(ey=None),                       # all six or they are not read
    "only_ex_is_not_checked": plan(ex=([NAN, 0.0, 0.0],), ey=None),
    # refused -- the observers' checks come through with this product's prefix
    "no_observer": plan(n_obs=0, n=(), cos_acc=(), ex=(), ey=()),
    "dir_nan": plan(n=([0.0, NAN, 1.0],)),
    "dir_long": plan(n=([0.0, 0.0, 1.0 + 1e-11],)),
    "cone_wide": plan(cos_acc=(1.5,)), "cone_nan": plan(cos_acc=(NAN,)),
    "order_2": plan(order=2), "order_negative": plan(order=-1),
    "frame_2": plan(frame=2), "frame_negative": plan(frame=-1),
    "axes_nan": plan(ey=([0.0, NAN, 0.0],)),
    "axes_long": plan(ex=([1.0 + 1e-11, 0.0, 0.0],)),
    "axes_parallel": plan(ey=(X,)),
    "axes_tilted": plan(ex=([1.0, 0.0, -TILT],), n=([TILT, 0.0, 1.0],), ey=([0.0, 1.0, TILT],)),
    "sky_plane_bare": bare(frame=SKY_PLANE),
    "sky_plane_only_ex": plan(frame=SKY_PLANE, ey=None),
    "xy_bare": bare(want_xy=True),
    "t_lo_nan": bare(window=(NAN, 1.0, 0.0, 1.0)), "t_hi_nan": bare(window=(0.0, NAN, 0.0, 1.0)),
    "e_lo_nan": bare(window=(0.0, 1.0, NAN, 1.0)), "e_hi_nan": bare(window=(0.0, 1.0, 0.0, NAN)),
    "t_equal": bare(window=(1.0, 1.0, 0.0, 1.0)), "t_descending": bare(window=(INF, -INF, 0.0, 1.0)),
    "e_equal": bare(window=(0.0, 1.0, 2.0, 2.0)), "e_descending": bare(window=(0.0, 1.0, 2.0, 1.0)),
    "capacity_negative": bare(capacity=-1),
    "capacity_beyond_int": bare(capacity=2 ** 31),
    "too_many_observers": many(MAX_OBS + 1),
    # two faults at once: the first in the order decides
    "cone_before_order": plan(cos_acc=(-2.0,), order=7),
    "order_before_frame": plan(order=7, frame=7),
    "frame_before_axes": plan(frame=7, ey=(X,)),
    "axes_before_frame_needs": plan(frame=SKY_PLANE, ex=([NAN, 0.0, 0.0],)),
    "frame_needs_before_xy": bare(frame=SKY_PLANE, want_xy=True),
    "xy_before_window": bare(want_xy=True, window=(NAN, 1.0, 0.0, 1.0)),
    "nan_before_empty": bare(window=(2.0, 1.0, 0.0, NAN)),
    "window_before_capacity": bare(window=(2.0, 1.0, 0.0, 1.0), capacity=-5),
    "negative_before_observers": many(MAX_OBS + 1, capacity=-5),
    "beyond_int_before_observers": many(MAX_OBS + 1, capacity=2 ** 40),
}
REFUSED = {
    "no_observer": P.NO_BINS, "dir_nan": P.DIR_NOT_FINITE, "dir_long": P.DIR_NOT_UNIT, "cone_wide": P.BAD_CONE, "cone_nan": P.BAD_CONE,
    "order_2": BAD_ORDER, "order_negative": BAD_ORDER, "frame_2": BAD_FRAME, "frame_negative": BAD_FRAME, "axes_nan": AXES_NOT_FINITE,
    "axes_long": AXES_NOT_UNIT, "axes_parallel": AXES_NOT_ORTHOGONAL, "axes_tilted": AXES_NOT_ORTHOGONAL, "sky_plane_bare": FRAME_NEEDS_AXES,
    "sky_plane_only_ex": FRAME_NEEDS_AXES, "xy_bare": XY_NEED_AXES, "t_lo_nan": WINDOW_NAN, "t_hi_nan": WINDOW_NAN, "e_lo_nan": WINDOW_NAN,
    "e_hi_nan": WINDOW_NAN, "t_equal": WINDOW_EMPTY, "t_descending": WINDOW_EMPTY, "e_equal": WINDOW_EMPTY, "e_descending": WINDOW_EMPTY,
    "capacity_negative": CAPACITY_NEGATIVE, "capacity_beyond_int": CAPACITY_TOO_LARGE, "too_many_observers": TOO_MANY_OBSERVERS,
    "cone_before_order": P.BAD_CONE, "order_before_frame": BAD_ORDER, "frame_before_axes": BAD_FRAME, "axes_before_frame_needs": AXES_NOT_FINITE,
    "frame_needs_before_xy": FRAME_NEEDS_AXES, "xy_before_window": XY_NEED_AXES, "nan_before_empty": WINDOW_NAN,
    "window_before_capacity": WINDOW_EMPTY, "negative_before_observers": CAPACITY_NEGATIVE, "beyond_int_before_observers": CAPACITY_TOO_LARGE,
}
LAYOUT_SLOTS, LAYOUT_CLOCKS = 1300, 3
CHUNK_SLOTS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * MAX_CHUNKS, CHUNK * MAX_CHUNKS + 1, 2 ** 31 - 1]
LADDER = [-INF, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, INF]
ALL = 2 ** 64 - 1
# (OR, AND, n_obs): all keys equal; only the lowest byte varies; only the top byte varies; all vary; two digits in the middle; many observers
MASKS = {
    "all_equal": (0xC07F000000000000, 0xC07F000000000000, 1),
    "lowest_byte": (0xC07F0000000000FF, 0xC07F000000000000, 1),
    "lowest_bit": (0xC07F000000000001, 0xC07F000000000000, 1),
    "top_byte": (0xFF7F000000000000, 0x007F000000000000, 1),
    "all_vary": (ALL, 0, 1),
    "middle_two": (0xC07F00FF00010000, 0xC07F000000000000, 2),
    "all_equal_two_observers": (5, 5, 2),
    "observers_256": (0xFF, 0xF0, 256),
    "observers_257": (0xFF, 0xF0, 257),
    "observers_most": (ALL, 0, MAX_OBS),
}

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "events_plan.hpp"
using namespace mcrat;
typedef std::vector<double> V;

static const double *col(const V &v, int k, int n_obs) { return v.data() + (size_t)k * (n_obs > 0 ? n_obs : 0); }
static V repeat(int n_obs, double a, double b, double c) { V v; for (double x : {a, b, c}) for (int k = 0; k < n_obs; ++k) v.push_back(x); return v; }
static V fill(int n_obs, double a) { return V((size_t)n_obs, a); }
static void plan(const char *name, int n_obs, V n, V ca, int has_x, V ex, int has_y, V ey, double t_lo, double t_hi, double e_lo, double e_hi, int order, int frame,
                 long long capacity, int want_xy)
{
    EventsArgs a{};
    a.n_obs = n_obs; a.n0 = col(n, 0, n_obs); a.n1 = col(n, 1, n_obs); a.n2 = col(n, 2, n_obs); a.cos_acc = ca.data();
    if (has_x) { a.x0 = col(ex, 0, n_obs); a.x1 = col(ex, 1, n_obs); a.x2 = col(ex, 2, n_obs); }
    if (has_y) { a.y0 = col(ey, 0, n_obs); a.y1 = col(ey, 1, n_obs); a.y2 = col(ey, 2, n_obs); }
    a.t_lo = t_lo; a.t_hi = t_hi; a.e_lo = e_lo; a.e_hi = e_hi; a.order = order; a.stokes_frame = frame; a.capacity = capacity; a.want_xy = want_xy != 0;
    EventsPlan p;
    const EventsRefusal why = events_plan(a, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why != EVENTS_OK) return;
    const EventsLayout l = events_layout(p, @LAYOUT_SLOTS@, @LAYOUT_CLOCKS@);
    printf("planv_%s: %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", name, p.n_obs, p.order, p.frame, (int)p.axes, p.capacity,
           p.head_words, p.staged_doubles, events_head_offsets_word(p), events_head_or_word(p), l.staged_offset, l.clocks_offset, l.table_offset, l.rank_offset,
           l.slot_offset, l.f8_offset, l.f8_pitch, l.type_offset, l.sort_table_offset, l.source_offset, l.keys_offset, l.keys_pitch, l.index_offset, l.index_pitch,
           l.total_bytes);
}

int main(int argc, char **argv)
{
@CASES@
    char buf[EVENTS_TEXT_BYTES];
    for (int k : {@CODES@}) printf("text_%d:%s\n", k, events_refusal_text((EventsRefusal)k, buf));
    printf("constants: %d %d %d %d %d %d %d %d %d %zu %d %d %d %d\n", EVENTS_MAX_OBS, EVENTS_BLOCK, EVENTS_WAVE, EVENTS_MIN_TRIPS, EVENTS_MAX_CHUNKS, EVENTS_DIGIT_BITS,
           EVENTS_SORT_TILE, EVENTS_SCAN_BLOCK, EVENTS_SCAN_ITEMS, EVENTS_ALIGN, EVENTS_KEY_PASSES, EVENTS_MAX_PASSES, EVENTS_COUNTERS, EVENTS_F8_COLUMNS);
    printf("chunks:");
    for (long long n : {@CHUNK_SLOTS@}) printf(" %d %d", events_chunk_slots((int)n), events_n_chunks((int)n));
    printf("\ntiles:");
    for (long long c : {0ll, 1ll, 2047ll, 2048ll, 2049ll, 2147483647ll}) printf(" %d", events_sort_tiles(c));
    printf("\nobserver_passes:");
    for (int n : {1, 2, 256, 257, 512}) printf(" %d", events_observer_passes(n));
    printf("\n");
    const double ladder[] = {@LADDER@};
    printf("keys:");
    for (double t : ladder) printf(" %llu", (unsigned long long)events_key(t));
    printf("\n");
    const unsigned long long ors[] = {@ORS@}, ands[] = {@ANDS@};
    const int observers[] = {@MASK_OBS@};
    for (size_t i = 0; i < sizeof ors / sizeof ors[0]; ++i) {
        EventsPass launched[EVENTS_MAX_PASSES], run[EVENTS_MAX_PASSES];
        const int n_launched = events_launch_list(observers[i], launched), n_run = events_pass_list(ors[i], ands[i], observers[i], run);
        printf("passes_%zu: %d %d", i, n_launched, n_run);
        for (int k = 0; k < n_run; ++k) printf(" %d %d", run[k].observer, run[k].digit);
        printf("\nbuffers_%zu:", i);
        for (int k = 0; k <= n_launched; ++k) printf(" %d", events_source_buffer(ors[i], ands[i], k));
        printf("\n");
    }
    {
        const unsigned long long offsets[] = {0, 0, 3, 3, 3, 10};     // five observers, three of them without rows
        printf("row_observer:");
        for (unsigned long long row : {0ull, 2ull, 3ull, 9ull}) printf(" %d", events_row_observer(offsets, 5, row));
        const unsigned long long one[] = {0, 4};
        printf(" %d %d\n", events_row_observer(one, 1, 0), events_row_observer(one, 1, 3));
    }
    printf("window: %d %d %d %d %d %d %d\n", (int)events_in_window(1.0, 1.0, 1.0, 2.0, 1.0, 2.0), (int)events_in_window(2.0, 1.0, 1.0, 2.0, 1.0, 2.0),
           (int)events_in_window(1.0, 2.0, 1.0, 2.0, 1.0, 2.0), (int)events_in_window(NAN, 1.0, -INFINITY, INFINITY, 0.0, INFINITY),
           (int)events_in_window(-INFINITY, 1.0, -INFINITY, INFINITY, 0.0, INFINITY), (int)events_in_window(INFINITY, 1.0, -INFINITY, INFINITY, 0.0, INFINITY),
           (int)events_in_window(0.0, NAN, -INFINITY, INFINITY, 0.0, INFINITY));
    (void)argc; (void)argv;
    return 0;
}
'''


def _num(x):
    return "NAN" if x != x else {INF: "INFINITY", -INF: "-INFINITY"}.get(x, repr(float(x)))


def _cases():
    lines = []
    for name, c in PLANS.items():
        n_obs = c["n_obs"]
        if n_obs > 3:                                                  # many equal observers: built in the driver
            n, ca = "repeat(%d, 0.0, 0.0, 1.0)" % n_obs, "fill(%d, 0.5)" % n_obs
        else:
            n, ca = P._vec3(c["n"]), P._vec(c["cos_acc"], 0)
        lines.append('plan("%s", %d, %s, %s, %d, %s, %d, %s, %s, %s, %s, %s, %d, %d, %dll, %d);' % (
            name, n_obs, n, ca, c["ex"] is not None, P._vec3(c["ex"] or ()), c["ey"] is not None, P._vec3(c["ey"] or ()),
            *[_num(x) for x in c["window"]], c["order"], c["frame"], c["capacity"], c["want_xy"]))
    return "\n".join("    " + l for l in lines)


def _build(d, src, name, extra):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", P.os.path.join(P.ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("events_plan")
    src = d / "driver.cpp"
    text = DRIVER.replace("@CASES@", _cases()).replace("@CODES@", ", ".join(str(k) for k in sorted(TEXTS)))
    text = text.replace("@LAYOUT_SLOTS@", str(LAYOUT_SLOTS)).replace("@LAYOUT_CLOCKS@", str(LAYOUT_CLOCKS))
    text = text.replace("@CHUNK_SLOTS@", ", ".join("%dll" % n for n in CHUNK_SLOTS)).replace("@LADDER@", ", ".join(_num(x) for x in LADDER))
    text = text.replace("@ORS@", ", ".join("%dull" % m[0] for m in MASKS.values())).replace("@ANDS@", ", ".join("%dull" % m[1] for m in MASKS.values()))
    text = text.replace("@MASK_OBS@", ", ".join(str(m[2]) for m in MASKS.values()))
    src.write_text(text)
    return d, src


@pytest.fixture(scope="module")
def text(built):
    d, src = built
    return subprocess.run([str(_build(d, src, "driver", []))], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def out(text):
    res = {}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        res[key] = vals if key.startswith("text_") else [int(v) for v in vals.split()]
    return res


def plan_rule(c):
    """events_plan restated: the checks in their order"""
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    if c["n_obs"] < 1:
        return P.NO_BINS
    if not all(np.isfinite(v).all() for v in c["n"]):
        return P.DIR_NOT_FINITE
    if any(abs(dot(v, v) - 1.0) > 1e-12 for v in c["n"]):
        return P.DIR_NOT_UNIT
    if not all(-1.0 <= x <= 1.0 for x in c["cos_acc"]):
        return P.BAD_CONE
    if c["order"] not in (BY_PHOTON, BY_TIME):
        return BAD_ORDER
    if c["frame"] not in (AS_STORED, SKY_PLANE):
        return BAD_FRAME
    axes = c["ex"] is not None and c["ey"] is not None
    if axes:
        if not all(np.isfinite(v).all() for v in tuple(c["ex"]) + tuple(c["ey"])):
            return AXES_NOT_FINITE
        if any(abs(dot(v, v) - 1.0) > 1e-12 for v in tuple(c["ex"]) + tuple(c["ey"])):
            return AXES_NOT_UNIT
        if any(abs(dot(x, n)) > 1e-12 or abs(dot(y, n)) > 1e-12 or abs(dot(x, y)) > 1e-12 for n, x, y in zip(c["n"], c["ex"], c["ey"])):
            return AXES_NOT_ORTHOGONAL
    if c["frame"] == SKY_PLANE and not axes:
        return FRAME_NEEDS_AXES
    if c["want_xy"] and not axes:
        return XY_NEED_AXES
    t_lo, t_hi, e_lo, e_hi = c["window"]
    if any(x != x for x in c["window"]):
        return WINDOW_NAN
    if not (t_lo < t_hi and e_lo < e_hi):
        return WINDOW_EMPTY
    if c["capacity"] < 0:
        return CAPACITY_NEGATIVE
    if c["capacity"] > 2 ** 31 - 1:
        return CAPACITY_TOO_LARGE
    if c["n_obs"] > MAX_OBS:
        return TOO_MANY_OBSERVERS
    return OK


def chunk_rule(n_slots):
    """-> (slots of a chunk, chunks): 64 slots a trip, eight trips at least, more when the chunks would outnumber MAX_CHUNKS"""
    trips = max(MIN_TRIPS, -(-max(n_slots, 0) // (WAVE * MAX_CHUNKS)))
    return WAVE * trips, -(-n_slots // (WAVE * trips)) if n_slots > 0 else 0


def layout_rule(c):
    """events_layout restated from the header's text: every part on a multiple of ALIGN bytes"""
    up = lambda x: -(-x // ALIGN) * ALIGN
    n_obs, cap = c["n_obs"], c["capacity"]
    axes = c["ex"] is not None and c["ey"] is not None
    head_words = 3 * n_obs + n_obs + 1 + 2
    staged_doubles = (10 if axes else 4) * n_obs
    l = {}
    at = up(8 * head_words)
    l["staged"] = at; at = up(at + 8 * staged_doubles)
    l["clocks"] = at; at = up(at + 8 * LAYOUT_CLOCKS)
    l["table"] = at; at = up(at + 8 * n_obs * chunk_rule(LAYOUT_SLOTS)[1])
    l["rank"] = at; at = up(at + 4 * cap)
    l["slot"] = at; at = up(at + 4 * cap)
    l["f8"], l["f8_pitch"] = at, up(8 * cap); at += l["f8_pitch"] * (10 if axes else 8)
    l["type"] = at; at = up(at + cap)
    for k in ("sort_table", "source", "keys", "keys_pitch", "index", "index_pitch"):
        l[k] = 0
    if c["order"] == BY_TIME:
        l["sort_table"] = at; at = up(at + 4 * 256 * (-(-cap // SORT_TILE)))
        l["source"] = at; at = up(at + 4 * cap)
        l["keys"], l["keys_pitch"] = at, up(8 * cap); at += 2 * l["keys_pitch"]
        l["index"], l["index_pitch"] = at, up(4 * cap); at += 2 * l["index_pitch"]
    return [n_obs, c["order"], c["frame"], int(axes), cap, head_words, staged_doubles, 3 * n_obs, 3 * n_obs + n_obs + 1, l["staged"], l["clocks"], l["table"],
            l["rank"], l["slot"], l["f8"], l["f8_pitch"], l["type"], l["sort_table"], l["source"], l["keys"], l["keys_pitch"], l["index"], l["index_pitch"], at]


def pass_rule(key_or, key_and, n_obs):
    """-> (passes launched, the passes that run as (observer, digit) pairs, the buffer each launched pass reads and the one that holds the result)"""
    varies = key_or ^ key_and
    observer_digits = 0
    most = n_obs - 1
    while most:
        observer_digits, most = observer_digits + 1, most >> DIGIT_BITS
    launched = [(0, d) for d in range(KEY_PASSES)] + [(1, j) for j in range(observer_digits)]
    run = [(o, d) for o, d in launched if o or (varies >> (DIGIT_BITS * d)) & 0xFF]
    buffers, done = [], 0
    for p in launched:
        buffers.append(done & 1)
        done += p in run
    return len(launched), run, buffers + [done & 1]


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan(out, name):
    c = PLANS[name]
    why = plan_rule(c)
    assert why == REFUSED.get(name, OK), (name, why)
    assert out["plan_" + name] == [why], (name, out["plan_" + name], why)
    if why == OK:
        assert out["planv_" + name] == layout_rule(c), name
    else:
        assert "planv_" + name not in out


def test_every_refusal_is_reached_and_the_order_is_the_documented_one():
    assert set(REFUSED.values()) == set(TEXTS)
    own = [BAD_ORDER, BAD_FRAME, AXES_NOT_FINITE, AXES_NOT_UNIT, AXES_NOT_ORTHOGONAL, FRAME_NEEDS_AXES, XY_NEED_AXES, WINDOW_NAN, WINDOW_EMPTY, CAPACITY_NEGATIVE,
           CAPACITY_TOO_LARGE, TOO_MANY_OBSERVERS]
    assert own == sorted(own)
    # every neighbouring pair of the order has a case with both faults (the *_before_* cases and the window's two)
    assert plan_rule(PLANS["t_equal"]) == WINDOW_EMPTY and plan_rule(PLANS["capacity_beyond_int"]) == CAPACITY_TOO_LARGE


def test_refusal_texts(out):
    for k, t in TEXTS.items():
        assert out["text_%d" % k] == t and t.startswith(PREFIX + " ")
    assert len(set(TEXTS.values())) == len(TEXTS)


def test_constants(out):
    assert out["constants"] == [MAX_OBS, BLOCK, WAVE, MIN_TRIPS, MAX_CHUNKS, DIGIT_BITS, SORT_TILE, SCAN_BLOCK, SCAN_ITEMS, ALIGN, KEY_PASSES, KEY_PASSES + 2, 3, 10]
    assert SORT_TILE % BLOCK == 0 and 2 ** DIGIT_BITS == BLOCK and 16 * 4 * MAX_OBS <= 64 * 1024


def test_layout_of_two_capacities():
    a, b = layout_rule(PLANS["axes"]), layout_rule(PLANS["three"])
    assert a[-1] % ALIGN == 0 and b[-1] % ALIGN == 0
    # what a row costs in a BY_TIME list with axes: 2 ints, 10 doubles, a char, the slot, two keys and two indices
    grow = layout_rule(dict(PLANS["axes"], capacity=1000 + 256 * 100))[-1] - a[-1]
    assert grow >= 256 * 100 * (2 * 4 + 10 * 8 + 1 + 4 + 2 * 8 + 2 * 4)
    assert layout_rule(PLANS["by_photon"])[-1] < layout_rule(PLANS["bare"])[-1]      # no sort buffers


def test_chunks(out):
    want = []
    for n in CHUNK_SLOTS:
        want += list(chunk_rule(n))
    assert out["chunks"] == want
    assert [chunk_rule(n) for n in CHUNK_SLOTS[:5]] == [(CHUNK, 0), (CHUNK, 1), (CHUNK, 1), (CHUNK, 1), (CHUNK, 2)]
    assert chunk_rule(CHUNK * MAX_CHUNKS) == (CHUNK, MAX_CHUNKS) and chunk_rule(CHUNK * MAX_CHUNKS + 1)[0] == CHUNK + WAVE
    assert all(chunk_rule(n)[1] <= MAX_CHUNKS for n in CHUNK_SLOTS)
    assert out["tiles"] == [0, 1, 1, 1, 2, 2 ** 20]


def test_key_map_on_the_ladder(out):
    want = [int(k) for k in E.key(np.array(LADDER))]
    assert out["keys"] == want and want == sorted(want) and len(set(want)) == len(want)


def test_pass_lists(out):
    assert out["observer_passes"] == [0, 1, 1, 2, 2]
    for i, (name, (key_or, key_and, n_obs)) in enumerate(MASKS.items()):
        launched, run, buffers = pass_rule(key_or, key_and, n_obs)
        got = out["passes_%d" % i]
        assert got[:2] == [launched, len(run)] and list(zip(got[2::2], got[3::2])) == run, name
        assert out["buffers_%d" % i] == buffers, name
    rule = lambda name: pass_rule(*MASKS[name])[1]
    assert rule("all_equal") == []                                               # no key pass, and one observer: no pass at all
    assert rule("lowest_byte") == [(0, 0)] == rule("lowest_bit")
    assert rule("top_byte") == [(0, 7)]
    assert rule("all_vary") == [(0, d) for d in range(8)]
    assert rule("middle_two") == [(0, 2), (0, 4), (1, 0)]
    assert rule("all_equal_two_observers") == [(1, 0)]
    assert rule("observers_256") == [(0, 0), (1, 0)] and rule("observers_257") == [(0, 0), (1, 0), (1, 1)]      # 257 observers need a second digit


def test_small_functions(out):
    assert out["row_observer"] == [1, 1, 4, 4, 0, 0]                             # rows 0 .. 2 are observer 1's, 3 .. 9 observer 4's
    assert out["window"] == [1, 0, 0, 0, 1, 0, 0]


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
