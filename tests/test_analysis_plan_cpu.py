"""The host rules that the analysis products' entry points share (mcrat_amd/csrc/analysis_plan.hpp) on the CPU: the two makers of a photon source
against the literals the entry points used to write out, the staging order of the sky family's observer inputs against the sequence restated here
and against the staged_doubles of the real plans (sky_plan, escape_plan, resample_plan, events_plan), and the frame verdict over its whole truth
table.  They are plain C++: a small driver is compiled with g++ and what it prints is compared.  The same driver is built a second time with
-fsanitize=address,undefined and run once."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MISMATCH, NO_FRAME, NO_TABLE = range(4)
N_TAU = 3
# every input array holds values no other array holds: array a's entry i is 1000 * (a + 1) + i
ARRAYS = ("n0", "n1", "n2", "cos_acc", "x0", "x1", "x2", "y0", "y1", "y2", "t_edges", "e_edges", "x_edges", "y_edges", "tau_edges")
# name: (shape, n_obs, n_t, n_e, n_x, n_y, STOKES_SKY_PLANE or the events' axes given)
CASES = {
    "sky_curve": ("sky", 3, 4, 5, 0, 0, 0),
    "sky_image": ("sky", 3, 4, 5, 6, 2, 0),
    "sky_corner": ("sky", 1, 1, 1, 0, 0, 0),
    "sky_corner_image": ("sky", 1, 1, 1, 1, 2, 0),
    "escape_curve": ("escape", 3, 4, 5, 0, 0, 0),
    "escape_image": ("escape", 2, 3, 2, 1, 2, 0),
    "escape_corner": ("escape", 1, 1, 1, 0, 0, 0),
    "resample_stored": ("resample", 3, 4, 5, 0, 0, 0),
    "resample_axes_no_image": ("resample", 3, 4, 5, 0, 0, 1),
    "resample_image": ("resample", 2, 2, 3, 1, 2, 0),
    "resample_image_sky_plane": ("resample", 2, 2, 3, 4, 3, 1),
    "resample_corner": ("resample", 1, 1, 1, 0, 0, 1),
    "events_vectors": ("events", 3, 1, 1, 0, 0, 0),
    "events_axes": ("events", 3, 1, 1, 0, 0, 1),
    "events_corner": ("events", 1, 1, 1, 0, 0, 1),
}

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "analysis_plan.hpp"
#include "escape_plan.hpp"
#include "resample_plan.hpp"
#include "events_plan.hpp"
using namespace mcrat;
typedef std::vector<double> V;

static V marked(int array, int n) { V v; for (int i = 0; i < n; ++i) v.push_back(1000.0 * (array + 1) + i); return v; }
static V ramp(int n) { V v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }

// the plan's answer for arguments it accepts -- observers on the r2 axis, ramps for edges --, then the staging function on marked arrays of the
// same counts, told what the plan says is present, as engine.hip tells it
static void stage(const char *name, const char *shape, int n_obs, int n_t, int n_e, int n_x, int n_y, int sky_plane)
{
    const V zero(n_obs, 0.0), one(n_obs, 1.0), half(n_obs, 0.5), te = ramp(n_t), ee = ramp(n_e), xe = ramp(n_x), ye = ramp(n_y), tau = ramp(@N_TAU@);
    const bool give_axes = n_x > 0 || sky_plane;
    SkyArgs good{n_obs, zero.data(), zero.data(), one.data(), half.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                 n_t, te.data(), n_e, ee.data(), n_x, n_x ? xe.data() : nullptr, n_y, n_y ? ye.data() : nullptr};
    if (give_axes) { good.x0 = one.data(); good.x1 = good.x2 = zero.data(); good.y0 = good.y2 = zero.data(); good.y1 = one.data(); }
    std::vector<V> m;
    for (int a = 0; a < 10; ++a) m.push_back(marked(a, n_obs));
    m.push_back(marked(10, n_t + 1)); m.push_back(marked(11, n_e + 1)); m.push_back(marked(12, n_x + 1)); m.push_back(marked(13, n_y + 1));
    const SkyArgs s{n_obs, m[0].data(), m[1].data(), m[2].data(), m[3].data(), m[4].data(), m[5].data(), m[6].data(), m[7].data(), m[8].data(), m[9].data(),
                    n_t, m[10].data(), n_e, m[11].data(), n_x, m[12].data(), n_y, m[13].data()};
    int refused = -1;
    size_t staged_doubles = 0;
    V in;
    if (shape[0] == 's') {
        SkyPlan p;
        if (!(refused = (int)sky_plan(good, nullptr, &p))) { staged_doubles = p.staged_doubles; stage_observer_inputs(s, p.image, true, p.image, &in); }
    } else if (shape[0] == 'e' && shape[1] == 's') {
        EscapeArgs a{good, @N_TAU@, tau.data(), SightlineParams{1e-3, 1e8, 400, INFINITY, -1.0}};
        EscapePlan p;
        if (!(refused = (int)escape_plan(a, nullptr, &p))) {
            staged_doubles = p.staged_doubles;
            stage_observer_inputs(s, p.image, true, p.image, &in);
            const V mt = marked(14, p.n_tau + 1);
            in.insert(in.end(), mt.begin(), mt.end());               // (what the caller appends)
        }
    } else if (shape[0] == 'r') {
        const ResampleArgs a{good, RESAMPLE_JACKKNIFE, 4, sky_plane ? STOKES_SKY_PLANE : STOKES_AS_STORED};
        ResamplePlan p;
        if (!(refused = (int)resample_plan(a, nullptr, &p))) { staged_doubles = p.staged_doubles; stage_observer_inputs(s, p.axes, true, p.image, &in); }
    } else {
        const EventsArgs a{n_obs, good.n0, good.n1, good.n2, good.cos_acc, good.x0, good.x1, good.x2, good.y0, good.y1, good.y2,
                           0.0, 1.0, 0.0, 1.0, EVENTS_BY_TIME, sky_plane ? STOKES_SKY_PLANE : STOKES_AS_STORED, 0, false};
        EventsPlan p;
        if (!(refused = (int)events_plan(a, &p))) { staged_doubles = p.staged_doubles; stage_observer_inputs(s, p.axes, false, false, &in); }
    }
    printf("stage_%s: %d %zu", name, refused, staged_doubles);
    for (double v : in) printf(" %.17g", v);
    printf("\n");
}

int main()
{
@CASES@
    const double clocks[5] = {1.0, 2.0, 3.0, 4.0, 5.0};
    const PhotonSource l = list_source(64, 12.5, 3), p = pool_source(35, 5, 7, clocks);
    printf("list_source: %d %d %d %d %.17g %d %d\n", l.n_slots, (int)(l.clocks == nullptr), l.n_clocks, l.slots_per_clock, l.time_now, l.rank_base, l.rank_stride);
    printf("pool_source: %d %d %d %d %.17g %d %d\n", p.n_slots, (int)(p.clocks == clocks), p.n_clocks, p.slots_per_clock, p.time_now, p.rank_base, p.rank_stride);
    // the frame verdict: same, which switch of h differs (0: none; dimensions, geometry, table, device), c's table, have_hydro, M, hot table, with_table, need_cells
    for (int same = 0; same < 2; ++same) for (int differs = 0; differs < 5; ++differs) for (int table = 0; table < 2; ++table)
    for (int have = 0; have < 2; ++have) for (int M = 0; M < 2; ++M) for (int hot = 0; hot < 2; ++hot) for (int wt = 0; wt < 2; ++wt) for (int nc = 0; nc < 2; ++nc) {
        const FrameSwitches c{2, 1, table, 0};
        FrameSwitches h = c;
        if (differs == 1) h.dimensions = 3;
        if (differs == 2) h.geometry = 0;
        if (differs == 3) h.table = !table;
        if (differs == 4) h.device = 1;
        printf("frame: %d %d %d %d %d %d %d %d %d\n", same, differs, table, have, M, hot, wt, nc, (int)frame_verdict(c, h, same, have, M, hot, wt, nc));
    }
    printf("verdicts: %d %d %d %d\n", (int)FRAME_OK, (int)FRAME_MISMATCH, (int)FRAME_NONE, (int)FRAME_NO_TABLE);
    return 0;
}
'''


def _build(d, src, name, extra):
    exe = d / name
    # (-Wno-unknown-pragmas: resample_plan.hpp reads rng.hpp, whose unroll pragmas are the device compiler's)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("analysis_plan")
    src = d / "driver.cpp"
    cases = "\n".join('    stage("%s", "%s", %d, %d, %d, %d, %d, %d);' % ((name,) + c) for name, c in CASES.items())
    src.write_text(DRIVER.replace("@CASES@", cases).replace("@N_TAU@", str(N_TAU)))
    return d, src


@pytest.fixture(scope="module")
def text(built):
    d, src = built
    return subprocess.run([str(_build(d, src, "driver", []))], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def out(text):
    res = {"frame": {}}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        if key == "frame":
            v = [int(x) for x in vals.split()]
            res["frame"][tuple(v[:-1])] = v[-1]
        else:
            res[key] = [float(x) for x in vals.split()]
    return res


def marked(name, n):
    return [1000.0 * (ARRAYS.index(name) + 1) + i for i in range(n)]


def staged(shape, n_obs, n_t, n_e, n_x, n_y, sky_plane):
    """the sequence restated: what is present in each of the four shapes, and in what order"""
    image = n_x > 0
    axes = {"sky": image, "escape": image, "resample": image or bool(sky_plane), "events": bool(sky_plane)}[shape]
    seq = [(k, n_obs) for k in ("n0", "n1", "n2", "cos_acc")]
    if axes:
        seq += [(k, n_obs) for k in ("x0", "x1", "x2", "y0", "y1", "y2")]
    if shape != "events":
        seq += [("t_edges", n_t + 1), ("e_edges", n_e + 1)]
        if image:
            seq += [("x_edges", n_x + 1), ("y_edges", n_y + 1)]
    if shape == "escape":
        seq += [("tau_edges", N_TAU + 1)]
    return [v for k, n in seq for v in marked(k, n)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_staging_order_and_length(out, name):
    refused, staged_doubles, got = int(out["stage_" + name][0]), int(out["stage_" + name][1]), out["stage_" + name][2:]
    assert refused == 0                                          # the real plan took the arguments
    want = staged(*CASES[name])
    assert got == want
    assert len(got) == staged_doubles                            # for escape: with the n_tau + 1 edges that the caller appends
    assert len(set(got)) == len(got)                             # no array twice: the markers are all different


def test_staging_cases_are_what_they_are_meant_to_be():
    """all four shapes, with and without axes and image where the shape has the choice; the corner of one observer and one bin per axis; an image
    of 1 x 2 pixels"""
    shapes = {c[0] for c in CASES.values()}
    assert shapes == {"sky", "escape", "resample", "events"}
    for shape in ("sky", "escape", "resample"):
        assert {c[4] > 0 for c in CASES.values() if c[0] == shape} == {False, True}
    assert {(c[4] > 0, c[6]) for c in CASES.values() if c[0] == "resample"} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert {c[6] for c in CASES.values() if c[0] == "events"} == {0, 1}
    assert sum(c[1:4] == (1, 1, 1) for c in CASES.values()) >= 4 and any(c[4:6] == (1, 2) for c in CASES.values())
    assert len(staged("sky", 3, 4, 5, 0, 0, 0)) == 4 * 3 + 5 + 6 and len(staged("escape", 2, 3, 2, 1, 2, 0)) == 10 * 2 + 4 + 3 + 2 + 3 + N_TAU + 1
    assert len(staged("resample", 3, 4, 5, 0, 0, 1)) == 10 * 3 + 5 + 6 and len(staged("events", 3, 1, 1, 0, 0, 1)) == 10 * 3


def test_sources_are_the_literals_the_entry_points_wrote(out):
    """a list: c->ph.n, nullptr, 0, 1, time_now, view_rank, 0; a pool: c->ph.n, time_now, c->n_ranks, c->rank_stride, 0.0, 0, c->rank_stride"""
    #                            n_slots clocks n_clocks slots_per_clock time_now rank_base rank_stride
    assert out["list_source"] == [64, 1, 0, 1, 12.5, 3, 0]       # (clocks: 1 stands for nullptr)
    assert out["pool_source"] == [35, 1, 5, 7, 0.0, 0, 7]        # (clocks: 1 stands for the caller's array)


def verdict(same, differs, table, have, M, hot, with_table, need_cells):
    """the rule restated: the switches of another context (its table only for a product that marches), then the frame (its cells only for a product
    that sums per cell), then the hot table (for a product that marches, on a context with TAU_CALCULATION == TABLE)"""
    if not same and (differs in (1, 2, 4) or (differs == 3 and with_table)):
        return MISMATCH
    if not have or (need_cells and M <= 0):
        return NO_FRAME
    if with_table and table and not hot:
        return NO_TABLE
    return OK


def test_frame_verdict_truth_table(out):
    assert out["verdicts"] == [OK, MISMATCH, NO_FRAME, NO_TABLE]
    keys = list(itertools.product(range(2), range(5), *[range(2)] * 6))
    assert sorted(out["frame"]) == keys and len(keys) == 640
    for k in keys:
        assert out["frame"][k] == verdict(*k), k
    assert {out["frame"][k] for k in keys} == {OK, MISMATCH, NO_FRAME, NO_TABLE}


def test_frame_verdict_precedence(out):
    """mismatch before no frame before no table, and what each flag switches off"""
    f = out["frame"]
    #        same differs table have M hot with_table need_cells
    assert f[(0, 1, 1, 0, 0, 0, 1, 1)] == MISMATCH               # everything wrong at once
    assert f[(1, 1, 1, 0, 0, 0, 1, 1)] == NO_FRAME               # the context's own frame: no switches to compare
    assert f[(0, 0, 1, 0, 1, 0, 1, 0)] == NO_FRAME               # no frame and no table
    assert f[(0, 0, 1, 1, 1, 0, 1, 0)] == NO_TABLE
    assert f[(0, 0, 1, 1, 1, 0, 0, 0)] == OK                     # a product that does not march does not ask for the table
    assert f[(0, 0, 0, 1, 1, 0, 1, 0)] == OK                     # nor does a context without TAU_CALCULATION == TABLE
    assert f[(0, 3, 0, 1, 1, 0, 1, 0)] == MISMATCH and f[(0, 3, 0, 1, 1, 0, 0, 0)] == OK         # the table switch differs: only a marching product minds
    assert f[(1, 0, 0, 1, 0, 0, 0, 1)] == NO_FRAME and f[(1, 0, 0, 1, 0, 0, 0, 0)] == OK         # a frame without cells: only a summing product minds
    for differs in (1, 2, 4):
        assert f[(0, differs, 0, 1, 1, 1, 0, 0)] == MISMATCH and f[(1, differs, 0, 1, 1, 1, 0, 0)] == OK


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
