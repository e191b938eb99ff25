"""The covered-octant table of the cell-lookup grid (hydro_plan.hpp: octant_covered, covered_table_ints, bucket_covered; GridDev::cov_back).

An entry >= 0 lets the device take a position with GRID_CODE_HINT_OK into that cell without reading the bucket's record, the hinted list entry or
running the in-cell test, so for every such position the entry must be the decision the hinted path takes: the hinted entry passes
well_in_fat_cell's inequality, and its cell is the linear scan's lowest-index containing cell (geometry.c:350-391).  A g++ driver over
hydro_plan.hpp (as tests/test_hydro_plan_cpu.py has one) builds the grid of a mesh with build_grid and takes positions through the device's own
accept rule (physics.hpp, grid_bucket_axes, restated in the same double arithmetic): seeded ones over the mesh's extent, and for a sample of the
covered octants their corners at the accept margin -- fr = 1e-6 (1 + j ulp) and 0.5 - 1e-6 (1 + j ulp) inside the octant's half, j = -3 .. 3: the
positions nearest a cell face that a covered entry can ever serve, on either side of the accept rule's comparison.

The guard of the rule is 64 DBL_EPSILON (|c| + s) on top of 1e-8 s against the 0.5e-6 bucket widths that are left of the margin: with unit buckets
and unit cells it switches covering off from |c| + s = (0.5e-6 - 1e-8) / (64 DBL_EPSILON) = 3.448e7 on, which the driver probes cell by cell."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from mcrat_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cfloat>
#include <vector>
#include "hydro_plan.hpp"
using namespace mcrat;

template <class T> static std::vector<T> get(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }

static int M, naxes;
static std::vector<double> col[6];
static const double *c[3], *s[3];
static GridHost g;

// physics.hpp, grid_bucket_axes: bucket, octant and whether the position may use a hint
static bool code_of(const double *a, long long &b, int &oct)
{
    const GridPlan &p = g.plan;
    int bk[3] = {0, 0, 0};
    bool ok = true;
    oct = 0;
    for (int k = 0; k < naxes; ++k) {
        double u = a[k];
        if (p.logmap[k]) u = log(a[k]);
        const double x = (u - p.org[k]) * p.inv[k];
        const double f = floor(x);
        const double fr = x - f;
        const double hi = (double)(p.dim[k] - 1);
        ok = ok & (f >= 0.0) & (f <= hi) & (fr > 1e-6) & (fabs(fr - 0.5) > 1e-6) & (1.0 - fr > 1e-6);
        oct |= (fr >= 0.5 ? 1 : 0) << k;
        bk[k] = (int)fmin(fmax(f, 0.0), hi);
    }
    b = ((long long)bk[2] * p.dim[1] + bk[1]) * p.dim[0] + bk[0];
    return ok;
}
// geometry.c:350-391
static int linear_scan(const double *a)
{
    for (int i = 0; i < M; ++i) {
        bool in = true;
        for (int k = 0; k < naxes && in; ++k) in = 2 * fabs(a[k] - c[k][i]) - s[k][i] <= 0;
        if (in) return i;
    }
    return -1;
}
// physics.hpp, well_in_fat_cell on cell ci
static bool well_in(const double *a, int ci)
{
    bool in = true;
    for (int k = 0; k < naxes; ++k) in = in & (2 * fabs(a[k] - c[k][ci]) - s[k][ci] < -1e-8 * s[k][ci]);
    return in;
}

struct Tally { long long points = 0, in_covered = 0, decided = 0, not_ok = 0, bad_hint = 0, bad_well_in = 0, bad_cell = 0, found = 0; };
static void take(const double *a, Tally &t)
{
    long long b;
    int oct;
    const bool ok = code_of(a, b, oct);
    t.points += 1;
    const int scan = linear_scan(a);
    t.found += scan >= 0;
    if (g.covered.empty()) return;
    const int e = g.covered[((size_t)b << naxes) + oct];
    if (e < 0) return;
    t.in_covered += 1;
    if (!ok) { t.not_ok += 1; return; }                     // the device does not read the table for this position
    t.decided += 1;
    const unsigned hint = (g.hints[(size_t)b] >> (4 * oct)) & 15u;
    if (hint == GRID_NO_HINT || g.cells[g.start[(size_t)b] + hint] != e) { t.bad_hint += 1; return; }
    t.bad_well_in += !well_in(a, e);
    t.bad_cell += scan != e;
}
static void print(const char *tag, const Tally &t)
{
    printf("%s: %lld %lld %lld %lld %lld %lld %lld %lld\n", tag, t.points, t.in_covered, t.decided, t.not_ok, t.bad_hint, t.bad_well_in, t.bad_cell, t.found);
}
static double step_ulps(double x, int j) { for (; j > 0; --j) x = nextafter(x, INFINITY); for (; j < 0; ++j) x = nextafter(x, -INFINITY); return x; }

static int mesh(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    const std::vector<int> head = get<int>(f, 5);
    M = head[0]; naxes = head[1];
    const int n_seeded = head[2], n_octants = head[3], n_given = head[4];
    for (int k = 0; k < 2 * naxes; ++k) col[k] = get<double>(f, M);
    std::vector<double> given[3];
    for (int k = 0; k < naxes; ++k) given[k] = get<double>(f, n_given);
    fclose(f);
    for (int k = 0; k < 3; ++k) { c[k] = k < naxes ? col[2 * k].data() : nullptr; s[k] = k < naxes ? col[2 * k + 1].data() : nullptr; }
    g = GridHost{};
    if (!build_grid(c, s, M, naxes, g)) { printf("grid: 0\n"); return 0; }
    const GridPlan &p = g.plan;
    const int nocts = 1 << naxes;
    printf("grid: 1 %lld %d %d %d %zu %zu\n", g.nb, p.logmap[0], p.logmap[1], p.logmap[2], g.covered.size(), covered_table_ints(p, g.nb, true));
    double lo[3], hi[3];
    for (int k = 0; k < naxes; ++k) {
        lo[k] = INFINITY; hi[k] = -INFINITY;
        for (int i = 0; i < M; ++i) { lo[k] = fmin(lo[k], c[k][i] - 0.5 * s[k][i]); hi[k] = fmax(hi[k], c[k][i] + 0.5 * s[k][i]); }
    }
    // octants: all, hinted, covered; and of the interior ones (a bucket width inside the mesh's extent on every axis) the hinted and the covered
    long long hinted = 0, covered = 0, interior_hinted = 0, interior_covered = 0, wide_covered = 0;
    std::vector<long long> cov_list;
    for (long long b = 0; b < g.nb; ++b) {
        const int bi[3] = {(int)(b % p.dim[0]), (int)((b / p.dim[0]) % p.dim[1]), (int)(b / ((long long)p.dim[0] * p.dim[1]))};
        for (int o = 0; o < nocts; ++o) {
            const bool h = ((g.hints[(size_t)b] >> (4 * o)) & 15u) != GRID_NO_HINT;
            const int e = g.covered.empty() ? -1 : g.covered[((size_t)b << naxes) + o];
            bool interior = true;
            for (int k = 0; k < naxes; ++k) {
                const double w = 1.0 / p.inv[k], olo = p.org[k] + (bi[k] + 0.5 * ((o >> k) & 1)) * w;
                interior = interior && olo - w >= lo[k] && olo + 1.5 * w <= hi[k];
            }
            hinted += h; covered += e >= 0;
            interior_hinted += interior && h; interior_covered += interior && e >= 0;
            if (e >= 0) {
                cov_list.push_back(b * nocts + o);
                for (int k = 0; k < naxes; ++k) wide_covered += s[k][e] * p.inv[k] > 50.0 * (1 + 1e-9);
            }
        }
    }
    printf("octants: %lld %lld %lld %lld %lld %lld\n", g.nb * nocts, hinted, covered, interior_hinted, interior_covered, wide_covered);
    // seeded positions over the extent, a twentieth of a width beyond it
    Tally seeded;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (int q = 0; q < n_seeded; ++q) {
        double a[3] = {0, 0, 0};
        for (int k = 0; k < naxes; ++k) {
            rng = rng * 6364136223846793005ull + 1442695040888963407ull;
            const double u = (double)(rng >> 11) / 9007199254740992.0;
            a[k] = lo[k] + (hi[k] - lo[k]) * (1.1 * u - 0.05);
        }
        take(a, seeded);
    }
    print("seeded", seeded);
    // the corners of covered octants at the accept margin
    Tally margin;
    const size_t stride = cov_list.empty() ? 1 : std::max<size_t>(1, cov_list.size() / (size_t)std::max(1, n_octants));
    for (size_t q = 0; q < cov_list.size(); q += stride) {
        const long long b = cov_list[q] / nocts;
        const int o = (int)(cov_list[q] % nocts);
        const int bi[3] = {(int)(b % p.dim[0]), (int)((b / p.dim[0]) % p.dim[1]), (int)(b / ((long long)p.dim[0] * p.dim[1]))};
        for (int corner = 0; corner < nocts; ++corner)
            for (int j = -3; j <= 3; ++j) {
                double a[3] = {0, 0, 0};
                for (int k = 0; k < naxes; ++k) {
                    const double d = step_ulps(1e-6, j);
                    const double fr = 0.5 * ((o >> k) & 1) + (((corner >> k) & 1) ? 0.5 - d : d);
                    a[k] = p.org[k] + (bi[k] + fr) / p.inv[k];
                }
                take(a, margin);
            }
    }
    print("margin", margin);
    // the caller's positions, and for each whether the table settles it
    Tally tg;
    std::vector<char> flags((size_t)n_given + 1, 0);
    for (int q = 0; q < n_given; ++q) {
        const double a[3] = {given[0][q], given[1][q], naxes == 3 ? given[2][q] : 0.0};
        const long long before = tg.decided;
        take(a, tg);
        flags[q] = tg.decided > before ? '1' : '0';
    }
    print("given", tg);
    printf("flags: %s\n", flags.data());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (argv[1][0] != '-') return mesh(argv[1]);
    // ---- the guard at its threshold: unit buckets from 0, unit cells on them; cell k's lower half is octant 0 of bucket k
    {
        GridPlan p{};
        p.naxes = 2;
        for (int k = 0; k < 3; ++k) { p.org[k] = 0; p.inv[k] = 1; p.dim[k] = 1 << 30; }
        const double limit = (0.5e-6 - 1e-8) / GRID_COVER_GUARD;            // of |c| + s
        printf("guard: %.17g %.17g\n", GRID_COVER_GUARD, limit);
        long long last_covered = -1, first_uncovered = -1;
        for (long long kk = (long long)limit - 40; kk < (long long)limit + 40; ++kk) {
            const int bi[3] = {(int)kk, 3, 0};
            const double cc[3] = {kk + 0.5, 3.5, 0}, ss[3] = {1, 1, 0};
            const bool cov = octant_covered(p, bi, 0, cc, ss);
            if (cov) last_covered = kk;
            if (!cov && first_uncovered < 0) first_uncovered = kk;
        }
        printf("threshold: %lld %lld\n", last_covered, first_uncovered);
        // the other terms of the rule, one at a time, on bucket (10, 3): the cell [10, 11] x [3, 4]
        const int bi[3] = {10, 3, 0};
        const double c0[3] = {10.5, 3.5, 0}, s1[3] = {1, 1, 0};
        const double c_short[3] = {10.5 + 1e-6, 3.5, 0};                   // its lower face 1e-6 inside the octant: more than the 0.5e-6 allowed
        const double c_touch[3] = {10.5 + 0.4e-6, 3.5, 0};                 // 0.4e-6: allowed
        const double c_wide[3] = {10 + 30, 3.5, 0}, s_wide[3] = {60, 1, 0}, s_50[3] = {49, 1, 0}, c_50[3] = {10 + 24.5, 3.5, 0};
        const double c_nan[3] = {NAN, 3.5, 0};
        GridPlan pl = p;
        pl.logmap[1] = 1;
        printf("terms: %d %d %d %d %d %d %d %d\n", (int)octant_covered(p, bi, 0, c0, s1), (int)octant_covered(p, bi, 0, c_short, s1),
               (int)octant_covered(p, bi, 0, c_touch, s1), (int)octant_covered(p, bi, 0, c_wide, s_wide), (int)octant_covered(p, bi, 0, c_50, s_50),
               (int)octant_covered(p, bi, 0, c_nan, s1), (int)octant_covered(pl, bi, 0, c0, s1), (int)octant_covered(p, bi, 3, c0, s1));
    }
    // ---- the size rule and the layout
    {
        GridPlan p2{}, p3{}, pl{};
        p2.naxes = 2; p3.naxes = 3; pl.naxes = 2; pl.logmap[0] = 1;
        const long long cap = GRID_COVERED_MAX_INTS;
        printf("sizes: %zu %zu %zu %zu %zu %zu %zu %zu %lld\n", covered_table_ints(p2, 1000, true), covered_table_ints(p3, 1000, true), covered_table_ints(p2, 1000, false),
               covered_table_ints(pl, 1000, true), covered_table_ints(p2, cap / 4, true), covered_table_ints(p2, cap / 4 + 1, true),
               covered_table_ints(p3, cap / 8, true), covered_table_ints(p3, cap / 8 + 1, true), cap);
        const GridLayout with = grid_layout(1089, 4096, 7, 4356), without = grid_layout(1089, 4096, 7, 0), old = grid_layout(1089, 4096, 7);
        printf("layout: %zu %zu %zu %zu %zu %zu %zu\n", with.covered, with.dir, with.cells, with.start, with.scan, with.entries, with.total);
        printf("layout_none: %zu %zu %zu %zu %zu %zu %zu\n", without.covered, without.dir, without.cells, without.start, without.scan, without.entries, without.total);
        printf("layout_old: %zu %zu %zu %zu %zu %zu %zu\n", old.covered, old.dir, old.cells, old.start, old.scan, old.entries, old.total);
        printf("index: %d %d %d\n", covered_index(5 | (3 << GRID_CODE_OCT_SHIFT) | GRID_CODE_HINT_OK, 2), covered_index(5 | (7 << GRID_CODE_OCT_SHIFT), 3),
               covered_index(GRID_CODE_BUCKET_MASK >> 3, 3));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the covered-octant rule's driver")
    d = str(tmp_path_factory.mktemp("covered"))
    src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), src, "-o", exe], check=True)
    return d, exe


def _rows(text):
    rows = {}
    for line in text.splitlines():
        tag, _, rest = line.partition(": ")
        rows[tag] = [float(v) for v in rest.split()]
    return rows


TALLY = ("points", "in_covered", "decided", "not_ok", "bad_hint", "bad_well_in", "bad_cell", "found")


def run_mesh(driver, name, columns, n_seeded=20000, n_octants=1500, points=None):
    """columns: per axis (centres, widths); points: per axis the coordinates of positions of the caller's -> dict(grid, octants, seeded, margin,
    given, flags: per position of the caller's whether the table settles it)"""
    d, exe = driver
    path = os.path.join(d, name + ".in")
    M = len(columns[0][0])
    with open(path, "wb") as f:
        np.array([M, len(columns), n_seeded, n_octants, 0 if points is None else len(points[0])], dtype=np.int32).tofile(f)
        for ctr, wid in columns:
            np.ascontiguousarray(ctr, dtype=np.float64).tofile(f)
            np.ascontiguousarray(wid, dtype=np.float64).tofile(f)
        for x in (points or []):
            np.ascontiguousarray(x, dtype=np.float64).tofile(f)
    text = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout
    rows = _rows("\n".join(line for line in text.splitlines() if not line.startswith("flags: ")))
    flags = [line[7:] for line in text.splitlines() if line.startswith("flags: ")]
    assert rows["grid"][0] == 1, "build_grid refused the mesh"
    out = dict(nb=int(rows["grid"][1]), logmap=tuple(int(v) for v in rows["grid"][2:5]), table=int(rows["grid"][5]), rule=int(rows["grid"][6]))
    out["octants"] = dict(zip(("all", "hinted", "covered", "interior_hinted", "interior_covered", "wide_covered"), (int(v) for v in rows["octants"])))
    for k in ("seeded", "margin", "given"):
        out[k] = dict(zip(TALLY, (int(v) for v in rows[k])))
    out["flags"] = np.array([ch == "1" for ch in flags[0]], dtype=bool)
    return out


def check_decisions(got, what):
    """every position the device would settle by the table is settled as the hinted path settles it"""
    for k in ("seeded", "margin", "given"):
        t = got[k]
        assert t["bad_hint"] == 0 and t["bad_well_in"] == 0 and t["bad_cell"] == 0, (what, k, t)
    print("%s: %d buckets, %d of %d octants hinted, %d covered (interior: %d of %d hinted ones); seeded %s; margin %s"
          % (what, got["nb"], got["octants"]["hinted"], got["octants"]["all"], got["octants"]["covered"], got["octants"]["interior_covered"],
             got["octants"]["interior_hinted"], got["seeded"], got["margin"]))


def frame_columns(frame, naxes=2):
    return [(frame["r%d" % k], frame["r%d_size" % k]) for k in range(naxes)]


def two_level(x0=0.0, y0=0.0, w=1.0):
    """16 x 16 fine cells of width w beside 8 x 8 coarse ones of 2 w, from (x0, y0): the lower-quartile width is the fine one"""
    fx, fy = np.meshgrid(x0 + (np.arange(16) + 0.5) * w, y0 + (np.arange(16) + 0.5) * w, indexing="ij")
    cx, cy = np.meshgrid(x0 + 16 * w + (np.arange(8) + 0.5) * 2 * w, y0 + (np.arange(8) + 0.5) * 2 * w, indexing="ij")
    c0 = np.concatenate([fx.ravel(), cx.ravel()])
    c1 = np.concatenate([fy.ravel(), cy.ravel()])
    s = np.concatenate([np.full(256, w), np.full(64, 2 * w)])
    return [(c0, s), (c1, s.copy())]


def cut_mesh(n_photons, lumi=1e51):
    """config2(nzc=8)'s mesh cut as tests/test_gpu_pass_serial.py cuts it: all coarse cells, and of the fine ones those beside the first column
    within 4e9 cm of the photons' shell -- the buckets get the coarse width and drift against the cells (159.5 coarse widths across), so that a
    quadrant in two straddles a cell face, and the mesh has gaps"""
    frame, _, cfg = synth.config2(n_photons=16, nzc=8, stokes=0, lumi=lumi)
    fine = frame["r0_size"] == frame["r0_size"].min()
    w = float(frame["r0_size"].min())
    keep = ~fine | ((frame["r0"] > w) & (np.abs(frame["r1"] - 1e12) < 4e9))
    sub = synth.select_slab(frame, keep)
    ph = synth.inject_photons(sub, n_photons, 1e12, 0.0, 3.0 * np.pi / 180, 77)
    return sub, ph, cfg


def test_config2_mesh_every_interior_hinted_octant_is_covered(driver):
    frame, _, _ = synth.config2(n_photons=16, nzc=8)
    got = run_mesh(driver, "cfg2", frame_columns(frame))
    check_decisions(got, "config2(nzc=8)")
    o = got["octants"]
    assert got["logmap"] == (0, 0, 0) and got["table"] == got["rule"] == 4 * got["nb"]
    assert o["interior_hinted"] > 0.9 * o["hinted"]
    assert o["interior_covered"] == o["interior_hinted"]                  # fraction 1: buckets half a fine cell off the mesh, a quadrant inside one cell
    assert o["covered"] >= o["interior_covered"] and o["covered"] <= o["hinted"]
    print("covered fraction of all octants %.4f, of the hinted ones %.4f" % (o["covered"] / o["all"], o["covered"] / o["hinted"]))
    for k in ("seeded", "margin"):
        assert got[k]["decided"] > 1000
    assert 0 < got["margin"]["not_ok"] < got["margin"]["points"]          # the margin positions fall on both sides of the accept rule


def test_two_level_regular_and_permuted(driver):
    cols = two_level()
    got = run_mesh(driver, "two_level", cols)
    check_decisions(got, "two-level")
    assert got["octants"]["interior_covered"] == got["octants"]["interior_hinted"] > 0
    assert got["seeded"]["decided"] > 10000 and got["margin"]["decided"] > 1000
    perm = np.random.default_rng(5).permutation(len(cols[0][0]))
    gotp = run_mesh(driver, "permuted", [(c[perm], s[perm]) for c, s in cols])
    check_decisions(gotp, "two-level, permuted")
    assert gotp["octants"] == got["octants"]
    assert {k: gotp["seeded"][k] for k in ("in_covered", "decided", "found")} == {k: got["seeded"][k] for k in ("in_covered", "decided", "found")}


def test_mesh_with_gaps_and_straddled_quadrants(driver):
    frame, _, _ = cut_mesh(16)
    got = run_mesh(driver, "cut", frame_columns(frame))
    check_decisions(got, "cut mesh")
    o = got["octants"]
    assert 0 < o["covered"] < o["hinted"] < o["all"]                      # gaps: no hint; straddled quadrants: no hint or not covered
    assert got["seeded"]["found"] < got["seeded"]["points"]               # positions in the gaps
    assert 0 < got["seeded"]["decided"] < got["seeded"]["found"]
    # a regular mesh with a hole: the quadrants in the hole have no cell and those around it keep theirs
    cols = two_level()
    c0, c1 = cols[0][0], cols[1][0]
    keep = ~((np.abs(c0 - 6.5) < 2) & (np.abs(c1 - 6.5) < 2))
    hole = run_mesh(driver, "hole", [(c[keep], s[keep]) for c, s in cols])
    check_decisions(hole, "two-level with a hole")
    whole = run_mesh(driver, "whole", cols)
    assert hole["octants"]["covered"] == whole["octants"]["covered"] - 4 * int(np.count_nonzero(~keep))
    assert hole["seeded"]["found"] < whole["seeded"]["found"]


def test_cells_wider_than_fifty_buckets_are_not_covered(driver):
    """60 x 60 unit cells left of x = 0 and two cells of 60 x 60 right of it (the mesh starts below 0: no log-mapped axis): unit buckets, and
    0.5e-6 w < 1e-8 s for the wide cells"""
    fx, fy = np.meshgrid(-60 + np.arange(60) + 0.5, np.arange(60) + 0.5, indexing="ij")
    c0 = np.concatenate([fx.ravel(), [30.0, 90.0]])
    c1 = np.concatenate([fy.ravel(), [30.0, 30.0]])
    s = np.concatenate([np.ones(3600), [60.0, 60.0]])
    got = run_mesh(driver, "wide", [(c0, s), (c1, s.copy())])
    check_decisions(got, "wide cells")
    o = got["octants"]
    assert got["logmap"] == (0, 0, 0)
    assert o["wide_covered"] == 0 and 0 < o["covered"] < o["hinted"]
    assert o["hinted"] - o["covered"] > 2 * 4 * 58 * 58                    # the wide cells' quadrants are hinted and not covered
    assert got["seeded"]["in_covered"] < 0.5 * got["seeded"]["found"]


def test_far_from_the_origin_the_guard_switches_covering_off(driver):
    far = run_mesh(driver, "far", two_level(1e9, 1e9))                     # (the hint rule's own 1e-9 (|c| + s) is a whole width here: no hints either)
    check_decisions(far, "1e9 widths from the origin")
    assert far["table"] > 0 and far["octants"]["covered"] == 0
    far = run_mesh(driver, "far8", two_level(1e8, 1e8))                    # 64 ulp are 1.4e-6 of a width, the hints' margin a tenth of one
    check_decisions(far, "1e8 widths from the origin")
    assert far["table"] > 0 and far["octants"]["hinted"] > 1000 and far["octants"]["covered"] == 0
    near = run_mesh(driver, "near", two_level(1e6, 1e6))                   # 1e6 widths: 64 ulp are 1.4e-8 of a width
    check_decisions(near, "1e6 widths from the origin")
    assert near["octants"]["interior_covered"] == near["octants"]["interior_hinted"] > 0


def test_log_mapped_axis_gets_no_table(driver):
    frame, _, _ = synth.config3(n_photons=16, nr=64, nth=32)
    got = run_mesh(driver, "log", frame_columns(frame))
    check_decisions(got, "log-r mesh")
    assert got["logmap"][0] == 1
    assert got["table"] == 0 and got["rule"] == 0 and got["octants"]["covered"] == 0 and got["octants"]["hinted"] > 0


def test_guard_threshold_rule_terms_size_rule_and_layout(driver):
    _, exe = driver
    rows = _rows(subprocess.run([exe, "-"], check=True, capture_output=True, text=True).stdout)
    guard, limit = rows["guard"]
    assert guard == 64 * np.finfo(np.float64).eps
    assert limit == pytest.approx(3.448e7, rel=1e-3)
    last_covered, first_uncovered = (int(v) for v in rows["threshold"])
    # cell k has |c| + s = k + 1.5: covered up to the limit, not beyond (the comparison's own roundings move it by less than a cell: 1e-8 of 0.5e-6
    # is 64 ulp of 3.4e7 x 2e-9)
    assert first_uncovered == last_covered + 1
    assert abs((last_covered + 1.5) - limit) <= 1.0
    # the cell on its bucket; its face 1e-6 inside the quadrant; 0.4e-6 inside; a cell 60 buckets wide; 49 wide; a NaN centre; a log-mapped axis;
    # the bucket's last quadrant (all four lie in [10, 11] x [3, 4])
    assert rows["terms"] == [1, 0, 1, 0, 1, 0, 0, 1]
    cap = int(rows["sizes"][8])
    assert cap == 1 << 26
    assert rows["sizes"][:8] == [4000, 8000, 0, 0, cap, 0, cap, 0]
    # 4356 ints = 17 424 B -> 17 664 with the 256-B rule: the table first, everything else behind it as before
    old = rows["layout_old"]
    assert rows["layout_none"] == old and old[:3] == [0, 0, 17664]
    assert rows["layout"] == [0] + [v + 17664 for v in old[1:]]
    assert rows["index"] == [5 * 4 + 3, 5 * 8 + 7, ((1 << 27) - 1 >> 3) * 8]
