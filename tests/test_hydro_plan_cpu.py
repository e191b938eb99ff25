"""The host's rules for staging a hydro frame (mcrat_amd/csrc/hydro_plan.hpp) on the CPU: the bucket grid's plan, the one coarsening rule, the
host build of the cell-lookup grid -- the cross-check of grid_build.hip -- against the thing it accelerates, the lowest-index linear scan over ALL
cells (geometry.c:350-391), the two buffers' layouts, an ingest's slab and a PLUTO-Chombo frame's box table.  They are plain C++: a small driver
is compiled with g++; it reads the meshes written here, and what it writes and prints is compared with the rules restated in Python.  Integers
exactly, doubles for equality (the driver is built with -ffp-contract=off, and numpy's double arithmetic is IEEE as well).

write_inputs(directory) leaves driver.cpp and the meshes in a directory, for a build of the driver by hand (with a sanitizer, say):
    g++ -std=c++17 -ffp-contract=off -I mcrat_amd/csrc driver.cpp -o driver && ./driver <directory> <mesh names>"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_LIGHT = 2.99792458e10
NO_HINT = 15
BUCKET_MASK = (1 << 27) - 1
TWO, TWO_POINT_FIVE, THREE = 0, 1, 2
OK, NONE_FITS, ABANDONED = 0, 1, 2


# ------------------------------------------------------------------ meshes: (centres per axis, widths per axis), all cells listed
def _tensor(edges):
    """cells of a tensor-product mesh from per-axis edge arrays, axis 0 fastest"""
    ctr = [0.5 * (e[1:] + e[:-1]) for e in edges]
    wid = [e[1:] - e[:-1] for e in edges]
    C = np.meshgrid(*ctr, indexing="ij")
    W = np.meshgrid(*wid, indexing="ij")
    order = "F"
    return [c.ravel(order=order).copy() for c in C], [w.ravel(order=order).copy() for w in W]


def _uniform():
    return _tensor([np.linspace(0.0, 3.2e9, 33), np.linspace(1e11, 1.032e11, 33)])


def _logradial():
    return _tensor([np.geomspace(1e9, 1e12, 49), np.linspace(0.01, 0.5, 25)])


def _refined():
    """32 x 32 cells of width 1, the quarter [0, 16)^2 of the domain replaced by cells of width 1/2; coarse cells first"""
    c, s = _tensor([np.linspace(0.0, 32.0, 33), np.linspace(0.0, 32.0, 33)])
    keep = ~((c[0] < 16) & (c[1] < 16))
    fc, fs = _tensor([np.linspace(0.0, 16.0, 33), np.linspace(0.0, 16.0, 33)])
    return [np.concatenate([c[k][keep], fc[k]]) for k in range(2)], [np.concatenate([s[k][keep], fs[k]]) for k in range(2)]


def _permuted():
    c, s = _refined()
    perm = np.random.default_rng(20240607).permutation(c[0].size)
    return [a[perm] for a in c], [a[perm] for a in s]


def _gapped():
    """the uniform mesh without the band of rows 12 .. 15"""
    c, s = _uniform()
    row = np.arange(c[0].size) // 32
    keep = (row < 12) | (row > 15)
    return [a[keep] for a in c], [a[keep] for a in s]


def _cube():
    return _tensor([np.linspace(-4e8, 4e8, 9), np.linspace(0.0, 8e8, 9), np.linspace(1e9, 1.8e9, 9)])


def _ratio(r):
    """one row of cells along axis 0 whose widths are 1 and r (above 0): smax / smin == r"""
    w = np.array([1.0, r, 1.0, r, 1.0, 1.0, 1.0, 1.0])
    e = 10.0 + np.concatenate([[0.0], np.cumsum(w)])
    return _tensor([e, np.array([5.0, 6.0])])


def _sparse():
    """8 cells of width 1 spread over an extent of 1000: more buckets' worth of typical cells than min(4 M, 2^24)"""
    c0 = np.array([0.5, 100.5, 250.5, 400.5, 600.5, 800.5, 900.5, 999.5])
    return [c0, np.full(8, 0.5)], [np.ones(8), np.ones(8)]


MESHES = {"uniform": _uniform, "logradial": _logradial, "refined": _refined, "permuted": _permuted, "gapped": _gapped, "cube": _cube,
          "ratio4": lambda: _ratio(4.0), "ratio4plus": lambda: _ratio(4.0 + 2 ** -40), "sparse": _sparse}
LOOKUP_MESHES = ["uniform", "logradial", "refined", "permuted", "gapped", "cube"]


def _points(name, c, s):
    """interior points, points snapped to faces and corners, points in the gap, points outside the mesh"""
    rng = np.random.default_rng(sum(map(ord, name)))
    M, nax = c[0].size, len(c)
    pick = rng.integers(0, M, 3000)
    u = rng.random((nax, pick.size)) - 0.5
    snap = np.arange(pick.size) % 3 == 0
    u[:, snap] = np.sign(u[:, snap]) * 0.5                             # corners ...
    u[1, snap & (np.arange(pick.size) % 2 == 0)] = 0.123              # ... and faces
    pts = [c[k][pick] + u[k] * s[k][pick] for k in range(nax)]
    lo = [float((c[k] - 0.5 * s[k]).min()) for k in range(nax)]
    hi = [float((c[k] + 0.5 * s[k]).max()) for k in range(nax)]
    outside = [[hi[0] * 3.0, lo[0] * 0.5 if lo[0] > 0 else lo[0] - 1.0, 0.5 * (lo[0] + hi[0]), hi[0] + (hi[0] - lo[0]) * 1e-6],
               [hi[1] * 3.0, 0.5 * (lo[1] + hi[1]), lo[1] - (hi[1] - lo[1]), 0.5 * (lo[1] + hi[1])]]
    if nax == 3:
        outside.append([0.5 * (lo[2] + hi[2])] * 4)
    n_gap = 0
    if name == "gapped":                                               # rows 12 .. 15 of 32 are missing: the open band between their neighbours' faces
        n_gap = 200
        y0, y1 = 1e11 + 12 * 1e8, 1e11 + 16 * 1e8
        gap = [lo[0] + rng.random(n_gap) * (hi[0] - lo[0]), y0 + (0.001 + 0.998 * rng.random(n_gap)) * (y1 - y0)]
        pts = [np.concatenate([pts[k], gap[k]]) for k in range(2)]
    pts = [np.concatenate([pts[k], outside[k]]) for k in range(nax)]
    return pts, pick, snap, n_gap


def _mesh(name):
    c, s = MESHES[name]()
    if name in LOOKUP_MESHES:
        pts, pick, snap, n_gap = _points(name, c, s)
    else:
        pts, pick, snap, n_gap = [np.zeros(0) for _ in c], np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), 0
    return dict(c=c, s=s, pts=pts, pick=pick, snap=snap, n_gap=n_gap, M=c[0].size, naxes=len(c))


# ------------------------------------------------------------------ the PLUTO-Chombo trees: levels as (dict of attributes, boxes, offsets)
NV = 6
NAMES = ["rho", "vx1", "vx2", "vx3", "prs", "tr1"]


def _level(prob_domain, boxes, nd, dx, logr=0, ref_ratio=2, dombeg=(1.5, 0.25, -2.0), stretch=(1.25, 0.75), gap=0):
    """boxes laid out one after another in the level's data (gap: doubles left unused behind the last box)"""
    offs, off = [], 0
    for b in boxes:
        offs.append(off)
        off += NV * int(np.prod([b[nd + a] - b[a] + 1 for a in range(nd)]))
    return dict(prob_domain=list(prob_domain), boxes=[list(b) for b in boxes], offsets=offs, data_len=off + gap, logr=logr, ref_ratio=ref_ratio, dx=dx,
                dombeg=dombeg, stretch=stretch)


def _tree2d():
    return [_level((0, 0, 15, 7), [(0, 0, 7, 7), (8, 0, 15, 7)], 2, 0.5, logr=0),
            _level((0, 0, 31, 15), [(4, 2, 11, 9), (12, 2, 15, 5)], 2, 0.25, logr=1)]


def _tree3d():
    return [_level((0, 0, 0, 7, 7, 3), [(0, 0, 0, 7, 7, 3)], 3, 0.125, logr=1),
            _level((0, 0, 0, 15, 15, 7), [(2, 2, 0, 5, 5, 3), (6, 2, 0, 9, 5, 3)], 3, 0.0625, logr=0)]


def _bad(kind):
    t = _tree2d()
    if kind == "box_outside":
        t[1]["boxes"][1] = [28, 2, 32, 5]                              # hi_i = 32 is past prob_domain's 31
    elif kind == "data_outside":
        t[1]["data_len"] -= 1
    elif kind == "out_of_order":
        t[0]["offsets"] = t[0]["offsets"][::-1]                        # two boxes of one size, the second one's data first
    return t


# name: (dimensions, tree, variable names)
CHOMBO = {
    "2d": (TWO, _tree2d(), NAMES),
    "3d": (THREE, _tree3d(), NAMES),
    "box_outside": (TWO, _bad("box_outside"), NAMES),
    "data_outside": (TWO, _bad("data_outside"), NAMES),
    "out_of_order": (TWO, _bad("out_of_order"), NAMES),
    "no_prs": (TWO, _tree2d(), ["rho", "vx1", "vx2", "vx3", "p", "tr1"]),
    "no_vx3_2d": (TWO, _tree2d(), ["rho", "vx1", "vx2", "bx3", "prs", "tr1"]),
    "no_vx3_25d": (TWO_POINT_FIVE, _tree2d(), ["rho", "vx1", "vx2", "bx3", "prs", "tr1"]),
    "no_vx3_3d": (THREE, _tree3d(), ["rho", "vx1", "vx2", "bx3", "prs", "tr1"]),
    "no_boxes": (TWO, [_level((0, 0, 15, 7), [], 2, 0.5)], NAMES),                               # refused without a text
    "bad_ref_ratio": (TWO, [_level((0, 0, 15, 7), [(0, 0, 7, 7)], 2, 0.5, ref_ratio=0)], NAMES),  # refused without a text
}
CHOMBO_TEXTS = {
    "box_outside": "PLUTO-Chombo ingest: a box lies outside its level's prob_domain",
    "data_outside": "PLUTO-Chombo ingest: a box's data lies outside its level's data",
    "out_of_order": "PLUTO-Chombo ingest: box data do not follow one another in data:offsets order",
    "no_prs": "PLUTO-Chombo ingest: a component (rho, vx1, vx2, [vx3], prs) is missing",
    "no_vx3_25d": "PLUTO-Chombo ingest: a component (rho, vx1, vx2, [vx3], prs) is missing",
    "no_vx3_3d": "PLUTO-Chombo ingest: a component (rho, vx1, vx2, [vx3], prs) is missing",
    "no_boxes": "", "bad_ref_ratio": "",
}

# r_inj, ph_inj_switch, min_r, max_r, min_theta, max_theta, fps, elem_factor, dimensions, geometry
SLABS = [(1e12, 0, 9e11, 1.1e12, 0.05, 0.2, 5.0, 1, 0, 2), (1e12, 0, 9e11, 1.1e12, 0.05, 0.2, 5.0, 7, 2, 1), (3e11, 0, 1e11, 2e11, 0.0, 0.01, 0.5, 3, 1, 1),
         (1e12, 1, 9e11, 1.1e12, 0.05, 0.2, 5.0, 4, 0, 2)]
# ncell0, ncell1, f0, M, the attempt (from 0) at which the lists fit -- -1: never, -2: the count cannot be made
COARSEN = {"first": (32.0, 32.0, 1.0, 1024, 0), "fourth": (300.0, 20.0, 0.7, 500, 3), "last": (4000.0, 4000.0, 1.0, 100, 11), "never": (4000.0, 4000.0, 1.0, 100, -1),
           "too_many_buckets": (65536.0, 65536.0, 1.0, 1 << 25, 0), "abandoned": (32.0, 32.0, 1.0, 1024, -2)}
# name: naxes, M, (lo, hi, smin, smax) per axis -- one sample per axis, the cell [lo, hi]
STATS = {"fine": (2, 10, [(1.0, 2.0, 0.1, 0.1), (0.0, 1.0, 0.1, 0.2)]), "no_extent": (2, 10, [(1.0, 1.0, 0.1, 0.1), (0.0, 1.0, 0.1, 0.2)]),
         "backwards": (2, 10, [(1.0, 2.0, 0.1, 0.1), (1.0, 0.5, 0.1, 0.2)]), "zero_width": (2, 10, [(1.0, 2.0, 0.0, 0.1), (0.0, 1.0, 0.1, 0.2)]),
         "nan_width": (2, 10, [(1.0, 2.0, float("nan"), 0.1), (0.0, 1.0, 0.1, 0.2)]), "nan_extent": (2, 10, [(1.0, float("nan"), 0.1, 0.1), (0.0, 1.0, 0.1, 0.2)])}
# name: M, typical cells across axis 0 and axis 1 -- which side of min(4 M, 2^24) decides f0
TARGETS = {"four_per_cell": (1 << 21, 8192.0, 8192.0), "two_to_the_24": (1 << 23, 8192.0, 8192.0), "at_two_to_the_24": (1 << 23, 4096.0, 4096.0),
           "just_over_two_to_the_24": (1 << 23, 4096.0, 4097.0)}

DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "hydro_plan.hpp"
using namespace mcrat;

template <class T> static std::vector<T> get(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }
template <class T> static void put(FILE *f, const std::vector<T> &v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2); }

// physics.hpp's closed-interval test (walk_bucket, geometry.c:394-417), restated
static bool holds(const double *const c[3], const double *const s[3], int naxes, int i, const double a[3])
{
    bool in = (2 * fabs(a[0] - c[0][i]) - s[0][i] <= 0) && (2 * fabs(a[1] - c[1][i]) - s[1][i] <= 0);
    if (naxes == 3) in = in && (2 * fabs(a[2] - c[2][i]) - s[2][i] <= 0);
    return in;
}
static void print_stats(const char *key, const MeshStats &ms, int naxes)
{
    printf("%s:", key);
    for (int k = 0; k < naxes; ++k) printf(" %.17g %.17g %.17g %.17g", ms.lo[k], ms.hi[k], ms.smin[k], ms.smax[k]);
    for (int k = 0; k < naxes; ++k) { printf(" %d", (int)ms.sc[k].size()); for (double v : ms.sc[k]) printf(" %.17g", v); for (double v : ms.ss[k]) printf(" %.17g", v); }
    printf("\n");
}
// stage_cells_kernel's part of the reduction for cells [i0, i1): the extremes of one workgroup
static StagePartial partial_of(const double *const c[3], const double *const s[3], int naxes, int i0, int i1)
{
    StagePartial p{};
    for (int k = 0; k < naxes; ++k) {
        p.lo[k] = INFINITY; p.hi[k] = -INFINITY; p.smin[k] = INFINITY; p.smax[k] = 0;
        for (int i = i0; i < i1; ++i) {
            p.lo[k] = std::min(p.lo[k], c[k][i] - 0.5 * s[k][i]); p.hi[k] = std::max(p.hi[k], c[k][i] + 0.5 * s[k][i]);
            p.smin[k] = (s[k][i] < p.smin[k] || !(s[k][i] == s[k][i])) ? s[k][i] : p.smin[k];
            p.smax[k] = std::max(p.smax[k], s[k][i]);
        }
    }
    return p;
}
static void mesh(const std::string &dir, const std::string &name)
{
    FILE *f = fopen((dir + "/" + name + ".in").c_str(), "rb");
    if (!f) { fprintf(stderr, "no mesh %s\n", name.c_str()); exit(2); }
    const std::vector<int> head = get<int>(f, 4);
    const int M = head[0], naxes = head[1], np = head[2], nan_cell = head[3];
    std::vector<double> col[6], pt[3];
    for (int k = 0; k < 2 * naxes; ++k) col[k] = get<double>(f, M);
    for (int k = 0; k < naxes; ++k) pt[k] = get<double>(f, np);
    fclose(f);
    const double *c[3] = {col[0].data(), col[2].data(), naxes == 3 ? col[4].data() : nullptr};
    const double *s[3] = {col[1].data(), col[3].data(), naxes == 3 ? col[5].data() : nullptr};
    const char *n = name.c_str();

    const MeshStats ms = mesh_stats_from_columns(c, s, M, naxes);
    print_stats(("stats_columns_" + name).c_str(), ms, naxes);
    {   // the same mesh as several partials (of 100 cells) and the sample block
        std::vector<StagePartial> part;
        for (int i0 = 0; i0 < M; i0 += 100) part.push_back(partial_of(c, s, naxes, i0, std::min(M, i0 + 100)));
        part[part.size() / 2].any_hot = 1;
        const int stride = plan_stride(M), nsamp = (M + stride - 1) / stride;
        std::vector<double> samp((size_t)2 * naxes * nsamp);
        for (int k = 0; k < naxes; ++k)
            for (int j = 0; j < nsamp; ++j) { samp[(size_t)(2 * k) * nsamp + j] = c[k][j * stride]; samp[(size_t)(2 * k + 1) * nsamp + j] = s[k][j * stride]; }
        bool hot = false;
        const MeshStats mp = mesh_stats_from_partials(part.data(), (int)part.size(), samp.data(), nsamp, naxes, &hot);
        print_stats(("stats_partials_" + name).c_str(), mp, naxes);
        GridScale sc;
        printf("partials_%s: %d %d %d\n", n, (int)part.size(), (int)hot, (int)grid_plan_from_stats(mp, M, naxes, sc));
    }
    if (nan_cell >= 0) return;                                 // (a mesh with a NaN width: the statistics are what it is for)
    GridScale sc;
    const bool planned = grid_plan_from_stats(ms, M, naxes, sc);
    printf("scale_%s: %d %d %d %d %d %.17g", n, (int)planned, sc.naxes, sc.logmap[0], sc.logmap[1], sc.logmap[2], sc.f0);
    for (int k = 0; k < 3; ++k) printf(" %.17g %.17g %.17g", sc.ext_lo[k], sc.ext_hi[k], sc.ncell[k]);
    printf("\n");

    GridHost g;
    const bool ok = build_grid(c, s, M, naxes, g);
    printf("grid_%s: %d %lld %lld %d %d %d %d %d %d %d", n, (int)ok, g.nb, (long long)g.cells.size(), g.plan.naxes, g.plan.dim[0], g.plan.dim[1], g.plan.dim[2],
           g.plan.logmap[0], g.plan.logmap[1], g.plan.logmap[2]);
    for (int k = 0; k < 3; ++k) printf(" %.17g %.17g", g.plan.org[k], g.plan.inv[k]);
    printf("\n");
    if (!ok) return;
    GridDev dev{};
    grid_plan_to_dev(g.plan, dev);
    printf("dev_%s: %d %d %d %d %d %d %d", n, dev.naxes, dev.dim[0], dev.dim[1], dev.dim[2], dev.logmap[0], dev.logmap[1], dev.logmap[2]);
    for (int k = 0; k < 3; ++k) printf(" %.17g %.17g", dev.org[k], dev.inv[k]);
    printf("\n");
    // every point through its bucket's list: the first entry whose closed extent holds it
    std::vector<int> found(np, -1);
    for (int q = 0; q < np; ++q) {
        const double a[3] = {pt[0][q], pt[1][q], naxes == 3 ? pt[2][q] : 0.0};
        long long b = 0;
        for (int k = naxes - 1; k >= 0; --k) b = b * g.plan.dim[k] + bucket_of(a[k], g.plan.logmap[k], g.plan.org[k], g.plan.inv[k], g.plan.dim[k]);
        for (int e = g.start[(size_t)b]; e < g.start[(size_t)b + 1] && found[q] < 0; ++e)
            if (holds(c, s, naxes, g.cells[(size_t)e], a)) found[q] = g.cells[(size_t)e];
    }
    FILE *o = fopen((dir + "/" + name + ".out").c_str(), "wb");
    if (!o) exit(2);
    put(o, g.start); put(o, g.cells); put(o, g.hints); put(o, found);
    fclose(o);
}

static void coarsen(const char *name, double n0, double n1, double f0, int M, int fits_at)
{
    GridScale sc;
    sc.naxes = 2; sc.ext_hi[0] = n0; sc.ext_hi[1] = n1; sc.ncell[0] = n0; sc.ncell[1] = n1; sc.f0 = f0;
    int calls = 0;
    std::vector<long long> seen;
    const GridChoice ch = choose_grid_scale(sc, M, [&](const GridPlan &p, long long nb, long long limit) -> long long {
        seen.push_back(nb); seen.push_back(p.dim[0]); seen.push_back(limit);
        if (fits_at == -2) return -1;
        return calls++ == fits_at ? limit : limit + 1;
    });
    printf("coarsen_%s: %d %lld %lld %d %d", name, (int)ch.result, ch.nb, ch.entries, ch.plan.dim[0], ch.plan.dim[1]);
    for (long long v : seen) printf(" %lld", v);
    printf("\n");
}
static void stats_plan(const char *name, int naxes, int M, const double (*q)[4])
{
    MeshStats ms{};
    for (int k = 0; k < naxes; ++k) {
        ms.lo[k] = q[k][0]; ms.hi[k] = q[k][1]; ms.smin[k] = q[k][2]; ms.smax[k] = q[k][3];
        ms.sc[k].push_back(0.5 * (q[k][0] + q[k][1])); ms.ss[k].push_back(q[k][1] - q[k][0]);
    }
    GridScale sc;
    printf("statsplan_%s: %d\n", name, (int)grid_plan_from_stats(ms, M, naxes, sc));
}
// a mesh of M cells whose typical cell is 1 wide on two axes n0 and n1 long: the scale factor to start from
static void target(const char *name, int M, double n0, double n1)
{
    const double n[2] = {n0, n1};
    MeshStats ms{};
    for (int k = 0; k < 2; ++k) { ms.lo[k] = 0; ms.hi[k] = n[k]; ms.smin[k] = ms.smax[k] = 1; ms.sc[k].push_back(0.5); ms.ss[k].push_back(1.0); }
    GridScale sc;
    const bool ok = grid_plan_from_stats(ms, M, 2, sc);
    printf("target_%s: %d %.17g %.17g %.17g\n", name, (int)ok, sc.ncell[0], sc.ncell[1], sc.f0);
}
static void slab(int k, double r_inj, int sw, double min_r, double max_r, double min_t, double max_t, double fps, int elem_factor, int dims, int geom)
{
    mcrat_hip_slab s{};
    s.r_inj = r_inj; s.ph_inj_switch = sw; s.min_r = min_r; s.max_r = max_r; s.min_theta = min_t; s.max_theta = max_t; s.fps = fps;
    const SlabDev d = slab_for(dims, geom, &s, elem_factor);
    printf("slab_%d: %d %d %d %.17g %.17g %.17g %.17g %.17g\n", k, d.dimensions, d.geometry, d.ph_inj_switch, d.r_inj_095, d.r_lo, d.r_hi, d.th_lo, d.th_hi);
}
struct Lvl { std::vector<int> boxes, offsets; long long data_len; int pd[6], ref_ratio, logr; double dx, b1, b2, b3, s2, s3; };
static void chombo(const char *name, int dims, const std::vector<Lvl> &lv, const std::vector<const char *> &names)
{
    const int nd = dims == DIM_THREE ? 3 : 2;
    std::vector<mcrat_hip_chombo_level> L(lv.size());
    for (size_t i = 0; i < lv.size(); ++i) {
        L[i] = mcrat_hip_chombo_level{};
        L[i].n_boxes = (int)lv[i].offsets.size(); L[i].boxes = lv[i].boxes.data(); L[i].box_offsets = lv[i].offsets.data(); L[i].data_len = lv[i].data_len;
        for (int a = 0; a < 2 * nd; ++a) L[i].prob_domain[a] = lv[i].pd[a];
        L[i].ref_ratio = lv[i].ref_ratio; L[i].logr = lv[i].logr; L[i].dx = lv[i].dx; L[i].dombeg1 = lv[i].b1; L[i].dombeg2 = lv[i].b2; L[i].dombeg3 = lv[i].b3;
        L[i].g_x2stretch = lv[i].s2; L[i].g_x3stretch = lv[i].s3;
    }
    const double nothing = 0;
    mcrat_hip_chombo h{};
    h.num_levels = (int)L.size(); h.num_vars = (int)names.size(); h.levels = L.data(); h.var_names = names.data(); h.data = &nothing;
    ChomboPlan p;
    const char *why = chombo_plan(&h, dims, p);
    printf("chombo_%s:%s\n", name, why ? why : "planned");
    if (why) return;
    printf("chombov_%s: %lld %lld %d %d %d %d %d %d", name, p.total, p.cells, p.kv[0], p.kv[1], p.kv[2], p.kv[3], p.kv[4], (int)p.boxes.size());
    for (int v : p.level_first_box) printf(" %d", v);
    printf("\n");
    for (size_t j = 0; j < p.boxes.size(); ++j) {
        const ChomboBox &b = p.boxes[j];
        printf("chombobox_%s_%d: %lld %lld %d %d %d %d %d %d %d %d %d %d\n", name, (int)j, b.first_cell, b.data_off, b.level, b.lo[0], b.lo[1], b.lo[2], b.n[0], b.n[1], b.n[2],
               b.cb[0], b.cb[1], b.cb[2]);
    }
    for (int a = 0; a < 3; ++a) {
        printf("chombox_%s_%d:", name, a);
        for (double v : p.xs[a]) printf(" %.17g", v);
        for (double v : p.dxs[a]) printf(" %.17g", v);
        printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    for (int k = 2; k < argc; ++k) mesh(argv[1], argv[k]);
@CASES@
    for (int dims = 0; dims < 3; ++dims)
        for (int k2e = 0; k2e < 2; ++k2e) {
            const CellLayout l = cell_layout(dims, 1000, k2e != 0);
            printf("cells_%d_%d: %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", dims, k2e, l.geom, l.geom2, l.fluid, l.temp, l.fluid_c, l.k2e, l.gamma, l.total, (int)l.has_geom2,
                   (int)l.has_fluid_c, (int)l.has_k2e);
        }
    const GridLayout gl = grid_layout(1089, 4096, 7), g0 = grid_layout(4, 0, 1);
    printf("gridlayout: %zu %zu %zu %zu %zu %zu\n", gl.dir, gl.cells, gl.start, gl.scan, gl.entries, gl.total);
    printf("gridlayout_empty: %zu %zu %zu %zu %zu %zu\n", g0.dir, g0.cells, g0.start, g0.scan, g0.entries, g0.total);
    printf("sizes: %zu %zu %zu %zu %zu\n", sizeof(CellGeom), sizeof(CellGeom2), sizeof(CellFluid), sizeof(BucketDir), sizeof(FatCell));
    {
        mcrat_hip_slab s{};
        s.fps = 5.0;
        mcrat_hip_outflow o{};
        int okv[8];
        okv[0] = slab_ok(&s); s.ph_inj_switch = 1; okv[1] = slab_ok(&s); s.ph_inj_switch = 2; okv[2] = slab_ok(&s); s.ph_inj_switch = 0; s.fps = 0; okv[3] = slab_ok(&s);
        okv[4] = slab_ok(nullptr); okv[5] = outflow_ok(nullptr); o.simulation_type = 3; okv[6] = outflow_ok(&o); o.simulation_type = 4; okv[7] = outflow_ok(&o);
        printf("oks: %d %d %d %d %d %d %d %d\n", okv[0], okv[1], okv[2], okv[3], okv[4], okv[5], okv[6], okv[7]);
    }
    {   // the staged velocity and a bucket-list entry
        const double v0 = 0.3, v1 = -0.2, v2 = 0.1, x1 = 0.7, x2 = 2.1;
        const int pairs[7][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {2, 0}, {2, 1}, {2, 3}};
        for (const auto &pr : pairs) {
            double o[3];
            cell_velocity_staged(pr[0], pr[1], v0, v1, pr[0] == 0 ? 0.0 : v2, x1, x2, o);
            printf("velocity_%d_%d: %.17g %.17g %.17g\n", pr[0], pr[1], o[0], o[1], o[2]);
        }
        CellGeom cg{1.0, 2.0, 3.0, 4.0};
        CellFluid cf{};
        cell_staged_operands(0.1, 0.2, 0.3, 1.5, 1e-3, cf);
        const FatCell fc = fat_cell(cg, cf, 5.0, 6.0, 77);
        printf("fat: %d %d %d %d %d\n", (int)(fc.c0 == 1.0 && fc.c1 == 2.0 && fc.s0 == 3.0 && fc.s1 == 4.0), (int)(fc.a == cf.a && fc.b == cf.b && fc.c == cf.c && fc.w == cf.w),
               (int)(fc.nsig == cf.nsig && fc.gam == cf.gam), (int)(fc.c2 == 5.0 && fc.s2 == 6.0), fc.cell);
    }
    return 0;
}
'''


def _d(x):
    if isinstance(x, float) and math.isnan(x):
        return "NAN"
    return "%d" % x if isinstance(x, int) else "%r" % x


def _cases():
    lines = []
    for name, (n0, n1, f0, M, fits_at) in COARSEN.items():
        lines.append('coarsen("%s", %r, %r, %r, %d, %d);' % (name, n0, n1, f0, M, fits_at))
    for name, (naxes, M, q) in STATS.items():
        lines.append('{ const double q[2][4] = {%s}; stats_plan("%s", %d, %d, q); }' % (", ".join("{%s}" % ", ".join(_d(v) for v in row) for row in q), name, naxes, M))
    for name, (M, n0, n1) in TARGETS.items():
        lines.append('target("%s", %d, %r, %r);' % (name, M, n0, n1))
    for k, sl in enumerate(SLABS):
        lines.append("slab(%d, %s);" % (k, ", ".join(_d(v) for v in sl)))
    for name, (dims, tree, names) in CHOMBO.items():
        lv = []
        for L in tree:
            pd = L["prob_domain"] + [0] * (6 - len(L["prob_domain"]))
            lv.append("Lvl{{%s}, {%s}, %d, {%s}, %d, %d, %r, %r, %r, %r, %r, %r}" % (
                ", ".join(str(v) for b in L["boxes"] for v in b), ", ".join(str(v) for v in L["offsets"]), L["data_len"], ", ".join(map(str, pd)), L["ref_ratio"],
                L["logr"], L["dx"], L["dombeg"][0], L["dombeg"][1], L["dombeg"][2], L["stretch"][0], L["stretch"][1]))
        lines.append('chombo("%s", %d, {%s}, {%s});' % (name, dims, ", ".join(lv), ", ".join('"%s"' % v for v in names)))
    return "\n".join("    " + l for l in lines)


_cache = {}


def meshes():
    if not _cache:
        for name in MESHES:
            _cache[name] = _mesh(name)
        nan = _mesh("uniform")                                         # the uniform mesh with one NaN width, for the statistics alone
        nan["s"] = [a.copy() for a in nan["s"]]
        nan["s"][0][517] = float("nan")
        nan["nan_cell"] = 517
        _cache["nanwidth"] = nan
    return _cache


def write_inputs(directory):
    """driver.cpp and every mesh's input file; returns the mesh names in the order the driver is to be given them"""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "driver.cpp"), "w") as f:
        f.write(DRIVER.replace("@CASES@", _cases()))
    for name, m in meshes().items():
        with open(os.path.join(directory, name + ".in"), "wb") as f:
            np.array([m["M"], m["naxes"], m["pts"][0].size, m.get("nan_cell", -1)], dtype=np.int32).tofile(f)
            for k in range(m["naxes"]):
                m["c"][k].astype(np.float64).tofile(f)
                m["s"][k].astype(np.float64).tofile(f)
            for k in range(m["naxes"]):
                m["pts"][k].astype(np.float64).tofile(f)
    return list(meshes())


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    """what the driver printed: {key: [numbers]}, the texts as strings; and per mesh what it wrote: start, cells, hints, found"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = str(tmp_path_factory.mktemp("hydro_plan"))
    names = write_inputs(d)
    exe = os.path.join(d, "driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), os.path.join(d, "driver.cpp"),
                    "-o", exe], check=True)
    text = subprocess.run([exe, d] + names, check=True, capture_output=True, text=True).stdout
    res = {}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        res[key] = vals if key.startswith("chombo_") else [float(v) if any(ch in v for ch in ".naife") else int(v) for v in vals.split()]
    for name in names:
        g = res.get("grid_" + name)
        if not g or not g[0]:
            continue
        nb, total, npts = g[1], g[2], meshes()[name]["pts"][0].size
        with open(os.path.join(d, name + ".out"), "rb") as f:
            res["arrays_" + name] = (np.fromfile(f, np.int32, nb + 1), np.fromfile(f, np.int32, total), np.fromfile(f, np.uint32, nb), np.fromfile(f, np.int32, npts))
    return res


def same(got, want):
    """integers exactly, doubles for equality -- NaN where a NaN is due -- and of the same kind (an int where an int is due)"""
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        if isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), (got, want)
        else:
            assert float(g) == float(w) and (isinstance(w, float) or isinstance(g, int)), (got, want)


# ------------------------------------------------------------------ the rules, restated
def stats_rule(c, s):
    """extent, smallest and largest width per axis, NaN passed over; then the samples (every cell: these meshes are below 8192 cells)"""
    q = []
    for k in range(len(c)):
        q += [float(np.nanmin(c[k] - 0.5 * s[k])), float(np.nanmax(c[k] + 0.5 * s[k])), float(np.nanmin(s[k])), float(np.nanmax(s[k]))]
    for k in range(len(c)):
        q += [c[k].size] + [float(v) for v in c[k]] + [float(v) for v in s[k]]
    return q


def scale_rule(c, s):
    """grid_plan_from_stats: logmap, mapped extent, cells across (extent over the lower-quartile width), f0"""
    M, nax = c[0].size, len(c)
    logmap, lo_, hi_, ncell = [0, 0, 0], [0.0] * 3, [0.0] * 3, [1.0] * 3
    for k in range(nax):
        lo, hi, smin, smax = float((c[k] - 0.5 * s[k]).min()), float((c[k] + 0.5 * s[k]).max()), float(s[k].min()), float(s[k].max())
        logmap[k] = 1 if (lo > 0 and smax / smin > 4.0) else 0
        a, b = c[k] - 0.5 * s[k], c[k] + 0.5 * s[k]
        w = np.array([math.log(y) - math.log(max(x, 1e-300)) for x, y in zip(a, b)]) if logmap[k] else b - a
        med = float(np.sort(w)[w.size // 4])
        lo_[k], hi_[k] = (math.log(lo), math.log(hi)) if logmap[k] else (lo, hi)
        ncell[k] = max(1.0, (hi_[k] - lo_[k]) / med)
    prod = 1.0
    for k in range(nax):
        prod *= ncell[k]
    target = min(max(4.0 * M, 1.0), 16777216.0)
    f0 = math.pow(target / prod, 1.0 / nax) if prod > target else 1.0
    return logmap, lo_, hi_, ncell, f0


def dims_rule(nax, lo_, hi_, ncell, f):
    dim, org, inv = [1, 1, 1], [0.0] * 3, [0.0] * 3
    for k in range(nax):
        nbk = int(max(1.0, min(65536.0, math.floor(ncell[k] * f))))
        width = (hi_[k] - lo_[k]) / nbk
        dim[k], org[k], inv[k] = nbk + 1, lo_[k] - 0.5 * width, 1.0 / width
    return dim, org, inv


def _map(x, logmap):
    return np.log(np.maximum(x, 1e-300)) if logmap else x


def bucket_rule(x, logmap, org, inv, dim):
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.floor(((np.log(x) if logmap else x) - org) * inv)
    return np.where(np.isnan(f), 0, np.clip(f, 0, dim - 1)).astype(np.int64)


def linear_scan(c, s, pts):
    inside = np.ones((pts[0].size, c[0].size), dtype=bool)
    for k in range(len(c)):
        inside &= 2 * np.abs(pts[k][:, None] - c[k][None, :]) - s[k][None, :] <= 0
    return np.where(inside.any(axis=1), inside.argmax(axis=1), -1)


def grid_of(out, name):
    g = out["grid_" + name]
    assert g[0] == 1, name
    return dict(nb=g[1], total=g[2], naxes=g[3], dim=g[4:7], logmap=g[7:10], org=g[10::2], inv=g[11::2])


# ------------------------------------------------------------------ build_grid against the linear scan
@pytest.mark.parametrize("name", LOOKUP_MESHES)
def test_bucket_lists_hold_exactly_the_cells_that_touch_the_bucket(out, name):
    m, g = meshes()[name], grid_of(out, name)
    start, cells, _, _ = out["arrays_" + name]
    nax, dim = m["naxes"], g["dim"]
    assert start[0] == 0 and start[-1] == g["total"] == cells.size and np.all(np.diff(start) >= 0) and g["nb"] == dim[0] * dim[1] * dim[2]
    assert g["total"] <= 64 * m["M"] + 1024 and g["nb"] <= BUCKET_MASK
    bucket = np.repeat(np.arange(g["nb"]), np.diff(start))
    inner = np.ones(cells.size, dtype=bool)
    inner[start[:-1][np.diff(start) > 0]] = False                                  # the first entry of every list
    assert np.all(np.diff(cells)[inner[1:]] > 0)                                     # every list ascends
    # the buckets every cell's widened extent touches, by the rule: a box of buckets per cell
    rng = []
    for k in range(nax):
        c, s = m["c"][k], m["s"][k]
        marg = 1e-9 * (np.abs(c) + s)
        a, b = c - 0.5 * s - marg, c + 0.5 * s + marg
        if g["logmap"][k]:
            a = np.where(a <= 0, 1e-300, a)
        rng.append((bucket_rule(a, g["logmap"][k], g["org"][k], g["inv"][k], dim[k]), bucket_rule(b, g["logmap"][k], g["org"][k], g["inv"][k], dim[k])))
    want = set()
    for i in range(m["M"]):
        ax = [range(rng[k][0][i], rng[k][1][i] + 1) for k in range(nax)] + [range(1)] * (3 - nax)
        want.update(((z * dim[1] + y) * dim[0] + x, i) for z in ax[2] for y in ax[1] for x in ax[0])
    got = set(zip(bucket.tolist(), cells.tolist()))
    assert len(got) == cells.size and got == want


@pytest.mark.parametrize("name", LOOKUP_MESHES)
def test_first_hit_of_the_bucket_list_is_the_lowest_index_linear_scan(out, name):
    m = meshes()[name]
    found = out["arrays_" + name][3]
    want = linear_scan(m["c"], m["s"], m["pts"])
    assert np.array_equal(found, want)
    n, snap, pick = m["pick"].size, m["snap"], m["pick"]
    assert n >= 3000 and np.array_equal(want[:n][~snap], pick[~snap])              # interior points: the cell they were drawn in
    assert (want[:n][snap] != pick[snap]).sum() > 10                                # face and corner points: a lower-index neighbour's
    assert np.all(want[n:] == -1) and want.size - n == m["n_gap"] + 4               # the gap and the outside
    if name in ("refined", "permuted"):                                             # points on the faces between the two levels are among them
        on_x = (m["pts"][0][:n] == 16.0) & (m["pts"][1][:n] < 16.0)
        assert on_x.sum() > 3


@pytest.mark.parametrize("name", LOOKUP_MESHES)
def test_octant_hints_name_the_only_cell_of_the_mesh_in_the_octant(out, name):
    m, g = meshes()[name], grid_of(out, name)
    start, cells, hints, _ = out["arrays_" + name]
    nax, dim, nocts = m["naxes"], g["dim"], 1 << m["naxes"]
    reach = []                                                                       # per axis [bucket, half, cell]: the shrunk extent reaches into the half's interior
    for k in range(nax):
        c, s = m["c"][k], m["s"][k]
        marg = 1e-9 * (np.abs(c) + s)
        clo, chi = _map(c - 0.5 * s + marg, g["logmap"][k]), _map(c + 0.5 * s - marg, g["logmap"][k])
        w = 1.0 / g["inv"][k]
        olo = g["org"][k] + (np.arange(dim[k])[:, None] + 0.5 * np.arange(2)[None, :]) * w
        ohi = olo + 0.5 * w
        reach.append((clo[None, None, :] < ohi[:, :, None]) & (chi[None, None, :] > olo[:, :, None]))
    hinted = single = 0
    for b in range(g["nb"]):
        bi = (b % dim[0], (b // dim[0]) % dim[1], b // (dim[0] * dim[1]))
        lst = cells[start[b]:start[b + 1]]
        for o in range(8):
            h = (int(hints[b]) >> (4 * o)) & 15
            if o >= nocts:
                assert h == NO_HINT
                continue
            r = np.ones(m["M"], dtype=bool)
            for k in range(nax):
                r &= reach[k][bi[k], (o >> k) & 1]
            who = np.flatnonzero(r)                                                  # over ALL cells, not the list's
            if h != NO_HINT:
                hinted += 1
                assert who.size == 1 and h < lst.size and lst[h] == who[0], (b, o)
            if who.size == 1:
                pos = np.flatnonzero(lst == who[0])
                assert pos.size == 1, (b, o)                                         # a cell that reaches into the bucket is in its list
                if pos[0] < NO_HINT:
                    single += 1
                    assert h == pos[0], (b, o)
    assert hinted == single > 0


# ------------------------------------------------------------------ the plan's rules
@pytest.mark.parametrize("name", sorted(MESHES))
def test_scale_and_plan_of_a_mesh(out, name):
    m = meshes()[name]
    logmap, lo_, hi_, ncell, f0 = scale_rule(m["c"], m["s"])
    sc = out["scale_" + name]
    assert sc[:5] == [1, m["naxes"]] + logmap
    same(sc[5:], [f0] + [v for k in range(3) for v in (lo_[k], hi_[k], ncell[k])])
    g = grid_of(out, name)
    # the plan is the one of f0 halved some number of times (the first that fits: the coarsening tests)
    plans = [dims_rule(m["naxes"], lo_, hi_, ncell, f0 * 0.5 ** a) for a in range(12)]
    match = [a for a, (dim, org, inv) in enumerate(plans) if dim == g["dim"]]
    assert match, name
    dim, org, inv = plans[match[0]]
    same(g["org"], org)
    same(g["inv"], inv)
    assert g["logmap"] == logmap and g["naxes"] == m["naxes"]
    assert out["dev_" + name] == [g["naxes"]] + g["dim"] + g["logmap"] + [v for k in range(3) for v in (g["org"][k], g["inv"][k])]
    if name in ("uniform", "cube", "logradial", "gapped"):
        assert match[0] == 0                                                         # buckets of one cell fit these


def test_the_log_map_switches_on_above_a_width_ratio_of_four(out):
    assert out["scale_ratio4"][2:5] == [0, 0, 0] and out["scale_ratio4plus"][2:5] == [1, 0, 0]
    assert out["scale_logradial"][2:5] == [1, 0, 0]                                   # radius ratio 1000: on in r, off in theta
    assert out["scale_uniform"][2:5] == [0, 0, 0] and out["scale_cube"][2:5] == [0, 0, 0]     # (the cube's first axis starts below 0, too)


def test_buckets_of_one_cell_shifted_by_half_a_bucket(out):
    g = grid_of(out, "uniform")
    assert g["dim"] == [33, 33, 1] and g["nb"] == 1089                                # dim = nbk + 1
    same(g["org"], [0.0 - 0.5 * (3.2e9 / 32), 1e11 - 0.5 * ((1.032e11 - 1e11) / 32), 0.0])
    same(g["inv"], [1.0 / (3.2e9 / 32), 1.0 / ((1.032e11 - 1e11) / 32), 0.0])
    assert g["total"] == 4 * 1024                                                     # every cell straddles two buckets per axis
    assert grid_of(out, "cube")["dim"] == [9, 9, 9] and grid_of(out, "cube")["total"] == 8 * 512
    assert grid_of(out, "refined")["dim"] == [65, 65, 1]                              # the lower-quartile width is the fine cells'


def test_bucket_count_is_capped_at_four_per_cell(out):
    sc = out["scale_sparse"]
    ncell = sc[8::3]
    assert ncell[0] == 1000.0 and ncell[1] == 1.0
    assert sc[5] == math.pow(32.0 / 1000.0, 0.5) < 1.0                                # f0 brings 1000 x 1 typical cells down to 4 M = 32
    assert grid_of(out, "sparse")["dim"][0] <= int(1000.0 * sc[5]) + 1
    assert out["scale_uniform"][5] == 1.0                                              # 1024 typical cells for 1024 cells: no cap


def test_bucket_count_is_capped_at_two_to_the_24(out):
    """the other side of min(4 M, 2^24): with 2^23 cells, 4 M = 2^25 is NOT what the 2^26 typical cells are brought down to"""
    same(out["target_four_per_cell"], [1, 8192.0, 8192.0, math.pow(2.0 ** 23 / 2.0 ** 26, 0.5)])           # 4 M = 2^23 binds
    same(out["target_two_to_the_24"], [1, 8192.0, 8192.0, math.pow(2.0 ** 24 / 2.0 ** 26, 0.5)])           # 2^24 binds ...
    assert out["target_two_to_the_24"][3] == 0.5 != math.pow(2.0 ** 25 / 2.0 ** 26, 0.5)                  # ... not 4 M
    same(out["target_at_two_to_the_24"], [1, 4096.0, 4096.0, 1.0])                                        # exactly 2^24: no cap
    same(out["target_just_over_two_to_the_24"], [1, 4096.0, 4097.0, math.pow(16777216.0 / (4096.0 * 4097.0), 0.5)])
    assert out["target_just_over_two_to_the_24"][3] < 1.0


def test_a_degenerate_mesh_is_refused(out):
    want = {"fine": 1, "no_extent": 0, "backwards": 0, "zero_width": 0, "nan_width": 0, "nan_extent": 0}
    for name, ok in want.items():
        assert out["statsplan_" + name] == [ok], name


@pytest.mark.parametrize("name", sorted(COARSEN))
def test_the_coarsening_rule(out, name):
    n0, n1, f0, M, fits_at = COARSEN[name]
    limit = min(64 * M + 1024, 2000000000)
    got = out["coarsen_" + name]
    calls, seen, f = 0, [], f0
    want = [NONE_FITS]
    for attempt in range(12):
        dim = [int(max(1.0, min(65536.0, math.floor(n * f)))) + 1 for n in (n0, n1)]
        nb = dim[0] * dim[1]
        f *= 0.5
        if nb > BUCKET_MASK:
            continue
        seen += [nb, dim[0], limit]
        if fits_at == -2:
            want = [ABANDONED]
            break
        calls += 1
        if calls - 1 == fits_at:
            want = [OK, nb, limit, dim[0], dim[1]]
            break
    assert got[0] == want[0] and got[5:] == seen
    if want[0] == OK:
        assert got[:5] == want


def test_the_coarsening_cases_are_what_they_are_meant_to_be(out):
    c = lambda name: out["coarsen_" + name]
    assert c("first")[:5] == [OK, 33 * 33, 64 * 1024 + 1024, 33, 33] and len(c("first")[5:]) == 3
    assert c("fourth")[0] == OK and len(c("fourth")[5:]) == 3 * 4 and c("fourth")[3:5] == [int(300 * 0.7 / 8) + 1, int(20 * 0.7 / 8) + 1]     # halved three times
    assert c("last")[0] == OK and len(c("last")[5:]) == 3 * 12 and c("last")[3:5] == [2, 2]
    assert c("never")[0] == NONE_FITS and len(c("never")[5:]) == 3 * 12               # twelve attempts, then it gives up
    assert c("abandoned")[0] == ABANDONED and len(c("abandoned")[5:]) == 3
    # 65537^2, 32769^2 and 16385^2 buckets are more than 27 bits hold: not counted; 8193^2 is the first plan the callable sees
    assert c("too_many_buckets")[:5] == [OK, 8193 * 8193, 2000000000, 8193, 8193] and c("too_many_buckets")[5:] == [8193 * 8193, 8193, 2000000000]
    assert 16385 * 16385 > BUCKET_MASK >= 8193 * 8193 and 64 * (1 << 25) + 1024 > 2000000000             # (so many cells that the 2e9 limit is the one that binds)


# ------------------------------------------------------------------ MeshStats
@pytest.mark.parametrize("name", sorted(MESHES))
def test_mesh_stats_from_partials_equal_mesh_stats_from_columns(out, name):
    m = meshes()[name]
    want = stats_rule(m["c"], m["s"])
    same(out["stats_columns_" + name], want)
    same(out["stats_partials_" + name], want)
    assert out["partials_" + name] == [(m["M"] + 99) // 100, 1, 1]                   # several partials where the mesh has more than 100 cells; any_hot; planned
    if name in LOOKUP_MESHES:
        assert out["partials_" + name][0] > 5


def test_a_nan_width_takes_each_paths_own_route(out):
    m = meshes()["nanwidth"]
    want = stats_rule(m["c"], m["s"])                                                 # (nanmin, nanmax: the NaN is passed over)
    same(out["stats_columns_nanwidth"], want)
    assert want[2] == 1e8 and math.isnan(want[8 + 1 + 1024 + 517])                    # smin of axis 0; the NaN is among the samples
    got = out["stats_partials_nanwidth"]
    assert math.isnan(got[2])                                                         # from partials: smin IS the NaN ...
    same(got[:2] + got[3:], want[:2] + want[3:])
    assert out["partials_nanwidth"] == [11, 1, 0]                                     # ... and the plan refuses the mesh


# ------------------------------------------------------------------ layouts
def test_cell_buffer_layout(out):
    geom, geom2, fluid, bdir, fat = out["sizes"]
    assert (geom, geom2, fluid, bdir, fat) == (32, 16, 64, 16, 128)
    up = lambda x: (x + 255) // 256 * 256
    for dims in (TWO, TWO_POINT_FIVE, THREE):
        for k2e in (0, 1):
            o_geom, o_geom2, o_fluid, o_temp, o_fc, o_k2e, o_gamma, total, has_geom2, has_fc, has_k2e = out["cells_%d_%d" % (dims, k2e)]
            assert (has_geom2, has_fc, has_k2e) == (int(dims == THREE), int(dims != TWO), k2e)
            off, want = 0, []
            for present, size in ((1, 32), (has_geom2, 16), (1, 64), (1, 8), (has_fc, 8), (has_k2e, 8), (1, 8)):
                want.append(off if present else 0)
                off = up(off + size * 1000) if present else off
            assert [o_geom, o_geom2, o_fluid, o_temp, o_fc, o_k2e, o_gamma, total] == want + [off]
            assert all(v % 256 == 0 for v in want + [off])
    assert out["cells_0_0"][7] == 32000 + 64000 + 8192 + 8192 == 112384               # by hand: 2-D, 1000 cells, no hot cell
    assert out["cells_2_1"][7] == 112384 + 16128 + 2 * 8192


def test_grid_buffer_layout(out):
    assert out["gridlayout"] == [0, 17664, 17664 + 524288, 17664 + 524288 + 4608, 17664 + 524288 + 4608 + 256, 563200]     # by hand: 1089 buckets, 4096 entries, 7 ints
    assert all(v % 256 == 0 for v in out["gridlayout"] + out["gridlayout_empty"])
    assert out["gridlayout_empty"] == [0, 256, 512, 768, 1024, 1280]                  # room for one entry where there is none


# ------------------------------------------------------------------ ingest
@pytest.mark.parametrize("k", range(len(SLABS)))
def test_slab_for(out, k):
    r_inj, sw, min_r, max_r, min_t, max_t, fps, ef, dims, geom = SLABS[k]
    deg = 0.017453292519943295
    want = [dims, geom, sw, 0.95 * r_inj] + ([min_r - ef * C_LIGHT / fps, max_r + ef * C_LIGHT / fps, min_t - 2 * deg, max_t + 2 * deg] if sw == 0 else [0.0] * 4)
    same(out["slab_%d" % k], want)


def test_slab_cases_and_the_argument_checks(out):
    assert out["slab_1"][4] == 9e11 - 7 * C_LIGHT / 5.0 < out["slab_0"][4] and out["slab_0"][7] - 0.2 == pytest.approx(2 * math.pi / 180)
    assert out["slab_3"][2] == 1 and out["slab_3"][4:] == [0.0] * 4
    assert out["oks"] == [1, 1, 0, 0, 0, 1, 1, 0]


def test_staged_velocity_and_bucket_list_entry(out):
    v0, v1, v2, x1, x2 = 0.3, -0.2, 0.1, 0.7, 2.1
    sin, cos = math.sin, math.cos
    same(out["velocity_0_0"], [v0, v1, 0.0])
    same(out["velocity_0_2"], [v0, v1, 0.0])
    same(out["velocity_0_1"], [v0 * sin(x1) + v1 * cos(x1), v0 * cos(x1) - v1 * sin(x1), 0.0])
    same(out["velocity_1_1"], [v0 * sin(x1) + v1 * cos(x1), v0 * cos(x1) - v1 * sin(x1), v2])
    same(out["velocity_2_0"], [v0, v1, v2])
    same(out["velocity_2_1"], [v0 * sin(x1) * cos(x2) + v1 * cos(x1) * cos(x2) - v2 * sin(x2), v0 * sin(x1) * sin(x2) + v1 * cos(x1) * sin(x2) + v2 * cos(x2),
                               v0 * cos(x1) - v1 * sin(x1)])
    same(out["velocity_2_3"], [v0 * cos(x1) - v1 * sin(x1), v0 * sin(x1) + v1 * cos(x1), v2])
    assert out["fat"] == [1, 1, 1, 1, 77]


def chombo_rule(dims, tree, names):
    """the box table and the coordinate arrays by the formulas of hydro_plan.hpp's comment"""
    nd = 3 if dims == THREE else 2
    boxes, first, xs, dxs, total = [], [], [[], [], []], [[], [], []], 0
    for i, L in enumerate(tree):
        pd = L["prob_domain"]
        cb = [len(xs[a]) if a < nd else 0 for a in range(3)]
        for g in range(pd[0], pd[nd] + 1):
            if L["logr"]:
                xs[0].append(L["dombeg"][0] * 0.5 * (math.exp(L["dx"] * (g + 1)) + math.exp(L["dx"] * g)))
                dxs[0].append(L["dombeg"][0] * (math.exp(L["dx"] * (g + 1)) - math.exp(L["dx"] * g)))
            else:
                xs[0].append(L["dombeg"][0] + L["dx"] * (g + 0.5))
                dxs[0].append(L["dx"])
        for a in range(1, nd):
            for g in range(pd[a], pd[nd + a] + 1):
                xs[a].append(L["dombeg"][a] + L["dx"] * L["stretch"][a - 1] * (g + 0.5))
                dxs[a].append(L["dx"] * L["stretch"][a - 1])
        first.append(len(boxes))
        for b, off in zip(L["boxes"], L["offsets"]):
            lo = [b[a] if a < nd else 0 for a in range(3)]
            n = [b[nd + a] - b[a] + 1 if a < nd else 1 for a in range(3)]
            boxes.append([(total + off) // len(names), total + off, i] + lo + n + cb)
        total += L["data_len"]
    first.append(len(boxes))
    kv = [max([k for k, v in enumerate(names) if v == w], default=-1) for w in ("rho", "vx1", "vx2", "vx3", "prs")]
    return boxes, first, xs, dxs, total, kv


@pytest.mark.parametrize("name", ["2d", "3d", "no_vx3_2d"])
def test_chombo_plan(out, name):
    dims, tree, names = CHOMBO[name]
    assert out["chombo_" + name] == "planned"
    boxes, first, xs, dxs, total, kv = chombo_rule(dims, tree, names)
    assert out["chombov_" + name] == [total, total // NV] + kv + [len(boxes)] + first
    for j, b in enumerate(boxes):
        assert out["chombobox_%s_%d" % (name, j)] == b, j
    for a in range(3):
        same(out["chombox_%s_%d" % (name, a)], xs[a] + dxs[a])
    # the cells follow one another box by box, the levels' coordinate arrays level by level
    assert boxes[0][0] == 0 and all(boxes[j + 1][0] == boxes[j][0] + boxes[j][6] * boxes[j][7] * boxes[j][8] for j in range(len(boxes) - 1))
    assert boxes[-1][9] == tree[0]["prob_domain"][3 if dims == THREE else 2] + 1 and (len(xs[2]) > 0) == (dims == THREE)
    assert kv[3] == (-1 if name == "no_vx3_2d" else 3)                               # vx3 is not asked for in 2-D


@pytest.mark.parametrize("name", sorted(CHOMBO_TEXTS))
def test_chombo_refusals(out, name):
    assert out["chombo_" + name] == CHOMBO_TEXTS[name]
    assert "chombov_" + name not in out
