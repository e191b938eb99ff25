// hydro_plan.hpp -- the host's rules for staging a hydro frame: the bucket grid of the cell lookup (its plan from the mesh's statistics, the one
// coarsening rule, the host build that cross-checks grid_build.hip), the layouts of the per-cell buffer and of the grid buffer, the slab of an
// ingest and the box table of a PLUTO-Chombo frame.  engine.hip's stage_hydro and ingest entry points go through these functions.  Plain inline
// C++ -- no HIP call, no context, no device memory -- so that a CPU test can drive them (tests/test_hydro_plan_cpu.py).  Line numbers are the
// reference's.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/mcrat_hip.h"
#include "device_types.hpp"

namespace mcrat {

// ------------------------------------------------------------------ what the launchers and the host share
// the cell-lookup grid, built on the device (grid_build.hip)
struct GridPlan {
    double org[3], inv[3];
    int dim[3], logmap[3];
    int naxes;
};
struct StagePartial {       // one per workgroup of stage_cells_kernel
    double lo[3], hi[3], smin[3], smax[3];
    int any_hot, pad;
};
struct SlabDev {
    int dimensions, geometry, ph_inj_switch;
    double r_inj_095;                          // 0.95 r_inj
    double r_lo, r_hi, th_lo, th_hi;           // the widened slab for the current elem_factor
};
struct ChomboBox {          // one box of a PLUTO-Chombo level (mclib_pluto.c:520-545)
    long long first_cell;   // (start_displacement + box_offset) / num_vars: where its cells sit in the reader's cell numbering
    long long data_off;     // start_displacement + box_offset: its data in the concatenated "data:datatype=0" arrays
    int level;
    int lo[3], n[3];        // lo_i, lo_j, lo_k; cells per axis
    int cb[3];              // where this level's 1-D coordinate arrays start in ChomboDev::x / dx
    int pad[2];
};

// ------------------------------------------------------------------ the bucket grid
// Exact accelerator for the reference's linear findContainingBlock (geometry.c:350-391).  Every cell is entered into all buckets its closed
// extent, widened by 1e-9 relative, touches; cells are visited in ascending index so each bucket list is ascending.  The device walks the list
// of the bucket holding the point and applies the reference's own closed-interval test, so it returns the lowest-index containing cell exactly
// as the linear scan does.  (The reference's own buildSpatialGrid, geometry.c:526-676, is disabled at HEAD and tests DIMENSIONS against the
// wrong constants; it is not reproduced.)

// the bucket of coordinate x on one axis of a plan: floor((map(x) - org) * inv), clamped to 0 .. dim - 1; a NaN goes to bucket 0
inline int bucket_of(double x, int logmap, double org, double inv, int dim)
{
    double u = logmap ? log(x) : x;
    double f = floor((u - org) * inv);
    if (!(f == f)) return 0;
    if (f < 0.0) return 0;
    if (f > (double)(dim - 1)) return dim - 1;
    return (int)f;
}

// What the plan needs from the mesh: per axis the extent, the smallest and the largest width, and every stride-th cell's centre and width
// (stride = plan_stride(M)).
struct MeshStats {
    double lo[3], hi[3], smin[3], smax[3];
    std::vector<double> sc[3], ss[3];
};
inline int plan_stride(int M) { return std::max(1, M / 4096); }

// ... from a frame's host columns (the host build): c[k], s[k] = centres and widths of axis k < naxes, M cells.  Every extreme is taken with
// std::min / std::max from a finite start value, which never take a NaN: a NaN width (or centre) is passed over, smin included.
inline MeshStats mesh_stats_from_columns(const double *const c[3], const double *const s[3], int M, int naxes)
{
    MeshStats ms{};
    for (int k = 0; k < naxes; ++k) {
        double lo = INFINITY, hi = -INFINITY, smin = INFINITY, smax = 0;
        for (int i = 0; i < M; ++i) {
            lo = std::min(lo, c[k][i] - 0.5 * s[k][i]);
            hi = std::max(hi, c[k][i] + 0.5 * s[k][i]);
            smin = std::min(smin, s[k][i]);
            smax = std::max(smax, s[k][i]);
        }
        ms.lo[k] = lo; ms.hi[k] = hi; ms.smin[k] = smin; ms.smax[k] = smax;
        for (int i = 0; i < M; i += plan_stride(M)) { ms.sc[k].push_back(c[k][i]); ms.ss[k].push_back(s[k][i]); }
    }
    return ms;
}
// ... from what stage_cells_kernel reduced (the product path): part[0 .. nblk) and the sample block, per axis k nsamp centres at
// samp[2k * nsamp] and nsamp widths at samp[(2k + 1) * nsamp].  lo, hi and smax pass a NaN over as above.  smin does NOT: a partial whose smin
// is NaN becomes the result and stays it, so that a NaN width the kernel has let through makes grid_plan_from_stats refuse the mesh.
// *any_hot: some cell of the frame has T >= 1e7 K.
inline MeshStats mesh_stats_from_partials(const StagePartial *part, int nblk, const double *samp, int nsamp, int naxes, bool *any_hot)
{
    MeshStats ms{};
    for (int k = 0; k < naxes; ++k) {
        double lo = INFINITY, hi = -INFINITY, smin = INFINITY, smax = 0;
        for (int b = 0; b < nblk; ++b) {
            lo = std::min(lo, part[b].lo[k]);
            hi = std::max(hi, part[b].hi[k]);
            smin = (part[b].smin[k] < smin || !(part[b].smin[k] == part[b].smin[k])) ? part[b].smin[k] : smin;
            smax = std::max(smax, part[b].smax[k]);
        }
        ms.lo[k] = lo; ms.hi[k] = hi; ms.smin[k] = smin; ms.smax[k] = smax;
        ms.sc[k].assign(samp + (size_t)(2 * k) * nsamp, samp + (size_t)(2 * k + 1) * nsamp);
        ms.ss[k].assign(samp + (size_t)(2 * k + 1) * nsamp, samp + (size_t)(2 * k + 2) * nsamp);
    }
    *any_hot = false;
    for (int b = 0; b < nblk; ++b) *any_hot = *any_hot || part[b].any_hot;
    return ms;
}

// The bucket grid up to a scale factor f: per axis whether buckets are uniform in the logarithm of the coordinate (the mesh starts above 0 and
// its widths differ by more than a factor 4), the extent in the mapped coordinate, and how many typical cells span it.
struct GridScale {
    double ext_lo[3] = {0, 0, 0}, ext_hi[3] = {0, 0, 0}, ncell[3] = {1, 1, 1}, f0 = 1.0;
    int logmap[3] = {0, 0, 0}, naxes = 2;
};
// The typical cell is a small one -- the lower quartile of the sampled widths in the mapped coordinate: in a mesh with two refinement levels the
// fine cells, where the photons are, then get buckets of their own size instead of lists of nine.  f0, the scale to start from, is 1 unless that
// makes more than min(4 M, 2^24) buckets' worth of cells; then it brings the product down to that target.  false: a degenerate mesh -- an axis
// without extent (hi <= lo, or NaN), without a positive smallest width, or without a sample.
inline bool grid_plan_from_stats(const MeshStats &ms, int M, int naxes, GridScale &g)
{
    g.naxes = naxes;
    for (int k = 0; k < naxes; ++k) {
        const double lo = ms.lo[k], hi = ms.hi[k], smin = ms.smin[k], smax = ms.smax[k];
        if (!(hi > lo) || !(smin > 0)) return false;
        g.logmap[k] = (lo > 0 && smax / smin > 4.0) ? 1 : 0;
        std::vector<double> w;
        for (size_t i = 0; i < ms.sc[k].size(); ++i) {
            const double a = ms.sc[k][i] - 0.5 * ms.ss[k][i], b = ms.sc[k][i] + 0.5 * ms.ss[k][i];
            w.push_back(g.logmap[k] ? log(b) - log(std::max(a, 1e-300)) : b - a);
        }
        if (w.empty()) return false;
        std::nth_element(w.begin(), w.begin() + w.size() / 4, w.end());
        const double med = w[w.size() / 4];
        g.ext_lo[k] = g.logmap[k] ? log(lo) : lo;
        g.ext_hi[k] = g.logmap[k] ? log(hi) : hi;
        g.ncell[k] = std::max(1.0, (g.ext_hi[k] - g.ext_lo[k]) / med);
    }
    double prod = 1;
    for (int k = 0; k < naxes; ++k) prod *= g.ncell[k];
    const double target = std::min(std::max(4.0 * (double)M, 1.0), 16777216.0);
    g.f0 = (prod > target) ? pow(target / prod, 1.0 / naxes) : 1.0;
    return true;
}

// The plan for scale factor f; *nb receives its number of buckets.  Per axis nbk = floor(ncell * f) buckets (1 .. 65536) of about one cell,
// shifted by half a bucket against the mesh, which takes one bucket more (dim = nbk + 1): on a regular mesh a bucket then straddles 2 cells per
// axis (4 in 2-D); aligned buckets would each touch 3 per axis because cell faces lie on bucket faces.
inline GridPlan grid_dims(const GridScale &g, double f, long long *nb)
{
    GridPlan p{};
    p.naxes = g.naxes;
    *nb = 1;
    for (int k = 0; k < 3; ++k) {
        p.dim[k] = 1; p.org[k] = 0; p.inv[k] = 0; p.logmap[k] = g.logmap[k];
        if (k < g.naxes) {
            const int nbk = (int)std::max(1.0, std::min(65536.0, floor(g.ncell[k] * f)));
            const double width = (g.ext_hi[k] - g.ext_lo[k]) / nbk;
            p.dim[k] = nbk + 1;
            p.org[k] = g.ext_lo[k] - 0.5 * width;
            p.inv[k] = 1.0 / width;
        }
        *nb *= p.dim[k];
    }
    return p;
}
inline void grid_plan_to_dev(const GridPlan &p, GridDev &d)
{
    for (int k = 0; k < 3; ++k) { d.org[k] = p.org[k]; d.inv[k] = p.inv[k]; d.dim[k] = p.dim[k]; d.logmap[k] = p.logmap[k]; }
    d.naxes = p.naxes;
}

// The coarsening rule, once for the device build and the host build: up to 12 attempts from f0, f halved after each, for the first plan whose
// bucket lists hold no more than 64 M + 1024 entries and no more than 2e9.  A plan with more buckets than a bucket code has bits for
// (GRID_CODE_BUCKET_MASK, 27 bits) is passed over without being counted.  count(plan, nb, limit) says how many entries the plan's lists would
// hold -- it may stop counting once it is over `limit` and return what it has -- or a negative number when it could not count: then the search
// ends at once with GRID_SCALE_ABANDONED and the caller knows why.
enum GridScaleResult { GRID_SCALE_OK = 0, GRID_SCALE_NONE_FITS, GRID_SCALE_ABANDONED };
struct GridChoice {
    GridScaleResult result;
    GridPlan plan;
    long long nb, entries;
};
template <class Count>
inline GridChoice choose_grid_scale(const GridScale &g, int M, Count count)
{
    GridChoice ch{};
    const long long limit = std::min(64LL * M + 1024, 2000000000LL);
    double f = g.f0;
    for (int attempt = 0; attempt < 12; ++attempt, f *= 0.5) {
        ch.plan = grid_dims(g, f, &ch.nb);
        if (ch.nb > (long long)GRID_CODE_BUCKET_MASK) continue;
        ch.entries = count(ch.plan, ch.nb, limit);
        if (ch.entries < 0) { ch.result = GRID_SCALE_ABANDONED; return ch; }
        if (ch.entries > limit) continue;                      // too fine for this mesh: coarsen and retry
        ch.result = GRID_SCALE_OK;
        return ch;
    }
    ch.result = GRID_SCALE_NONE_FITS;
    return ch;
}

// ------------------------------------------------------------------ the host build (MCRAT_HIP_HOST_GRID=1): the cross-check of grid_build.hip
struct GridHost {
    GridPlan plan;
    long long nb = 0;
    std::vector<int> start, cells;    // bucket b's list: cells[start[b] .. start[b + 1])
    std::vector<unsigned> hints;      // per bucket, see BucketDir
    std::vector<int> covered;         // per bucket and octant, see GridDev::cov_back; empty: the plan gets no table (covered_table_ints)
};
// the buckets [b0, b1] of axis k that cell i's closed extent, widened by 1e-9 of (|centre| + width), touches
inline void cell_bucket_range(const GridPlan &p, int k, double c, double s, int &b0, int &b1)
{
    const double m = 1e-9 * (fabs(c) + s);
    double a = c - 0.5 * s - m, b = c + 0.5 * s + m;
    if (p.logmap[k] && a <= 0) a = 1e-300;
    b0 = bucket_of(a, p.logmap[k], p.org[k], p.inv[k], p.dim[k]);
    b1 = bucket_of(b, p.logmap[k], p.org[k], p.inv[k], p.dim[k]);
}
// The hint rule: an octant of a bucket (half a bucket per axis; a quadrant in 2-D) gets the offset of the list entry whose cell is the ONLY one
// of the list reaching into the octant's interior -- extents shrunk by the 1e-9 margin the lists were widened by, so cells that merely abut do
// not count.  GRID_NO_HINT where none or several do, or where the one sits at offset 15 or beyond; the octants a 2-D grid does not have are
// GRID_NO_HINT too.  list = the bucket's n entries, bi = its index per axis.
inline unsigned bucket_hints(const GridPlan &p, const int bi[3], const int *list, int n, const double *const c[3], const double *const s[3])
{
    const int naxes = p.naxes, nocts = 1 << naxes;
    unsigned h = 0;
    for (int o = 0; o < 8; ++o) {
        unsigned pick = GRID_NO_HINT;
        if (o < nocts) {
            int found = 0;
            for (int e = 0; e < n && found < 2; ++e) {
                const int ci = list[e];
                bool reaches = true;
                for (int k = 0; k < naxes && reaches; ++k) {
                    const double w = 1.0 / p.inv[k];
                    const double olo = p.org[k] + (bi[k] + 0.5 * ((o >> k) & 1)) * w, ohi = olo + 0.5 * w;
                    const double m = 1e-9 * (fabs(c[k][ci]) + s[k][ci]);
                    double clo = c[k][ci] - 0.5 * s[k][ci] + m, chi = c[k][ci] + 0.5 * s[k][ci] - m;
                    if (p.logmap[k]) { clo = log(std::max(clo, 1e-300)); chi = log(std::max(chi, 1e-300)); }
                    reaches = (clo < ohi) && (chi > olo);
                }
                if (reaches) { found += 1; if (e < (int)GRID_NO_HINT) pick = (unsigned)e; else found = 2; }
            }
            if (found != 1) pick = GRID_NO_HINT;
        }
        h |= pick << (4 * o);
    }
    return h;
}
// The covered rule, once for the host build and for grid_build.hip (GridDev::cov_back, device_types.hpp): octant o of bucket bi is covered by
// its hinted cell (centre c, width s per axis) when on every axis
//   (a) the cell's extent [c - s/2, c + s/2] holds the octant shrunk inward by m = 0.5e-6 w, half the accept margin of a bucket code (w = the
//       bucket's width), and
//   (b) m >= 1e-8 s + 64 DBL_EPSILON (|c| + s).
// Then every point whose code carries GRID_CODE_HINT_OK for this octant passes well_in_fat_cell on that cell: the point lies 1e-6 w inside the
// octant's faces (grid_bucket_axes), so by (a) at least m inside the cell's, and well_in asks for 0.5e-8 s.  (b) leaves m - 0.5e-8 s >= 0.5e-8 s
// + 64 ulp of the largest coordinate in play for what the roundings can move: the bucket coordinate x = (u - org) inv of at most 65 537 carries
// 2 roundings (1.5e-11 w), the faces org + (b + h/2) w of this function 4 (2^-52 (65 537 w + |c| + s)), the cell's faces c -+ s/2 one each,
// well_in's own 2 |a - c| - s two of at most 2^-53 s -- under 8 ulp of |c| + s and 4e-11 w together, and s > 0.49 w in a cell that holds an
// octant.  A NaN fails a comparison, and a log-mapped axis is never covered: in the mapped coordinate the margins are no fixed part of a width.
constexpr double GRID_COVER_GUARD = 64 * 2.220446049250313e-16;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool octant_covered(const GridPlan &p, const int bi[3], int o, const double c[3], const double s[3])
{
    bool covered = true;
    for (int k = 0; k < p.naxes; ++k) {
        const double w = 1.0 / p.inv[k];
        const double olo = p.org[k] + (bi[k] + 0.5 * ((o >> k) & 1)) * w, ohi = olo + 0.5 * w;      // as bucket_hints has them
        const double m = 0.5 * GRID_ACCEPT_MARGIN * w;
        const bool holds = (c[k] - 0.5 * s[k] <= olo + m) & (c[k] + 0.5 * s[k] >= ohi - m);
        const bool implied = m >= 1e-8 * s[k] + GRID_COVER_GUARD * (fabs(c[k]) + s[k]);
        covered = covered & holds & implied & (p.logmap[k] == 0);
    }
    return covered;
}
// The size rule: the ints of a plan's table, one per bucket and octant -- or 0, no table, when it is switched off (MCRAT_HIP_NO_COVERED), when
// an axis is log-mapped (nothing would be covered), or above GRID_COVERED_MAX_INTS (256 MiB; the benchmark's 2.6 M buckets take 42 MB, a 3-D
// grid 32 B per bucket, and the lists of a grid that size weigh gigabytes already).
inline size_t covered_table_ints(const GridPlan &p, long long nb, bool enabled)
{
    if (!enabled || nb <= 0) return 0;
    for (int k = 0; k < p.naxes; ++k)
        if (p.logmap[k]) return 0;
    const long long ints = nb << p.naxes;
    return ints > GRID_COVERED_MAX_INTS ? 0 : (size_t)ints;
}
// a bucket's 2^naxes table entries from its hints (bucket_hints): out[o] = the hinted cell where it covers octant o, else -1
inline void bucket_covered(const GridPlan &p, const int bi[3], const int *list, unsigned hints, const double *const c[3], const double *const s[3], int *out)
{
    for (int o = 0; o < (1 << p.naxes); ++o) {
        const unsigned pick = (hints >> (4 * o)) & 15u;
        out[o] = -1;
        if (pick == GRID_NO_HINT) continue;
        const int ci = list[pick];
        double cc[3] = {0, 0, 0}, ss[3] = {0, 0, 0};
        for (int k = 0; k < p.naxes; ++k) { cc[k] = c[k][ci]; ss[k] = s[k][ci]; }
        if (octant_covered(p, bi, o, cc, ss)) out[o] = ci;
    }
}
// The grid of a mesh given as host columns (c, s as for mesh_stats_from_columns).  false: a degenerate mesh, or no scale fits it.  The counting
// pass of an attempt ends as soon as the total is over the limit.  MCRAT_HIP_VERBOSE in the environment: two lines on stderr.
inline bool build_grid(const double *const c[3], const double *const s[3], int M, int naxes, GridHost &g)
{
    GridScale scale;
    if (!grid_plan_from_stats(mesh_stats_from_columns(c, s, M, naxes), M, naxes, scale)) return false;
    std::vector<long long> count;
    const GridChoice ch = choose_grid_scale(scale, M, [&](const GridPlan &p, long long nb, long long limit) {
        count.assign((size_t)nb + 1, 0);
        long long total = 0;
        for (int i = 0; i < M && total <= limit; ++i) {
            int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
            for (int k = 0; k < naxes; ++k) cell_bucket_range(p, k, c[k][i], s[k][i], lo[k], hi[k]);
            for (int z = lo[2]; z <= hi[2]; ++z)
                for (int y = lo[1]; y <= hi[1]; ++y)
                    for (int x = lo[0]; x <= hi[0]; ++x) count[((size_t)z * p.dim[1] + y) * p.dim[0] + x + 1]++;
            total += (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
        }
        return total;
    });
    if (ch.result != GRID_SCALE_OK) return false;
    const GridPlan &p = g.plan = ch.plan;
    const long long nb = g.nb = ch.nb, total = ch.entries;
    for (size_t b = 0; b < (size_t)nb; ++b) count[b + 1] += count[b];
    g.start.resize((size_t)nb + 1);
    for (size_t b = 0; b <= (size_t)nb; ++b) g.start[b] = (int)count[b];
    if (getenv("MCRAT_HIP_VERBOSE"))
        fprintf(stderr, "mcrat_hip: cell-lookup grid %d x %d x %d buckets, %lld entries for %d cells (%.2f per bucket)\n",
                p.dim[0], p.dim[1], p.dim[2], total, M, (double)total / (double)nb);
    g.cells.assign((size_t)total, -1);
    std::vector<int> fill(g.start.begin(), g.start.end() - 1);
    for (int i = 0; i < M; ++i) {
        int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        for (int k = 0; k < naxes; ++k) cell_bucket_range(p, k, c[k][i], s[k][i], lo[k], hi[k]);
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) g.cells[(size_t)fill[((size_t)z * p.dim[1] + y) * p.dim[0] + x]++] = i;
    }
    g.hints.assign((size_t)nb, 0);
    for (long long b = 0; b < nb; ++b) {
        const int bi[3] = {(int)(b % p.dim[0]), (int)((b / p.dim[0]) % p.dim[1]), (int)(b / ((long long)p.dim[0] * p.dim[1]))};
        const int e0 = g.start[(size_t)b];
        g.hints[(size_t)b] = bucket_hints(p, bi, g.cells.data() + e0, g.start[(size_t)b + 1] - e0, c, s);
    }
    g.covered.assign(covered_table_ints(p, nb, true), -1);
    for (long long b = 0; b < nb && !g.covered.empty(); ++b) {
        const int bi[3] = {(int)(b % p.dim[0]), (int)((b / p.dim[0]) % p.dim[1]), (int)(b / ((long long)p.dim[0] * p.dim[1]))};
        bucket_covered(p, bi, g.cells.data() + g.start[(size_t)b], g.hints[(size_t)b], c, s, g.covered.data() + ((size_t)b << naxes));
    }
    if (getenv("MCRAT_HIP_VERBOSE")) {
        const int nocts = 1 << naxes;
        long long hinted = 0;
        for (long long b = 0; b < nb; ++b)
            for (int o = 0; o < nocts; ++o) hinted += ((g.hints[(size_t)b] >> (4 * o)) & 15u) != GRID_NO_HINT;
        fprintf(stderr, "mcrat_hip: %.1f %% of the bucket octants have a single-cell hint\n", 100.0 * hinted / ((double)nb * nocts));
        long long cov = 0;
        for (int e : g.covered) cov += e >= 0;
        fprintf(stderr, "mcrat_hip: %.1f %% of the bucket octants are covered by their hinted cell\n", 100.0 * cov / ((double)nb * nocts));
    }
    return true;
}

// The per-cell part of hydroVectorToCartesian (geometry.c:189-253), applied once per frame; the device adds the photon-azimuth part
// (physics.hpp, cell_beta).  (v0, v1, v2) = the cell's velocity in the frame's coordinates (v2 = 0 in 2-D), x1, x2 = its second and third
// coordinate (x2 is read in 3-D spherical geometry only).  out = the three components CellFluid::a, b, c are staged from.
inline void cell_velocity_staged(int dimensions, int geometry, double v0, double v1, double v2, double x1, double x2, double out[3])
{
    if (dimensions != DIM_THREE) {
        if (geometry == GEOM_SPHERICAL) {
            out[0] = v0 * sin(x1) + v1 * cos(x1);
            out[1] = v0 * cos(x1) - v1 * sin(x1);
        } else {
            out[0] = v0;
            out[1] = v1;
        }
        out[2] = v2;
    } else if (geometry == GEOM_CARTESIAN) {
        out[0] = v0; out[1] = v1; out[2] = v2;
    } else if (geometry == GEOM_SPHERICAL) {
        out[0] = v0 * sin(x1) * cos(x2) + v1 * cos(x1) * cos(x2) - v2 * sin(x2);
        out[1] = v0 * sin(x1) * sin(x2) + v1 * cos(x1) * sin(x2) + v2 * cos(x2);
        out[2] = v0 * cos(x1) - v1 * sin(x1);
    } else {   // POLAR
        out[0] = v0 * cos(x1) - v1 * sin(x1);
        out[1] = v0 * sin(x1) + v1 * cos(x1);
        out[2] = v2;
    }
}
// a bucket-list entry: a complete copy of cell ci's records (device_types.hpp, FatCell); c2 = s2 = 0 where there is no third axis
inline FatCell fat_cell(const CellGeom &geom, const CellFluid &fluid, double c2, double s2, int ci)
{
    FatCell f{};
    f.c0 = geom.c0; f.c1 = geom.c1; f.s0 = geom.s0; f.s1 = geom.s1;
    f.a = fluid.a; f.b = fluid.b; f.c = fluid.c; f.w = fluid.w;
    f.nsig = fluid.nsig; f.gam = fluid.gam;
    f.c2 = c2; f.s2 = s2;
    f.cell = ci; f.pad = 0; f.pad2[0] = f.pad2[1] = f.pad2[2] = 0.0;
    return f;
}

// ------------------------------------------------------------------ the two buffers' layouts
// Every array starts on a 256-byte boundary, in the order of the members; an absent array has offset 0 and its has_ flag down.
inline size_t layout_take(size_t &off, size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; }
// The per-cell buffer of a frame of M cells.  geom2 (the third axis) exists in 3-D only, fluid_c (the third velocity component) in 2.5-D and
// 3-D.  k2e is reserved when the caller says so: the device staging learns only afterwards whether a cell is hot and always reserves it, the
// host staging knows beforehand and reserves it only then.
struct CellLayout {
    size_t geom, geom2, fluid, temp, fluid_c, k2e, gamma, total;
    bool has_geom2, has_fluid_c, has_k2e;
};
inline CellLayout cell_layout(int dimensions, int M, bool reserve_k2e)
{
    CellLayout l{};
    l.has_geom2 = dimensions == DIM_THREE; l.has_fluid_c = dimensions != DIM_TWO; l.has_k2e = reserve_k2e;
    size_t off = 0;
    l.geom = layout_take(off, sizeof(CellGeom) * M);
    l.geom2 = l.has_geom2 ? layout_take(off, sizeof(CellGeom2) * M) : 0;
    l.fluid = layout_take(off, sizeof(CellFluid) * M);
    l.temp = layout_take(off, sizeof(double) * M);
    l.fluid_c = l.has_fluid_c ? layout_take(off, sizeof(double) * M) : 0;
    l.k2e = l.has_k2e ? layout_take(off, sizeof(double) * M) : 0;
    l.gamma = layout_take(off, sizeof(double) * M);
    l.total = off;
    return l;
}
// The grid buffer of nb buckets and `entries` list entries: the covered-octant table (covered_ints of covered_table_ints; none: offset 0 like the
// bucket records, which then open the buffer), the bucket records and the lists (room for one entry where there is none), which
// the lookup reads, then what only the device build uses -- the lists' starts (nb + 1), the scan's scratch (scan_scratch_ints: the launcher's
// grid_scan_scratch_ints(nb)) and the entries' cell indices.  The host build uploads [0, start).
struct GridLayout {
    size_t dir, cells, start, scan, entries, total, covered;
};
inline GridLayout grid_layout(long long nb, long long entries, size_t scan_scratch_ints, size_t covered_ints = 0)
{
    GridLayout l{};
    size_t off = 0;
    l.covered = layout_take(off, sizeof(int) * covered_ints);
    l.dir = layout_take(off, sizeof(BucketDir) * (size_t)nb);
    l.cells = layout_take(off, sizeof(FatCell) * std::max<size_t>((size_t)entries, 1));
    l.start = layout_take(off, sizeof(int) * ((size_t)nb + 1));
    l.scan = layout_take(off, sizeof(int) * scan_scratch_ints);
    l.entries = layout_take(off, sizeof(int) * std::max<size_t>((size_t)entries, 1));
    l.total = off;
    return l;
}

// ------------------------------------------------------------------ ingest
// the slab for one elem_factor (mclib_flash.c:84-85,309 == mclib_pluto.c:1081-1082,1276): the photons' radial range widened by elem_factor
// frames of light travel on either side and their angle range by two degrees; an injection frame (ph_inj_switch != 0) takes every cell above
// 0.95 r_inj and leaves the ranges 0
inline SlabDev slab_for(int dimensions, int geometry, const mcrat_hip_slab *s, int elem_factor)
{
    SlabDev d{};
    d.dimensions = dimensions; d.geometry = geometry; d.ph_inj_switch = s->ph_inj_switch;
    d.r_inj_095 = 0.95 * s->r_inj;
    if (s->ph_inj_switch == 0) {
        d.r_lo = s->min_r - elem_factor * C_LIGHT / s->fps;
        d.r_hi = s->max_r + elem_factor * C_LIGHT / s->fps;
        d.th_lo = s->min_theta - 2 * 0.017453292519943295;
        d.th_hi = s->max_theta + 2 * 0.017453292519943295;
    }
    return d;
}
inline bool slab_ok(const mcrat_hip_slab *s) { return s && s->fps > 0 && (s->ph_inj_switch == 0 || s->ph_inj_switch == 1); }
inline bool outflow_ok(const mcrat_hip_outflow *o) { return !o || (o->simulation_type >= MCRAT_HIP_SCIENCE && o->simulation_type <= MCRAT_HIP_STRUCTURED_SPHERICAL_OUTFLOW); }

// A PLUTO-Chombo frame's box table in the reader's cell numbering and its per-level coordinate arrays (mclib_pluto.c:446-517).  Level i's
// arrays cover its prob_domain, index g = prob_domain[a] + j on axis a:
//   x1 = dombeg1 + dx (g + 0.5), width dx -- or, with logr, dombeg1 (e^(dx (g + 1)) + e^(dx g)) / 2, width dombeg1 (e^(dx (g + 1)) - e^(dx g));
//   x2 = dombeg2 + dx g_x2stretch (g + 0.5), width dx g_x2stretch; x3 likewise with dombeg3 and g_x3stretch (3-D only);
// the levels' arrays follow one another in xs[a] / dxs[a], and a box's cb[a] is where its level's start.  A box's data_off is the doubles of
// all coarser levels plus its "data:offsets=0" entry, its first_cell that over num_vars; level_first_box[i] is level i's first box
// (level_first_box[num_levels] = all boxes); total = the doubles of all levels, cells = total / num_vars; kv = the component index of rho, vx1,
// vx2, vx3 and prs (the last of that name; -1: absent).
struct ChomboPlan {
    std::vector<ChomboBox> boxes;
    std::vector<int> level_first_box;
    std::vector<double> xs[3], dxs[3];
    long long total = 0, cells = 0;
    int kv[5] = {-1, -1, -1, -1, -1};
};
// nullptr: planned.  Otherwise the frame is refused (MCRAT_HIP_EINVAL) and this is why -- "" where the refusal has no text of its own: a level
// record that makes no sense, no box at all, no cell or more than INT_MAX, a first box that does not start at cell 0.  h itself has been
// checked by the caller (levels, variables and data are there).
inline const char *chombo_plan(const mcrat_hip_chombo *h, int dimensions, ChomboPlan &p)
{
    const bool three = dimensions == DIM_THREE;
    const int nd = three ? 3 : 2, bi = 2 * nd, nl = h->num_levels, nv = h->num_vars;
    p = ChomboPlan{};
    p.level_first_box.assign(nl + 1, 0);
    std::vector<ChomboBox> &boxes = p.boxes;
    long long total = 0;                                         // doubles of all levels so far: start_displacement (:151-155)
    for (int i = 0; i < nl; ++i) {
        const mcrat_hip_chombo_level &L = h->levels[i];
        if (L.n_boxes < 0 || (L.n_boxes > 0 && (!L.boxes || !L.box_offsets)) || L.data_len < 0 || L.ref_ratio <= 0) return "";
        int ext[3] = {1, 1, 1}, cb[3] = {0, 0, 0};
        for (int a = 0; a < nd; ++a) {
            ext[a] = L.prob_domain[nd + a] - L.prob_domain[a] + 1;
            if (ext[a] <= 0) return "";
            cb[a] = (int)p.xs[a].size();
        }
        for (int j = 0; j < ext[0]; ++j) {
            const int g = L.prob_domain[0] + j;
            if (L.logr == 0) { p.xs[0].push_back(L.dombeg1 + L.dx * (g + 0.5)); p.dxs[0].push_back(L.dx); }
            else {
                p.xs[0].push_back(L.dombeg1 * 0.5 * (exp(L.dx * (g + 1)) + exp(L.dx * g)));
                p.dxs[0].push_back(L.dombeg1 * (exp(L.dx * (g + 1)) - exp(L.dx * g)));
            }
        }
        for (int j = 0; j < ext[1]; ++j) { p.xs[1].push_back(L.dombeg2 + L.dx * L.g_x2stretch * (L.prob_domain[1] + j + 0.5)); p.dxs[1].push_back(L.dx * L.g_x2stretch); }
        for (int j = 0; three && j < ext[2]; ++j) { p.xs[2].push_back(L.dombeg3 + L.dx * L.g_x3stretch * (L.prob_domain[2] + j + 0.5)); p.dxs[2].push_back(L.dx * L.g_x3stretch); }
        p.level_first_box[i] = (int)boxes.size();
        for (int j = 0; j < L.n_boxes; ++j) {
            const int *b = L.boxes + (size_t)j * bi;
            ChomboBox r{};
            r.level = i;
            long long ncell = 1;
            for (int a = 0; a < 3; ++a) {
                r.lo[a] = a < nd ? b[a] : 0;
                r.n[a] = a < nd ? b[nd + a] - b[a] + 1 : 1;
                r.cb[a] = cb[a];
                // the reader indexes its coordinate arrays with the box's own indices (:541): they must exist
                if (r.n[a] <= 0 || (a < nd && (r.lo[a] < 0 || r.lo[a] + r.n[a] > ext[a]))) return "PLUTO-Chombo ingest: a box lies outside its level's prob_domain";
                ncell *= r.n[a];
            }
            r.data_off = total + L.box_offsets[j];
            r.first_cell = r.data_off / nv;
            if (L.box_offsets[j] < 0 || L.box_offsets[j] + ncell * nv > L.data_len) return "PLUTO-Chombo ingest: a box's data lies outside its level's data";
            if (!boxes.empty() && r.first_cell != boxes.back().first_cell + (long long)boxes.back().n[0] * boxes.back().n[1] * boxes.back().n[2])
                return "PLUTO-Chombo ingest: box data do not follow one another in data:offsets order";
            boxes.push_back(r);
        }
        total += L.data_len;
    }
    p.level_first_box[nl] = (int)boxes.size();
    p.total = total;
    p.cells = total / nv;
    if (boxes.empty() || p.cells <= 0 || p.cells > 0x7fffffffLL || boxes.front().first_cell != 0) return "";
    static const char *want[5] = {"rho", "vx1", "vx2", "vx3", "prs"};
    for (int k = 0; k < nv; ++k)
        for (int w = 0; w < 5; ++w)
            if (h->var_names[k] && strcmp(h->var_names[k], want[w]) == 0) p.kv[w] = k;
    if (p.kv[0] < 0 || p.kv[1] < 0 || p.kv[2] < 0 || p.kv[4] < 0 || (dimensions != DIM_TWO && p.kv[3] < 0))
        return "PLUTO-Chombo ingest: a component (rho, vx1, vx2, [vx3], prs) is missing";
    return nullptr;
}

}  // namespace mcrat
