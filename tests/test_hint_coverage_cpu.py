"""The premise of the loop kernel's short pass on the benchmark frame: phase 2 has nothing to do there.

rank_loop_kernel's fused pass settles a slot in phase 1 when the quadrant of the cell-lookup bucket its position lies in has a single-cell hint
(hydro_plan.hpp, bucket_hints); only slots without one are queued for phase 2, and a pass whose queue is empty goes from the barrier behind
phase 1 straight to the merge of the waves' minima.  On synth.config2()'s mesh at nzc = 64 -- the benchmark's frame -- the plan rules give buckets
of one fine cell, half a cell off the mesh, so every quadrant lies inside exactly one cell, fine or coarse: every photon position has a hint.

The grid is built by hydro_plan.hpp's own build_grid through a small g++ driver (as tests/test_hydro_plan_cpu.py does); the driver finds a
position's bucket with bucket_of and its quadrant with the expression bucket_hints itself uses for a quadrant's lower face."""
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
#include <vector>
#include "hydro_plan.hpp"
using namespace mcrat;

template <class T> static std::vector<T> get(FILE *f, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int> head = get<int>(f, 2);
    const int M = head[0], np = head[1], naxes = 2;
    std::vector<double> col[4], pt[2];
    for (int k = 0; k < 4; ++k) col[k] = get<double>(f, M);
    for (int k = 0; k < 2; ++k) pt[k] = get<double>(f, np);
    fclose(f);
    const double *c[3] = {col[0].data(), col[2].data(), nullptr};
    const double *s[3] = {col[1].data(), col[3].data(), nullptr};
    GridHost g;
    if (!build_grid(c, s, M, naxes, g)) { printf("grid: 0\n"); return 0; }
    const GridPlan &p = g.plan;
    printf("grid: 1 %d %d %.17g %.17g %.17g %.17g\n", p.dim[0], p.dim[1], 1.0 / p.inv[0], 1.0 / p.inv[1], p.org[0], p.org[1]);
    long long hinted = 0, near_face = 0, quads = 0, quads_hinted = 0;
    for (int q = 0; q < np; ++q) {
        long long b = 0;
        int oct = 0;
        bool near = false;
        for (int k = naxes - 1; k >= 0; --k) {
            const double x = pt[k][q], u = p.logmap[k] ? log(x) : x, w = 1.0 / p.inv[k];
            const int bk = bucket_of(x, p.logmap[k], p.org[k], p.inv[k], p.dim[k]);
            const double mid = p.org[k] + (bk + 0.5) * w;          // the lower face of the upper quadrant (bucket_hints: olo of bit 1)
            if (u >= mid) oct |= 1 << k;
            const double fr = (u - p.org[k]) * p.inv[k] - bk;      // (the device uses a hint only 1e-6 bucket widths off the quadrant's faces)
            near = near || fr < 1e-6 || fabs(fr - 0.5) < 1e-6 || 1.0 - fr < 1e-6;
            b = b * p.dim[k] + bk;
        }
        hinted += ((g.hints[(size_t)b] >> (4 * oct)) & 15u) != GRID_NO_HINT;
        near_face += near;
    }
    for (long long b = 0; b < g.nb; ++b)
        for (int o = 0; o < 4; ++o) { quads += 1; quads_hinted += ((g.hints[(size_t)b] >> (4 * o)) & 15u) != GRID_NO_HINT; }
    printf("points: %d %lld %lld\n", np, hinted, near_face);
    printf("quadrants: %lld %lld\n", quads, quads_hinted);
    return 0;
}
'''


def hint_coverage(tmp_dir, frame, ph):
    """hydro_plan.hpp's grid of a 2-D cylindrical frame and the photons' positions in it -> dict(dim, width, org, points, hinted, near_face,
    quadrants, quadrants_hinted)"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the grid rules' driver")
    d = str(tmp_dir)
    src, exe, data = os.path.join(d, "driver.cpp"), os.path.join(d, "driver"), os.path.join(d, "mesh.in")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), src, "-o", exe], check=True)
    a0 = np.sqrt(ph["r0"] * ph["r0"] + ph["r1"] * ph["r1"])           # (r, z) of a photon: physics.hpp, hydro_coords, 2-D cylindrical
    a1 = np.asarray(ph["r2"], dtype=np.float64)
    with open(data, "wb") as f:
        np.array([frame["r0"].size, a0.size], dtype=np.int32).tofile(f)
        for k in ("r0", "r0_size", "r1", "r1_size"):
            np.ascontiguousarray(frame[k], dtype=np.float64).tofile(f)
        np.ascontiguousarray(a0, dtype=np.float64).tofile(f)
        a1.tofile(f)
    rows = {}
    for line in subprocess.run([exe, data], check=True, capture_output=True, text=True).stdout.splitlines():
        tag, _, rest = line.partition(": ")
        rows[tag] = [float(v) for v in rest.split()]
    assert rows["grid"][0] == 1, "build_grid refused the mesh"
    g, p, q = rows["grid"], rows["points"], rows["quadrants"]
    return dict(dim=(int(g[1]), int(g[2])), width=(g[3], g[4]), org=(g[5], g[6]), points=int(p[0]), hinted=int(p[1]), near_face=int(p[2]),
                quadrants=int(q[0]), quadrants_hinted=int(q[1]))


def test_every_photon_of_the_benchmark_frame_lies_in_a_hinted_quadrant(tmp_path):
    frame, ph, cfg = synth.config2(n_photons=200_000)                  # nzc = 64, the seeded positions of the benchmark's photons
    assert frame["r0"].size == 1 << 20
    got = hint_coverage(tmp_path, frame, ph)
    fine = float(frame["r0_size"].min())
    print("grid %d x %d buckets of %.6g x %.6g cm; %d of %d positions hinted, %d within 1e-6 of a quadrant face; %d of %d quadrants hinted"
          % (got["dim"] + got["width"] + (got["hinted"], got["points"], got["near_face"], got["quadrants_hinted"], got["quadrants"])))
    # the lower-quartile width is the fine cell's on both axes and the mesh has fewer than 4 M cells' worth of buckets: f0 = 1, 2560 x 1024 (+ 1)
    assert fine == 3.125e7
    assert got["dim"] == (2561, 1025)
    assert got["width"][0] == pytest.approx(fine, rel=1e-12) and got["width"][1] == pytest.approx(fine, rel=1e-12)
    # bucket faces half a fine cell off the mesh: the mesh starts half a bucket above the grid's origin
    assert (frame["r0"] - 0.5 * frame["r0_size"]).min() - got["org"][0] == pytest.approx(0.5 * fine, rel=1e-9)
    assert got["points"] == 200_000
    assert got["hinted"] == got["points"]
    assert got["near_face"] < 20                                       # ~1e-5 per position: 4 faces x 1e-6 per axis, two axes
