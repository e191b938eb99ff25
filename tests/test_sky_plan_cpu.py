"""The host's rules for a sky observation (mcrat_amd/csrc/sky_plan.hpp) on the CPU: every refusal with its text and in its order, the block's
layout, the rule that picks the accumulation path on both sides of its LDS boundary, the grid, the match table's hash, and the per-photon functions
the kernel uses -- accepted, t_det, xy, bin -- against the definitions restated in NumPy (tests/sky_checker.py): integers exactly, doubles (%.17g)
for equality.  They are plain C++: a small driver is compiled with g++ and what it prints is compared.  The same driver is built a second time
with -fsanitize=address,undefined and run once."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sky_checker as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(OK, NO_BINS, AXES_MISMATCH, TOO_MANY_BINS, DIR_NOT_FINITE, DIR_NOT_UNIT, BAD_CONE, AXES_NULL, AXES_NOT_FINITE, AXES_NOT_UNIT, AXES_NOT_ORTHOGONAL,
 T_NOT_FINITE, T_NOT_ASCENDING, E_NOT_FINITE, E_NOT_ASCENDING, X_NOT_FINITE, X_NOT_ASCENDING, Y_NOT_FINITE, Y_NOT_ASCENDING, STAGING_TOO_LARGE,
 BAD_PATH_SWITCH, LDS_FORCED_TOO_LARGE) = range(22)
PATH_LDS, PATH_GLOBAL = 1, 2
LDS_BUDGET = 80 * 1024            # half of gfx950's 160 KiB per CU: two workgroups share a CU
MATCH_BYTES = 4 * 2048            # the global path: a 2048-byte table for each of a workgroup's four wavefronts
BLOCK, MAX_GRID = 256, 2048

TEXTS = {
    NO_BINS: "observe_sky: n_obs, n_t and n_e must each be at least 1",
    AXES_MISMATCH: "observe_sky: n_x and n_y must both be 0 (no image axes) or both at least 1",
    TOO_MANY_BINS: "observe_sky: n_obs * n_t * n_e * n_y * n_x overflows an int",
    DIR_NOT_FINITE: "observe_sky: an observer's direction holds a value that is not finite",
    DIR_NOT_UNIT: "observe_sky: an observer's direction is not a unit vector (to 1e-12)",
    BAD_CONE: "observe_sky: cos_acc must be a number in [-1, 1]",
    AXES_NULL: "observe_sky: image axes need the sky-plane vectors x0 .. x2 and y0 .. y2",
    AXES_NOT_FINITE: "observe_sky: a sky-plane vector holds a value that is not finite",
    AXES_NOT_UNIT: "observe_sky: a sky-plane vector is not a unit vector (to 1e-12)",
    AXES_NOT_ORTHOGONAL: "observe_sky: the sky-plane vectors and the direction are not orthogonal (to 1e-12)",
    T_NOT_FINITE: "observe_sky: t_edges holds a value that is not finite",
    T_NOT_ASCENDING: "observe_sky: t_edges is not strictly ascending",
    E_NOT_FINITE: "observe_sky: e_edges holds a value that is not finite",
    E_NOT_ASCENDING: "observe_sky: e_edges is not strictly ascending",
    X_NOT_FINITE: "observe_sky: x_edges holds a value that is not finite",
    X_NOT_ASCENDING: "observe_sky: x_edges is not strictly ascending",
    Y_NOT_FINITE: "observe_sky: y_edges holds a value that is not finite",
    Y_NOT_ASCENDING: "observe_sky: y_edges is not strictly ascending",
    STAGING_TOO_LARGE: "observe_sky: the edges and the observers' vectors do not fit the kernel's LDS budget",
    BAD_PATH_SWITCH: "observe_sky: MCRAT_HIP_SKY_PATH must be lds or global",
    LDS_FORCED_TOO_LARGE: "observe_sky: MCRAT_HIP_SKY_PATH=lds, but the cube does not fit the kernel's LDS budget",
}

INF, NAN = float("inf"), float("nan")
Z, X, Y = [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]
TILT = 1e-11                      # sin of a tilt that the 1e-12 conditions must catch: (TILT, 0, 1) is unit to 1e-22 and 1e-11 off orthogonal to X


def plan(n_obs=1, n=(Z,), cos_acc=(0.5,), ex=(X,), ey=(Y,), n_t=4, te="ramp", n_e=8, ee="ramp", n_x=5, xe="ramp", n_y=3, ye="ramp", env=None):
    """one case: the arrays as they are handed over; "ramp" stands for 0, 1, 2, ... of the length the count asks for; ex / ey None: a NULL pointer"""
    return dict(n_obs=n_obs, n=n, cos_acc=cos_acc, ex=ex, ey=ey, n_t=n_t, te=te, n_e=n_e, ee=ee, n_x=n_x, xe=xe, n_y=n_y, ye=ye, env=env)


PLANS = {
    "image": plan(),
    "curve": plan(n_x=0, n_y=0, ex=None, ey=None),
    "three": plan(n_obs=3, n=(Z, X, Y), cos_acc=(1.0, -1.0, 0.0), ex=(X, Y, Z), ey=(Y, Z, X)),
    # 7 planes * 8 B * bins + 8 * staged doubles + 16: 38 x 38 pixels are 80 864 + 736 + 16 = 81 616 of the 81 920, 39 x 38 are 82 992 + 744 + 16
    "lds_last": plan(n_t=1, n_e=1, n_x=38, n_y=38),
    "global_first": plan(n_t=1, n_e=1, n_x=39, n_y=38),
    "lds_last_curve": plan(n_t=2, n_e=682, n_x=0, n_y=0),          # 76 384 + 8 * (4 + 3 + 683) + 16: the budget exactly
    "global_first_curve": plan(n_t=2, n_e=683, n_x=0, n_y=0),
    "bench_image": plan(n_t=8, n_e=1, n_x=256, n_y=256),
    "forced_global": plan(env="global"),
    "forced_lds": plan(env="lds"),
    "empty_switch": plan(env=""),
    "forced_lds_too_large": plan(n_t=1, n_e=1, n_x=39, n_y=38, env="lds"),
    "forced_global_beyond": plan(n_t=1, n_e=1, n_x=39, n_y=38, env="global"),
    "bad_switch": plan(env="hbm"),
    "bad_switch_upper": plan(env="LDS"),
    "staging_last": plan(n_t=9200, n_e=1, n_x=0, n_y=0),           # 8 * (4 + 9201 + 2) + 16 + 8192 = 81 864
    "staging_too_large": plan(n_t=9208, n_e=1, n_x=0, n_y=0),      # 8 * (4 + 9209 + 2) + 16 + 8192 = 81 928
    "no_observer": plan(n_obs=0, n=(), cos_acc=(), ex=(), ey=()),
    "no_t_bin": plan(n_t=0, te=[0.0]),
    "negative_e_bins": plan(n_e=-1, ee=[]),
    "x_without_y": plan(n_y=0, ye=[0.0]),
    "y_without_x": plan(n_x=0, xe=[0.0]),
    "negative_x": plan(n_x=-1, xe=[], n_y=0, ye=[0.0]),
    "product_overflow": plan(n_t=65536, te=[], n_e=32768, ee=[], n_x=0, n_y=0),                 # 2^31 (the arrays are not looked at)
    "image_overflow": plan(n_t=16, n_e=16, n_x=4096, xe=[], n_y=2048, ye=[]),                   # 2^31 with the image axes
    "image_last_int": plan(n_t=1, n_e=1, n_x=46340, n_y=46340, env="lds"),                     # 46340^2 < 2^31: the product passes; its 92 682 edges cannot be staged
    "dir_nan": plan(n=([NAN, 0.0, 1.0],)),
    "dir_inf": plan(n=([0.0, INF, 0.0],)),
    "dir_long": plan(n=([0.0, 0.0, 1.0 + 1e-11],)),
    "dir_zero": plan(n=([0.0, 0.0, 0.0],)),
    "dir_second": plan(n_obs=2, n=(Z, [0.6, 0.8, 0.1]), cos_acc=(0.5, 0.5), ex=(X, X), ey=(Y, Y)),
    "dir_just_unit": plan(n=([0.0, 0.0, 1.0 + 1e-13],)),           # |n.n - 1| = 2e-13: inside the condition
    "cone_nan": plan(cos_acc=(NAN,)),
    "cone_above": plan(cos_acc=(1.0 + 1e-15,)),
    "cone_below": plan(cos_acc=(-1.5,)),
    "cone_inf": plan(cos_acc=(INF,)),
    "axes_null_x": plan(ex=None),
    "axes_null_y": plan(ey=None),
    "axes_nan": plan(ey=([0.0, NAN, 0.0],)),
    "axes_long": plan(ex=([1.0 + 1e-11, 0.0, 0.0],)),
    "axes_tilted": plan(ex=([1.0, 0.0, -TILT],), n=([TILT, 0.0, 1.0],), ey=([0.0, 1.0, TILT],)),        # ex.n = 0 exactly, ey.n = 1e-11
    "axes_parallel": plan(ex=(X,), ey=(X,)),
    "axes_x_not_normal": plan(n=(Z,), ex=([1.0, 0.0, TILT],), ey=(Y,)),
    "t_inf": plan(te=[0.0, 1.0, 2.0, 3.0, INF]),
    "t_equal": plan(te=[0.0, 1.0, 1.0, 3.0, 4.0]),
    "e_nan": plan(n_e=2, ee=[1.0, NAN, 2.0]),
    "e_descending": plan(n_e=2, ee=[1.0, 3.0, 2.0]),
    "x_minus_inf": plan(n_x=2, xe=[-INF, 0.0, 1.0]),
    "x_equal": plan(n_x=2, xe=[0.0, 0.0, 1.0]),
    "y_nan": plan(n_y=1, ye=[0.0, NAN]),
    "y_descending": plan(n_y=1, ye=[1.0, 0.0]),
    # two faults at once: the first in the order decides
    "counts_before_axes": plan(n_t=0, te=[0.0], n_y=0, ye=[0.0]),
    "axes_before_product": plan(n_t=65536, te=[], n_e=65536, ee=[], n_y=0, ye=[0.0]),
    "product_before_dir": plan(n=([NAN, 0.0, 1.0],), n_t=65536, te=[], n_e=32768, ee=[], n_x=0, n_y=0),
    "finite_before_unit": plan(n_obs=2, n=([0.0, 0.0, 2.0], [NAN, 0.0, 0.0]), cos_acc=(0.5, 0.5), ex=(X, X), ey=(Y, Y)),   # every direction finite, before any unit
    "dir_before_cone": plan(n=([0.0, 0.0, 2.0],), cos_acc=(2.0,)),
    "cone_before_axes": plan(cos_acc=(2.0,), ex=None),
    "null_before_finite": plan(ex=None, ey=([NAN, 0.0, 0.0],)),
    "axes_finite_before_unit": plan(ex=([2.0, 0.0, 0.0],), ey=([0.0, NAN, 0.0],)),
    "axes_unit_before_orthogonal": plan(ex=(X,), ey=([2.0, 0.0, 0.0],)),
    "axes_before_edges": plan(ex=(X,), ey=(X,), te=[0.0, 1.0, 1.0, 3.0, 4.0]),
    "t_finite_before_ascending": plan(te=[1.0, 0.0, 2.0, 3.0, NAN]),
    "t_before_e": plan(te=[0.0, 0.0, 1.0, 2.0, 3.0], n_e=2, ee=[NAN, 1.0, 2.0]),
    "e_before_x": plan(n_e=2, ee=[1.0, 1.0, 2.0], n_x=2, xe=[NAN, 0.0, 1.0]),
    "x_before_y": plan(n_x=2, xe=[0.0, 0.0, 1.0], n_y=1, ye=[NAN, 0.0]),
    "edges_before_staging": plan(n_t=9208, te="ramp_descending", n_e=1, n_x=0, n_y=0),
    "staging_before_switch": plan(n_t=9208, n_e=1, n_x=0, n_y=0, env="hbm"),
    "switch_before_forced": plan(n_t=1, n_e=1, n_x=39, n_y=38, env="Lds"),
    "no_image_ignores_axes": plan(n_x=0, n_y=0, ex=([NAN, 0.0, 0.0],), ey=None, xe=[NAN], ye=[NAN]),     # without image axes nothing of them is read
}
REFUSED = {
    "forced_lds_too_large": LDS_FORCED_TOO_LARGE, "bad_switch": BAD_PATH_SWITCH, "bad_switch_upper": BAD_PATH_SWITCH, "staging_too_large": STAGING_TOO_LARGE,
    "no_observer": NO_BINS, "no_t_bin": NO_BINS, "negative_e_bins": NO_BINS, "x_without_y": AXES_MISMATCH, "y_without_x": AXES_MISMATCH,
    "negative_x": AXES_MISMATCH, "product_overflow": TOO_MANY_BINS, "image_overflow": TOO_MANY_BINS, "image_last_int": STAGING_TOO_LARGE,
    "dir_nan": DIR_NOT_FINITE, "dir_inf": DIR_NOT_FINITE, "dir_long": DIR_NOT_UNIT, "dir_zero": DIR_NOT_UNIT, "dir_second": DIR_NOT_UNIT,
    "cone_nan": BAD_CONE, "cone_above": BAD_CONE, "cone_below": BAD_CONE, "cone_inf": BAD_CONE, "axes_null_x": AXES_NULL, "axes_null_y": AXES_NULL,
    "axes_nan": AXES_NOT_FINITE, "axes_long": AXES_NOT_UNIT, "axes_tilted": AXES_NOT_ORTHOGONAL, "axes_parallel": AXES_NOT_ORTHOGONAL,
    "axes_x_not_normal": AXES_NOT_ORTHOGONAL, "t_inf": T_NOT_FINITE, "t_equal": T_NOT_ASCENDING, "e_nan": E_NOT_FINITE, "e_descending": E_NOT_ASCENDING,
    "x_minus_inf": X_NOT_FINITE, "x_equal": X_NOT_ASCENDING, "y_nan": Y_NOT_FINITE, "y_descending": Y_NOT_ASCENDING,
    "counts_before_axes": NO_BINS, "axes_before_product": AXES_MISMATCH, "product_before_dir": TOO_MANY_BINS, "finite_before_unit": DIR_NOT_FINITE,
    "dir_before_cone": DIR_NOT_UNIT, "cone_before_axes": BAD_CONE, "null_before_finite": AXES_NULL, "axes_finite_before_unit": AXES_NOT_FINITE,
    "axes_unit_before_orthogonal": AXES_NOT_UNIT, "axes_before_edges": AXES_NOT_ORTHOGONAL, "t_finite_before_ascending": T_NOT_FINITE,
    "t_before_e": T_NOT_ASCENDING, "e_before_x": E_NOT_ASCENDING, "x_before_y": X_NOT_ASCENDING, "edges_before_staging": T_NOT_ASCENDING,
    "staging_before_switch": STAGING_TOO_LARGE, "switch_before_forced": BAD_PATH_SWITCH,
}

N_PHOTONS, N_OBS = 2000, 3

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sky_plan.hpp"
using namespace mcrat;
typedef std::vector<double> V;

static V ramp(int n) { V v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }
static V ramp_descending(int n) { V v; for (int k = 0; k <= n; ++k) v.push_back((double)-k); return v; }
static const double *col(const V &v, int k, int n_obs) { return v.data() + (size_t)k * (n_obs > 0 ? n_obs : 0); }
// n, ex, ey: component-major [3][n_obs]; has_x / has_y 0: NULL pointers
static void plan(const char *name, int n_obs, V n, V ca, int has_x, V ex, int has_y, V ey, int n_t, V te, int n_e, V ee, int n_x, V xe, int n_y, V ye, const char *env)
{
    SkyArgs a{};
    a.n_obs = n_obs; a.n0 = col(n, 0, n_obs); a.n1 = col(n, 1, n_obs); a.n2 = col(n, 2, n_obs); a.cos_acc = ca.data();
    if (has_x) { a.x0 = col(ex, 0, n_obs); a.x1 = col(ex, 1, n_obs); a.x2 = col(ex, 2, n_obs); }
    if (has_y) { a.y0 = col(ey, 0, n_obs); a.y1 = col(ey, 1, n_obs); a.y2 = col(ey, 2, n_obs); }
    a.n_t = n_t; a.t_edges = te.data(); a.n_e = n_e; a.e_edges = ee.data(); a.n_x = n_x; a.x_edges = xe.data(); a.n_y = n_y; a.y_edges = ye.data();
    SkyPlan p;
    const SkyRefusal why = sky_plan(a, env, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why == SKY_OK)
        printf("planv_%s: %d %d %d %zu %zu %zu %zu %zu %d %d %d %d\n", name, (int)p.path, (int)p.image, p.n_bins, p.cube_bytes, p.out_bytes, p.staged_doubles,
               p.staged_bytes, p.lds_bytes, p.groups_per_cu, sky_grid(p, 1, 256), sky_grid(p, 100000, 256), sky_grid(p, 2000000000, 304));
}
static V read_doubles(FILE *f, size_t n)
{
    V v(n);
    if (fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
@CASES@
    for (int k = 1; k <= (int)SKY_LDS_FORCED_TOO_LARGE; ++k) printf("text_%d:%s\n", k, sky_refusal_text((SkyRefusal)k));
    printf("constants: %d %d %d %zu %d\n", SKY_BLOCK, SKY_MAX_GRID, SKY_MATCH_BITS, SKY_MATCH_BYTES, (int)(SKY_UNIT_TOLERANCE == 1e-12));
    printf("bin_index: %zu %zu %zu %zu\n", sky_bin_index(0, 0, 0, 0, 0, 4, 8, 3, 5), sky_bin_index(0, 0, 0, 0, 1, 4, 8, 3, 5), sky_bin_index(0, 0, 0, 1, 0, 4, 8, 3, 5),
           sky_bin_index(2, 3, 7, 2, 4, 4, 8, 3, 5));
    printf("hash:");
    for (int b : {0, 1, 2, 3, 64, 1000, 65535, 65536, 524287, 1000000, 2147483647}) printf(" %u", sky_match_hash(b));
    printf("\n");
    if (argc < 2) return 0;
    // the photons: header {n, n_obs, n_t, n_e, n_x, n_y} as doubles, then time_now, r0, r1, r2, p0, p1, p2, p3 [n each], n [3][n_obs], cos_acc, ex, ey
    // [3][n_obs], the four edge arrays
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const V head = read_doubles(f, 6);
    const size_t n = (size_t)head[0];
    const int n_obs = (int)head[1], n_t = (int)head[2], n_e = (int)head[3], n_x = (int)head[4], n_y = (int)head[5];
    const V tn = read_doubles(f, n), r0 = read_doubles(f, n), r1 = read_doubles(f, n), r2 = read_doubles(f, n), p0 = read_doubles(f, n), p1 = read_doubles(f, n),
            p2 = read_doubles(f, n), p3 = read_doubles(f, n), nv = read_doubles(f, 3 * n_obs), ca = read_doubles(f, n_obs), ex = read_doubles(f, 3 * n_obs),
            ey = read_doubles(f, 3 * n_obs), te = read_doubles(f, n_t + 1), ee = read_doubles(f, n_e + 1), xe = read_doubles(f, n_x + 1), ye = read_doubles(f, n_y + 1);
    fclose(f);
    for (size_t i = 0; i < n; ++i)
        for (int o = 0; o < n_obs; ++o) {
            const double n0 = nv[o], n1 = nv[n_obs + o], n2 = nv[2 * n_obs + o];
            const double t = sky_t_det(tn[i], r0[i], r1[i], r2[i], n0, n1, n2), e = observe_energy(p0[i]);
            double X, Y;
            sky_xy(r0[i], r1[i], r2[i], ex[o], ex[n_obs + o], ex[2 * n_obs + o], ey[o], ey[n_obs + o], ey[2 * n_obs + o], X, Y);
            printf("ph: %d %.17g %.17g %.17g %.17g %d %d\n", (int)sky_accepted(p0[i], p1[i], p2[i], p3[i], n0, n1, n2, ca[o]), t, e, X, Y,
                   sky_bin(o, te.data(), n_t, t, ee.data(), n_e, e, xe.data(), n_x, X, ye.data(), n_y, Y),
                   sky_bin(o, te.data(), n_t, t, ee.data(), n_e, e, nullptr, 0, NAN, nullptr, 0, NAN));
        }
    return 0;
}
'''

HASH_BINS = [0, 1, 2, 3, 64, 1000, 65535, 65536, 524287, 1000000, 2147483647]


def match_hash(b):
    """the header's sky_match_hash restated: Fibonacci hashing to 11 bits (tests/test_gpu_sky.py uses this replica to build collisions)"""
    return ((int(b) * 2654435761) & 0xFFFFFFFF) >> (32 - 11)


def _vec(v, n):
    if isinstance(v, str):
        return "%s(%d)" % (v, n)
    lit = {INF: "INFINITY", -INF: "-INFINITY"}
    return "V{%s}" % ", ".join("NAN" if x != x else lit.get(x, repr(float(x))) for x in v)


def _vec3(rows):
    """per-observer vectors -> component-major"""
    return _vec([r[k] for k in range(3) for r in rows], 0) if rows else "V{}"


def _cases():
    lines = []
    for name, c in PLANS.items():
        lines.append('plan("%s", %d, %s, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %s);' % (
            name, c["n_obs"], _vec3(c["n"]), _vec(c["cos_acc"], 0), c["ex"] is not None, _vec3(c["ex"] or ()), c["ey"] is not None, _vec3(c["ey"] or ()),
            c["n_t"], _vec(c["te"], c["n_t"]), c["n_e"], _vec(c["ee"], c["n_e"]), c["n_x"], _vec(c["xe"], c["n_x"]), c["n_y"], _vec(c["ye"], c["n_y"]),
            "nullptr" if c["env"] is None else '"%s"' % c["env"]))
    return "\n".join("    " + l for l in lines)


def photons():
    """~2000 seeded photons of a jet that is not axisymmetric and 3 observers -- one on the axis, two off it at different azimuths with overlapping
    cones; some edges are the exact t_det, e, X and Y of chosen photons"""
    ph = S.jet_photons(20250301, N_PHOTONS)
    g = np.random.default_rng(7)
    tn = g.uniform(300.0, 400.0, N_PHOTONS)
    n, cos_acc, ex, ey = S.observers([0.0, 0.2, 0.25], [0.0, 0.4, 1.0], [0.25, 0.2, 0.2])
    wide = S.per_photon(ph, n, cos_acc, [-1e9, 1e9], [0.0, 1e300], tn, ex, ey, [-1e300, 1e300], [-1e300, 1e300])
    te = np.unique(np.concatenate([np.linspace(wide["t"].min() - 1.0, np.percentile(wide["t"], 90), 12), wide["t"][1, [5, 17, 900]]]))
    ee = np.unique(np.concatenate([10.0 ** np.linspace(-9.5, -4.2, 20), wide["e"][0, [3, 11, 1200]]]))
    xe = np.unique(np.concatenate([np.linspace(-2.5e12, 2.5e12, 9), wide["X"][2, [8, 21]]]))
    ye = np.unique(np.concatenate([np.linspace(-2.0e12, 3.0e12, 6), wide["Y"][0, [13, 34]]]))
    return dict(ph=ph, tn=tn, n=n, cos_acc=cos_acc, ex=ex, ey=ey, te=te, ee=ee, xe=xe, ye=ye)


def _build(d, src, name, extra):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("sky_plan")
    src, data = d / "driver.cpp", d / "photons.bin"
    src.write_text(DRIVER.replace("@CASES@", _cases()))
    q = photons()
    head = np.array([N_PHOTONS, N_OBS] + [len(q[k]) - 1 for k in ("te", "ee", "xe", "ye")], dtype=np.float64)
    cols = [q["tn"]] + [q["ph"][k] for k in ("r0", "r1", "r2", "p0", "p1", "p2", "p3")]
    np.concatenate([head] + cols + [q["n"].ravel(), q["cos_acc"], q["ex"].ravel(), q["ey"].ravel(), q["te"], q["ee"], q["xe"], q["ye"]]).tofile(data)
    return d, src, data


@pytest.fixture(scope="module")
def text(built):
    d, src, data = built
    return subprocess.run([str(_build(d, src, "driver", [])), str(data)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def out(text):
    res = {"ph": []}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        if key == "ph":
            res["ph"].append(vals.split())
        else:
            res[key] = vals if key.startswith("text_") else [int(v) for v in vals.split()]
    return res


def plan_rule(c):
    """sky_plan restated: the checks in their order, the layout, the path, the grid"""
    def edges(v, n):
        if v == "ramp":
            return [float(k) for k in range(n + 1)]
        if v == "ramp_descending":
            return [float(-k) for k in range(n + 1)]
        return list(v)
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    n_obs, n_t, n_e, n_x, n_y = c["n_obs"], c["n_t"], c["n_e"], c["n_x"], c["n_y"]
    if n_obs < 1 or n_t < 1 or n_e < 1:
        return NO_BINS, None
    if not ((n_x == 0 and n_y == 0) or (n_x >= 1 and n_y >= 1)):
        return AXES_MISMATCH, None
    image = n_x >= 1
    n_bins = n_obs * n_t * n_e * (n_y * n_x if image else 1)
    if n_bins > 2 ** 31 - 1:
        return TOO_MANY_BINS, None
    if not all(np.isfinite(v).all() for v in c["n"]):
        return DIR_NOT_FINITE, None
    if any(abs(dot(v, v) - 1.0) > 1e-12 for v in c["n"]):
        return DIR_NOT_UNIT, None
    if not all(-1.0 <= a <= 1.0 for a in c["cos_acc"]):
        return BAD_CONE, None
    if image:
        if c["ex"] is None or c["ey"] is None:
            return AXES_NULL, None
        if not all(np.isfinite(v).all() for v in tuple(c["ex"]) + tuple(c["ey"])):
            return AXES_NOT_FINITE, None
        if any(abs(dot(v, v) - 1.0) > 1e-12 for v in tuple(c["ex"]) + tuple(c["ey"])):
            return AXES_NOT_UNIT, None
        if any(abs(dot(x, n)) > 1e-12 or abs(dot(y, n)) > 1e-12 or abs(dot(x, y)) > 1e-12 for n, x, y in zip(c["n"], c["ex"], c["ey"])):
            return AXES_NOT_ORTHOGONAL, None
    axes = [(edges(c["te"], n_t), T_NOT_FINITE, T_NOT_ASCENDING), (edges(c["ee"], n_e), E_NOT_FINITE, E_NOT_ASCENDING)]
    if image:
        axes += [(edges(c["xe"], n_x), X_NOT_FINITE, X_NOT_ASCENDING), (edges(c["ye"], n_y), Y_NOT_FINITE, Y_NOT_ASCENDING)]
    for e, not_finite, not_ascending in axes:
        if not all(np.isfinite(e)):
            return not_finite, None
        if not all(a < b for a, b in zip(e[:-1], e[1:])):
            return not_ascending, None
    cube = 7 * 8 * n_bins                                        # count, W, WE, I, Q, U, V: 8 bytes each
    staged_doubles = (10 if image else 4) * n_obs + n_t + 1 + n_e + 1 + (n_x + 1 + n_y + 1 if image else 0)
    staged = 8 * staged_doubles + 2 * 8 * n_obs                  # ... and the workgroup's two counters per observer
    if staged + MATCH_BYTES > LDS_BUDGET:
        return STAGING_TOO_LARGE, None
    if c["env"] not in (None, "", "lds", "global"):
        return BAD_PATH_SWITCH, None
    fits = staged + cube <= LDS_BUDGET
    if c["env"] == "lds" and not fits:
        return LDS_FORCED_TOO_LARGE, None
    path = {"lds": PATH_LDS, "global": PATH_GLOBAL}.get(c["env"]) or (PATH_LDS if fits else PATH_GLOBAL)
    lds = staged + (cube if path == PATH_LDS else MATCH_BYTES)
    groups = 2 if path == PATH_LDS else min(2 * LDS_BUDGET // lds, 8)
    grid = lambda slots, cus: min(-(-slots // BLOCK), cus * groups, MAX_GRID)
    return OK, [path, int(image), n_bins, cube, cube + 16 * n_obs, staged_doubles, staged, lds, groups, grid(1, 256), grid(100000, 256), grid(2000000000, 304)]


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan(out, name):
    why, plan_ = plan_rule(PLANS[name])
    assert out["plan_" + name] == [why]
    if why == OK:
        assert out["planv_" + name] == plan_
    else:
        assert "planv_" + name not in out


def test_plan_cases_are_what_they_are_meant_to_be(out):
    """... so that the table above cannot drift into testing nothing: every refusal occurs, where two faults meet the first in the order wins, and the
    path changes exactly at the LDS budget"""
    for name, why in REFUSED.items():
        assert out["plan_" + name] == [why], name
    assert set(REFUSED.values()) == set(TEXTS)
    for name in set(PLANS) - set(REFUSED):
        assert out["plan_" + name] == [OK], name
    assert out["constants"] == [BLOCK, MAX_GRID, 11, MATCH_BYTES, 1] and 2 * LDS_BUDGET == 160 * 1024
    #                              path   image bins  cube   out    doubles staged lds    groups, grids
    assert out["planv_image"] == [PATH_LDS, 1, 480, 26880, 26896, 34, 288, 27168, 2, 1, 391, 608]
    assert out["planv_curve"] == [PATH_LDS, 0, 32, 1792, 1808, 18, 160, 1952, 2, 1, 391, 608]
    assert out["planv_lds_last"][0] == PATH_LDS and out["planv_global_first"][0] == PATH_GLOBAL
    assert out["planv_lds_last"][7] <= LDS_BUDGET < out["planv_lds_last"][7] + 7 * 8 * 38                   # one more column of pixels would not fit
    assert out["planv_lds_last_curve"][7] == LDS_BUDGET                                                      # the budget exactly: still LDS
    assert out["planv_global_first"][6] + out["planv_global_first"][3] > LDS_BUDGET
    assert out["planv_global_first"][7] == out["planv_global_first"][6] + MATCH_BYTES                       # the global path: the staged inputs and the tables
    assert out["planv_global_first"][8:] == [8, 1, 391, MAX_GRID]                                           # eight per CU, and never more than the largest grid
    assert out["planv_lds_last_curve"][0] == PATH_LDS and out["planv_global_first_curve"][0] == PATH_GLOBAL
    assert out["planv_bench_image"][:4] == [PATH_GLOBAL, 1, 8 * 256 * 256, 56 * 8 * 256 * 256]
    assert out["planv_forced_global"][0] == PATH_GLOBAL and out["planv_forced_lds"][0] == PATH_LDS and out["planv_forced_global_beyond"][0] == PATH_GLOBAL
    assert out["planv_empty_switch"] == out["planv_image"]
    assert out["planv_staging_last"][0] == PATH_GLOBAL and out["planv_staging_last"][7] == 81864
    assert out["planv_three"][1:3] == [1, 3 * 480] and out["planv_no_image_ignores_axes"] == out["planv_curve"]
    assert out["planv_dir_just_unit"] == out["planv_image"]


def test_refusal_texts(out):
    for why, t in TEXTS.items():
        assert out["text_%d" % why] == t, why
    assert len(TEXTS) == LDS_FORCED_TOO_LARGE and len(set(TEXTS.values())) == len(TEXTS)


def test_layout(out):
    assert out["bin_index"] == [0, 1, 5, ((((2 * 4 + 3) * 8 + 7) * 3 + 2) * 5 + 4)]       # x fastest, then y, energy, time, observer


def test_match_table_hash(out):
    """printed by the header, so that the replica the GPU test builds its collisions with is pinned"""
    assert out["hash"] == [match_hash(b) for b in HASH_BINS]
    assert out["hash"][0] == 0 and max(out["hash"]) < 2048 and len(set(out["hash"])) > 8


def test_per_photon_functions_equal_the_numpy_restatement(out):
    q = photons()
    rows = out["ph"]
    assert len(rows) == N_PHOTONS * N_OBS
    col = lambda k, conv: np.array([conv(r[k]) for r in rows]).reshape(N_PHOTONS, N_OBS).T
    got_acc, got_t, got_e, got_x, got_y, got_bin, got_curve = col(0, int), col(1, float), col(2, float), col(3, float), col(4, float), col(5, int), col(6, int)
    ph = q["ph"]
    w = S.per_photon(ph, q["n"], q["cos_acc"], q["te"], q["ee"], q["tn"], q["ex"], q["ey"], q["xe"], q["ye"])
    assert (got_acc == w["accepted"]).all()
    for got, k in ((got_t, "t"), (got_e, "e"), (got_x, "X"), (got_y, "Y")):
        assert (got == w[k]).all(), k                                  # bit for bit (%.17g round-trips a double)
    n_t, n_e, n_x, n_y = (len(q[k]) - 1 for k in ("te", "ee", "xe", "ye"))
    o = np.arange(N_OBS)[:, None]
    everything = (w["it"] >= 0) & (w["ie"] >= 0) & (w["ix"] >= 0) & (w["iy"] >= 0)      # (the bin does not ask whether the photon is accepted)
    want_bin = np.where(everything, (((o * n_t + w["it"]) * n_e + w["ie"]) * n_y + w["iy"]) * n_x + w["ix"], -1)
    want_curve = np.where((w["it"] >= 0) & (w["ie"] >= 0), (o * n_t + w["it"]) * n_e + w["ie"], -1)
    assert (got_bin == want_bin).all() and (got_curve == want_curve).all()
    # the sample means something: every observer accepts some photons and not all, cones overlap, every axis has photons inside and outside, and
    # the photons whose coordinate IS an edge sit in the bin that edge opens
    acc = w["accepted"]
    assert (acc.sum(axis=1) > 50).all() and (acc.sum(axis=1) < N_PHOTONS - 50).all() and (acc.sum(axis=0) >= 2).sum() > 50
    for k in ("it", "ie", "ix", "iy"):
        assert (w[k] < 0).sum() > 10 and (w[k] >= 0).sum() > 1000, k
    for i in (5, 17, 900):
        assert q["te"][w["it"][1, i]] == w["t"][1, i]
    for i in (3, 11, 1200):
        assert q["ee"][w["ie"][0, i]] == w["e"][0, i]
    for i in (8, 21):
        assert q["xe"][w["ix"][2, i]] == w["X"][2, i]
    for i in (13, 34):
        assert q["ye"][w["iy"][0, i]] == w["Y"][0, i]


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
