"""The host's rules for a resampled sky observation (mcrat_amd/csrc/resample_plan.hpp) on the CPU: every refusal with its text and in its order,
the block's layout, the bin index with the replica axis, the rule that picks the path on both sides of each LDS boundary -- the whole cube, one
replica, one replica and one bin more -- the slice count and the grid, and the multiplicities and the Stokes rotation against the definitions restated
in NumPy (tests/resample_checker.py): integers exactly, doubles (%.17g) for equality.  Plain C++: a small driver is compiled with g++ and what it
prints is compared.  The same driver is built a second time with -fsanitize=address,undefined as a stand-alone program and run once.  (The pattern
of tests/test_sky_plan_cpu.py, whose cases and restated sky checks are used for the observers' part.)"""
import shutil
import subprocess

import numpy as np
import pytest

from tests import resample_checker as R
from tests import test_sky_plan_cpu as P
from tests.test_sky_plan_cpu import INF, NAN, X, Y, Z, TILT

NONE, JACKKNIFE, BOOTSTRAP = 0, 1, 2
AS_STORED, SKY_PLANE = 0, 1
PATH_LDS, PATH_GLOBAL, PATH_SLICED = 1, 2, 3
(BAD_MODE, BAD_FRAME, N_REP_NOT_ONE, N_REP_TOO_SMALL, TOO_MANY_BINS, AXES_NULL, AXES_NOT_FINITE, AXES_NOT_UNIT, AXES_NOT_ORTHOGONAL, STAGING_TOO_LARGE,
 BAD_PATH_SWITCH, LDS_FORCED_TOO_LARGE, SLICED_FORCED_TOO_LARGE) = range(32, 45)
OK = 0
LDS_BUDGET, MATCH_BYTES, BLOCK, MAX_GRID, MAX_GRID_Y, MAX_SLICES = P.LDS_BUDGET, P.MATCH_BYTES, 256, 2048, 65535, 12
PREFIX = "observe_sky_resampled:"

TEXTS = {k: PREFIX + t[len("observe_sky:"):] for k, t in P.TEXTS.items() if k <= P.Y_NOT_ASCENDING}       # the observers' checks, this product's prefix
TEXTS.update({
    BAD_MODE: "observe_sky_resampled: mode must be MCRAT_HIP_RESAMPLE_NONE, _JACKKNIFE or _BOOTSTRAP",
    BAD_FRAME: "observe_sky_resampled: stokes_frame must be MCRAT_HIP_STOKES_AS_STORED or _SKY_PLANE",
    N_REP_NOT_ONE: "observe_sky_resampled: n_rep must be 1 with MCRAT_HIP_RESAMPLE_NONE",
    N_REP_TOO_SMALL: "observe_sky_resampled: n_rep must be at least 2 (jackknife groups, or the sample and one bootstrap replica)",
    TOO_MANY_BINS: "observe_sky_resampled: n_obs * n_rep * n_t * n_e * n_y * n_x overflows an int",
    AXES_NULL: "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE needs the sky-plane vectors x0 .. x2 and y0 .. y2",
    AXES_NOT_FINITE: "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE: a sky-plane vector holds a value that is not finite",
    AXES_NOT_UNIT: "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE: a sky-plane vector is not a unit vector (to 1e-12)",
    AXES_NOT_ORTHOGONAL: "observe_sky_resampled: MCRAT_HIP_STOKES_SKY_PLANE: the sky-plane vectors and the direction are not orthogonal (to 1e-12)",
    STAGING_TOO_LARGE: "observe_sky_resampled: the edges and the observers' vectors do not fit the kernel's LDS budget",
    BAD_PATH_SWITCH: "observe_sky_resampled: MCRAT_HIP_RESAMPLE_PATH must be lds, sliced or global",
    LDS_FORCED_TOO_LARGE: "observe_sky_resampled: MCRAT_HIP_RESAMPLE_PATH=lds, but the cube does not fit the kernel's LDS budget",
    SLICED_FORCED_TOO_LARGE: "observe_sky_resampled: MCRAT_HIP_RESAMPLE_PATH=sliced, but one replica's part of the cube does not fit the kernel's LDS budget",
})


def plan(mode=JACKKNIFE, n_rep=2, frame=AS_STORED, **sky):
    c = P.plan(**sky)
    c.update(mode=mode, n_rep=n_rep, frame=frame)
    return c


def curve(**kw):
    """no image axes, no sky-plane vectors"""
    kw.setdefault("ex", None)
    kw.setdefault("ey", None)
    return plan(n_x=0, n_y=0, **kw)


PLANS = {
    "image": plan(),
    "none": curve(mode=NONE, n_rep=1),
    "none_sky_plane": curve(mode=NONE, n_rep=1, frame=SKY_PLANE, ex=(X,), ey=(Y,)),            # ex and ey are staged without image axes
    "image_sky_plane": plan(frame=SKY_PLANE),
    "three": plan(n_obs=3, n=(Z, X, Y), cos_acc=(1.0, -1.0, 0.0), ex=(X, Y, Z), ey=(Y, Z, X), mode=BOOTSTRAP, n_rep=5),
    # the benchmark's shapes: 32 groups of a 32 x 32 light curve would be 32 slices of one replica, too many for a jackknife: global; 201 entries of
    # 8 x 16 are 19 slices of 11
    "bench_jackknife": curve(n_t=32, n_e=32, n_rep=32),
    "bench_bootstrap": curve(n_t=8, n_e=16, mode=BOOTSTRAP, n_rep=201),
    # the whole cube: 56 B * 2 replicas * n_e + 8 * (4 + 2 + n_e + 1) + 24 = 120 n_e + 80: 682 bins are the budget exactly, 683 two slices of one
    "lds_last": curve(n_t=1, n_e=682, n_rep=2),
    "sliced_first": curve(n_t=1, n_e=683, n_rep=2),
    # one replica: 56 n_e + 8 n_e + 80 <= 81920 up to n_e = 1278; one bin more and no replica fits
    "sliced_last": curve(n_t=1, n_e=1278, n_rep=3),
    "global_first": curve(n_t=1, n_e=1279, n_rep=3),
    # as many slices as the rule allows a jackknife, and one more; a bootstrap is sliced whatever their number
    "slices_12": curve(n_t=1, n_e=1000, n_rep=12),
    "slices_13": curve(n_t=1, n_e=1000, n_rep=13),
    "slices_13_forced": curve(n_t=1, n_e=1000, n_rep=13, env="sliced"),
    "slices_65_bootstrap": curve(n_t=1, n_e=1000, mode=BOOTSTRAP, n_rep=65),
    "forced_lds": plan(env="lds"),
    "forced_sliced_small": plan(env="sliced"),                 # one slice that holds every replica
    "forced_global": plan(env="global"),
    "forced_global_beyond": curve(n_t=1, n_e=1279, n_rep=3, env="global"),
    "empty_switch": plan(env=""),
    "staging_last": curve(n_t=9206, n_e=1),                     # 8 * (4 + 9207 + 2) + 24 + 8192 = 81 920
    "two_groups": curve(n_rep=2),
    "sample_and_one": curve(mode=BOOTSTRAP, n_rep=2),
    "stored_ignores_axes": curve(ex=([NAN, 0.0, 0.0],), ey=None),
    # refused -- the observers' checks come through with this product's prefix
    "no_observer": plan(n_obs=0, n=(), cos_acc=(), ex=(), ey=()),
    "dir_long": plan(n=([0.0, 0.0, 1.0 + 1e-11],)),
    "image_axes_null": plan(ex=None),
    "t_equal": plan(te=[0.0, 1.0, 1.0, 3.0, 4.0]),
    "y_descending": plan(n_y=1, ye=[1.0, 0.0]),
    "mode_3": plan(mode=3), "mode_negative": plan(mode=-1),
    "frame_2": plan(frame=2), "frame_negative": plan(frame=-1),
    "none_with_two": plan(mode=NONE, n_rep=2), "none_with_zero": plan(mode=NONE, n_rep=0),
    "jackknife_one": plan(n_rep=1), "bootstrap_one": plan(mode=BOOTSTRAP, n_rep=1), "bootstrap_negative": plan(mode=BOOTSTRAP, n_rep=-3),
    "product_overflow": curve(n_t=1024, n_e=1024, n_rep=2048),                    # 2^31 with the replicas (the sky cube alone fits)
    "sky_plane_null_x": curve(frame=SKY_PLANE, ey=(Y,)),
    "sky_plane_null_y": curve(frame=SKY_PLANE, ex=(X,)),
    "sky_plane_nan": curve(frame=SKY_PLANE, ex=(X,), ey=([0.0, NAN, 0.0],)),
    "sky_plane_long": curve(frame=SKY_PLANE, ex=([1.0 + 1e-11, 0.0, 0.0],), ey=(Y,)),
    "sky_plane_parallel": curve(frame=SKY_PLANE, ex=(X,), ey=(X,)),
    "sky_plane_tilted": curve(frame=SKY_PLANE, ex=([1.0, 0.0, -TILT],), n=([TILT, 0.0, 1.0],), ey=([0.0, 1.0, TILT],)),
    "staging_too_large": curve(n_t=9207, n_e=1),
    "bad_switch": plan(env="hbm"), "bad_switch_upper": plan(env="LDS"),
    "forced_lds_too_large": curve(n_t=1, n_e=683, n_rep=2, env="lds"),
    "forced_sliced_too_large": curve(n_t=1, n_e=1279, n_rep=3, env="sliced"),
    # two faults at once: the first in the order decides
    "sky_before_mode": plan(te=[0.0, 1.0, 1.0, 3.0, 4.0], mode=7),
    "mode_before_frame": plan(mode=7, frame=7),
    "frame_before_n_rep": plan(frame=7, n_rep=0),
    "n_rep_before_product": curve(n_t=1024, n_e=1024, mode=NONE, n_rep=2048),                  # 2^31 bins, but NONE with n_rep != 1 is refused first
    "product_before_axes": curve(n_t=1024, n_e=1024, n_rep=2048, frame=SKY_PLANE),
    "axes_before_staging": curve(n_t=9207, n_e=1, frame=SKY_PLANE, ex=(X,), ey=(X,)),
    "staging_before_switch": curve(n_t=9207, n_e=1, env="hbm"),
    "switch_before_forced": curve(n_t=1, n_e=683, n_rep=2, env="Lds"),
}
REFUSED = {
    "no_observer": P.NO_BINS, "dir_long": P.DIR_NOT_UNIT, "image_axes_null": P.AXES_NULL, "t_equal": P.T_NOT_ASCENDING, "y_descending": P.Y_NOT_ASCENDING,
    "mode_3": BAD_MODE, "mode_negative": BAD_MODE, "frame_2": BAD_FRAME, "frame_negative": BAD_FRAME, "none_with_two": N_REP_NOT_ONE,
    "none_with_zero": N_REP_NOT_ONE, "jackknife_one": N_REP_TOO_SMALL, "bootstrap_one": N_REP_TOO_SMALL, "bootstrap_negative": N_REP_TOO_SMALL,
    "product_overflow": TOO_MANY_BINS, "sky_plane_null_x": AXES_NULL, "sky_plane_null_y": AXES_NULL, "sky_plane_nan": AXES_NOT_FINITE,
    "sky_plane_long": AXES_NOT_UNIT, "sky_plane_parallel": AXES_NOT_ORTHOGONAL, "sky_plane_tilted": AXES_NOT_ORTHOGONAL,
    "staging_too_large": STAGING_TOO_LARGE, "bad_switch": BAD_PATH_SWITCH, "bad_switch_upper": BAD_PATH_SWITCH,
    "forced_lds_too_large": LDS_FORCED_TOO_LARGE, "forced_sliced_too_large": SLICED_FORCED_TOO_LARGE,
    "sky_before_mode": P.T_NOT_ASCENDING, "mode_before_frame": BAD_MODE, "frame_before_n_rep": BAD_FRAME, "n_rep_before_product": N_REP_NOT_ONE,
    "product_before_axes": TOO_MANY_BINS, "axes_before_staging": AXES_NOT_ORTHOGONAL, "staging_before_switch": STAGING_TOO_LARGE,
    "switch_before_forced": BAD_PATH_SWITCH,
}
OWN_CODES = sorted(set(TEXTS) - set(range(1, P.Y_NOT_ASCENDING + 1)))

IDENTITIES = [(0, 0, 0), (1, 0, 0), (0x1234567890ABCDEF, 3, 77), (2 ** 64 - 1, 1024, 2 ** 31 - 1), (42, 0, 1), (42, 1, 0)]      # (seed, rank, slot)
GROUPS, RHO_MAX, N_ROT = (2, 3, 64, 1000), 10, 400

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "resample_plan.hpp"
using namespace mcrat;
typedef std::vector<double> V;

static V ramp(int n) { V v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }
static const double *col(const V &v, int k, int n_obs) { return v.data() + (size_t)k * (n_obs > 0 ? n_obs : 0); }
static void plan(const char *name, int n_obs, V n, V ca, int has_x, V ex, int has_y, V ey, int n_t, V te, int n_e, V ee, int n_x, V xe, int n_y, V ye, const char *env,
                 int mode, int n_rep, int frame)
{
    ResampleArgs r{};
    SkyArgs &a = r.sky;
    a.n_obs = n_obs; a.n0 = col(n, 0, n_obs); a.n1 = col(n, 1, n_obs); a.n2 = col(n, 2, n_obs); a.cos_acc = ca.data();
    if (has_x) { a.x0 = col(ex, 0, n_obs); a.x1 = col(ex, 1, n_obs); a.x2 = col(ex, 2, n_obs); }
    if (has_y) { a.y0 = col(ey, 0, n_obs); a.y1 = col(ey, 1, n_obs); a.y2 = col(ey, 2, n_obs); }
    a.n_t = n_t; a.t_edges = te.data(); a.n_e = n_e; a.e_edges = ee.data(); a.n_x = n_x; a.x_edges = xe.data(); a.n_y = n_y; a.y_edges = ye.data();
    r.mode = mode; r.n_rep = n_rep; r.stokes_frame = frame;
    ResamplePlan p;
    const ResampleRefusal why = resample_plan(r, env, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why != RESAMPLE_OK) return;
    const ResampleLayout l = resample_layout(p, 5);
    const ResampleGrid g1 = resample_grid(p, 1, 256), g2 = resample_grid(p, 1000000, 256), g3 = resample_grid(p, 2000000000, 304);
    printf("planv_%s: %d %d %d %d %d %zu %zu %zu %zu %zu %d %d %zu %d %zu %zu %zu %zu %d %d %d %d %d %d\n", name, (int)p.path, (int)p.image, (int)p.axes, p.per_rep, p.n_bins,
           p.cube_bytes, p.out_bytes, p.staged_doubles, p.staged_bytes, p.replica_bytes, p.slice_reps, p.n_slices, p.lds_bytes, p.groups_per_cu,
           l.counters_offset, l.staged_offset, l.clocks_offset, l.total_bytes, g1.x, g1.y, g2.x, g2.y, g3.x, g3.y);
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
    char buf[RESAMPLE_TEXT_BYTES];
    for (int k : {@CODES@}) printf("text_%d:%s\n", k, resample_refusal_text((ResampleRefusal)k, buf));
    printf("constants: %d %d %d %d %zu %d %d %d\n", RESAMPLE_BLOCK, RESAMPLE_MAX_GRID, RESAMPLE_MAX_GRID_Y, RESAMPLE_JACKKNIFE_MAX_SLICES, RESAMPLE_MATCH_BYTES, RESAMPLE_COUNTERS,
           (int)RNG_RESAMPLE, RESAMPLE_POISSON_MAX);
    printf("bin_index: %zu %zu %zu %zu\n", resample_bin_index(0, 0, 0, 0, 0, 0, 6, 4, 8, 3, 5), resample_bin_index(0, 1, 0, 0, 0, 0, 6, 4, 8, 3, 5),
           resample_bin_index(1, 0, 0, 0, 0, 0, 6, 4, 8, 3, 5), resample_bin_index(2, 5, 3, 7, 2, 4, 6, 4, 8, 3, 5));
    {
        const double te[3] = {0.0, 1.0, 2.0}, ee[2] = {0.0, 1.0};
        printf("bin0: %d %d %d\n", resample_bin0(0, 6, te, 2, 1.5, ee, 1, 0.5, nullptr, 0, NAN, nullptr, 0, NAN), resample_bin0(2, 6, te, 2, 0.5, ee, 1, 0.5, nullptr, 0, NAN, nullptr, 0, NAN),
               resample_bin0(2, 6, te, 2, 2.0, ee, 1, 0.5, nullptr, 0, NAN, nullptr, 0, NAN));
    }
    printf("poisson:");
    for (uint32_t w : {0u, 1580030167u, 1580030168u, 3160060337u, 4294967291u, 4294967292u, 4294967295u}) printf(" %u", resample_poisson(w));
    printf("\n");
    const unsigned long long seeds[] = {@SEEDS@};
    const unsigned ranks[] = {@RANKS@}, slots[] = {@SLOTS@};
    for (size_t i = 0; i < sizeof seeds / sizeof seeds[0]; ++i) {
        const Philox4 b = resample_block(seeds[i], ranks[i], slots[i], 5u, RESAMPLE_BOOTSTRAP);
        printf("id_%zu: %u %u %u %u", i, b.w[0], b.w[1], b.w[2], b.w[3]);
        for (int G : {@GROUPS@}) printf(" %d", resample_group(seeds[i], ranks[i], slots[i], G));
        for (int rho = 0; rho < @RHO_MAX@; ++rho) printf(" %u", resample_multiplicity(RESAMPLE_BOOTSTRAP, seeds[i], ranks[i], slots[i], @RHO_MAX@, rho));
        for (int rho = 0; rho < 3; ++rho) printf(" %u", resample_multiplicity(RESAMPLE_JACKKNIFE, seeds[i], ranks[i], slots[i], 3, rho));
        printf(" %u\n", resample_multiplicity(RESAMPLE_NONE, seeds[i], ranks[i], slots[i], 1, 0));
    }
    if (argc < 2) return 0;
    // the rotation: n, then p1, p2, p3, ey0, ey1, ey2, Q, U [n each]
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const size_t n = (size_t)read_doubles(f, 1)[0];
    const V p1 = read_doubles(f, n), p2 = read_doubles(f, n), p3 = read_doubles(f, n), e0 = read_doubles(f, n), e1 = read_doubles(f, n), e2 = read_doubles(f, n),
            Q = read_doubles(f, n), U = read_doubles(f, n);
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        double q = Q[i], u = U[i];
        const bool ok = resample_rotation(p1[i], p2[i], p3[i], e0[i], e1[i], e2[i], q, u);
        printf("rot: %d %.17g %.17g\n", (int)ok, q, u);
    }
    return 0;
}
'''


def _cases():
    lines = []
    for name, c in PLANS.items():
        lines.append('plan("%s", %d, %s, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %s, %d, %d, %d);' % (
            name, c["n_obs"], P._vec3(c["n"]), P._vec(c["cos_acc"], 0), c["ex"] is not None, P._vec3(c["ex"] or ()), c["ey"] is not None, P._vec3(c["ey"] or ()),
            c["n_t"], P._vec(c["te"], c["n_t"]), c["n_e"], P._vec(c["ee"], c["n_e"]), c["n_x"], P._vec(c["xe"], c["n_x"]), c["n_y"], P._vec(c["ye"], c["n_y"]),
            "nullptr" if c["env"] is None else '"%s"' % c["env"], c["mode"], c["n_rep"], c["frame"]))
    return "\n".join("    " + l for l in lines)


def rotations():
    """directions all over the sphere with axes anywhere, momenta over many decades; then the special ones: along z_hat, along -z_hat, along ey, in the
    observer's direction with natural axes, a hair off the pole, and components that are zero"""
    g = np.random.default_rng(77)
    n = N_ROT - 8
    v = g.standard_normal((3, n))
    v /= np.sqrt((v * v).sum(axis=0))
    p = v * 10.0 ** g.uniform(-22.0, -12.0, n)
    ey = np.cross(v.T + 0.3 * g.standard_normal((n, 3)), g.standard_normal((n, 3))).T
    ey /= np.sqrt((ey * ey).sum(axis=0))
    special_p = np.array([[0, 0, 1e-17], [0, 0, -1e-17], [0, 2e-17, 0], [3e-18, 0, 4e-18], [1e-21, -1e-21, 1e-17], [1e-17, 0, 0], [0, 1e-17, 1e-17], [1e-300, 0, 1e-300]]).T
    special_ey = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.float64).T
    p, ey = np.concatenate([p, special_p], axis=1), np.concatenate([ey, special_ey], axis=1)
    return p, ey, g.uniform(-1.0, 1.0, N_ROT), g.uniform(-1.0, 1.0, N_ROT)


def _build(d, src, name, extra):
    exe = d / name
    # (-Wno-unknown-pragmas: rng.hpp, which the header includes for the keyed Philox block, unrolls its rounds with a pragma that only hipcc knows)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", P.os.path.join(P.ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("resample_plan")
    src, data = d / "driver.cpp", d / "rotations.bin"
    text = DRIVER.replace("@CASES@", _cases()).replace("@CODES@", ", ".join(str(k) for k in sorted(TEXTS)))
    text = text.replace("@SEEDS@", ", ".join("%dull" % s for s, _, _ in IDENTITIES)).replace("@RANKS@", ", ".join("%du" % r for _, r, _ in IDENTITIES))
    text = text.replace("@SLOTS@", ", ".join("%du" % s for _, _, s in IDENTITIES)).replace("@GROUPS@", ", ".join(str(G) for G in GROUPS)).replace("@RHO_MAX@", str(RHO_MAX))
    src.write_text(text)
    p, ey, Q, Uq = rotations()
    np.concatenate([[float(N_ROT)], p[0], p[1], p[2], ey[0], ey[1], ey[2], Q, Uq]).tofile(data)
    return d, src, data


@pytest.fixture(scope="module")
def text(built):
    d, src, data = built
    return subprocess.run([str(_build(d, src, "driver", [])), str(data)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def out(text):
    res = {"rot": []}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        if key == "rot":
            res["rot"].append(vals.split())
        else:
            res[key] = vals if key.startswith("text_") else [int(v) for v in vals.split()]
    return res


def plan_rule(c):
    """resample_plan restated: the checks in their order, the layout, the path, the slices, the grid"""
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    sky, _ = P.plan_rule(dict(c, env=None))
    if P.OK < sky <= P.Y_NOT_ASCENDING:
        return sky, None                                                 # one of the observers' checks (what follows them in sky_plan is not asked here)
    n_obs, n_t, n_e, n_x, n_y, mode, n_rep, frame = (c[k] for k in ("n_obs", "n_t", "n_e", "n_x", "n_y", "mode", "n_rep", "frame"))
    if mode not in (NONE, JACKKNIFE, BOOTSTRAP):
        return BAD_MODE, None
    if frame not in (AS_STORED, SKY_PLANE):
        return BAD_FRAME, None
    if mode == NONE and n_rep != 1:
        return N_REP_NOT_ONE, None
    if mode != NONE and n_rep < 2:
        return N_REP_TOO_SMALL, None
    image = n_x >= 1
    per_rep = n_t * n_e * (n_y * n_x if image else 1)
    n_bins = n_obs * n_rep * per_rep
    if n_bins > 2 ** 31 - 1:
        return TOO_MANY_BINS, None
    if frame == SKY_PLANE and not image:
        if c["ex"] is None or c["ey"] is None:
            return AXES_NULL, None
        if not all(np.isfinite(v).all() for v in tuple(c["ex"]) + tuple(c["ey"])):
            return AXES_NOT_FINITE, None
        if any(abs(dot(v, v) - 1.0) > 1e-12 for v in tuple(c["ex"]) + tuple(c["ey"])):
            return AXES_NOT_UNIT, None
        if any(abs(dot(x, n)) > 1e-12 or abs(dot(y, n)) > 1e-12 or abs(dot(x, y)) > 1e-12 for n, x, y in zip(c["n"], c["ex"], c["ey"])):
            return AXES_NOT_ORTHOGONAL, None
    axes = image or frame == SKY_PLANE
    cube = 7 * 8 * n_bins
    out_bytes = cube + 3 * 8 * n_obs                                     # ... and the three counters per observer
    staged_doubles = (10 if axes else 4) * n_obs + n_t + 1 + n_e + 1 + (n_x + 1 + n_y + 1 if image else 0)
    staged = 8 * staged_doubles + 3 * 8 * n_obs
    if staged + MATCH_BYTES > LDS_BUDGET:
        return STAGING_TOO_LARGE, None
    if c["env"] not in (None, "", "lds", "sliced", "global"):
        return BAD_PATH_SWITCH, None
    replica = 7 * 8 * n_obs * per_rep
    room = LDS_BUDGET - staged
    whole_fits, one_fits = cube <= room, replica <= room
    if c["env"] == "lds" and not whole_fits:
        return LDS_FORCED_TOO_LARGE, None
    if c["env"] == "sliced" and not one_fits:
        return SLICED_FORCED_TOO_LARGE, None
    reps = min(room // replica, n_rep) if one_fits else 0
    slices = -(-n_rep // reps) if one_fits else 0
    path = {"lds": PATH_LDS, "sliced": PATH_SLICED, "global": PATH_GLOBAL}.get(c["env"])
    if path is None:
        path = PATH_LDS if whole_fits else (PATH_SLICED if one_fits and (mode == BOOTSTRAP or slices <= MAX_SLICES) else PATH_GLOBAL)
    if path == PATH_GLOBAL:
        reps, slices, lds = n_rep, 1, staged + MATCH_BYTES
        groups = min(2 * LDS_BUDGET // lds, 8)
    else:
        lds, groups = staged + reps * replica, 2
    def grid(slots, cus):
        x, y = min(-(-slots // BLOCK), cus * groups, MAX_GRID), min(slices, MAX_GRID_Y)
        if y > 1 and x > 1:
            x = max(-(-x // y), 1)
        return [x, y]
    clocks = out_bytes + 8 * staged_doubles
    return OK, ([path, int(image), int(axes), per_rep, n_bins, cube, out_bytes, staged_doubles, staged, replica, reps, slices, lds, groups, cube, out_bytes, clocks,
                 clocks + 8 * 5] + grid(1, 256) + grid(1000000, 256) + grid(2000000000, 304))


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan(out, name):
    why, plan_ = plan_rule(PLANS[name])
    assert out["plan_" + name] == [why]
    if why == OK:
        assert out["planv_" + name] == plan_
    else:
        assert "planv_" + name not in out


def test_plan_cases_are_what_they_are_meant_to_be(out):
    """... so that the table above cannot drift into testing nothing: every refusal of this product occurs, where two faults meet the first in the
    order wins, and the path changes exactly at each LDS boundary"""
    for name, why in REFUSED.items():
        assert out["plan_" + name] == [why], name
    assert set(OWN_CODES) <= set(REFUSED.values())
    for name in set(PLANS) - set(REFUSED):
        assert out["plan_" + name] == [OK], name
    assert out["constants"] == [BLOCK, MAX_GRID, MAX_GRID_Y, MAX_SLICES, MATCH_BYTES, 3, 2, 12]
    v = lambda name: out["planv_" + name]
    PATH, REPLICA, REPS, SLICES, LDS = 0, 9, 10, 11, 12
    #                       path  image axes per_rep bins cube out doubles staged replica reps slices lds groups, offsets
    assert v("none")[:18] == [PATH_LDS, 0, 0, 32, 32, 1792, 1816, 18, 168, 1792, 1, 1, 1960, 2, 1792, 1816, 1960, 2000]
    assert v("none_sky_plane")[2] == 1 and v("none_sky_plane")[7] == 24 and v("image_sky_plane")[7] == v("image")[7] == 34
    assert v("image")[:14] == [PATH_LDS, 1, 1, 480, 960, 53760, 53784, 34, 296, 26880, 2, 1, 296 + 53760, 2]
    assert v("three")[:14] == [PATH_SLICED, 1, 1, 480, 7200, 403200, 403272, 54, 504, 80640, 1, 5, 504 + 80640, 2]
    # the whole cube: the budget exactly is LDS, one bin more is two slices of one replica each
    assert v("lds_last")[PATH] == PATH_LDS and v("lds_last")[LDS] == LDS_BUDGET and v("lds_last")[REPS:LDS] == [2, 1]
    assert v("sliced_first")[PATH] == PATH_SLICED and v("sliced_first")[REPS:LDS] == [1, 2] and v("sliced_first")[LDS] + v("sliced_first")[REPLICA] > LDS_BUDGET
    # one replica: the last that fits is sliced, one bin more is global
    assert v("sliced_last")[PATH] == PATH_SLICED and v("sliced_last")[REPS:LDS] == [1, 3] and LDS_BUDGET - 64 < v("sliced_last")[LDS] <= LDS_BUDGET
    assert v("global_first")[PATH] == PATH_GLOBAL and v("global_first")[REPS:LDS] == [3, 1] and v("global_first")[LDS] == v("global_first")[8] + MATCH_BYTES
    assert v("global_first")[8] + v("global_first")[REPLICA] > LDS_BUDGET
    # the slice count at which the rule changes, and the switch overrides it
    assert v("slices_12")[PATH] == PATH_SLICED and v("slices_12")[SLICES] == 12 and v("slices_13")[PATH] == PATH_GLOBAL
    assert v("slices_13_forced")[PATH] == PATH_SLICED and v("slices_13_forced")[SLICES] == 13
    assert v("slices_65_bootstrap")[PATH] == PATH_SLICED and v("slices_65_bootstrap")[SLICES] == 65
    assert v("bench_jackknife")[PATH] == PATH_GLOBAL and v("bench_jackknife")[REPS:LDS] == [32, 1]
    assert v("bench_bootstrap")[PATH] == PATH_SLICED and v("bench_bootstrap")[REPS:LDS] == [11, 19]
    # the grid: 512 workgroups shared among the slices, one row of them per slice
    assert v("bench_jackknife")[-4:-2] == [2048, 1] and v("slices_12")[-4:-2] == [43, 12] and v("bench_bootstrap")[-4:-2] == [27, 19] and v("none")[-6:] == [1, 1, 512, 1, 608, 1]
    assert v("forced_lds")[PATH] == PATH_LDS and v("forced_global")[PATH] == PATH_GLOBAL and v("forced_global_beyond")[PATH] == PATH_GLOBAL
    assert v("forced_sliced_small")[PATH] == PATH_SLICED and v("forced_sliced_small")[REPS:LDS] == [2, 1] and v("forced_sliced_small")[LDS] == v("forced_lds")[LDS]
    assert v("empty_switch") == v("image")
    assert v("staging_last")[8] + MATCH_BYTES == LDS_BUDGET
    assert v("stored_ignores_axes")[:14] == [PATH_LDS, 0, 0, 32, 64, 3584, 3608, 18, 168, 1792, 2, 1, 168 + 3584, 2]


def test_refusal_texts(out):
    for why, t in TEXTS.items():
        assert out["text_%d" % why] == t, why
        assert t.startswith(PREFIX + " ")
    assert len(set(TEXTS.values())) == len(TEXTS) == P.Y_NOT_ASCENDING + 13


def test_bin_index_with_the_replica_axis(out):
    per_rep = 4 * 8 * 3 * 5
    assert out["bin_index"] == [0, per_rep, 6 * per_rep, (2 * 6 + 5) * per_rep + ((3 * 8 + 7) * 3 + 2) * 5 + 4]      # x fastest ... time, replica, observer
    assert out["bin0"] == [1, 2 * 6 * 2 + 0, -1]                            # replica 0 of observer o; an edge's last value is outside


def test_multiplicities_equal_the_numpy_restatement(out):
    assert out["poisson"] == [0, 0, 1, 2, 11, 12, 12]
    for i, (seed, rank, slot) in enumerate(IDENTITIES):
        row = out["id_%d" % i]
        assert row[:4] == [int(w[0]) for w in R.block(seed, [rank], [slot], 5, R.BOOTSTRAP)]
        groups = [int(R.group(seed, np.array([rank]), np.array([slot]), G)[0]) for G in GROUPS]
        assert row[4:4 + len(GROUPS)] == groups and all(0 <= g < G for g, G in zip(groups, GROUPS))
        k = R.multiplicities(R.BOOTSTRAP, seed, [rank], [slot], RHO_MAX)[:, 0]
        at = 4 + len(GROUPS)
        assert row[at:at + RHO_MAX] == k.tolist() and k[0] == 1
        assert row[at + RHO_MAX:at + RHO_MAX + 3] == R.multiplicities(R.JACKKNIFE, seed, [rank], [slot], 3)[:, 0].tolist()
        assert row[-1] == 1
    assert out["id_4"] != out["id_5"]                                        # (rank 0, slot 1) is not (rank 1, slot 0)


def test_rotation_equals_the_numpy_restatement(out):
    p, ey, Q, Uq = rotations()
    q, u, undefined = R.rotation(p[0], p[1], p[2], ey[0], ey[1], ey[2], Q, Uq)
    rows = out["rot"]
    assert len(rows) == N_ROT
    assert [int(r[0]) for r in rows] == (~undefined).astype(int).tolist()
    assert np.array_equal(np.array([float(r[1]) for r in rows]), q) and np.array_equal(np.array([float(r[2]) for r in rows]), u)      # bit for bit
    special = undefined[-8:].tolist()
    assert special[:3] == [True, True, True] and special[3:7] == [False] * 4 and not undefined[:-8].any()
    assert q[-8:][:3].tolist() == Q[-8:][:3].tolist()                        # undefined: as stored
    assert q[-5] == Q[-5] and u[-5] == Uq[-5]                                # along n = (0.6, 0, 0.8) with ey = y_hat: the natural axes keep the pair


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
