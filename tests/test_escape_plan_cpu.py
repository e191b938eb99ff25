"""The host's rules for an escape-weighted sky observation (mcrat_amd/csrc/escape_plan.hpp) on the CPU: every refusal with its text and in its order
-- the observers' (sky_plan.hpp's, with this product's prefix), n_tau, the product, tau_edges, the march's (sightline_plan.hpp's), staging, the
switch --, the block's layout, the rule that picks the accumulation path on both sides of its LDS boundary, the three grids, and the per-photon
function escape_bin against tests/escape_checker.py on random photons.  Plain C++: a small driver is compiled with g++, as
tests/test_sky_plan_cpu.py does for its header, and what it prints is compared; the same driver is built a second time with
-fsanitize=address,undefined and run once as a stand-alone program."""
import shutil
import subprocess

import numpy as np
import pytest

from tests import escape_checker as ec
from tests import sightline_checker as sc
from tests import sky_checker as S
from tests.test_sky_plan_cpu import _build, _vec, _vec3, INF, NAN, X, Y, Z, TEXTS as SKY_TEXTS, LDS_BUDGET, MATCH_BYTES, PATH_LDS, PATH_GLOBAL

OK = 0
(SKY_NO_BINS, SKY_AXES_MISMATCH, SKY_TOO_MANY_BINS, SKY_DIR_NOT_FINITE, SKY_DIR_NOT_UNIT, SKY_BAD_CONE, SKY_AXES_NULL, SKY_AXES_NOT_FINITE, SKY_AXES_NOT_UNIT,
 SKY_AXES_NOT_ORTHOGONAL, SKY_T_NOT_FINITE, SKY_T_NOT_ASCENDING, SKY_E_NOT_FINITE, SKY_E_NOT_ASCENDING, SKY_X_NOT_FINITE, SKY_X_NOT_ASCENDING, SKY_Y_NOT_FINITE,
 SKY_Y_NOT_ASCENDING) = range(1, 19)
NO_TAU_BINS, TOO_MANY_BINS, TAU_NOT_FINITE, TAU_NOT_ASCENDING = 32, 33, 34, 35
BAD_STEP_FRAC, BAD_H_MIN, BAD_MAX_STEPS, BAD_TAU_STOP = 48 + 2, 48 + 3, 48 + 4, 48 + 5
STAGING_TOO_LARGE, BAD_PATH_SWITCH, LDS_FORCED_TOO_LARGE, HYDRO_MISMATCH = 64, 65, 66, 67
BLOCK, MAX_GRID, MARCH_MAX_GRID, PLANES = 256, 2048, 65536, 9

TEXTS = {k: "observe_escaping:" + t.split(":", 1)[1] for k, t in SKY_TEXTS.items() if k <= SKY_Y_NOT_ASCENDING}
TEXTS.update({
    NO_TAU_BINS: "observe_escaping: n_tau must be at least 1",
    TOO_MANY_BINS: "observe_escaping: n_obs * n_tau * n_t * n_e * n_y * n_x overflows an int",
    TAU_NOT_FINITE: "observe_escaping: tau_edges holds a value that is not finite",
    TAU_NOT_ASCENDING: "observe_escaping: tau_edges is not strictly ascending",
    BAD_STEP_FRAC: "observe_escaping: step_frac must be finite and not negative",
    BAD_H_MIN: "observe_escaping: h_min must be finite and positive",
    BAD_MAX_STEPS: "observe_escaping: max_steps must lie between 1 and 1048576",
    BAD_TAU_STOP: "observe_escaping: tau_stop must be positive (+inf: never opaque)",
    STAGING_TOO_LARGE: "observe_escaping: the edges and the observers' vectors do not fit the kernel's LDS budget",
    BAD_PATH_SWITCH: "observe_escaping: MCRAT_HIP_ESCAPE_PATH must be lds or global",
    LDS_FORCED_TOO_LARGE: "observe_escaping: MCRAT_HIP_ESCAPE_PATH=lds, but the cube does not fit the kernel's LDS budget",
    HYDRO_MISMATCH: "observe_escaping: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY, TAU_CALCULATION) or on another device",
})


def plan(n_obs=1, n=(Z,), cos_acc=(0.5,), ex=(X,), ey=(Y,), n_t=4, te="ramp", n_e=8, ee="ramp", n_x=5, xe="ramp", n_y=3, ye="ramp", n_tau=6, taue="ramp",
         step_frac=1e-3, h_min=1e8, max_steps=400, tau_stop=INF, surface_level=-1.0, env=None):
    """one case: the arrays as they are handed over; "ramp" stands for 0, 1, 2, ... of the length the count asks for; ex / ey None: a NULL pointer"""
    return dict(n_obs=n_obs, n=n, cos_acc=cos_acc, ex=ex, ey=ey, n_t=n_t, te=te, n_e=n_e, ee=ee, n_x=n_x, xe=xe, n_y=n_y, ye=ye, n_tau=n_tau, taue=taue,
                step_frac=step_frac, h_min=h_min, max_steps=max_steps, tau_stop=tau_stop, surface_level=surface_level, env=env)


CURVE = dict(n_x=0, n_y=0, ex=None, ey=None)
PLANS = {
    "image": plan(),
    "curve": plan(**CURVE),
    "three": plan(n_obs=3, n=(Z, X, Y), cos_acc=(1.0, -1.0, 0.0), ex=(X, Y, Z), ey=(Y, Z, X)),
    # 9 planes * 8 B * 2 k bins + 8 * (4 + 2 + k + 1 + 3) + 32: k = 538 are 77 472 + 4 416 + 32 = 81 920 - 32, k = 539 are 82 072
    "lds_last_curve": plan(n_t=1, n_e=538, n_tau=2, **CURVE),
    "global_first_curve": plan(n_t=1, n_e=539, n_tau=2, **CURVE),
    "bench_image": plan(n_t=8, n_e=1, n_x=256, n_y=256, n_tau=6),
    "forced_global": plan(env="global", **CURVE),
    "forced_lds": plan(env="lds", **CURVE),
    "forced_global_beyond": plan(env="global"),
    "empty_switch": plan(env=""),
    "surface_level_is_not_read": plan(surface_level=NAN),
    "tau_stop_finite": plan(tau_stop=2.0),
    "staging_last": plan(n_t=9190, n_e=1, n_tau=1, **CURVE),          # 8 * (4 + 9191 + 2 + 2) + 32 + 8192 = 81 816
    # ... refused, one of each
    "sky_no_t_bin": plan(n_t=0, te=[0.0]),
    "sky_x_without_y": plan(n_y=0, ye=[0.0]),
    "sky_product_overflow": plan(n_t=65536, te=[], n_e=32768, ee=[], **CURVE),
    "sky_dir_nan": plan(n=([NAN, 0.0, 1.0],)),
    "sky_dir_long": plan(n=([0.0, 0.0, 1.0 + 1e-11],)),
    "sky_cone_above": plan(cos_acc=(1.0 + 1e-15,)),
    "sky_axes_null": plan(ex=None),
    "sky_axes_nan": plan(ey=([0.0, NAN, 0.0],)),
    "sky_axes_long": plan(ex=([1.0 + 1e-11, 0.0, 0.0],)),
    "sky_axes_parallel": plan(ex=(X,), ey=(X,)),
    "sky_t_inf": plan(te=[0.0, 1.0, 2.0, 3.0, INF]),
    "sky_t_equal": plan(te=[0.0, 1.0, 1.0, 3.0, 4.0]),
    "sky_e_nan": plan(n_e=2, ee=[1.0, NAN, 2.0]),
    "sky_e_descending": plan(n_e=2, ee=[1.0, 3.0, 2.0]),
    "sky_x_minus_inf": plan(n_x=2, xe=[-INF, 0.0, 1.0]),
    "sky_x_equal": plan(n_x=2, xe=[0.0, 0.0, 1.0]),
    "sky_y_nan": plan(n_y=1, ye=[0.0, NAN]),
    "sky_y_descending": plan(n_y=1, ye=[1.0, 0.0]),
    "no_tau_bin": plan(n_tau=0, taue=[0.0]),
    "negative_tau_bins": plan(n_tau=-3, taue=[]),
    "product_overflow": plan(n_t=65536, n_e=16384, n_tau=2, **CURVE),                      # 2^30 sky bins pass, two tau bins make 2^31
    "product_last_int": plan(n_t=46340, n_e=46340, n_tau=1, env="lds", **CURVE),          # < 2^31: the product passes; its edges cannot be staged
    "tau_inf": plan(n_tau=2, taue=[0.0, 1.0, INF]),
    "tau_nan": plan(n_tau=2, taue=[NAN, 1.0, 2.0]),
    "tau_equal": plan(n_tau=2, taue=[0.0, 0.0, 1.0]),
    "tau_descending": plan(n_tau=2, taue=[0.0, 2.0, 1.0]),
    "step_frac_negative": plan(step_frac=-1.0),
    "step_frac_nan": plan(step_frac=NAN),
    "h_min_zero": plan(h_min=0.0),
    "h_min_inf": plan(h_min=INF),
    "max_steps_zero": plan(max_steps=0),
    "max_steps_beyond": plan(max_steps=(1 << 20) + 1),
    "tau_stop_zero": plan(tau_stop=0.0),
    "tau_stop_nan": plan(tau_stop=NAN),
    "staging_too_large": plan(n_t=9204, n_e=1, n_tau=1, **CURVE),     # 8 * (4 + 9205 + 2 + 2) + 32 + 8192 = 81 928
    "bad_switch": plan(env="hbm"),
    "bad_switch_upper": plan(env="LDS"),
    "forced_lds_too_large": plan(n_t=1, n_e=539, n_tau=2, env="lds", **CURVE),
    # two faults at once: the first in the order decides
    "sky_before_tau_count": plan(n_t=0, te=[0.0], n_tau=0, taue=[0.0]),
    "sky_edges_before_tau_count": plan(n_y=1, ye=[1.0, 0.0], n_tau=0, taue=[0.0]),
    "tau_count_before_product": plan(n_t=65536, n_e=16384, n_tau=0, taue=[0.0], **CURVE),
    "product_before_tau_edges": plan(n_t=65536, n_e=16384, n_tau=2, taue=[NAN, 0.0, 1.0], **CURVE),
    "tau_finite_before_ascending": plan(n_tau=2, taue=[1.0, 0.0, NAN]),
    "tau_edges_before_march": plan(n_tau=2, taue=[0.0, 0.0, 1.0], step_frac=-1.0),
    "step_frac_before_h_min": plan(step_frac=INF, h_min=-1.0, max_steps=0),
    "max_steps_before_tau_stop": plan(max_steps=0, tau_stop=-1.0),
    "march_before_staging": plan(n_t=9204, n_e=1, n_tau=1, tau_stop=0.0, **CURVE),
    "staging_before_switch": plan(n_t=9204, n_e=1, n_tau=1, env="hbm", **CURVE),
    "switch_before_forced": plan(n_t=1, n_e=539, n_tau=2, env="Lds", **CURVE),
}
REFUSED = {
    "sky_no_t_bin": SKY_NO_BINS, "sky_x_without_y": SKY_AXES_MISMATCH, "sky_product_overflow": SKY_TOO_MANY_BINS, "sky_dir_nan": SKY_DIR_NOT_FINITE,
    "sky_dir_long": SKY_DIR_NOT_UNIT, "sky_cone_above": SKY_BAD_CONE, "sky_axes_null": SKY_AXES_NULL, "sky_axes_nan": SKY_AXES_NOT_FINITE,
    "sky_axes_long": SKY_AXES_NOT_UNIT, "sky_axes_parallel": SKY_AXES_NOT_ORTHOGONAL, "sky_t_inf": SKY_T_NOT_FINITE, "sky_t_equal": SKY_T_NOT_ASCENDING,
    "sky_e_nan": SKY_E_NOT_FINITE, "sky_e_descending": SKY_E_NOT_ASCENDING, "sky_x_minus_inf": SKY_X_NOT_FINITE, "sky_x_equal": SKY_X_NOT_ASCENDING,
    "sky_y_nan": SKY_Y_NOT_FINITE, "sky_y_descending": SKY_Y_NOT_ASCENDING, "no_tau_bin": NO_TAU_BINS, "negative_tau_bins": NO_TAU_BINS,
    "product_overflow": TOO_MANY_BINS, "product_last_int": STAGING_TOO_LARGE, "tau_inf": TAU_NOT_FINITE, "tau_nan": TAU_NOT_FINITE, "tau_equal": TAU_NOT_ASCENDING,
    "tau_descending": TAU_NOT_ASCENDING, "step_frac_negative": BAD_STEP_FRAC, "step_frac_nan": BAD_STEP_FRAC, "h_min_zero": BAD_H_MIN, "h_min_inf": BAD_H_MIN,
    "max_steps_zero": BAD_MAX_STEPS, "max_steps_beyond": BAD_MAX_STEPS, "tau_stop_zero": BAD_TAU_STOP, "tau_stop_nan": BAD_TAU_STOP,
    "staging_too_large": STAGING_TOO_LARGE, "bad_switch": BAD_PATH_SWITCH, "bad_switch_upper": BAD_PATH_SWITCH, "forced_lds_too_large": LDS_FORCED_TOO_LARGE,
    "sky_before_tau_count": SKY_NO_BINS, "sky_edges_before_tau_count": SKY_Y_NOT_ASCENDING, "tau_count_before_product": NO_TAU_BINS,
    "product_before_tau_edges": TOO_MANY_BINS, "tau_finite_before_ascending": TAU_NOT_FINITE, "tau_edges_before_march": TAU_NOT_ASCENDING,
    "step_frac_before_h_min": BAD_STEP_FRAC, "max_steps_before_tau_stop": BAD_MAX_STEPS, "march_before_staging": BAD_TAU_STOP,
    "staging_before_switch": STAGING_TOO_LARGE, "switch_before_forced": BAD_PATH_SWITCH,
}
ALL_CODES = sorted(TEXTS)

N_PHOTONS, N_OBS = 1500, 3

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "escape_plan.hpp"
using namespace mcrat;
typedef std::vector<double> V;

static V ramp(int n) { V v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }
static const double *col(const V &v, int k, int n_obs) { return v.data() + (size_t)k * (n_obs > 0 ? n_obs : 0); }
// n, ex, ey: component-major [3][n_obs]; has_x / has_y 0: NULL pointers
static void plan(const char *name, int n_obs, V n, V ca, int has_x, V ex, int has_y, V ey, int n_t, V te, int n_e, V ee, int n_x, V xe, int n_y, V ye, int n_tau, V taue,
                 double step_frac, double h_min, int max_steps, double tau_stop, double surface_level, const char *env)
{
    EscapeArgs a{};
    SkyArgs &s = a.sky;
    s.n_obs = n_obs; s.n0 = col(n, 0, n_obs); s.n1 = col(n, 1, n_obs); s.n2 = col(n, 2, n_obs); s.cos_acc = ca.data();
    if (has_x) { s.x0 = col(ex, 0, n_obs); s.x1 = col(ex, 1, n_obs); s.x2 = col(ex, 2, n_obs); }
    if (has_y) { s.y0 = col(ey, 0, n_obs); s.y1 = col(ey, 1, n_obs); s.y2 = col(ey, 2, n_obs); }
    s.n_t = n_t; s.t_edges = te.data(); s.n_e = n_e; s.e_edges = ee.data(); s.n_x = n_x; s.x_edges = xe.data(); s.n_y = n_y; s.y_edges = ye.data();
    a.n_tau = n_tau; a.tau_edges = taue.data();
    a.march = SightlineParams{step_frac, h_min, max_steps, tau_stop, surface_level};
    EscapePlan p;
    const EscapeRefusal why = escape_plan(a, env, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why != ESCAPE_OK) return;
    const EscapeLayout l = escape_layout(p, 1000, 3);
    printf("planv_%s: %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu\n", name, (int)p.path, (int)p.image, p.n_bins, p.cube_bytes,
           p.counters_offset, p.head_offset, p.out_bytes, p.staged_doubles, p.staged_bytes, p.lds_bytes, p.select_lds_bytes, p.groups_per_cu,
           escape_select_grid(1, 256), escape_select_grid(100000, 256), escape_select_grid(2000000000, 304), escape_march_grid(1), escape_march_grid(100000),
           escape_march_grid(2000000000), escape_bin_grid(p, 100000, 256), escape_bin_grid(p, 2000000000, 304), l.staged_offset, l.clocks_offset, l.tau_offset,
           l.index_offset, l.status_offset, l.total_bytes);
    printf("march_%s: %d %d\n", name, p.march.max_steps, (int)(p.march.step_frac == step_frac && p.march.h_min == h_min && p.march.tau_stop == tau_stop));
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
    char text[ESCAPE_TEXT_BYTES];
    for (int k : {@CODES@}) printf("text_%d:%s\n", k, escape_refusal_text((EscapeRefusal)k, text));
    printf("constants: %d %d %d %d %d %d %d %d %d %zu\n", ESCAPE_PLANES, ESCAPE_COUNTERS, ESCAPE_HEAD_WORDS, ESCAPE_SELECTED_WORD, ESCAPE_OBSERVABLE_WORD, ESCAPE_BLOCK,
           ESCAPE_MAX_GRID, ESCAPE_MARCH_MAX_GRID, (int)ESC_WEX, ESCAPE_MATCH_BYTES);
    printf("bin_index: %zu %zu %zu %zu %zu\n", escape_bin_index(0, 0, 0, 0, 0, 0, 6, 4, 8, 3, 5), escape_bin_index(0, 0, 0, 0, 0, 1, 6, 4, 8, 3, 5),
           escape_bin_index(0, 1, 0, 0, 0, 0, 6, 4, 8, 3, 5), escape_bin_index(1, 0, 0, 0, 0, 0, 6, 4, 8, 3, 5), escape_bin_index(2, 5, 3, 7, 2, 4, 6, 4, 8, 3, 5));
    printf("weight: %d %d\n", (int)(escape_weight(0.0) == 1.0), (int)(escape_weight(1.0) == exp(-1.0)));
    if (argc < 2) return 0;
    // the photons: header {n, n_obs, n_t, n_e, n_x, n_y, n_tau} as doubles, then time_now, tau, r0, r1, r2, p0 [n each], n [3][n_obs], ex, ey [3][n_obs], the
    // five edge arrays
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const V head = read_doubles(f, 7);
    const size_t n = (size_t)head[0];
    const int n_obs = (int)head[1], n_t = (int)head[2], n_e = (int)head[3], n_x = (int)head[4], n_y = (int)head[5], n_tau = (int)head[6];
    const V tn = read_doubles(f, n), tau = read_doubles(f, n), r0 = read_doubles(f, n), r1 = read_doubles(f, n), r2 = read_doubles(f, n), p0 = read_doubles(f, n),
            nv = read_doubles(f, 3 * n_obs), ex = read_doubles(f, 3 * n_obs), ey = read_doubles(f, 3 * n_obs), te = read_doubles(f, n_t + 1), ee = read_doubles(f, n_e + 1),
            xe = read_doubles(f, n_x + 1), ye = read_doubles(f, n_y + 1), taue = read_doubles(f, n_tau + 1);
    fclose(f);
    for (size_t i = 0; i < n; ++i)
        for (int o = 0; o < n_obs; ++o) {
            const double n0 = nv[o], n1 = nv[n_obs + o], n2 = nv[2 * n_obs + o];
            const double t = sky_t_det(tn[i], r0[i], r1[i], r2[i], n0, n1, n2), e = observe_energy(p0[i]);
            double X, Y;
            sky_xy(r0[i], r1[i], r2[i], ex[o], ex[n_obs + o], ex[2 * n_obs + o], ey[o], ey[n_obs + o], ey[2 * n_obs + o], X, Y);
            printf("ph: %d %d\n", escape_bin(o, taue.data(), n_tau, tau[i], te.data(), n_t, t, ee.data(), n_e, e, xe.data(), n_x, X, ye.data(), n_y, Y),
                   escape_bin(o, taue.data(), n_tau, tau[i], te.data(), n_t, t, ee.data(), n_e, e, nullptr, 0, NAN, nullptr, 0, NAN));
        }
    return 0;
}
'''


def _num(x):
    return "NAN" if x != x else {INF: "INFINITY", -INF: "-INFINITY"}.get(x, repr(float(x)))


def _cases():
    lines = []
    for name, c in PLANS.items():
        lines.append('plan("%s", %d, %s, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %d, %s, %s, %s, %d, %s, %s, %s);' % (
            name, c["n_obs"], _vec3(c["n"]), _vec(c["cos_acc"], 0), c["ex"] is not None, _vec3(c["ex"] or ()), c["ey"] is not None, _vec3(c["ey"] or ()),
            c["n_t"], _vec(c["te"], c["n_t"]), c["n_e"], _vec(c["ee"], c["n_e"]), c["n_x"], _vec(c["xe"], c["n_x"]), c["n_y"], _vec(c["ye"], c["n_y"]),
            c["n_tau"], _vec(c["taue"], c["n_tau"]), _num(c["step_frac"]), _num(c["h_min"]), c["max_steps"], _num(c["tau_stop"]), _num(c["surface_level"]),
            "nullptr" if c["env"] is None else '"%s"' % c["env"]))
    return "\n".join("    " + l for l in lines)


def photons():
    """1500 seeded photons of the sky checker's jet, 3 observers, and optical depths over the whole axis and beyond it: zeros, values ON edges, NaN"""
    ph = S.jet_photons(20260114, N_PHOTONS)
    g = np.random.default_rng(11)
    tn = g.uniform(300.0, 400.0, N_PHOTONS)
    n, cos_acc, ex, ey = S.observers([0.0, 0.2, 0.25], [0.0, 0.4, 1.0], [0.25, 0.2, 0.2])
    tau = 10.0 ** g.uniform(-2.0, 2.0, N_PHOTONS)
    tau[::50] = 0.0
    tau[1::50] = ec.TAU_EDGES[g.integers(0, len(ec.TAU_EDGES), len(tau[1::50]))]
    tau[2::97] = np.nan
    wide = S.per_photon(ph, n, cos_acc, [-1e9, 1e9], [0.0, 1e300], tn, ex, ey, [-1e300, 1e300], [-1e300, 1e300])
    te = np.linspace(wide["t"].min() - 1.0, np.percentile(wide["t"], 90), 7)
    ee = 10.0 ** np.linspace(-9.5, -4.2, 6)
    return dict(ph=ph, tn=tn, tau=tau, n=n, cos_acc=cos_acc, ex=ex, ey=ey, te=te, ee=ee, xe=np.linspace(-2.5e12, 2.5e12, 6), ye=np.linspace(-2.0e12, 3.0e12, 5),
                taue=ec.TAU_EDGES)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("escape_plan")
    src, data = d / "driver.cpp", d / "photons.bin"
    src.write_text(DRIVER.replace("@CASES@", _cases()).replace("@CODES@", ", ".join(str(k) for k in ALL_CODES)))
    q = photons()
    head = np.array([N_PHOTONS, N_OBS] + [len(q[k]) - 1 for k in ("te", "ee", "xe", "ye", "taue")], dtype=np.float64)
    cols = [q["tn"], q["tau"]] + [q["ph"][k] for k in ("r0", "r1", "r2", "p0")]
    np.concatenate([head] + cols + [q["n"].ravel(), q["ex"].ravel(), q["ey"].ravel(), q["te"], q["ee"], q["xe"], q["ye"], q["taue"]]).tofile(data)
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
            res["ph"].append([int(v) for v in vals.split()])
        else:
            res[key] = vals if key.startswith("text_") else [int(v) for v in vals.split()]
    return res


def plan_rule(c):
    """escape_plan restated: the checks in their order, the layout, the path, the grids"""
    def edges(v, n):
        return [float(k) for k in range(n + 1)] if v == "ramp" else list(v)

    def axis(v, n, not_finite, not_ascending):
        e = edges(v, n)
        if not all(np.isfinite(e)):
            return not_finite
        return OK if all(a < b for a, b in zip(e[:-1], e[1:])) else not_ascending
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    n_obs, n_t, n_e, n_x, n_y, n_tau = c["n_obs"], c["n_t"], c["n_e"], c["n_x"], c["n_y"], c["n_tau"]
    if n_obs < 1 or n_t < 1 or n_e < 1:
        return SKY_NO_BINS, None
    if not ((n_x == 0 and n_y == 0) or (n_x >= 1 and n_y >= 1)):
        return SKY_AXES_MISMATCH, None
    image = n_x >= 1
    per_tau = n_obs * n_t * n_e * (n_y * n_x if image else 1)
    if per_tau > 2 ** 31 - 1:
        return SKY_TOO_MANY_BINS, None
    if not all(np.isfinite(v).all() for v in c["n"]):
        return SKY_DIR_NOT_FINITE, None
    if any(abs(dot(v, v) - 1.0) > 1e-12 for v in c["n"]):
        return SKY_DIR_NOT_UNIT, None
    if not all(-1.0 <= a <= 1.0 for a in c["cos_acc"]):
        return SKY_BAD_CONE, None
    if image:
        if c["ex"] is None or c["ey"] is None:
            return SKY_AXES_NULL, None
        both = tuple(c["ex"]) + tuple(c["ey"])
        if not all(np.isfinite(v).all() for v in both):
            return SKY_AXES_NOT_FINITE, None
        if any(abs(dot(v, v) - 1.0) > 1e-12 for v in both):
            return SKY_AXES_NOT_UNIT, None
        if any(abs(dot(x, n)) > 1e-12 or abs(dot(y, n)) > 1e-12 or abs(dot(x, y)) > 1e-12 for n, x, y in zip(c["n"], c["ex"], c["ey"])):
            return SKY_AXES_NOT_ORTHOGONAL, None
    axes = [(c["te"], n_t, SKY_T_NOT_FINITE, SKY_T_NOT_ASCENDING), (c["ee"], n_e, SKY_E_NOT_FINITE, SKY_E_NOT_ASCENDING)]
    if image:
        axes += [(c["xe"], n_x, SKY_X_NOT_FINITE, SKY_X_NOT_ASCENDING), (c["ye"], n_y, SKY_Y_NOT_FINITE, SKY_Y_NOT_ASCENDING)]
    for a in axes:
        why = axis(*a)
        if why != OK:
            return why, None
    if n_tau < 1:
        return NO_TAU_BINS, None
    n_bins = per_tau * n_tau
    if n_bins > 2 ** 31 - 1:
        return TOO_MANY_BINS, None
    why = axis(c["taue"], n_tau, TAU_NOT_FINITE, TAU_NOT_ASCENDING)
    if why != OK:
        return why, None
    if not np.isfinite(c["step_frac"]) or c["step_frac"] < 0:
        return BAD_STEP_FRAC, None
    if not np.isfinite(c["h_min"]) or not c["h_min"] > 0:
        return BAD_H_MIN, None
    if not 1 <= c["max_steps"] <= 1 << 20:
        return BAD_MAX_STEPS, None
    if not c["tau_stop"] > 0:
        return BAD_TAU_STOP, None
    cube = PLANES * 8 * n_bins
    counters, head = cube, cube + 4 * 8 * n_obs
    out_bytes = head + 8 * 8
    staged_doubles = (10 if image else 4) * n_obs + n_t + 1 + n_e + 1 + (n_x + 1 + n_y + 1 if image else 0) + n_tau + 1
    staged = 8 * staged_doubles + 4 * 8 * n_obs                  # ... and the workgroup's four counters per observer
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
    grid = lambda slots, cus, per_cu: min(-(-slots // BLOCK), cus * per_cu, MAX_GRID)
    march = lambda slots: min(-(-slots // BLOCK), MARCH_MAX_GRID)
    staged_at = out_bytes
    clocks_at = staged_at + 8 * staged_doubles
    tau_at = clocks_at + 8 * 3
    index_at = tau_at + 8 * 1000
    status_at = index_at + 4 * 1000
    return OK, [path, int(image), n_bins, cube, counters, head, out_bytes, staged_doubles, staged, lds, 32 * n_obs, groups,
                grid(1, 256, 8), grid(100000, 256, 8), grid(2000000000, 304, 8), march(1), march(100000), march(2000000000),
                grid(100000, 256, groups), grid(2000000000, 304, groups), staged_at, clocks_at, tau_at, index_at, status_at, status_at + 4 * 1000]


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan(out, name):
    why, plan_ = plan_rule(PLANS[name])
    assert out["plan_" + name] == [why]
    if why == OK:
        assert out["planv_" + name] == plan_
        assert out["march_" + name] == [PLANS[name]["max_steps"], 1]
    else:
        assert "planv_" + name not in out


def test_plan_cases_are_what_they_are_meant_to_be(out):
    """every refusal the header can give occurs, where two faults meet the first in the order wins, and the path changes exactly at the LDS budget"""
    for name, why in REFUSED.items():
        assert out["plan_" + name] == [why], name
    assert set(REFUSED.values()) | {HYDRO_MISMATCH} == set(TEXTS)                   # (the engine checks the frame's context)
    for name in set(PLANS) - set(REFUSED):
        assert out["plan_" + name] == [OK], name
    assert out["constants"] == [PLANES, 4, 8, 5, 6, BLOCK, MAX_GRID, MARCH_MAX_GRID, 8, MATCH_BYTES]
    #                             path    image bins   cube  counters head  out
    assert out["planv_curve"][:7] == [PATH_LDS, 0, 6 * 32, 13824, 13824, 13856, 13920]
    assert out["planv_image"][:3] == [PATH_GLOBAL, 1, 6 * 480] == out["planv_empty_switch"][:3]                  # 9 x 8 x 2880 bytes: beyond the budget
    assert out["planv_lds_last_curve"][0] == PATH_LDS and out["planv_global_first_curve"][0] == PATH_GLOBAL
    assert out["planv_lds_last_curve"][9] <= LDS_BUDGET < out["planv_lds_last_curve"][9] + 2 * PLANES * 8 + 8             # one more energy bin would not fit
    assert out["planv_global_first_curve"][9] == out["planv_global_first_curve"][8] + MATCH_BYTES and out["planv_global_first_curve"][11] == 8
    assert out["planv_bench_image"][:4] == [PATH_GLOBAL, 1, 6 * 8 * 256 * 256, 72 * 6 * 8 * 256 * 256]
    assert out["planv_forced_global"][0] == PATH_GLOBAL and out["planv_forced_lds"] == out["planv_curve"] and out["planv_forced_global_beyond"] == out["planv_image"]
    assert out["planv_staging_last"][0] == PATH_GLOBAL and out["planv_staging_last"][9] == 81816
    assert out["planv_three"][2] == 3 * 6 * 480 and out["planv_surface_level_is_not_read"] == out["planv_image"] == out["planv_tau_stop_finite"]


def test_refusal_texts(out):
    for why, t in TEXTS.items():
        assert out["text_%d" % why] == t, why
    assert len(set(TEXTS.values())) == len(TEXTS) == 18 + 4 + 4 + 4 and all(t.startswith("observe_escaping: ") for t in TEXTS.values())


def test_layout_and_weight(out):
    per_tau = 4 * 8 * 3 * 5
    assert out["bin_index"] == [0, 1, per_tau, 6 * per_tau, (((((2 * 6 + 5) * 4 + 3) * 8 + 7) * 3 + 2) * 5 + 4)]      # x fastest ... then optical depth, then observer
    assert out["weight"] == [1, 1]                                                     # exp(-0) is 1 exactly


def test_escape_bin_equals_the_checker(out):
    q = photons()
    rows = np.array(out["ph"]).reshape(N_PHOTONS, N_OBS, 2)
    marched = dict(tau=q["tau"], status=np.full(N_PHOTONS, sc.LEFT_MESH), bound=np.zeros(N_PHOTONS), fragile=np.zeros(N_PHOTONS, dtype=bool))
    everyone = np.full(N_OBS, -1.0)                                                    # (the bin does not ask whether the photon is accepted)
    n_tau, n_t, n_e, n_x, n_y = (len(q[k]) - 1 for k in ("taue", "te", "ee", "xe", "ye"))
    for col, image in ((0, True), (1, False)):
        kw = dict(ex=q["ex"], ey=q["ey"], x_edges=q["xe"], y_edges=q["ye"]) if image else {}
        want = ec.observation(q["ph"], marched, q["n"], everyone, q["te"], q["ee"], q["taue"], q["tn"], **kw)
        per_obs = n_tau * n_t * n_e * (n_y * n_x if image else 1)
        flat = np.where(want["bin"] >= 0, want["bin"] + per_obs * np.arange(N_OBS)[:, None], -1)
        assert np.array_equal(rows[:, :, col].T, flat), image
        assert (flat >= 0).sum() > 1000 and (flat < 0).sum() > 100
    on_edge = np.isin(q["tau"], ec.TAU_EDGES[:-1]) & (q["tau"] > 0)
    assert on_edge.sum() > 10 and (q["tau"] == 0).sum() >= 30 and np.isnan(q["tau"]).sum() > 10
    itau = S.find_bin(q["taue"], q["tau"])
    assert (ec.TAU_EDGES[itau[on_edge]] == q["tau"][on_edge]).all() and (itau[q["tau"] == 0] == 0).all() and (itau[np.isnan(q["tau"])] == -1).all()


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
