"""The host's rules for line-of-sight optical depths (mcrat_amd/csrc/sightline_plan.hpp) on the CPU: every refusal, its text and the order in which
they fire, the layout of the output block, the grid rule, and the five per-ray functions the kernel calls -- direction, step length, midpoint,
advance, surface predicate -- against the definitions restated here in NumPy, compared as %.17g strings.  They are plain C++: a small driver is
compiled with g++ and what it prints is compared.  The same driver is built a second time with -fsanitize=address,undefined and run once."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NO_RAYS, BAD_STEP_FRAC, BAD_H_MIN, BAD_MAX_STEPS, BAD_TAU_STOP, BAD_SURFACE_LEVEL, BAD_REFILL_SWITCH = range(8)
TEXTS = {
    NO_RAYS: "sightline: n must be at least 1",
    BAD_STEP_FRAC: "sightline: step_frac must be finite and not negative",
    BAD_H_MIN: "sightline: h_min must be finite and positive",
    BAD_MAX_STEPS: "sightline: max_steps must lie between 1 and 1048576",
    BAD_TAU_STOP: "sightline: tau_stop must be positive (+inf: never opaque)",
    BAD_SURFACE_LEVEL: "sightline: surface_level must be a number below +inf (negative: no surface)",
    BAD_REFILL_SWITCH: "sightline: MCRAT_HIP_SIGHTLINE_REFILL must be 0 or 1",
}
INF, NAN = float("inf"), float("nan")
GOOD = dict(n=1000, step_frac=0.01, h_min=1e6, max_steps=1024, tau_stop=INF, surface_level=1.0, forced=-1)
# name: what differs from GOOD, and the refusal expected.  The later entries break several rules at once: the first in the documented order decides.
PLANS = {
    "good": ({}, OK),
    "one_ray": (dict(n=1), OK),
    "step_frac_zero": (dict(step_frac=0.0), OK),
    "max_steps_1": (dict(max_steps=1), OK),
    "max_steps_2_20": (dict(max_steps=1 << 20), OK),
    "tau_stop_20": (dict(tau_stop=20.0), OK),
    "surface_off": (dict(surface_level=-1.0), OK),
    "surface_minus_inf": (dict(surface_level=-INF), OK),
    "surface_zero": (dict(surface_level=0.0), OK),
    "forced_plain": (dict(forced=0), OK),
    "forced_refill": (dict(forced=1), OK),
    "odd_n": (dict(n=257, forced=1), OK),
    "n_zero": (dict(n=0), NO_RAYS),
    "n_negative": (dict(n=-5), NO_RAYS),
    "step_frac_negative": (dict(step_frac=-1e-9), BAD_STEP_FRAC),
    "step_frac_inf": (dict(step_frac=INF), BAD_STEP_FRAC),
    "step_frac_nan": (dict(step_frac=NAN), BAD_STEP_FRAC),
    "h_min_zero": (dict(h_min=0.0), BAD_H_MIN),
    "h_min_negative": (dict(h_min=-1.0), BAD_H_MIN),
    "h_min_inf": (dict(h_min=INF), BAD_H_MIN),
    "h_min_nan": (dict(h_min=NAN), BAD_H_MIN),
    "max_steps_zero": (dict(max_steps=0), BAD_MAX_STEPS),
    "max_steps_beyond": (dict(max_steps=(1 << 20) + 1), BAD_MAX_STEPS),
    "tau_stop_zero": (dict(tau_stop=0.0), BAD_TAU_STOP),
    "tau_stop_negative": (dict(tau_stop=-3.0), BAD_TAU_STOP),
    "tau_stop_nan": (dict(tau_stop=NAN), BAD_TAU_STOP),
    "surface_nan": (dict(surface_level=NAN), BAD_SURFACE_LEVEL),
    "surface_inf": (dict(surface_level=INF), BAD_SURFACE_LEVEL),
    "order_n_first": (dict(n=0, step_frac=-1.0, h_min=0.0, max_steps=0, tau_stop=0.0, surface_level=NAN), NO_RAYS),
    "order_step_frac": (dict(step_frac=NAN, h_min=0.0, max_steps=0, tau_stop=0.0, surface_level=NAN), BAD_STEP_FRAC),
    "order_h_min": (dict(h_min=NAN, max_steps=0, tau_stop=0.0, surface_level=NAN), BAD_H_MIN),
    "order_max_steps": (dict(max_steps=-1, tau_stop=NAN, surface_level=INF), BAD_MAX_STEPS),
    "order_tau_stop": (dict(tau_stop=-1.0, surface_level=INF), BAD_TAU_STOP),
}
SWITCHES = {"unset": (None, OK, -1), "empty": ("", OK, -1), "zero": ("0", OK, 0), "one": ("1", OK, 1), "two": ("2", BAD_REFILL_SWITCH, -1),
            "word": ("on", BAD_REFILL_SWITCH, -1), "padded": ("1 ", BAD_REFILL_SWITCH, -1)}
GRIDS = [(1, 0, 256), (256, 0, 256), (257, 0, 256), (1000000, 0, 256), (1, 1, 256), (257, 1, 256), (1000000, 1, 256), (1000000, 1, 0), (5000, 1, 4)]
N_RAYS = 2000

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sightline_plan.hpp"
using namespace mcrat;

static void plan(const char *name, int n, double step_frac, double h_min, int max_steps, double tau_stop, double surface_level, int forced)
{
    SightlinePlan p;
    const SightlineParams q{step_frac, h_min, max_steps, tau_stop, surface_level};
    const SightlineRefusal why = sightline_plan(n, q, forced, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why == SIGHTLINE_OK)
        printf("planv_%s: %d %d %zu %zu %zu %zu %zu %zu %zu\n", name, p.n, (int)p.refill, p.f8_offset, p.i4_offset, p.out_bytes, p.ray_offset, p.ray_bytes,
               sightline_f8_plane(p, SL_SURFACE_R2), sightline_i4_plane(p, SL_SURFACE_STEP));
}
static void refill_switch(const char *name, const char *env)
{
    int forced = 7;
    const SightlineRefusal why = sightline_refill_switch(env, &forced);
    printf("switch_%s: %d %d\n", name, (int)why, forced);
}
static void grid(int n, int refill, int cus)
{
    SightlinePlan p;
    const SightlineParams q{0.01, 1.0, 16, INFINITY, -1.0};
    if (sightline_plan(n, q, refill, &p) != SIGHTLINE_OK) exit(3);
    const int g = sightline_grid(p, cus);
    printf("grid_%d_%d_%d: %d %d\n", n, refill, cus, g, sightline_own_rays(n, g));
}
static std::vector<double> read_doubles(FILE *f, size_t n)
{
    std::vector<double> v(n);
    if (fread(v.data(), sizeof(double), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
@CASES@
    for (int k = 1; k <= (int)SIGHTLINE_BAD_REFILL_SWITCH; ++k) printf("text_%d:%s\n", k, sightline_refusal_text((SightlineRefusal)k));
    printf("status: %d %d %d %d %d %d\n", (int)SIGHTLINE_SKIPPED, (int)SIGHTLINE_LEFT_MESH, (int)SIGHTLINE_OPAQUE, (int)SIGHTLINE_STEP_CAP, (int)SIGHTLINE_OFF_TABLE,
           SIGHTLINE_N_STATUS);
    printf("constants: %d %d %d %d\n", SIGHTLINE_BLOCK, SIGHTLINE_HEAD_WORDS, SIGHTLINE_COUNTER_WORD, (int)SIGHTLINE_REFILL_DEFAULT);
    printf("surface: %d %d %d %d %d\n", (int)sightline_surface_reached(3.0, 2.0, 1.0), (int)sightline_surface_reached(3.0, 1.5, 1.0),
           (int)sightline_surface_reached(NAN, 0.0, 1.0), (int)sightline_surface_reached(INFINITY, INFINITY, 1.0), (int)sightline_surface_reached(0.0, 0.0, 0.0));
    if (argc < 2) return 0;
    // the rays: header {n} as a double, then x, y, z, p1, p2, p3, step_frac, h_min, total, partial, level [n each]
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const size_t n = (size_t)read_doubles(f, 1)[0];
    const std::vector<double> x = read_doubles(f, n), y = read_doubles(f, n), z = read_doubles(f, n), p1 = read_doubles(f, n), p2 = read_doubles(f, n),
                              p3 = read_doubles(f, n), sf = read_doubles(f, n), hm = read_doubles(f, n), tot = read_doubles(f, n), par = read_doubles(f, n),
                              lev = read_doubles(f, n);
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        double nx, ny, nz, mx, my, mz, ax = x[i], ay = y[i], az = z[i];
        sightline_direction(p1[i], p2[i], p3[i], nx, ny, nz);
        const double h = sightline_step_length(x[i], y[i], z[i], sf[i], hm[i]);
        sightline_midpoint(x[i], y[i], z[i], h, nx, ny, nz, mx, my, mz);
        sightline_advance(ax, ay, az, h, nx, ny, nz);
        printf("ray: %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", nx, ny, nz, h, mx, my, mz, ax, ay, az,
               (int)sightline_surface_reached(tot[i], par[i], lev[i]));
    }
    return 0;
}
'''


def _lit(v):
    if isinstance(v, int):
        return "%d" % v
    return "NAN" if v != v else {INF: "INFINITY", -INF: "-INFINITY"}.get(v, repr(v))


def _cases():
    lines = []
    for name, (change, _) in PLANS.items():
        q = dict(GOOD, **change)
        lines.append('plan("%s", %s);' % (name, ", ".join(_lit(q[k]) for k in ("n", "step_frac", "h_min", "max_steps", "tau_stop", "surface_level", "forced"))))
    for name, (env, _, _) in SWITCHES.items():
        lines.append('refill_switch("%s", %s);' % (name, "nullptr" if env is None else '"%s"' % env))
    for n, refill, cus in GRIDS:
        lines.append("grid(%d, %d, %d);" % (n, refill, cus))
    return "\n".join("    " + l for l in lines)


def rays():
    """2000 seeded rays: positions 1e9 .. 1e13 cm, momenta over six decades in any direction.  The first 200 have step_frac = 0, the next 200 an
    h_min above step_frac * rho, the next 20 start at the origin; partial sums on total - level and one spacing to either side of it"""
    g = np.random.default_rng(20250301)
    n = N_RAYS
    r = 10.0 ** g.uniform(9, 13, n)
    d = g.standard_normal((3, n))
    x, y, z = r * d / np.sqrt((d * d).sum(axis=0))
    p = 10.0 ** g.uniform(-20, -14, n) * g.standard_normal((3, n))
    sf = 10.0 ** g.uniform(-4, -1, n)
    hm = 10.0 ** g.uniform(3, 7, n)
    sf[:200] = 0.0
    hm[200:400] = 10.0 ** g.uniform(12, 14, 200)
    x[400:420] = y[400:420] = z[400:420] = 0.0
    tot = 10.0 ** g.uniform(-3, 3, n)
    lev = np.where(g.random(n) < 0.5, 1.0, 10.0 ** g.uniform(-2, 1, n))
    par = tot * g.random(n)
    tot[500:800] = g.integers(32, 800, 300) / 8.0          # multiples of 1/8 with tot >= 2 * lev: tot - lev and the differences below are exact
    lev[500:800] = g.integers(1, 16, 300) / 8.0
    exact = tot - lev
    par[500:600] = exact[500:600]
    par[600:700] = np.nextafter(exact[600:700], -INF)
    par[700:800] = np.nextafter(exact[700:800], INF)
    return dict(x=x, y=y, z=z, p1=p[0], p2=p[1], p3=p[2], sf=sf, hm=hm, tot=tot, par=par, lev=lev)


def _build(d, src, name, extra):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("sightline_plan")
    src, data = d / "driver.cpp", d / "rays.bin"
    src.write_text(DRIVER.replace("@CASES@", _cases()))
    q = rays()
    np.concatenate([np.array([float(N_RAYS)])] + [q[k] for k in ("x", "y", "z", "p1", "p2", "p3", "sf", "hm", "tot", "par", "lev")]).tofile(data)
    return d, src, data


@pytest.fixture(scope="module")
def text(built):
    d, src, data = built
    return subprocess.run([str(_build(d, src, "driver", [])), str(data)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def out(text):
    res = {"ray": []}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        if key == "ray":
            res["ray"].append(vals.split())
        else:
            res[key] = vals if key.startswith("text_") else [int(v) for v in vals.split()]
    return res


def test_refusals_their_texts_and_their_order(out):
    for name, (_, want) in PLANS.items():
        assert out["plan_" + name] == [want], name
        assert ("planv_" + name in out) == (want == OK), name
    for k, t in TEXTS.items():
        assert out["text_%d" % k] == t
    assert len(set(TEXTS.values())) == len(TEXTS) == 7


def test_refill_switch(out):
    for name, (_, why, forced) in SWITCHES.items():
        assert out["switch_" + name] == [why, forced], name


def test_status_values_and_layout(out):
    assert out["status"] == [0, 1, 2, 3, 4, 5]
    block, head_words, counter_word, default = out["constants"]
    assert block == 256 and head_words == 8 and counter_word == 5 and default in (0, 1)
    for name, (change, want) in PLANS.items():
        if want != OK:
            continue
        q = dict(GOOD, **change)
        n = q["n"]
        refill = default if q["forced"] < 0 else q["forced"]
        f8, i4 = 64, 64 + 8 * 5 * n
        out_bytes = i4 + 4 * 3 * n
        ray_offset = -(-out_bytes // 256) * 256
        assert out["planv_" + name] == [n, refill, f8, i4, out_bytes, ray_offset, 8 * 7 * n, f8 + 8 * 4 * n, i4 + 4 * 2 * n], name


def test_grid_rule(out):
    for n, refill, cus in GRIDS:
        want = -(-n // 256)
        if refill:
            want = min(want, (cus if cus > 0 else 256) * 4)
        own = (n * 3 // 4 // want) // 64 * 64
        assert out["grid_%d_%d_%d" % (n, refill, cus)] == [want, own]
        assert own * want <= n                       # the own ranges never reach beyond the rays


def test_surface_predicate_edge_cases(out):
    assert out["surface"] == [1, 0, 0, 0, 1]      # on the level: reached; NaN and inf - inf: not


def test_per_ray_functions_bit_for_bit(out):
    q = rays()
    x, y, z, p1, p2, p3, sf, hm = (q[k] for k in ("x", "y", "z", "p1", "p2", "p3", "sf", "hm"))
    ipn = 1 / np.sqrt((p1 * p1 + p2 * p2) + p3 * p3)
    nx, ny, nz = p1 * ipn, p2 * ipn, p3 * ipn
    rho = np.sqrt((x * x + y * y) + z * z)
    h = sf * rho
    h = np.where(h > hm, h, hm)
    half = 0.5 * h
    m = (x + half * nx, y + half * ny, z + half * nz)
    a = (x + h * nx, y + h * ny, z + h * nz)
    reached = (q["tot"] - q["par"]) <= q["lev"]
    want = [nx, ny, nz, h, *m, *a]
    got = out["ray"]
    assert len(got) == N_RAYS
    for i, row in enumerate(got):
        assert row[:10] == ["%.17g" % w[i] for w in want], i
        assert int(row[10]) == int(reached[i]), i
    # what the sample holds: the floor in use, step_frac = 0, starts at the origin, and the predicate decided on its boundary both ways
    assert (h[:200] == hm[:200]).all() and (h[200:400] == hm[200:400]).all() and (h[420:] > hm[420:]).sum() > 1000
    assert (rho[400:420] == 0).all() and (h[400:420] == hm[400:420]).all()
    assert reached[500:600].all() and not reached[600:700].any() and reached[700:800].all()


def test_driver_under_sanitizers(built):
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("\nray:") == N_RAYS
