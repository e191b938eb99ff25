"""The host's rules for a mock observation (mcrat_amd/csrc/observe_plan.hpp) on the CPU: every refusal and its text, the cube's layout, the rule
that picks the accumulation path on both sides of its LDS boundary, and the three per-photon functions the kernel uses -- accepted, t_det, find_bin
-- against the definitions restated here in NumPy: integers exactly, doubles (%.17g) for equality.  They are plain C++: a small driver is compiled
with g++ and what it prints is compared.  The same driver is built a second time with -fsanitize=address,undefined and run once."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_LIGHT = 2.99792458e10
(OK, NO_BINS, TOO_MANY_BINS, BAD_CONE, T_NOT_FINITE, T_NOT_ASCENDING, E_NOT_FINITE, E_NOT_ASCENDING, STAGING_TOO_LARGE, BAD_PATH_SWITCH,
 LDS_FORCED_TOO_LARGE) = range(11)
PATH_NONE, PATH_LDS, PATH_GLOBAL = 0, 1, 2
LDS_BUDGET = 80 * 1024            # half of gfx950's 160 KiB per CU: two workgroups share a CU

TEXTS = {
    NO_BINS: "observe: n_obs, n_t and n_e must each be at least 1",
    TOO_MANY_BINS: "observe: n_obs * n_t * n_e overflows an int",
    BAD_CONE: "observe: an observer's cone needs cos_lo > cos_hi",
    T_NOT_FINITE: "observe: t_edges holds a value that is not finite",
    T_NOT_ASCENDING: "observe: t_edges is not strictly ascending",
    E_NOT_FINITE: "observe: e_edges holds a value that is not finite",
    E_NOT_ASCENDING: "observe: e_edges is not strictly ascending",
    STAGING_TOO_LARGE: "observe: the edges and the observers' cosines do not fit the kernel's LDS budget",
    BAD_PATH_SWITCH: "observe: MCRAT_HIP_OBSERVE_PATH must be lds or global",
    LDS_FORCED_TOO_LARGE: "observe: MCRAT_HIP_OBSERVE_PATH=lds, but the cube does not fit the kernel's LDS budget",
}

INF, NAN = float("inf"), float("nan")
# name: (n_obs, cos_lo, cos_hi, n_t, t_edges, n_e, e_edges, forced path) -- the arrays as they are handed over; "ramp" stands for 0, 1, 2, ... of the
# length the count asks for
PLANS = {
    "small": (2, [1.0, 0.9], [0.9, 0.5], 4, [0.0, 1.0, 2.0, 3.0, 4.0], 8, "ramp", PATH_NONE),
    "one_bin": (1, [1.0], [0.9], 1, [0.0, 1.0], 1, [1.0, 2.0], PATH_NONE),
    "lds_last": (1, [1.0], [0.9], 2, "ramp", 682, "ramp", PATH_NONE),             # 120 * 682 + 80 bytes: the budget exactly
    "global_first": (1, [1.0], [0.9], 2, "ramp", 683, "ramp", PATH_NONE),
    "lds_last_1t": (1, [1.0], [0.9], 1, "ramp", 1278, "ramp", PATH_NONE),
    "global_first_1t": (1, [1.0], [0.9], 1, "ramp", 1279, "ramp", PATH_NONE),
    "beyond_lds": (4, [1.0, 0.9, 0.8, 0.7], [0.9, 0.8, 0.7, 0.6], 512, "ramp", 64, "ramp", PATH_NONE),
    "forced_global": (2, [1.0, 0.9], [0.9, 0.5], 4, "ramp", 8, "ramp", PATH_GLOBAL),
    "forced_lds": (2, [1.0, 0.9], [0.9, 0.5], 4, "ramp", 8, "ramp", PATH_LDS),
    "forced_lds_too_large": (1, [1.0], [0.9], 2, "ramp", 683, "ramp", PATH_LDS),
    "forced_global_beyond": (1, [1.0], [0.9], 2, "ramp", 683, "ramp", PATH_GLOBAL),
    "staging_last": (1, [1.0], [0.9], 10230, "ramp", 1, "ramp", PATH_NONE),       # 8 * (4 + 10231 + 2) + 16 = 81912 bytes staged
    "staging_too_large": (1, [1.0], [0.9], 10232, "ramp", 1, "ramp", PATH_NONE),
    "no_observer": (0, [], [], 4, "ramp", 8, "ramp", PATH_NONE),
    "no_t_bin": (1, [1.0], [0.9], 0, [0.0], 8, "ramp", PATH_NONE),
    "negative_e_bins": (1, [1.0], [0.9], 4, "ramp", -1, [], PATH_NONE),
    "per_observer_overflow": (1, [1.0], [0.9], 65536, [], 65536, [], PATH_NONE),          # 2^32 (the arrays are not looked at)
    "product_overflow": (3, [1.0], [0.9], 65536, [], 16384, [], PATH_NONE),               # 3 * 2^30
    "cone_equal": (2, [1.0, 0.5], [0.9, 0.5], 4, "ramp", 8, "ramp", PATH_NONE),
    "cone_backwards": (1, [0.5], [0.9], 4, "ramp", 8, "ramp", PATH_NONE),
    "cone_nan": (1, [NAN], [0.9], 4, "ramp", 8, "ramp", PATH_NONE),
    "t_inf": (1, [1.0], [0.9], 2, [0.0, 1.0, INF], 8, "ramp", PATH_NONE),
    "t_nan": (1, [1.0], [0.9], 2, [0.0, NAN, 2.0], 8, "ramp", PATH_NONE),
    "t_equal": (1, [1.0], [0.9], 2, [0.0, 1.0, 1.0], 8, "ramp", PATH_NONE),
    "t_descending": (1, [1.0], [0.9], 2, [0.0, 2.0, 1.0], 8, "ramp", PATH_NONE),
    "e_minus_inf": (1, [1.0], [0.9], 2, "ramp", 2, [-INF, 1.0, 2.0], PATH_NONE),
    "e_equal": (1, [1.0], [0.9], 2, "ramp", 2, [1.0, 1.0, 2.0], PATH_NONE),
    "t_before_e": (1, [1.0], [0.9], 2, [0.0, 0.0, 1.0], 2, [NAN, 1.0, 2.0], PATH_NONE),           # the first check to fire decides
    "cone_before_edges": (1, [0.5], [0.5], 2, [0.0, 0.0, 1.0], 2, "ramp", PATH_NONE),
}
# The rule the three binned sums share (accumulate_rule): name: (staged bytes, accumulator bytes, match-table bytes, forced path), at the boundaries
# the products pin -- observe 1 x 2 x 682 | 683 (5536 B staged, 112 B per energy bin), observe_sky the same cube behind 8 KiB of match tables,
# radiation_field 1462 | 1463 x 1 shells (8 * (n_r + 3) + 24 B staged, 48 B per shell)
MATCH_BYTES = 4 * 2048
RULES = {
    "observe_last": (5536, LDS_BUDGET - 5536, 0, PATH_NONE),                       # the cube is the budget minus the staged part: still LDS
    "observe_first": (5544, 112 * 683, 0, PATH_NONE),                              # one bin more
    "sky_last": (5536, LDS_BUDGET - 5536, MATCH_BYTES, PATH_NONE),
    "sky_first": (5544, 112 * 683, MATCH_BYTES, PATH_NONE),
    "radfield_last": (8 * 1465 + 24, 48 * 1462, MATCH_BYTES, PATH_NONE),
    "radfield_first": (8 * 1466 + 24, 48 * 1463, MATCH_BYTES, PATH_NONE),
    "one_byte_over": (5536, LDS_BUDGET - 5536 + 1, 0, PATH_NONE),
    "forced_lds_fits": (208, 3584, MATCH_BYTES, PATH_LDS),
    "forced_global_fits": (208, 3584, MATCH_BYTES, PATH_GLOBAL),
    "forced_lds_beyond": (5544, 112 * 683, MATCH_BYTES, PATH_LDS),                 # does not fit: the caller refuses, told by `fits`
    "forced_global_beyond": (5544, 112 * 683, MATCH_BYTES, PATH_GLOBAL),
    "no_room_for_match": (LDS_BUDGET - MATCH_BYTES + 8, 56 * 10 ** 6, MATCH_BYTES, PATH_NONE),      # staged + tables beyond the budget: one workgroup per CU is all that is left (observe_sky refuses this)
    "room_for_match_exactly": (LDS_BUDGET - MATCH_BYTES, 56 * 10 ** 6, MATCH_BYTES, PATH_NONE),
    "tiny_global": (24, 56 * 10 ** 6, 0, PATH_NONE),                               # hundreds would share a CU's LDS: eight
    "cells": (24, 48 * 2 ** 20, MATCH_BYTES, PATH_GLOBAL),                         # radiation_field CELLS
}
EDGES = {"ramp": [0.0, 1.0, 2.0], "one_bin": [1.0, 2.0], "nan": [0.0, NAN, 2.0], "inf": [0.0, 1.0, INF], "minus_inf": [-INF, 1.0, 2.0], "equal": [0.0, 1.0, 1.0],
         "descending": [0.0, 2.0, 1.0], "nan_and_equal": [1.0, 1.0, NAN], "equal_first_pair": [0.0, 0.0, 1.0]}
EDGES_OK, EDGES_NOT_FINITE, EDGES_NOT_ASCENDING = 0, 1, 2
# (items, block, CUs, workgroups per CU, hard maximum or 0)
GRIDS = {"one": (1, 256, 256, 8, 0), "ragged": (4099, 256, 256, 8, 0), "capped": (10 ** 6, 256, 256, 2, 0), "cus_unknown": (10 ** 6, 256, 0, 8, 0),
         "hard_max": (10 ** 7, 256, 304, 8, 2048), "hard_max_unreached": (10 ** 6, 256, 256, 2, 2048), "few_cus": (10 ** 6, 256, 4, 8, 2048)}
SWITCHES = {"unset": None, "empty": "", "lds": "lds", "global": "global", "upper": "LDS", "other": "hbm", "number": "1"}

N_PHOTONS, N_OBS = 2000, 3

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <vector>
#include "observe_plan.hpp"
using namespace mcrat;

static std::vector<double> ramp(int n) { std::vector<double> v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }
static void plan(const char *name, int n_obs, std::vector<double> lo, std::vector<double> hi, int n_t, std::vector<double> te, int n_e, std::vector<double> ee, int forced)
{
    ObservePlan p;
    const ObserveRefusal why = observe_plan(n_obs, lo.data(), hi.data(), n_t, te.data(), n_e, ee.data(), (ObservePath)forced, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why == OBSERVE_OK)
        printf("planv_%s: %d %d %zu %zu %zu %zu %zu %d\n", name, (int)p.path, p.n_bins, p.cube_bytes, p.out_bytes, p.staged_doubles, p.staged_bytes, p.lds_bytes,
               p.groups_per_cu);
}
static void path_switch(const char *name, const char *env)
{
    ObservePath forced = OBSERVE_PATH_GLOBAL;
    const ObserveRefusal why = observe_path_switch(env, &forced);
    printf("switch_%s: %d %d\n", name, (int)why, (int)forced);
}
static void rule(const char *name, size_t staged, size_t acc, size_t match, int forced)
{
    const AccumulateRule r = accumulate_rule(staged, acc, match, (ObservePath)forced);
    printf("rule_%s: %d %d %zu %d\n", name, (int)r.fits, (int)r.path, r.lds_bytes, r.groups_per_cu);
}
static void edges(const char *name, std::vector<double> e)
{
    printf("edges_%s: %d %d\n", name, (int)edges_check(e.data(), (int)e.size() - 1), (int)edges_refusal(e.data(), (int)e.size() - 1, 7, 8, 9));
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
    for (int k = 1; k <= (int)OBSERVE_LDS_FORCED_TOO_LARGE; ++k) printf("text_%d:%s\n", k, observe_refusal_text((ObserveRefusal)k));
    printf("constants: %d %zu\n", OBSERVE_PLANES, OBSERVE_LDS_BUDGET);
    printf("match: %d %d %zu %u %u %u\n", OBSERVE_BLOCK, OBSERVE_MATCH_BITS, OBSERVE_MATCH_BYTES, observe_match_hash(0), observe_match_hash(1), observe_match_hash(2147483647));
    printf("bin_index: %zu %zu %zu\n", observe_bin(0, 0, 0, 4, 8), observe_bin(1, 2, 3, 4, 8), observe_bin(2, 3, 7, 4, 8));
    printf("observable: %d %d %d %d %d %d\n", (int)observe_observable(FLAG_VALID, 'i', 1.0), (int)observe_observable(FLAG_VALID | FLAG_MOVES, 'c', 2.5),
           (int)observe_observable(FLAG_MOVES, 'i', 1.0), (int)observe_observable(FLAG_VALID, 'i', 0.0), (int)observe_observable(FLAG_VALID, 'p', 1.0),
           (int)observe_observable(FLAG_VALID, 'N', 1.0));
    if (argc < 2) return 0;
    // the photons: header {n, n_obs, n_t, n_e} as doubles, then time_now[n], r0, r1, r2, p0, p3 [n each], cos_obs, sin_obs, cos_lo, cos_hi, the edges
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<double> head = read_doubles(f, 4);
    const size_t n = (size_t)head[0];
    const int n_obs = (int)head[1], n_t = (int)head[2], n_e = (int)head[3];
    const std::vector<double> tn = read_doubles(f, n), r0 = read_doubles(f, n), r1 = read_doubles(f, n), r2 = read_doubles(f, n), p0 = read_doubles(f, n),
                              p3 = read_doubles(f, n), co = read_doubles(f, n_obs), so = read_doubles(f, n_obs), lo = read_doubles(f, n_obs),
                              hi = read_doubles(f, n_obs), te = read_doubles(f, n_t + 1), ee = read_doubles(f, n_e + 1);
    fclose(f);
    printf("ends: %d %d %d %d %d\n", observe_find_bin(ee.data(), n_e, ee[0]), observe_find_bin(ee.data(), n_e, ee[n_e]),
           observe_find_bin(ee.data(), n_e, nextafter(ee[n_e], 0.0)), observe_find_bin(ee.data(), n_e, nextafter(ee[0], 0.0)), observe_find_bin(ee.data(), n_e, NAN));
    for (size_t i = 0; i < n; ++i)
        for (int o = 0; o < n_obs; ++o) {
            const double t = observe_t_det(tn[i], r0[i], r1[i], r2[i], co[o], so[o]), e = observe_energy(p0[i]);
            printf("ph: %d %.17g %.17g %d %d\n", (int)observe_accepted(p0[i], p3[i], lo[o], hi[o]), t, e, observe_find_bin(te.data(), n_t, t),
                   observe_find_bin(ee.data(), n_e, e));
        }
    return 0;
}
'''


def _vec(v, n):
    if isinstance(v, str):
        return "ramp(%d)" % n
    lit = {INF: "INFINITY", -INF: "-INFINITY"}
    return "{%s}" % ", ".join("NAN" if x != x else lit.get(x, repr(x)) for x in v)


def _cases():
    lines = []
    for name, (n_obs, lo, hi, n_t, te, n_e, ee, forced) in PLANS.items():
        lines.append('plan("%s", %d, %s, %s, %d, %s, %d, %s, %d);' % (name, n_obs, _vec(lo, 0), _vec(hi, 0), n_t, _vec(te, n_t), n_e, _vec(ee, n_e), forced))
    for name, env in SWITCHES.items():
        lines.append('path_switch("%s", %s);' % (name, "nullptr" if env is None else '"%s"' % env))
    for name, (staged, acc, match, forced) in RULES.items():
        lines.append('rule("%s", %d, %d, %d, %d);' % (name, staged, acc, match, forced))
    for name, e in EDGES.items():
        lines.append('edges("%s", %s);' % (name, _vec(e, 0)))
    for name, g in GRIDS.items():
        lines.append('printf("grid_%s: %%d\\n", accumulate_grid(%dLL, %d, %d, %d, %d));' % ((name,) + g))
    return "\n".join("    " + l for l in lines)


def photons():
    """~2000 seeded photons and 3 observers whose cones overlap; some edges are the exact t_det and e of chosen photons"""
    g = np.random.default_rng(20240611)
    n = N_PHOTONS
    r = 10.0 ** g.uniform(12, 13, n)
    th, phi = g.uniform(0, 0.3, n), g.uniform(0, 2 * np.pi, n)
    r0, r1, r2 = r * np.sin(th) * np.cos(phi), r * np.sin(th) * np.sin(phi), r * np.cos(th)
    p0 = 10.0 ** g.uniform(-20, -14, n)
    p3 = p0 * np.cos(g.uniform(0, 0.3, n))
    tn = g.uniform(300.0, 400.0, n)
    theta_obs = np.array([0.02, 0.1, 0.18])
    co, so = np.cos(theta_obs), np.sin(theta_obs)
    lo, hi = np.cos(np.maximum(theta_obs - 0.07, 0.0)), np.cos(theta_obs + 0.07)
    lo[0] = 1.0
    e = p0 * C_LIGHT
    t1 = tn - ((r2 * co[1] + np.sqrt(r0 * r0 + r1 * r1) * so[1]) / C_LIGHT)
    te = np.unique(np.concatenate([np.linspace(t1.min() - 1.0, np.percentile(t1, 90), 12), t1[[5, 17, 900]]]))
    ee = np.unique(np.concatenate([10.0 ** np.linspace(-9.5, -4.2, 20), e[[3, 11, 1200]]]))
    return dict(tn=tn, r0=r0, r1=r1, r2=r2, p0=p0, p3=p3, co=co, so=so, lo=lo, hi=hi, te=te, ee=ee)


def find_bin(edges, x):
    """edges[k] <= x < edges[k + 1], else -1"""
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1), k, -1)


def _build(d, src, name, extra):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("observe_plan")
    src, data = d / "driver.cpp", d / "photons.bin"
    src.write_text(DRIVER.replace("@CASES@", _cases()))
    q = photons()
    head = np.array([N_PHOTONS, N_OBS, len(q["te"]) - 1, len(q["ee"]) - 1], dtype=np.float64)
    np.concatenate([head] + [q[k] for k in ("tn", "r0", "r1", "r2", "p0", "p3", "co", "so", "lo", "hi", "te", "ee")]).tofile(data)
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


def plan_rule(n_obs, lo, hi, n_t, te, n_e, ee, forced):
    """observe_plan restated: the checks in their order, the layout, the path"""
    ramp = lambda v, n: [float(k) for k in range(n + 1)] if isinstance(v, str) else v
    if n_obs < 1 or n_t < 1 or n_e < 1:
        return NO_BINS, None
    if n_t * n_e > 2 ** 31 - 1 or n_t * n_e * n_obs > 2 ** 31 - 1:
        return TOO_MANY_BINS, None
    if not all(a > b for a, b in zip(lo, hi)):
        return BAD_CONE, None
    for edges, not_finite, not_ascending in ((ramp(te, n_t), T_NOT_FINITE, T_NOT_ASCENDING), (ramp(ee, n_e), E_NOT_FINITE, E_NOT_ASCENDING)):
        if not all(np.isfinite(edges)):
            return not_finite, None
        if not all(a < b for a, b in zip(edges[:-1], edges[1:])):
            return not_ascending, None
    n_bins = n_obs * n_t * n_e
    cube = 7 * 8 * n_bins                                        # count, W, WE, I, Q, U, V: 8 bytes each
    staged_doubles = 4 * n_obs + n_t + 1 + n_e + 1
    staged = 8 * staged_doubles + 2 * 8 * n_obs                  # ... and the workgroup's two counters per observer
    if staged > LDS_BUDGET:
        return STAGING_TOO_LARGE, None
    fits = staged + cube <= LDS_BUDGET
    if forced == PATH_LDS and not fits:
        return LDS_FORCED_TOO_LARGE, None
    path = forced if forced != PATH_NONE else (PATH_LDS if fits else PATH_GLOBAL)
    lds = staged + (cube if path == PATH_LDS else 0)
    return OK, [path, n_bins, cube, cube + 16 * n_obs, staged_doubles, staged, lds, 2 if path == PATH_LDS else min(2 * LDS_BUDGET // lds, 8)]  # workgroups per CU: two on the LDS path (the flushes meet at the same addresses), up to 8 on the global path


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan(out, name):
    why, plan = plan_rule(*PLANS[name])
    assert out["plan_" + name] == [why]
    if why == OK:
        assert out["planv_" + name] == plan
    else:
        assert "planv_" + name not in out


def test_plan_cases_are_what_they_are_meant_to_be(out):
    """... so that the table above cannot drift into testing nothing: every refusal occurs, and the path changes exactly at the LDS budget"""
    refused = {"no_observer": NO_BINS, "no_t_bin": NO_BINS, "negative_e_bins": NO_BINS, "per_observer_overflow": TOO_MANY_BINS, "product_overflow": TOO_MANY_BINS,
               "cone_equal": BAD_CONE, "cone_backwards": BAD_CONE, "cone_nan": BAD_CONE, "t_inf": T_NOT_FINITE, "t_nan": T_NOT_FINITE, "t_equal": T_NOT_ASCENDING,
               "t_descending": T_NOT_ASCENDING, "e_minus_inf": E_NOT_FINITE, "e_equal": E_NOT_ASCENDING, "t_before_e": T_NOT_ASCENDING, "cone_before_edges": BAD_CONE,
               "staging_too_large": STAGING_TOO_LARGE, "forced_lds_too_large": LDS_FORCED_TOO_LARGE}
    for name, why in refused.items():
        assert out["plan_" + name] == [why], name
    assert set(refused.values()) | {BAD_PATH_SWITCH} == set(TEXTS)
    assert out["constants"] == [7, LDS_BUDGET] and 2 * LDS_BUDGET == 160 * 1024
    assert out["planv_small"] == [PATH_LDS, 64, 3584, 3616, 22, 208, 3792, 2]
    assert out["planv_lds_last"][0] == PATH_LDS and out["planv_lds_last"][6:] == [LDS_BUDGET, 2]       # the budget exactly: still LDS, two workgroups per CU
    assert out["planv_global_first"][7] == 8 and out["planv_beyond_lds"][7] == 8                        # the global path: LDS is no limit
    assert out["planv_global_first"][0] == PATH_GLOBAL and out["planv_global_first"][5] + out["planv_global_first"][2] == LDS_BUDGET + 120
    assert out["planv_global_first"][6] == out["planv_global_first"][5]                                 # the global path keeps only the staged inputs in LDS
    assert out["planv_lds_last_1t"][0] == PATH_LDS and out["planv_global_first_1t"][0] == PATH_GLOBAL
    assert out["planv_beyond_lds"][:3] == [PATH_GLOBAL, 4 * 512 * 64, 56 * 4 * 512 * 64]
    assert out["planv_one_bin"][0] == PATH_LDS
    assert out["planv_forced_global"][0] == PATH_GLOBAL and out["planv_forced_lds"][0] == PATH_LDS and out["planv_forced_global_beyond"][0] == PATH_GLOBAL
    assert out["planv_staging_last"][0] == PATH_GLOBAL and out["planv_staging_last"][5] == 81912


def accumulate_rule(staged, acc, match, forced):
    """the shared rule restated: fits, path, the kernel's dynamic LDS, workgroups per CU"""
    fits = staged + acc <= LDS_BUDGET
    path = forced if forced != PATH_NONE else (PATH_LDS if fits else PATH_GLOBAL)
    lds = staged + (acc if path == PATH_LDS else match)
    return [int(fits), path, lds, 2 if path == PATH_LDS else min(2 * LDS_BUDGET // lds, 8)]


@pytest.mark.parametrize("name", sorted(RULES))
def test_accumulate_rule(out, name):
    assert out["rule_" + name] == accumulate_rule(*RULES[name])


def test_accumulate_rule_cases_are_what_they_are_meant_to_be(out):
    """the path changes exactly where the staged part and the accumulator reach the budget, for each product's own boundary"""
    for product, match in (("observe", 0), ("sky", MATCH_BYTES), ("radfield", MATCH_BYTES)):
        last, first = RULES[product + "_last"], RULES[product + "_first"]
        assert last[0] + last[1] == LDS_BUDGET and LDS_BUDGET < first[0] + first[1] <= LDS_BUDGET + 120
        assert out["rule_%s_last" % product] == [1, PATH_LDS, LDS_BUDGET, 2]
        assert out["rule_%s_first" % product] == [0, PATH_GLOBAL, first[0] + match, 8]
    assert out["rule_one_byte_over"][:2] == [0, PATH_GLOBAL]
    assert out["rule_forced_lds_fits"] == [1, PATH_LDS, 208 + 3584, 2] and out["rule_forced_global_fits"] == [1, PATH_GLOBAL, 208 + MATCH_BYTES, 8]
    assert out["rule_forced_lds_beyond"][:2] == [0, PATH_LDS] and out["rule_forced_lds_beyond"][2] > LDS_BUDGET       # fits says no: every caller refuses
    assert out["rule_forced_global_beyond"] == [0, PATH_GLOBAL, 5544 + MATCH_BYTES, 8]
    assert out["rule_no_room_for_match"] == [0, PATH_GLOBAL, LDS_BUDGET + 8, 1] and out["rule_room_for_match_exactly"] == [0, PATH_GLOBAL, LDS_BUDGET, 2]
    assert out["rule_tiny_global"] == [0, PATH_GLOBAL, 24, 8] and out["rule_cells"] == [0, PATH_GLOBAL, 24 + MATCH_BYTES, 8]
    assert out["match"] == [256, 11, MATCH_BYTES, 0, (2654435761 >> 21), ((2147483647 * 2654435761) % 2 ** 32) >> 21]


def test_edges_check(out):
    """all finite first, then strictly ascending: which of the two failed, and the caller's own codes for them"""
    want = {"ramp": EDGES_OK, "one_bin": EDGES_OK, "nan": EDGES_NOT_FINITE, "inf": EDGES_NOT_FINITE, "minus_inf": EDGES_NOT_FINITE, "equal": EDGES_NOT_ASCENDING,
            "descending": EDGES_NOT_ASCENDING, "nan_and_equal": EDGES_NOT_FINITE, "equal_first_pair": EDGES_NOT_ASCENDING}
    assert set(want) == set(EDGES)
    for name, e in EDGES.items():
        rule = EDGES_NOT_FINITE if not all(np.isfinite(e)) else (EDGES_OK if all(a < b for a, b in zip(e[:-1], e[1:])) else EDGES_NOT_ASCENDING)
        assert rule == want[name], name
        assert out["edges_" + name] == [want[name], 7 + want[name]], name


def test_accumulate_grid(out):
    """what covers the items, at most the workgroups per CU on every CU (256 when the device does not say), never more than the hard maximum"""
    for name, (n, block, cus, per_cu, hard) in GRIDS.items():
        cap = (cus if cus > 0 else 256) * per_cu
        cap = min(cap, hard) if hard > 0 else cap
        assert out["grid_" + name] == [min(-(-n // block), cap)], name
    assert [out["grid_" + k][0] for k in ("one", "ragged", "capped", "cus_unknown", "hard_max", "hard_max_unreached", "few_cus")] == [1, 17, 512, 2048, 2048, 512, 32]


def test_path_switch(out):
    want = {"unset": [OK, PATH_NONE], "empty": [OK, PATH_NONE], "lds": [OK, PATH_LDS], "global": [OK, PATH_GLOBAL], "upper": [BAD_PATH_SWITCH, PATH_NONE],
            "other": [BAD_PATH_SWITCH, PATH_NONE], "number": [BAD_PATH_SWITCH, PATH_NONE]}
    for name in SWITCHES:
        assert out["switch_" + name] == want[name], name


def test_refusal_texts(out):
    for why, t in TEXTS.items():
        assert out["text_%d" % why] == t, why
    assert len(TEXTS) == LDS_FORCED_TOO_LARGE and len(set(TEXTS.values())) == len(TEXTS)


def test_layout_and_observable(out):
    assert out["bin_index"] == [0, (1 * 4 + 2) * 8 + 3, (2 * 4 + 3) * 8 + 7]             # observer-major, then time, then energy
    assert out["observable"] == [1, 1, 0, 0, 0, 0]                                        # not FLAG_VALID, weight 0, 'p', 'N'


def test_per_photon_functions_equal_the_numpy_restatement(out):
    q = photons()
    rows = out["ph"]
    assert len(rows) == N_PHOTONS * N_OBS
    got_acc = np.array([int(r[0]) for r in rows]).reshape(N_PHOTONS, N_OBS)
    got_t = np.array([float(r[1]) for r in rows]).reshape(N_PHOTONS, N_OBS)
    got_e = np.array([float(r[2]) for r in rows]).reshape(N_PHOTONS, N_OBS)
    got_it = np.array([int(r[3]) for r in rows]).reshape(N_PHOTONS, N_OBS)
    got_ie = np.array([int(r[4]) for r in rows]).reshape(N_PHOTONS, N_OBS)
    p0, p3, r0, r1, r2, tn = (q[k][:, None] for k in ("p0", "p3", "r0", "r1", "r2", "tn"))
    co, so, lo, hi = (q[k][None, :] for k in ("co", "so", "lo", "hi"))
    acc = (p3 <= p0 * lo) & (p3 > p0 * hi)
    e = np.broadcast_to(p0 * C_LIGHT, acc.shape)
    t = tn - ((r2 * co + np.sqrt(r0 * r0 + r1 * r1) * so) / C_LIGHT)
    assert (got_acc == acc).all()
    assert (got_t == t).all() and (got_e == e).all()                   # bit for bit (%.17g round-trips a double)
    it, ie = find_bin(q["te"], t), find_bin(q["ee"], e)
    assert (got_it == it).all() and (got_ie == ie).all()
    # the sample means something: every observer accepts some photons and not all, cones overlap, both axes have photons inside and outside, and
    # the photons whose t_det or e IS an edge sit in the bin that edge opens
    assert (acc.sum(axis=0) > 50).all() and (acc.sum(axis=0) < N_PHOTONS - 50).all() and (acc.sum(axis=1) >= 2).sum() > 50
    assert (it < 0).sum() > 10 and (it >= 0).sum() > 1000 and (ie < 0).sum() > 10 and (ie >= 0).sum() > 1000
    for i in (5, 17, 900):
        assert q["te"][it[i, 1]] == t[i, 1]
    for i in (3, 11, 1200):
        assert q["ee"][ie[i, 0]] == e[i, 0]


def test_find_bin_at_the_ends(out):
    """the first edge is inside, the last outside, the doubles next to them the other way round; a NaN is in no bin"""
    edges = photons()["ee"]
    assert out["ends"] == [0, -1, len(edges) - 2, -1, -1]
    assert find_bin(edges, np.array([edges[0], edges[-1], np.nextafter(edges[-1], 0.0), np.nextafter(edges[0], 0.0), NAN])).tolist() == out["ends"]


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
