"""The host's rules for the radiation field on the hydro mesh (mcrat_amd/csrc/radfield_plan.hpp) on the CPU: every refusal and its text and the order
in which the checks fire, the block's layout in both accumulator layouts, the rule that picks the accumulation path on both sides of its LDS
boundary, the grid size, and the per-photon functions the kernel uses -- r_mu and the shell bin -- against the definitions restated here in NumPy:
integers exactly, doubles (%.17g) for equality.  They are plain C++: a small driver is compiled with g++ and what it prints is compared.  The same
driver is built a second time with -fsanitize=address,undefined and run once."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(OK, BAD_MODE, NULL_EDGES, NO_BINS, TOO_MANY_BINS, R_NOT_FINITE, MU_NOT_FINITE, R_NOT_ASCENDING, MU_NOT_ASCENDING, STAGING_TOO_LARGE, BAD_PATH_SWITCH,
 LDS_ON_CELLS, LDS_TOO_LARGE, HYDRO_MISMATCH) = range(14)
CELLS, SHELLS = 0, 1
PATH_LDS, PATH_GLOBAL = 1, 2
LDS_BUDGET, LDS_PER_CU = 80 * 1024, 160 * 1024
MATCH_BYTES = 4 * 2048            # global path: a one-byte table of 2048 entries per wavefront of the 256-thread workgroup

TEXTS = {
    BAD_MODE: "radiation_field: mode must be MCRAT_HIP_RADFIELD_CELLS or MCRAT_HIP_RADFIELD_SHELLS",
    NULL_EDGES: "radiation_field: SHELLS needs r_edges and mu_edges",
    NO_BINS: "radiation_field: n_r and n_mu must each be at least 1",
    TOO_MANY_BINS: "radiation_field: n_r * n_mu overflows an int",
    R_NOT_FINITE: "radiation_field: r_edges holds a value that is not finite",
    MU_NOT_FINITE: "radiation_field: mu_edges holds a value that is not finite",
    R_NOT_ASCENDING: "radiation_field: r_edges is not strictly ascending",
    MU_NOT_ASCENDING: "radiation_field: mu_edges is not strictly ascending",
    STAGING_TOO_LARGE: "radiation_field: the edges do not fit the kernel's LDS budget",
    BAD_PATH_SWITCH: "radiation_field: MCRAT_HIP_RADFIELD_PATH must be lds or global",
    LDS_ON_CELLS: "radiation_field: MCRAT_HIP_RADFIELD_PATH=lds, but CELLS always accumulates in global memory",
    LDS_TOO_LARGE: "radiation_field: MCRAT_HIP_RADFIELD_PATH=lds, but the planes do not fit the kernel's LDS budget",
    HYDRO_MISMATCH: "radiation_field: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY) or on another device",
}

INF, NAN = float("inf"), float("nan")
# name: (mode, n_r, r_edges, n_mu, mu_edges, the switch) -- the arrays as they are handed over; "ramp": 0, 1, 2, ... of the length the count asks for;
# None: a null pointer
CHECKS = {
    "cells": (CELLS, 0, None, 0, None, None),
    "cells_ignores_edges": (CELLS, -3, None, 7, [NAN], ""),
    "cells_global": (CELLS, 0, None, 0, None, "global"),
    "cells_lds": (CELLS, 0, None, 0, None, "lds"),
    "cells_bad_switch": (CELLS, 0, None, 0, None, "hbm"),
    "mode_2": (2, 4, "ramp", 4, "ramp", None),
    "mode_negative": (-1, 4, "ramp", 4, "ramp", "hbm"),                          # the mode is checked before the switch
    "null_r": (SHELLS, 4, None, 4, "ramp", None),
    "null_mu": (SHELLS, 4, "ramp", 4, None, None),
    "null_before_counts": (SHELLS, 0, None, 0, None, None),
    "small": (SHELLS, 8, "ramp", 4, "ramp", None),
    "one_bin": (SHELLS, 1, [1.0, 2.0], 1, [-1.0, 1.5], None),
    "no_r": (SHELLS, 0, [1.0], 4, "ramp", None),
    "negative_mu": (SHELLS, 4, "ramp", -1, [1.0], None),
    "overflow": (SHELLS, 65536, [NAN], 32768, [NAN], None),                        # 2^31 (the arrays are not looked at)
    "largest_product": (SHELLS, 46340, "ramp", 46340, "ramp", None),               # 2 147 395 600 bins, but 92 682 edges: the staging check fires
    "r_inf": (SHELLS, 2, [0.0, 1.0, INF], 2, "ramp", None),
    "r_nan": (SHELLS, 2, [0.0, NAN, 2.0], 2, "ramp", None),
    "mu_minus_inf": (SHELLS, 2, "ramp", 2, [-INF, 0.0, 1.0], None),
    "r_equal": (SHELLS, 2, [0.0, 1.0, 1.0], 2, "ramp", None),
    "r_descending": (SHELLS, 2, [0.0, 2.0, 1.0], 2, "ramp", None),
    "mu_equal": (SHELLS, 2, "ramp", 2, [0.5, 0.5, 1.0], None),
    "finite_before_ascending": (SHELLS, 2, [0.0, 0.0, 1.0], 2, [0.0, NAN, 1.0], None),      # mu_edges not finite fires before r_edges not ascending
    "r_before_mu": (SHELLS, 2, [0.0, NAN, 1.0], 2, [0.0, NAN, 1.0], None),
    "edges_before_switch": (SHELLS, 2, [0.0, 0.0, 1.0], 2, "ramp", "hbm"),
    "lds_last": (SHELLS, 1462, "ramp", 1, "ramp", None),                           # 8 * 1465 + 24 + 48 * 1462 bytes: the budget exactly
    "global_first": (SHELLS, 1463, "ramp", 1, "ramp", None),
    "lds_last_64x": (SHELLS, 64, "ramp", 26, "ramp", None),                        # 760 + 48 * 64 * 26 = 80 632 bytes
    "global_first_64x": (SHELLS, 64, "ramp", 27, "ramp", None),                    # 768 + 48 * 64 * 27 = 83 712 bytes
    "bench_shells": (SHELLS, 64, "ramp", 32, "ramp", None),
    "forced_global": (SHELLS, 8, "ramp", 4, "ramp", "global"),
    "forced_lds": (SHELLS, 8, "ramp", 4, "ramp", "lds"),
    "forced_lds_too_large": (SHELLS, 1463, "ramp", 1, "ramp", "lds"),
    "forced_global_beyond": (SHELLS, 1463, "ramp", 1, "ramp", "global"),
    "bad_switch": (SHELLS, 8, "ramp", 4, "ramp", "LDS"),
    "staging_last": (SHELLS, 10234, "ramp", 1, "ramp", None),                      # 8 * (10235 + 2) + 24 = 81 920 bytes staged
    "staging_too_large": (SHELLS, 10235, "ramp", 1, "ramp", None),
    "staging_before_switch": (SHELLS, 10235, "ramp", 1, "ramp", "hbm"),
}
REFUSED = {"cells_lds": LDS_ON_CELLS, "cells_bad_switch": BAD_PATH_SWITCH, "mode_2": BAD_MODE, "mode_negative": BAD_MODE, "null_r": NULL_EDGES,
           "null_mu": NULL_EDGES, "null_before_counts": NULL_EDGES, "no_r": NO_BINS, "negative_mu": NO_BINS, "overflow": TOO_MANY_BINS,
           "largest_product": STAGING_TOO_LARGE, "r_inf": R_NOT_FINITE, "r_nan": R_NOT_FINITE, "mu_minus_inf": MU_NOT_FINITE, "r_equal": R_NOT_ASCENDING,
           "r_descending": R_NOT_ASCENDING, "mu_equal": MU_NOT_ASCENDING, "finite_before_ascending": MU_NOT_FINITE, "r_before_mu": R_NOT_FINITE,
           "edges_before_switch": R_NOT_ASCENDING, "forced_lds_too_large": LDS_TOO_LARGE, "bad_switch": BAD_PATH_SWITCH,
           "staging_too_large": STAGING_TOO_LARGE, "staging_before_switch": STAGING_TOO_LARGE}
N_CELLS = (1, 256, 1048576)
N_PHOTONS = 2000

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "radfield_plan.hpp"
using namespace mcrat;

static std::vector<double> ramp(int n) { std::vector<double> v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }
static void check(const char *name, int mode, int n_r, bool has_r, std::vector<double> re, int n_mu, bool has_mu, std::vector<double> me, const char *env)
{
    RadfieldShape s;
    const RadfieldRefusal why = radfield_check(mode, n_r, has_r ? re.data() : nullptr, n_mu, has_mu ? me.data() : nullptr, env, &s);
    printf("check_%s: %d\n", name, (int)why);
    if (why != RADFIELD_OK) return;
    printf("shape_%s: %d %d %d %d %zu %zu %d\n", name, s.mode, s.n_r, s.n_mu, s.n_shell_bins, s.staged_doubles, s.staged_bytes, (int)s.path);
    const int cells[3] = {1, 256, 1048576};
    for (int k = 0; k < 3; ++k)
        for (int bm = 0; bm < 2; ++bm) {
            const RadfieldPlan p = radfield_layout(s, cells[k], bm != 0);
            printf("layout_%s_%d_%d: %d %d %zu %zu %zu %zu %zu %zu %d %d %d\n", name, cells[k], bm, p.n_bins, (int)p.bin_major, p.acc_bytes, p.zeroed_bytes,
                   p.planes_offset, p.staged_offset, p.total_bytes, p.lds_bytes, p.groups_per_cu, radfield_grid(p, 1000000, 256), radfield_grid(p, 257, 256));
        }
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
    for (int k = 1; k <= (int)RADFIELD_HYDRO_MISMATCH; ++k) printf("text_%d:%s\n", k, radfield_refusal_text((RadfieldRefusal)k));
    printf("constants: %d %d %d %d %zu %d %zu %d\n", RADFIELD_PLANES, RADFIELD_RECORD_WORDS, RADFIELD_HEAD_WORDS, RADFIELD_N_SCALARS, RADFIELD_ACC_OFFSET,
           RADFIELD_BLOCK, RADFIELD_MATCH_BYTES, (int)RADFIELD_BIN_MAJOR);
    printf("words: %zu %zu %zu %zu %zu %zu\n", radfield_word(false, RF_COUNT, 5, 100), radfield_word(false, RF_WT, 5, 100), radfield_word(false, RF_WE_COMV, 99, 100),
           radfield_word(true, RF_COUNT, 5, 100), radfield_word(true, RF_WT, 5, 100), radfield_word(true, RF_WE_COMV, 99, 100));
    printf("planes: %d %d %d %d %d %d\n", (int)RF_COUNT, (int)RF_W, (int)RF_WE_LAB, (int)RF_WE_COMV, (int)RF_WNS, (int)RF_WT);
    if (argc < 2) return 0;
    // the photons: header {n, n_r, n_mu} as doubles, then r0, r1, r2 [n each], r_edges, mu_edges
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<double> head = read_doubles(f, 3);
    const size_t n = (size_t)head[0];
    const int n_r = (int)head[1], n_mu = (int)head[2];
    const std::vector<double> r0 = read_doubles(f, n), r1 = read_doubles(f, n), r2 = read_doubles(f, n), re = read_doubles(f, n_r + 1), me = read_doubles(f, n_mu + 1);
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        double r, mu;
        radfield_r_mu(r0[i], r1[i], r2[i], r, mu);
        printf("ph: %.17g %.17g %d %.17g\n", r, mu, radfield_shell_bin(re.data(), n_r, me.data(), n_mu, r, mu), radfield_e_lab(r0[i]));
    }
    return 0;
}
'''


def _vec(v, n):
    if v is None:
        return "false, {}"
    if isinstance(v, str):
        return "true, ramp(%d)" % n
    lit = {INF: "INFINITY", -INF: "-INFINITY"}
    return "true, {%s}" % ", ".join("NAN" if x != x else lit.get(x, repr(x)) for x in v)


def _cases():
    lines = []
    for name, (mode, n_r, re_, n_mu, me, env) in CHECKS.items():
        lines.append('check("%s", %d, %d, %s, %d, %s, %s);' % (name, mode, n_r, _vec(re_, n_r), n_mu, _vec(me, n_mu), "nullptr" if env is None else '"%s"' % env))
    return "\n".join("    " + l for l in lines)


def photons():
    """~2000 seeded positions around r = 1e12 cm; some on the polar axis, some edges the exact r and mu of chosen photons"""
    g = np.random.default_rng(20260114)
    n = N_PHOTONS
    r = 10.0 ** g.uniform(11.9, 12.2, n)
    th, phi = g.uniform(0, 0.25, n), g.uniform(0, 2 * np.pi, n)
    r0, r1, r2 = r * np.sin(th) * np.cos(phi), r * np.sin(th) * np.sin(phi), r * np.cos(th)
    r0[:20], r1[:20] = 0.0, 0.0                                      # on the axis: r == |r2|, mu == 1
    r2[10:15] *= -1.0                                                # ... and mu == -1
    r0[20], r1[20], r2[20] = 0.0, 0.0, 0.0                           # the origin: mu is 0 / 0
    with np.errstate(invalid="ignore"):
        rr = np.sqrt((r0 * r0 + r1 * r1) + r2 * r2)
        mu = r2 / rr
    re_ = np.unique(np.concatenate([np.linspace(0.9e12, 1.5e12, 12), rr[[3, 500, 900]]]))
    me = np.unique(np.concatenate([[-1.0, 0.0, 0.97, 0.98, 0.99, 1.0], mu[[600, 700]]]))
    return dict(r0=r0, r1=r1, r2=r2, re=re_, me=me, r=rr, mu=mu)


def find_bin(edges, x):
    """edges[k] <= x < edges[k + 1], else -1"""
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1) & (x == x), k, -1)


def _build(d, src, name, extra):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("radfield_plan")
    src, data = d / "driver.cpp", d / "photons.bin"
    src.write_text(DRIVER.replace("@CASES@", _cases()))
    q = photons()
    head = np.array([N_PHOTONS, len(q["re"]) - 1, len(q["me"]) - 1], dtype=np.float64)
    np.concatenate([head] + [q[k] for k in ("r0", "r1", "r2", "re", "me")]).tofile(data)
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


def check_rule(mode, n_r, re_, n_mu, me, env):
    """radfield_check restated: the checks in their order, what is staged, the path"""
    ramp = lambda v, n: [float(k) for k in range(n + 1)] if isinstance(v, str) else v
    if mode not in (CELLS, SHELLS):
        return BAD_MODE, None
    bins = staged_doubles = 0
    if mode == SHELLS:
        if re_ is None or me is None:
            return NULL_EDGES, None
        if n_r < 1 or n_mu < 1:
            return NO_BINS, None
        if n_r * n_mu > 2 ** 31 - 1:
            return TOO_MANY_BINS, None
        re_, me = ramp(re_, n_r), ramp(me, n_mu)
        if not all(np.isfinite(re_)):
            return R_NOT_FINITE, None
        if not all(np.isfinite(me)):
            return MU_NOT_FINITE, None
        if not all(a < b for a, b in zip(re_[:-1], re_[1:])):
            return R_NOT_ASCENDING, None
        if not all(a < b for a, b in zip(me[:-1], me[1:])):
            return MU_NOT_ASCENDING, None
        bins, staged_doubles = n_r * n_mu, n_r + 1 + n_mu + 1
    else:
        n_r = n_mu = 0
    staged = 8 * staged_doubles + 3 * 8                            # ... and the workgroup's three counters
    if staged > LDS_BUDGET:
        return STAGING_TOO_LARGE, None
    fits = mode == SHELLS and staged + 6 * 8 * bins <= LDS_BUDGET
    if env not in (None, "", "lds", "global"):
        return BAD_PATH_SWITCH, None
    if env == "lds" and mode == CELLS:
        return LDS_ON_CELLS, None
    if env == "lds" and not fits:
        return LDS_TOO_LARGE, None
    path = {"lds": PATH_LDS, "global": PATH_GLOBAL}.get(env, PATH_LDS if fits else PATH_GLOBAL)
    return OK, [mode, n_r, n_mu, bins, staged_doubles, staged, path]


def layout_rule(shape, n_cells, bin_major):
    mode, _, _, bins, staged_doubles, staged, path = shape
    up = lambda x: (x + 255) // 256 * 256
    n_bins = n_cells if mode == CELLS else bins
    planes = 48 * n_bins
    acc = 64 * n_bins if bin_major else planes
    zeroed = 256 + acc
    planes_offset = up(zeroed) if bin_major else 256
    staged_offset = up(planes_offset + planes if bin_major else zeroed)
    lds = staged + (planes if path == PATH_LDS else MATCH_BYTES)
    groups = 2 if path == PATH_LDS else min(LDS_PER_CU // lds, 8)
    grid = lambda n: min((n + 255) // 256, 256 * groups)
    return [n_bins, int(bin_major), acc, zeroed, planes_offset, staged_offset, staged_offset + 8 * staged_doubles, lds, groups, grid(1000000), grid(257)]


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_check_and_layout(out, name):
    why, shape = check_rule(*CHECKS[name])
    assert out["check_" + name] == [why]
    assert why == REFUSED.get(name, OK)
    if why != OK:
        assert "shape_" + name not in out
        return
    assert out["shape_" + name] == shape
    for n_cells in N_CELLS:
        for bm in (0, 1):
            assert out["layout_%s_%d_%d" % (name, n_cells, bm)] == layout_rule(shape, n_cells, bm), (n_cells, bm)


def test_cases_are_what_they_are_meant_to_be(out):
    """... so that the table above cannot drift into testing nothing: every refusal of the rules occurs, and the path changes exactly at the budget"""
    assert set(REFUSED.values()) | {HYDRO_MISMATCH} == set(TEXTS)
    assert out["constants"][:7] == [6, 8, 8, 3, 256, 256, MATCH_BYTES] and out["constants"][7] in (0, 1)
    assert out["shape_small"] == [SHELLS, 8, 4, 32, 14, 136, PATH_LDS]
    assert out["layout_small_256_0"] == [32, 0, 1536, 1792, 256, 1792, 1904, 136 + 1536, 2, 512, 2]
    assert out["layout_small_256_1"] == [32, 1, 2048, 2304, 2304, 3840, 3952, 136 + 1536, 2, 512, 2]       # records, then the planes the caller receives
    assert out["shape_cells"] == [CELLS, 0, 0, 0, 0, 24, PATH_GLOBAL] and out["shape_cells_ignores_edges"] == out["shape_cells"]
    assert out["layout_cells_1048576_0"] == [1048576, 0, 48 << 20, 256 + (48 << 20), 256, 256 + (48 << 20), 256 + (48 << 20), 24 + MATCH_BYTES, 8, 2048, 2]
    assert out["layout_cells_1048576_1"][2:5] == [64 << 20, 256 + (64 << 20), 256 + (64 << 20)]
    assert out["shape_lds_last"][6] == PATH_LDS and out["layout_lds_last_1_0"][7:9] == [LDS_BUDGET, 2]       # the budget exactly: still LDS
    assert out["shape_global_first"][6] == PATH_GLOBAL and out["layout_global_first_1_0"][7] == 8 * 1466 + 24 + MATCH_BYTES
    assert out["shape_lds_last_64x"][6] == PATH_LDS and out["shape_global_first_64x"][6] == PATH_GLOBAL and out["shape_bench_shells"][6] == PATH_GLOBAL
    assert out["shape_forced_global"][6] == PATH_GLOBAL and out["shape_forced_lds"][6] == PATH_LDS and out["shape_forced_global_beyond"][6] == PATH_GLOBAL
    assert out["shape_staging_last"][5:] == [LDS_BUDGET, PATH_GLOBAL] and out["layout_staging_last_1_0"][7:9] == [LDS_BUDGET + MATCH_BYTES, 1]
    assert out["shape_one_bin"][6] == PATH_LDS


def test_refusal_texts(out):
    for why, t in TEXTS.items():
        assert out["text_%d" % why] == t, why
    assert len(TEXTS) == HYDRO_MISMATCH and len(set(TEXTS.values())) == len(TEXTS)


def test_words_of_both_layouts(out):
    assert out["planes"] == [0, 1, 2, 3, 4, 5]                           # count, W, WE_lab, WE_comv, WNS, WT
    assert out["words"] == [5, 505, 399, 40, 45, 99 * 8 + 3]             # plane-major: plane * n_bins + bin; bin-major: bin * 8 + plane


def test_per_photon_functions_equal_the_numpy_restatement(out):
    q = photons()
    rows = out["ph"]
    assert len(rows) == N_PHOTONS
    got_r, got_mu = np.array([float(r[0]) for r in rows]), np.array([float(r[1]) for r in rows])
    got_bin = np.array([int(r[2]) for r in rows])
    same = lambda a, b: np.array_equal(a.view(np.int64)[a == a], b.view(np.int64)[b == b]) and np.array_equal(a != a, b != b)
    assert same(got_r, q["r"]) and same(got_mu, q["mu"])              # bit for bit (%.17g round-trips a double)
    assert same(np.array([float(r[3]) for r in rows]), q["r0"] * 2.99792458e10)
    ir, imu = find_bin(q["re"], q["r"]), find_bin(q["me"], q["mu"])
    n_mu = len(q["me"]) - 1
    want = np.where((ir >= 0) & (imu >= 0), ir * n_mu + imu, -1)
    assert np.array_equal(got_bin, want)
    # the sample means something: both axes have photons inside and outside; on the axis r == |r2| and mu == +-1, which the last edge 1 leaves
    # outside; the origin is in no bin; the photons whose r or mu IS an edge sit in the bin that edge opens
    assert (ir < 0).sum() > 10 and (imu < 0).sum() > 10 and (want >= 0).sum() > 500 and len(np.unique(want)) > 20
    assert (q["r"][:20] == np.abs(q["r2"][:20])).all() and (q["mu"][:10] == 1.0).all() and (q["mu"][10:15] == -1.0).all()
    assert (imu[:10] == -1).all() and (imu[10:15] == 0).all() and q["mu"][20] != q["mu"][20] and want[20] == -1
    for i in (3, 500, 900):
        assert q["re"][ir[i]] == q["r"][i]
    for i in (600, 700):
        assert q["me"][imu[i]] == q["mu"][i]


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
