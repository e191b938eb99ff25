"""The host's rules for the comoving radiation field (mcrat_amd/csrc/comoving_plan.hpp) on the CPU: every refusal and its text and the order in which
the checks fire, the block's layout, the rule that picks the accumulation path on both sides of its LDS boundary, the grid size, and the per-photon
functions the kernel uses -- the lab cosine m, the fluid-frame cosine a, the bin and the seven terms -- against the definitions restated here in
NumPy: integers exactly, doubles (%.17g) for equality.  They are plain C++: a small driver is compiled with g++ and what it prints is compared.  The
same driver is built a second time with -fsanitize=address,undefined and run once."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
(OK, BAD_MODE, NULL_EDGES, NO_BINS, TOO_MANY_BINS, R_NOT_FINITE, MU_NOT_FINITE, E_NOT_FINITE, A_NOT_FINITE, R_NOT_ASCENDING, MU_NOT_ASCENDING,
 E_NOT_ASCENDING, A_NOT_ASCENDING, STAGING_TOO_LARGE, BAD_PATH_SWITCH, LDS_ON_CELLS, LDS_TOO_LARGE, HYDRO_MISMATCH) = range(18)
CELLS, SHELLS = 0, 1
PATH_LDS, PATH_GLOBAL = 1, 2
LDS_BUDGET, LDS_PER_CU = 80 * 1024, 160 * 1024
MATCH_BYTES = 4 * 2048            # global path: a one-byte table of 2048 entries per wavefront of the 256-thread workgroup
C_LIGHT = 2.99792458e10

TEXTS = {
    BAD_MODE: "comoving_field: mode must be MCRAT_HIP_COMOVING_CELLS or MCRAT_HIP_COMOVING_SHELLS",
    NULL_EDGES: "comoving_field: e_edges and a_edges are needed, and SHELLS needs r_edges and mu_edges",
    NO_BINS: "comoving_field: n_e and n_a, and with SHELLS n_r and n_mu, must each be at least 1",
    TOO_MANY_BINS: "comoving_field: the number of position bins * n_e * n_a overflows an int",
    R_NOT_FINITE: "comoving_field: r_edges holds a value that is not finite",
    MU_NOT_FINITE: "comoving_field: mu_edges holds a value that is not finite",
    E_NOT_FINITE: "comoving_field: e_edges holds a value that is not finite",
    A_NOT_FINITE: "comoving_field: a_edges holds a value that is not finite",
    R_NOT_ASCENDING: "comoving_field: r_edges is not strictly ascending",
    MU_NOT_ASCENDING: "comoving_field: mu_edges is not strictly ascending",
    E_NOT_ASCENDING: "comoving_field: e_edges is not strictly ascending",
    A_NOT_ASCENDING: "comoving_field: a_edges is not strictly ascending",
    STAGING_TOO_LARGE: "comoving_field: the edges do not fit the kernel's LDS budget",
    BAD_PATH_SWITCH: "comoving_field: MCRAT_HIP_COMOVING_PATH must be lds or global",
    LDS_ON_CELLS: "comoving_field: MCRAT_HIP_COMOVING_PATH=lds, but CELLS always accumulates in global memory",
    LDS_TOO_LARGE: "comoving_field: MCRAT_HIP_COMOVING_PATH=lds, but the planes do not fit the kernel's LDS budget",
    HYDRO_MISMATCH: "comoving_field: a frame staged on a context with other switches (DIMENSIONS, GEOMETRY) or on another device",
}

INF, NAN = float("inf"), float("nan")
R, ONE = "ramp", [0.0, 1.0]
# name: (mode, (n_r, r_edges), (n_mu, mu_edges), (n_e, e_edges), (n_a, a_edges), the switch) -- the arrays as they are handed over; "ramp": 0, 1, 2, ...
# of the length the count asks for; None: a null pointer
CHECKS = {
    "cells": (CELLS, (0, None), (0, None), (4, R), (8, R), None),
    "cells_ignores_shell_edges": (CELLS, (-3, None), (7, [NAN]), (4, R), (8, R), ""),
    "cells_global": (CELLS, (0, None), (0, None), (1, R), (1, R), "global"),
    "cells_lds": (CELLS, (0, None), (0, None), (1, R), (1, R), "lds"),
    "cells_bad_switch": (CELLS, (0, None), (0, None), (1, R), (1, R), "hbm"),
    "cells_null_e": (CELLS, (0, None), (0, None), (1, None), (1, R), None),
    "cells_no_a": (CELLS, (0, None), (0, None), (1, R), (0, [1.0]), None),
    "cells_e_times_a_overflows": (CELLS, (0, None), (0, None), (65536, [NAN]), (32768, [NAN]), None),
    "cells_a_nan": (CELLS, (0, None), (0, None), (2, [0.0, 0.0, 1.0]), (2, [0.0, NAN, 1.0]), None),      # a not finite before e not ascending
    "cells_e_equal": (CELLS, (0, None), (0, None), (2, [0.0, 0.0, 1.0]), (2, [0.0, 0.0, 1.0]), None),
    "mode_2": (2, (4, R), (4, R), (4, R), (4, R), None),
    "mode_negative": (-1, (4, None), (4, R), (0, R), (4, R), "hbm"),                   # the mode is checked before everything else
    "null_r": (SHELLS, (4, None), (4, R), (4, R), (4, R), None),
    "null_mu": (SHELLS, (4, R), (4, None), (4, R), (4, R), None),
    "null_e": (SHELLS, (4, R), (4, R), (4, None), (4, R), None),
    "null_a": (SHELLS, (4, R), (4, R), (4, R), (4, None), None),
    "null_before_counts": (SHELLS, (0, None), (0, None), (0, None), (0, None), None),
    "small": (SHELLS, (8, R), (4, R), (32, R), (8, R), None),
    "one_bin": (SHELLS, (1, [1.0, 2.0]), (1, [-1.0, 1.5]), (1, [0.0, 1.0]), (1, [-1.0, 1.5]), None),
    "no_r": (SHELLS, (0, [1.0]), (4, R), (4, R), (4, R), None),
    "negative_mu": (SHELLS, (4, R), (-1, [1.0]), (4, R), (4, R), None),
    "no_e": (SHELLS, (4, R), (4, R), (0, [1.0]), (4, R), None),
    "no_a": (SHELLS, (4, R), (4, R), (4, R), (0, [1.0]), None),
    "counts_before_product": (SHELLS, (65536, [NAN]), (65536, [NAN]), (0, [NAN]), (1, [NAN]), None),
    "overflow_shells": (SHELLS, (65536, [NAN]), (32768, [NAN]), (1, [NAN]), (1, [NAN]), None),      # 2^31 (the arrays are not looked at)
    "overflow_four": (SHELLS, (256, [NAN]), (256, [NAN]), (256, [NAN]), (128, [NAN]), None),       # 2^31 over four axes
    "overflow_wide": (SHELLS, (65536, [NAN]), (65536, [NAN]), (65536, [NAN]), (65536, [NAN]), None),      # 2^64: the product is not formed in one go
    "largest_product": (SHELLS, (46340, R), (46340, R), (1, R), (1, R), None),         # fits an int, but 92 682 edges: the staging check fires
    "r_inf": (SHELLS, (2, [0.0, 1.0, INF]), (2, R), (2, R), (2, R), None),
    "mu_nan": (SHELLS, (2, R), (2, [0.0, NAN, 2.0]), (2, R), (2, R), None),
    "e_minus_inf": (SHELLS, (2, R), (2, R), (2, [-INF, 0.0, 1.0]), (2, R), None),
    "a_nan": (SHELLS, (2, R), (2, R), (2, R), (2, [NAN, 0.0, 1.0]), None),
    "r_equal": (SHELLS, (2, [0.0, 1.0, 1.0]), (2, R), (2, R), (2, R), None),
    "mu_descending": (SHELLS, (2, R), (2, [0.0, 2.0, 1.0]), (2, R), (2, R), None),
    "e_equal": (SHELLS, (2, R), (2, R), (2, [0.5, 0.5, 1.0]), (2, R), None),
    "a_descending": (SHELLS, (2, R), (2, R), (2, R), (2, [1.0, 0.0, -1.0]), None),
    "finite_before_ascending": (SHELLS, (2, [0.0, 0.0, 1.0]), (2, [1.0, 0.0, 2.0]), (2, [1.0, 1.0, 2.0]), (2, [0.0, NAN, 1.0]), None),
    "finite_in_axis_order": (SHELLS, (2, R), (2, [0.0, NAN, 1.0]), (2, [0.0, NAN, 1.0]), (2, [0.0, NAN, 1.0]), None),
    "e_before_a_finite": (SHELLS, (2, R), (2, R), (2, [0.0, NAN, 1.0]), (2, [0.0, NAN, 1.0]), None),
    "ascending_in_axis_order": (SHELLS, (2, R), (2, [0.0, 0.0, 1.0]), (2, [0.0, 0.0, 1.0]), (2, [0.0, 0.0, 1.0]), None),
    "e_before_a_ascending": (SHELLS, (2, R), (2, R), (2, [0.0, 0.0, 1.0]), (2, [0.0, 0.0, 1.0]), None),
    "edges_before_switch": (SHELLS, (2, R), (2, R), (2, R), (2, [0.0, 0.0, 1.0]), "hbm"),
    "lds_last": (SHELLS, (1, R), (1, R), (1136, R), (1, R), None),                     # 8 * 1136 + 80 + 64 * 1136 = 81 872 bytes
    "global_first": (SHELLS, (1, R), (1, R), (1137, R), (1, R), None),                 # 81 944 bytes
    "bench_spectra": (SHELLS, (8, R), (4, R), (32, R), (8, R), None),                  # 8192 bins: 512 KiB of planes
    "bench_yardstick": (SHELLS, (64, R), (32, R), (1, R), (1, R), None),
    "forced_global": (SHELLS, (2, R), (2, R), (4, R), (4, R), "global"),
    "forced_lds": (SHELLS, (2, R), (2, R), (4, R), (4, R), "lds"),
    "forced_lds_too_large": (SHELLS, (1, R), (1, R), (1137, R), (1, R), "lds"),
    "forced_global_beyond": (SHELLS, (1, R), (1, R), (1137, R), (1, R), "global"),
    "bad_switch": (SHELLS, (2, R), (2, R), (4, R), (4, R), "LDS"),
    "staging_last": (SHELLS, (1, R), (1, R), (10230, R), (1, R), None),                # 8 * (10231 + 6) + 24 = 81 920 bytes staged
    "staging_too_large": (SHELLS, (1, R), (1, R), (10231, R), (1, R), None),
    "staging_before_switch": (SHELLS, (1, R), (1, R), (10231, R), (1, R), "hbm"),
}
REFUSED = {"cells_lds": LDS_ON_CELLS, "cells_bad_switch": BAD_PATH_SWITCH, "cells_null_e": NULL_EDGES, "cells_no_a": NO_BINS,
           "cells_e_times_a_overflows": TOO_MANY_BINS, "cells_a_nan": A_NOT_FINITE, "cells_e_equal": E_NOT_ASCENDING, "mode_2": BAD_MODE,
           "mode_negative": BAD_MODE, "null_r": NULL_EDGES, "null_mu": NULL_EDGES, "null_e": NULL_EDGES, "null_a": NULL_EDGES,
           "null_before_counts": NULL_EDGES, "no_r": NO_BINS, "negative_mu": NO_BINS, "no_e": NO_BINS, "no_a": NO_BINS, "counts_before_product": NO_BINS,
           "overflow_shells": TOO_MANY_BINS, "overflow_four": TOO_MANY_BINS, "overflow_wide": TOO_MANY_BINS, "largest_product": STAGING_TOO_LARGE,
           "r_inf": R_NOT_FINITE, "mu_nan": MU_NOT_FINITE, "e_minus_inf": E_NOT_FINITE, "a_nan": A_NOT_FINITE, "r_equal": R_NOT_ASCENDING,
           "mu_descending": MU_NOT_ASCENDING, "e_equal": E_NOT_ASCENDING, "a_descending": A_NOT_ASCENDING, "finite_before_ascending": A_NOT_FINITE,
           "finite_in_axis_order": MU_NOT_FINITE, "e_before_a_finite": E_NOT_FINITE, "ascending_in_axis_order": MU_NOT_ASCENDING,
           "e_before_a_ascending": E_NOT_ASCENDING, "edges_before_switch": A_NOT_ASCENDING, "forced_lds_too_large": LDS_TOO_LARGE,
           "bad_switch": BAD_PATH_SWITCH, "staging_too_large": STAGING_TOO_LARGE, "staging_before_switch": STAGING_TOO_LARGE}
N_CELLS = (1, 256, 1048576, 100000000)          # the last: CELLS x 4 x 8 overflows an int once the frame is known
N_PHOTONS = 2000

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "comoving_plan.hpp"
using namespace mcrat;

static std::vector<double> ramp(int n) { std::vector<double> v; for (int k = 0; k <= n; ++k) v.push_back((double)k); return v; }
struct Axis { int n; bool has; std::vector<double> v; const double *p() const { return has ? v.data() : nullptr; } };
static void check(const char *name, int mode, Axis r, Axis mu, Axis e, Axis a, const char *env)
{
    ComovingShape s;
    const ComovingRefusal why = comoving_check(mode, r.n, r.p(), mu.n, mu.p(), e.n, e.p(), a.n, a.p(), env, &s);
    printf("check_%s: %d\n", name, (int)why);
    if (why != COMOVING_OK) return;
    printf("shape_%s: %d %d %d %d %d %d %d %zu %zu %d\n", name, s.mode, s.n_r, s.n_mu, s.n_e, s.n_a, s.n_shells, s.n_shell_bins, s.staged_doubles,
           s.staged_bytes, (int)s.path);
    const int cells[4] = {1, 256, 1048576, 100000000};
    for (int k = 0; k < 4; ++k) {
        ComovingPlan p;
        const ComovingRefusal bad = comoving_layout(s, cells[k], &p);
        if (bad != COMOVING_OK) { printf("layout_%s_%d: %d\n", name, cells[k], -(int)bad); continue; }
        printf("layout_%s_%d: %d %d %zu %zu %zu %zu %zu %zu %d %d %d\n", name, cells[k], p.n_s, p.n_bins, p.acc_bytes, p.zeroed_bytes, p.planes_offset,
               p.staged_offset, p.total_bytes, p.lds_bytes, p.groups_per_cu, comoving_grid(p, 1000000, 256), comoving_grid(p, 257, 256));
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
    for (int k = 1; k <= (int)COMOVING_HYDRO_MISMATCH; ++k) printf("text_%d:%s\n", k, comoving_refusal_text((ComovingRefusal)k));
    printf("constants: %d %d %d %zu %d %zu\n", COMOVING_PLANES, COMOVING_SUMS, COMOVING_N_SCALARS, COMOVING_ACC_OFFSET, COMOVING_BLOCK, COMOVING_MATCH_BYTES);
    printf("planes: %d %d %d %d %d %d %d %d\n", (int)CF_COUNT, (int)CF_W, (int)CF_WE, (int)CF_WEA, (int)CF_WEAA, (int)CF_WE_LAB, (int)CF_WEM, (int)CF_WEMM);
    if (argc < 2) return 0;
    // the photons: header {n, n_e, n_a} as doubles, then r0, r1, r2, p0 .. p3, beta0 .. beta2, g, w [n each], s [n, as doubles], e_edges, a_edges
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<double> head = read_doubles(f, 3);
    const size_t n = (size_t)head[0];
    const int n_e = (int)head[1], n_a = (int)head[2];
    std::vector<double> c[13];
    for (int k = 0; k < 13; ++k) c[k] = read_doubles(f, n);
    const std::vector<double> ee = read_doubles(f, n_e + 1), ae = read_doubles(f, n_a + 1);
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        double r, mu, v[COMOVING_SUMS];
        radfield_r_mu(c[0][i], c[1][i], c[2][i], r, mu);
        const double p0 = c[3][i], p1 = c[4][i], p2 = c[5][i], p3 = c[6][i], beta[3] = {c[7][i], c[8][i], c[9][i]};
        const double bp = comoving_bp(beta, p1, p2, p3), e = comoving_e(c[10][i], p0, bp);
        const double m = comoving_m(c[0][i], c[1][i], c[2][i], p0, p1, p2, p3, r), a = comoving_a(beta, bp, p0, m);
        comoving_terms(c[11][i], e, a, radfield_e_lab(p0), m, v);
        printf("ph: %.17g %.17g %.17g %d", e, m, a, comoving_bin((int)c[12][i], ee.data(), n_e, ae.data(), n_a, e, a));
        for (int k = 0; k < COMOVING_SUMS; ++k) printf(" %.17g", v[k]);
        printf("\n");
    }
    return 0;
}
'''


def _axis(ax):
    n, v = ax
    if v is None:
        return "{%d, false, {}}" % n
    if isinstance(v, str):
        return "{%d, true, ramp(%d)}" % (n, n)
    lit = {INF: "INFINITY", -INF: "-INFINITY"}
    return "{%d, true, {%s}}" % (n, ", ".join("NAN" if x != x else lit.get(x, repr(x)) for x in v))


def _cases():
    lines = []
    for name, (mode, r, mu, e, a, env) in CHECKS.items():
        lines.append('check("%s", %d, %s, %s, %s, %s, %s);' % (name, mode, _axis(r), _axis(mu), _axis(e), _axis(a), "nullptr" if env is None else '"%s"' % env))
    return "\n".join("    " + l for l in lines)


COLS = ("r0", "r1", "r2", "p0", "p1", "p2", "p3", "b0", "b1", "b2", "g", "w", "s")


def photons():
    """~2000 seeded photons around r = 1e12 cm in fluids of Lorentz factor up to 100 in random directions; the first ones are special: along and
    against the flow, a cell at rest, radial, p0 == 0 (0 / 0), no position bin; some edges are the exact e and a of chosen photons"""
    g = np.random.default_rng(20261020)
    n = N_PHOTONS
    unit = lambda: (lambda d: d / np.sqrt((d * d).sum(axis=0)))(g.standard_normal((3, n)))
    pos = 10.0 ** g.uniform(11.9, 12.2, n) * unit()
    d, bh = unit(), unit()
    p0 = 10.0 ** g.uniform(-20.0, -16.0, n)
    gam = 10.0 ** g.uniform(0.0, 2.0, n)
    beta = np.sqrt(1.0 - 1.0 / (gam * gam)) * bh
    d[:, 0:10] = bh[:, 0:10]                    # along the flow
    d[:, 10:20] = -bh[:, 10:20]                 # against it
    beta[:, 20:40] = 0.0                        # a cell at rest
    gam[20:40] = 1.0
    d[:, 30:50] = pos[:, 30:50] / np.sqrt((pos[:, 30:50] ** 2).sum(axis=0))      # radial
    p = p0 * d
    p0[50] = 0.0                                # m and a are 0 / 0 ...
    p[:, 50] = 0.0
    pos[:, 51] = 0.0                            # ... and m is x / 0 at the origin
    s = g.integers(0, 7, n).astype(np.float64)
    s[52:60] = -1.0
    q = dict(r0=pos[0], r1=pos[1], r2=pos[2], p0=p0, p1=p[0], p2=p[1], p3=p[2], b0=beta[0], b1=beta[1], b2=beta[2], g=gam,
             w=10.0 ** g.uniform(48.0, 51.0, n), s=s)
    q.update(restate(q))
    q["ee"] = np.unique(np.concatenate([10.0 ** np.linspace(-10.5, -4.0, 14), q["e"][[300, 800, 1300]]]))
    q["ae"] = np.unique(np.concatenate([[-1.0, -0.5, 0.0, 0.5, 0.9, 0.99, 1.0], q["a"][[600, 700]]]))
    return q


def clamp(x):
    return np.where(x < -1.0, -1.0, np.where(x > 1.0, 1.0, x))


def restate(q):
    """the definition's expressions in NumPy, in their order: e, m, a and the seven terms"""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.sqrt((q["r0"] * q["r0"] + q["r1"] * q["r1"]) + q["r2"] * q["r2"])
        bp = (q["b0"] * q["p1"] + q["b1"] * q["p2"]) + q["b2"] * q["p3"]
        e = (q["g"] * (q["p0"] - bp)) * C_LIGHT
        e_lab = q["p0"] * C_LIGHT
        m = clamp(((q["p1"] * q["r0"] + q["p2"] * q["r1"]) + q["p3"] * q["r2"]) / (q["p0"] * r))
        b2 = (q["b0"] * q["b0"] + q["b1"] * q["b1"]) + q["b2"] * q["b2"]
        b = np.sqrt(b2)
        a = np.where(b2 > 0, clamp(((bp / b) - b * q["p0"]) / (q["p0"] - bp)), m)
    we, wl = q["w"] * e, q["w"] * e_lab
    return dict(e=e, m=m, a=a, terms=np.stack([q["w"], we, we * a, (we * a) * a, wl, wl * m, (wl * m) * m], axis=1))


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
    d = tmp_path_factory.mktemp("comoving_plan")
    src, data = d / "driver.cpp", d / "photons.bin"
    src.write_text(DRIVER.replace("@CASES@", _cases()))
    q = photons()
    head = np.array([N_PHOTONS, len(q["ee"]) - 1, len(q["ae"]) - 1], dtype=np.float64)
    np.concatenate([head] + [q[k] for k in COLS] + [q["ee"], q["ae"]]).tofile(data)
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


def check_rule(mode, r, mu, e, a, env):
    """comoving_check restated: the checks in their order, what is staged, the path"""
    ramp = lambda ax: [float(k) for k in range(ax[0] + 1)] if isinstance(ax[1], str) else ax[1]
    if mode not in (CELLS, SHELLS):
        return BAD_MODE, None
    axes = [r, mu, e, a] if mode == SHELLS else [e, a]
    if any(ax[1] is None for ax in axes):
        return NULL_EDGES, None
    if any(ax[0] < 1 for ax in axes):
        return NO_BINS, None
    n_e, n_a = e[0], a[0]
    n_r, n_mu = (r[0], mu[0]) if mode == SHELLS else (0, 0)
    if n_e * n_a > 2 ** 31 - 1 or n_r * n_mu * n_e * n_a > 2 ** 31 - 1:
        return TOO_MANY_BINS, None
    first = R_NOT_FINITE + (4 - len(axes))
    for k, ax in enumerate(axes):
        if not all(np.isfinite(ramp(ax))):
            return first + k, None
    for k, ax in enumerate(axes):
        v = ramp(ax)
        if not all(x < y for x, y in zip(v[:-1], v[1:])):
            return first + 4 + k, None
    staged_doubles = sum(ax[0] + 1 for ax in axes)
    staged = 8 * staged_doubles + 3 * 8                            # ... and the workgroup's three counters
    if staged > LDS_BUDGET:
        return STAGING_TOO_LARGE, None
    bins = n_r * n_mu * n_e * n_a
    fits = mode == SHELLS and staged + 8 * 8 * bins <= LDS_BUDGET
    if env not in (None, "", "lds", "global"):
        return BAD_PATH_SWITCH, None
    if env == "lds" and mode == CELLS:
        return LDS_ON_CELLS, None
    if env == "lds" and not fits:
        return LDS_TOO_LARGE, None
    path = {"lds": PATH_LDS, "global": PATH_GLOBAL}.get(env, PATH_LDS if fits else PATH_GLOBAL)
    return OK, [mode, n_r, n_mu, n_e, n_a, n_r * n_mu, bins, staged_doubles, staged, path]


def layout_rule(shape, n_cells):
    mode, _, _, n_e, n_a, shells, _, staged_doubles, staged, path = shape
    up = lambda x: (x + 255) // 256 * 256
    n_s = n_cells if mode == CELLS else shells
    n_bins = n_s * n_e * n_a
    if n_bins > 2 ** 31 - 1:
        return [-TOO_MANY_BINS]
    acc = 64 * n_bins
    zeroed = 256 + acc
    staged_offset = up(zeroed)
    lds = staged + (acc if path == PATH_LDS else MATCH_BYTES)
    groups = 2 if path == PATH_LDS else min(LDS_PER_CU // lds, 8)
    grid = lambda n: min((n + 255) // 256, 256 * groups)
    return [n_s, n_bins, acc, zeroed, 256, staged_offset, staged_offset + 8 * staged_doubles, lds, groups, grid(1000000), grid(257)]


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
        assert out["layout_%s_%d" % (name, n_cells)] == layout_rule(shape, n_cells), n_cells


def test_cases_are_what_they_are_meant_to_be(out):
    """... so that the table above cannot drift into testing nothing: every refusal of the rules occurs, and the path changes exactly at the budget"""
    assert set(REFUSED.values()) | {HYDRO_MISMATCH} == set(TEXTS)
    assert out["constants"] == [8, 7, 3, 256, 256, MATCH_BYTES]
    assert out["shape_one_bin"] == [SHELLS, 1, 1, 1, 1, 1, 1, 8, 88, PATH_LDS]
    assert out["layout_one_bin_1"] == [1, 1, 64, 320, 256, 512, 576, 88 + 64, 2, 512, 2]        # 256 + 64 + 64 B before padding
    assert out["shape_small"] == [SHELLS, 8, 4, 32, 8, 32, 8192, 56, 472, PATH_GLOBAL]
    assert out["shape_cells"] == [CELLS, 0, 0, 4, 8, 0, 0, 14, 136, PATH_GLOBAL] and out["shape_cells_ignores_shell_edges"] == out["shape_cells"]
    assert out["layout_cells_1048576"] == [1048576, 1 << 25, 1 << 31, 256 + (1 << 31), 256, 256 + (1 << 31), 256 + (1 << 31) + 112, 136 + MATCH_BYTES, 8, 2048, 2]
    assert out["layout_cells_100000000"] == [-TOO_MANY_BINS] and out["layout_small_100000000"][0:2] == [32, 8192]      # CELLS alone hangs on the frame
    assert out["layout_cells_global_100000000"][0:2] == [100000000, 100000000]
    # 1136 energies: the staged part 8 * 1136 + 80 and the planes 64 * 1136 are 81 872 B, the last LDS shape; 1137: 81 944 B, the first global one
    assert out["shape_lds_last"][8:] == [8 * 1136 + 80, PATH_LDS] and out["layout_lds_last_1"][7:9] == [81872, 2]
    assert out["shape_global_first"][8:] == [8 * 1137 + 80, PATH_GLOBAL] and out["layout_global_first_1"][7] == 8 * 1137 + 80 + MATCH_BYTES
    assert 81872 <= LDS_BUDGET < 81944
    assert out["shape_bench_yardstick"][9] == PATH_GLOBAL and out["shape_bench_spectra"][9] == PATH_GLOBAL
    assert out["shape_forced_global"][9] == PATH_GLOBAL and out["shape_forced_lds"][9] == PATH_LDS and out["shape_forced_global_beyond"][9] == PATH_GLOBAL
    assert out["shape_staging_last"][8:] == [LDS_BUDGET, PATH_GLOBAL] and out["layout_staging_last_1"][7:9] == [LDS_BUDGET + MATCH_BYTES, 1]


def test_refusal_texts(out):
    for why, t in TEXTS.items():
        assert out["text_%d" % why] == t, why
    assert len(TEXTS) == HYDRO_MISMATCH and len(set(TEXTS.values())) == len(TEXTS)
    assert out["planes"] == list(range(8))               # count, w, we, wea, weaa, we_lab, wem, wemm


def test_per_photon_functions_equal_the_numpy_restatement(out):
    q = photons()
    rows = out["ph"]
    assert len(rows) == N_PHOTONS
    col = lambda k: np.array([float(r[k]) for r in rows])
    same = lambda x, y: np.array_equal(x.view(np.int64)[x == x], y.view(np.int64)[y == y]) and np.array_equal(x != x, y != y)
    e, m, a = col(0), col(1), col(2)
    assert same(e, q["e"]) and same(m, q["m"]) and same(a, q["a"])              # bit for bit (%.17g round-trips a double)
    for k in range(7):
        assert same(col(4 + k), q["terms"][:, k]), k
    ie, ia = find_bin(q["ee"], q["e"]), find_bin(q["ae"], q["a"])
    n_e, n_a = len(q["ee"]) - 1, len(q["ae"]) - 1
    s = q["s"].astype(np.int64)
    want = np.where((s >= 0) & (ie >= 0) & (ia >= 0), (s * n_e + ie) * n_a + ia, -1)
    got = np.array([int(r[3]) for r in rows])
    assert np.array_equal(got, want)
    # the sample means something: along the flow a == 1 and against it a == -1, up to the closed form's rounding, clamped; a cell at rest has a == m
    # (the same bits); a radial photon has m == 1 within rounding; 0 / 0 stays a NaN and is in no bin; a top edge of exactly 1 leaves a == 1 outside;
    # the photons whose e or a IS an edge sit in the bin that edge opens
    assert (np.abs(a[0:10] - 1.0) < 1e-10).all() and (np.abs(a[10:20] + 1.0) < 1e-10).all() and (np.abs(a) <= 1.0)[a == a].all()
    assert same(a[20:40], m[20:40]) and (np.abs(m[30:50] - 1.0) < 1e-14).all()
    assert a[50] != a[50] and m[50] != m[50] and want[50] == -1 and m[51] != m[51] and (want[52:60] == -1).all()
    assert (ia[a == 1.0] == -1).all() and (a == 1.0).sum() >= 1
    assert (ie < 0).sum() > 10 and (want >= 0).sum() > 1000 and len(np.unique(want)) > 200
    for i in (300, 800, 1300):
        assert q["ee"][ie[i]] == q["e"][i]
    for i in (600, 700):
        assert q["ae"][ia[i]] == q["a"][i]


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, data = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
