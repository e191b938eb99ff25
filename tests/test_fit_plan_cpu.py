"""The host's rules for the spectral fit (mcrat_amd/csrc/fit_plan.hpp) on the CPU: every refusal with its text and in its order, the block's layout,
fit_exp, fit_log and a candidate's chi^2 bit for bit against the NumPy restatement (tests/fit_checker.py) on 10^4 inputs, and whole fits driven on
the host by the header's serial loop against the checker's, every output column by its bytes.  Plain C++: a small driver is compiled with g++, reads
its inputs as hexadecimal floating-point text and prints bit patterns.  The same driver is built a second time with -fsanitize=address,undefined as
a stand-alone program and run once.  (The pattern of tests/test_events_plan_cpu.py.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fit_checker as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
(BAD_MODEL, NULL_ARRAY, BAD_N_E, EDGES_NOT_FINITE, EDGES_NOT_ASCENDING, EDGES_NOT_POSITIVE, LOG_E_NOT_FINITE, BAD_PIVOT, BOUNDS_NOT_FINITE, BOUNDS_EMPTY,
 BOUNDS_NO_CANDIDATE, BAD_GRID, GRID_TOO_LARGE, BAD_ROUNDS, BAD_SHRINK, BAD_MIN_COUNT, BAD_N_SPEC) = range(1, 18)
TEXTS = {
    BAD_MODEL: "fit_spectra: model must be MCRAT_HIP_FIT_COMP or MCRAT_HIP_FIT_BAND",
    NULL_ARRAY: "fit_spectra: count, w, e_edges and log_e must not be NULL",
    BAD_N_E: "fit_spectra: n_e must be between 1 and 512",
    EDGES_NOT_FINITE: "fit_spectra: an energy edge is not finite",
    EDGES_NOT_ASCENDING: "fit_spectra: the energy edges must ascend strictly",
    EDGES_NOT_POSITIVE: "fit_spectra: the energy edges must be positive",
    LOG_E_NOT_FINITE: "fit_spectra: a value of log_e is not finite",
    BAD_PIVOT: "fit_spectra: e_piv must be positive and finite",
    BOUNDS_NOT_FINITE: "fit_spectra: a bound of the search is not finite",
    BOUNDS_EMPTY: "fit_spectra: the bounds need lo < hi for alpha, lambda and (Band) beta",
    BOUNDS_NO_CANDIDATE: "fit_spectra: the bounds allow no candidate with 2 + alpha > 0 and (Band) alpha > beta",
    BAD_GRID: "fit_spectra: g_alpha, g_lambda and g_beta must be at least 1",
    GRID_TOO_LARGE: "fit_spectra: the coarse grid has more than 1048576 candidates",
    BAD_ROUNDS: "fit_spectra: n_rounds must be between 0 and 4096",
    BAD_SHRINK: "fit_spectra: shrink must lie in (0.25, 1)",
    BAD_MIN_COUNT: "fit_spectra: min_count must be at least 1",
    BAD_N_SPEC: "fit_spectra: n_spec must be between 0 and INT_MAX",
}
# a case: statements that spoil the good arguments `a` (three bins, two spectra, BAND; the arrays are edges[4], log_e[3]) -> the refusal
PLANS = {
    "good": ("", OK),
    "comp": ("a.model = 0;", OK),
    "comp_reads_no_beta_bounds": ("a.model = 0; a.beta_lo = NAN; a.beta_hi = -INFINITY;", OK),
    "comp_grid_beta_not_counted": ("a.model = 0; a.g_alpha = 1024; a.g_lambda = 1024; a.g_beta = 1000;", OK),
    "no_spectra": ("a.n_spec = 0;", OK),
    "most_bins": ("a.n_e = 512; a.e_edges = many_edges; a.log_e = many_log_e; a.n_spec = 0;", OK),
    "largest_grid": ("a.g_alpha = 128; a.g_lambda = 128; a.g_beta = 64;", OK),
    "rounds_0": ("a.n_rounds = 0;", OK), "rounds_most": ("a.n_rounds = 4096;", OK),
    "most_spectra": ("a.n_spec = 2147483647ll;", OK),
    "model_2": ("a.model = 2;", BAD_MODEL), "model_negative": ("a.model = -1;", BAD_MODEL),
    "count_null": ("a.count = nullptr;", NULL_ARRAY), "w_null": ("a.w = nullptr;", NULL_ARRAY),
    "edges_null": ("a.e_edges = nullptr;", NULL_ARRAY), "log_e_null": ("a.log_e = nullptr;", NULL_ARRAY),
    "n_e_0": ("a.n_e = 0;", BAD_N_E), "n_e_513": ("a.n_e = 513;", BAD_N_E), "n_e_negative": ("a.n_e = -3;", BAD_N_E),
    "edge_nan": ("edges[1] = NAN;", EDGES_NOT_FINITE), "edge_inf": ("edges[3] = INFINITY;", EDGES_NOT_FINITE),
    "edges_equal": ("edges[2] = edges[1];", EDGES_NOT_ASCENDING), "edges_descending": ("edges[3] = 0.5 * edges[2];", EDGES_NOT_ASCENDING),
    "edge_zero": ("edges[0] = 0.0;", EDGES_NOT_POSITIVE), "edge_negative": ("edges[0] = -1.0;", EDGES_NOT_POSITIVE),
    "log_e_nan": ("log_e[2] = NAN;", LOG_E_NOT_FINITE), "log_e_inf": ("log_e[0] = -INFINITY;", LOG_E_NOT_FINITE),
    "pivot_zero": ("a.e_piv = 0.0;", BAD_PIVOT), "pivot_nan": ("a.e_piv = NAN;", BAD_PIVOT), "pivot_inf": ("a.e_piv = INFINITY;", BAD_PIVOT),
    "alpha_lo_nan": ("a.alpha_lo = NAN;", BOUNDS_NOT_FINITE), "lambda_hi_inf": ("a.lambda_hi = INFINITY;", BOUNDS_NOT_FINITE),
    "beta_lo_inf": ("a.beta_lo = -INFINITY;", BOUNDS_NOT_FINITE),
    "alpha_empty": ("a.alpha_lo = a.alpha_hi;", BOUNDS_EMPTY), "lambda_empty": ("a.lambda_lo = 9.0;", BOUNDS_EMPTY), "beta_empty": ("a.beta_hi = -7.0;", BOUNDS_EMPTY),
    "alpha_below_minus_two": ("a.alpha_lo = -5.0; a.alpha_hi = -2.0;", BOUNDS_NO_CANDIDATE),
    "beta_above_alpha": ("a.beta_lo = 2.0; a.beta_hi = 3.0;", BOUNDS_NO_CANDIDATE),
    "g_alpha_0": ("a.g_alpha = 0;", BAD_GRID), "g_lambda_negative": ("a.g_lambda = -4;", BAD_GRID), "g_beta_0": ("a.g_beta = 0;", BAD_GRID),
    "comp_g_beta_0": ("a.model = 0; a.g_beta = 0;", BAD_GRID),
    "grid_too_large": ("a.g_alpha = 128; a.g_lambda = 128; a.g_beta = 65;", GRID_TOO_LARGE),
    "grid_overflows_an_int": ("a.g_alpha = 65536; a.g_lambda = 65536; a.g_beta = 65536;", GRID_TOO_LARGE),
    "rounds_negative": ("a.n_rounds = -1;", BAD_ROUNDS), "rounds_4097": ("a.n_rounds = 4097;", BAD_ROUNDS),
    "shrink_quarter": ("a.shrink = 0.25;", BAD_SHRINK), "shrink_one": ("a.shrink = 1.0;", BAD_SHRINK), "shrink_nan": ("a.shrink = NAN;", BAD_SHRINK),
    "min_count_0": ("a.min_count = 0;", BAD_MIN_COUNT),
    "n_spec_negative": ("a.n_spec = -1;", BAD_N_SPEC), "n_spec_beyond_int": ("a.n_spec = 2147483648ll;", BAD_N_SPEC),
    # two faults at once: the first in the order decides
    "model_before_null": ("a.model = 5; a.w = nullptr;", BAD_MODEL),
    "null_before_n_e": ("a.count = nullptr; a.n_e = 0;", NULL_ARRAY),
    "n_e_before_edges": ("a.n_e = 600; edges[1] = NAN;", BAD_N_E),
    "finite_before_ascending": ("edges[3] = NAN; edges[1] = edges[0];", EDGES_NOT_FINITE),
    "ascending_before_positive": ("edges[0] = -2.0; edges[1] = -3.0;", EDGES_NOT_ASCENDING),
    "positive_before_log_e": ("edges[0] = 0.0; log_e[0] = NAN;", EDGES_NOT_POSITIVE),
    "log_e_before_pivot": ("log_e[1] = NAN; a.e_piv = -1.0;", LOG_E_NOT_FINITE),
    "pivot_before_bounds": ("a.e_piv = -1.0; a.alpha_lo = NAN;", BAD_PIVOT),
    "not_finite_before_empty": ("a.beta_hi = NAN; a.alpha_lo = 3.0;", BOUNDS_NOT_FINITE),
    "empty_before_no_candidate": ("a.alpha_lo = -4.0; a.alpha_hi = -5.0;", BOUNDS_EMPTY),
    "no_candidate_before_grid": ("a.alpha_lo = -5.0; a.alpha_hi = -2.5; a.g_alpha = 0;", BOUNDS_NO_CANDIDATE),
    "grid_before_too_large": ("a.g_alpha = 0; a.g_lambda = 2000000;", BAD_GRID),
    "too_large_before_rounds": ("a.g_lambda = 2000000; a.n_rounds = -1;", GRID_TOO_LARGE),
    "rounds_before_shrink": ("a.n_rounds = -1; a.shrink = 2.0;", BAD_ROUNDS),
    "shrink_before_min_count": ("a.shrink = 0.1; a.min_count = 0;", BAD_SHRINK),
    "min_count_before_n_spec": ("a.min_count = -1; a.n_spec = -1;", BAD_MIN_COUNT),
}

DRIVER = r'''
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fit_plan.hpp"
using namespace mcrat;
typedef std::vector<double> V;

static unsigned long long bits(double x) { unsigned long long b; memcpy(&b, &x, sizeof b); return b; }
static FILE *in;
static double rd() { char tok[64]; if (fscanf(in, "%63s", tok) != 1) { fprintf(stderr, "input ends early\n"); exit(2); } return strtod(tok, nullptr); }
static long long ri() { long long v; if (fscanf(in, "%lld", &v) != 1) { fprintf(stderr, "input ends early\n"); exit(2); } return v; }
static V rv(size_t n) { V v(n); for (double &x : v) x = rd(); return v; }

static double many_edges[513], many_log_e[512];
static void plan(const char *name, void (*spoil)(FitArgs &, double *, double *))
{
    double edges[4] = {1.0, 2.0, 4.0, 8.0}, log_e[3] = {0.25, 0.75, 1.25};
    const long long count[6] = {1, 2, 3, 4, 5, 6};
    const double w[6] = {1, 2, 3, 4, 5, 6};
    FitArgs a{};
    a.model = FIT_BAND; a.n_spec = 2; a.n_e = 3; a.count = count; a.w = w; a.e_edges = edges; a.log_e = log_e; a.e_piv = 1.0;
    a.alpha_lo = -1.9; a.alpha_hi = 2.0; a.lambda_lo = 0.0; a.lambda_hi = 2.0; a.beta_lo = -6.0; a.beta_hi = -2.05;
    a.g_alpha = 16; a.g_lambda = 16; a.g_beta = 8; a.n_rounds = 10; a.shrink = 0.5; a.min_count = 1;
    spoil(a, edges, log_e);
    FitPlan p;
    const FitRefusal why = fit_plan(a, &p);
    printf("plan_%s: %d\n", name, (int)why);
    if (why != FIT_OK) return;
    printf("planv_%s: %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", name, p.search.model, p.n_spec, p.n_e, p.search.g0, p.search.g1, p.search.g2,
           p.search.n_rounds, p.edges_offset, p.log_e_offset, p.count_offset, p.w_offset, p.input_bytes, p.f8_offset, p.f8_pitch, p.i4_offset, p.i4_pitch,
           p.total_bytes, fit_grid(p.n_spec));
}

static void print_row(const char *key, const FitRow &r)
{
    printf("%s: %llu %llu %llu %llu %llu %d %d %d\n", key, bits(r.alpha), bits(r.beta), bits(r.e_peak), bits(r.amplitude), bits(r.chi2), r.n_used, r.dof, r.status);
}

int main(int argc, char **argv)
{
    for (int i = 0; i <= 512; ++i) many_edges[i] = 1.0 + i;
    for (int i = 0; i < 512; ++i) many_log_e[i] = 0.001 * i;
@CASES@
    for (int k = 0; k <= @LAST@; ++k) printf("text_%d:%s\n", k, fit_refusal_text((FitRefusal)k));
    printf("constants: %d %d %d %d %d %d %d %d %d %zu %d %d\n", FIT_MAX_BINS, FIT_WAVE, FIT_WAVES, FIT_BLOCK, FIT_MAX_GRID, FIT_MAX_COARSE, FIT_MAX_ROUNDS, FIT_REFINE_BAND,
           FIT_REFINE_COMP, FIT_ALIGN, FIT_F8_COLUMNS, FIT_I4_COLUMNS);
    printf("grid:");
    for (int n : {0, 1, 4, 5, 262144, 262145, 2147483647}) printf(" %d", fit_grid(n));
    printf("\nnan: %llu %llu\n", bits(fit_nan()), bits(fit_inf()));
    if (argc < 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "no input file\n"); return 2; }
    {
        const size_t n = (size_t)ri();
        const V x = rv(n);
        printf("exp:");
        for (double v : x) printf(" %llu", bits(fit_exp(v)));
        printf("\n");
    }
    {
        const size_t n = (size_t)ri();
        const V x = rv(n);
        printf("log:");
        for (double v : x) printf(" %llu", bits(fit_log(v)));
        printf("\n");
    }
    {   // candidates on one compacted spectrum: chi^2 and, where it is finite, the amplitude
        const int n = (int)ri();
        const V L = rv(n), y = rv(n), g = rv(n);
        const size_t k = (size_t)ri();
        printf("chi2:");
        for (size_t j = 0; j < k; ++j) {
            const int model = (int)ri();
            const double alpha = rd(), lambda = rd(), beta = rd();
            double amp = 0.0;
            const double c = fit_chi2(model, n, L.data(), y.data(), g.data(), fit_candidate(model, alpha, lambda, beta), &amp);
            printf(" %llu %llu", bits(c), c <= DBL_MAX ? bits(amp) : 0ull);
        }
        printf("\n");
    }
    const int n_fits = (int)ri();
    for (int f = 0; f < n_fits; ++f) {       // whole fits through fit_plan and the serial loop
        FitArgs a{};
        a.model = (int)ri(); a.n_spec = ri(); a.n_e = (int)ri();
        a.e_piv = rd(); a.alpha_lo = rd(); a.alpha_hi = rd(); a.lambda_lo = rd(); a.lambda_hi = rd(); a.beta_lo = rd(); a.beta_hi = rd();
        a.g_alpha = (int)ri(); a.g_lambda = (int)ri(); a.g_beta = (int)ri(); a.n_rounds = (int)ri(); a.shrink = rd(); a.min_count = ri();
        const V edges = rv((size_t)a.n_e + 1), log_e = rv((size_t)a.n_e);
        std::vector<long long> count((size_t)a.n_spec * a.n_e);
        for (long long &c : count) c = ri();
        const V w = rv((size_t)a.n_spec * a.n_e);
        a.e_edges = edges.data(); a.log_e = log_e.data(); a.count = count.data(); a.w = w.data();
        FitPlan p;
        if (fit_plan(a, &p) != FIT_OK) { fprintf(stderr, "fit %d is refused\n", f); return 2; }
        V L((size_t)a.n_e), y((size_t)a.n_e), g((size_t)a.n_e);
        for (int s = 0; s < p.n_spec; ++s) {
            char key[32];
            snprintf(key, sizeof key, "fit_%d_%d", f, s);
            print_row(key, fit_spectrum(p.search, p.n_e, count.data() + (size_t)s * a.n_e, w.data() + (size_t)s * a.n_e, edges.data(), log_e.data(), L.data(), y.data(), g.data()));
        }
    }
    fclose(in);
    return 0;
}
'''

N_EXP = N_LOG = 4000
N_CHI2 = 2000


def _hex(a):
    return " ".join(float(x).hex() if x == x else "nan" for x in np.asarray(a, dtype=np.float64).ravel())


def edges_of(n_e, lo_kev=10.0, hi_kev=1e4):
    return np.logspace(np.log10(lo_kev), np.log10(hi_kev), n_e + 1) * F.KEV


def synthetic(rng, model, n_spec, n_e, total=3e4):
    """Poisson spectra of random Band or cutoff power-law shapes on n_e bins over three decades -> edges, log_e, count, w"""
    edges = edges_of(n_e)
    cen = np.sqrt(edges[:-1] * edges[1:])
    count, w = np.zeros((n_spec, n_e), dtype=np.int64), np.zeros((n_spec, n_e))
    for s in range(n_spec):
        shape = F.band_shape(rng.uniform(-1.5, 0.3), rng.uniform(-3.5, -2.2) if model == F.BAND else None, rng.uniform(50.0, 2000.0) * F.KEV, cen) * np.diff(edges)
        count[s] = rng.poisson(total * shape / shape.sum())
        w[s] = count[s] * rng.uniform(0.5, 2.0) * 1e50
    return edges, F.log_e_of(edges), count, w


def exp_inputs():
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-745.0, 50.0, N_EXP - 1020), rng.uniform(-760.0, -690.0, 500), rng.uniform(700.0, 712.0, 200), rng.uniform(-1e-3, 1e-3, 300),
                        [0.0, -0.0, -746.0, -746.0000001, 709.78, 709.7800001, np.inf, -np.inf, np.nan, -745.2, -708.4, 1.0, -1.0, 0.5 * np.log(2.0), -0.5 * np.log(2.0),
                         -1000.0 * np.log(2.0), -1001.0 * np.log(2.0), -1074.0 * np.log(2.0), -1075.0 * np.log(2.0), 1e300]])
    assert len(x) == N_EXP
    return x


def log_inputs():
    rng = np.random.default_rng(12)
    x = np.concatenate([10.0 ** rng.uniform(-12.0, 12.0, N_LOG - 2016), rng.uniform(0.5, 2.0, 1000), 1.0 + rng.uniform(-1e-6, 1e-6, 500),
                        10.0 ** rng.uniform(-320.0, 308.0, 500),
                        [1.0, 2.0, 0.5, np.sqrt(0.5), np.sqrt(2.0), F.SQRT_HALF, np.nextafter(F.SQRT_HALF, 0.0), 5e-324, 1.7976931348623157e308, 0.0, -0.0, -1.0, np.inf,
                         -np.inf, np.nan, 1e-12]])
    assert len(x) == N_LOG
    return x


def chi2_inputs():
    """one Poisson spectrum of 40 bins, compacted, and N_CHI2 candidates of both models: inside the default bounds, a tenth of them outside validity"""
    rng = np.random.default_rng(13)
    edges, log_e, count, w = synthetic(rng, F.BAND, 1, 40)
    n_used, L, y, g = F.compact(count, w, edges, log_e, 1)
    n = int(n_used[0])
    model = rng.integers(0, 2, N_CHI2)
    alpha, lam, beta = rng.uniform(-1.9, 2.0, N_CHI2), rng.uniform(np.log(0.1), np.log(100.0), N_CHI2), rng.uniform(-6.0, -2.05, N_CHI2)
    alpha[::20] = rng.uniform(-3.0, -2.0, len(alpha[::20]))                # 2 + alpha <= 0
    beta[10::20] = alpha[10::20] + rng.uniform(0.0, 1.0, len(beta[10::20]))      # alpha - beta <= 0
    alpha[5], alpha[6], beta[6] = -2.0, 1.0, 1.0
    lam[7], lam[8] = 800.0, -800.0                                          # every bin far below the peak (x == 0); every bin far above it (x == +inf)
    return n, L[0, :n], y[0, :n], g[0, :n], model, alpha, lam, beta


def fit_inputs():
    """whole fits: (model, bounds, grid, n_rounds, shrink, min_count, edges, log_e, count, w) -- small searches, so that the serial loop stays quick"""
    rng = np.random.default_rng(14)
    fits = []
    for model, n_e, grid, n_rounds, shrink, min_count in ((F.BAND, 40, (5, 7, 3), 12, 0.7, 1), (F.COMP, 40, (9, 4, 1), 12, 0.6, 3), (F.BAND, 5, (4, 4, 4), 0, 0.5, 1),
                                                           (F.BAND, 70, (1, 1, 1), 6, 0.9, 2)):
        edges, log_e, count, w = synthetic(rng, model, 3, n_e, total=2e3)
        count[1, ::2] = 0                                                  # gaps: the compaction is not the identity
        w[2, 1] = np.inf
        if n_e == 5:
            count[2, :3] = 0                                               # two used bins: TOO_FEW_BINS
        fits.append((model, F.default_bounds(edges), grid, n_rounds, shrink, min_count, edges, log_e, count, w))
    # a spectrum far below every break the bounds allow: beta is not constrained, equal chi^2 for every beta of an (alpha, lambda)
    edges = edges_of(12, 10.0, 40.0)
    cen = np.sqrt(edges[:-1] * edges[1:])
    w = (F.band_shape(-1.0, None, 3000.0 * F.KEV, cen) * np.diff(edges))[None, :] * 1e55
    fits.append((F.BAND, ((-1.9, 2.0), (np.log(20.0), np.log(100.0)), (-6.0, -2.05)), (4, 4, 4), 5, 0.6, 1, edges, F.log_e_of(edges), np.full((1, 12), 50, dtype=np.int64), w))
    return fits


def _input_text():
    parts = ["%d %s" % (N_EXP, _hex(exp_inputs())), "%d %s" % (N_LOG, _hex(log_inputs()))]
    n, L, y, g, model, alpha, lam, beta = chi2_inputs()
    parts.append("%d %s %s %s %d" % (n, _hex(L), _hex(y), _hex(g), N_CHI2))
    parts.append(" ".join("%d %s" % (m, _hex([a, l, b])) for m, a, l, b in zip(model, alpha, lam, beta)))
    fits = fit_inputs()
    parts.append(str(len(fits)))
    for model, bounds, grid, n_rounds, shrink, min_count, edges, log_e, count, w in fits:
        parts.append("%d %d %d %s %s %d %d %d %d %s %d" % (model, count.shape[0], count.shape[1], _hex([F.E_PIV]), _hex([b for pair in bounds for b in pair]), grid[0], grid[1],
                                                       grid[2], n_rounds, _hex([shrink]), min_count))
        parts.append(_hex(edges) + " " + _hex(log_e))
        parts.append(" ".join(str(int(c)) for c in count.ravel()) + " " + " ".join("inf" if np.isinf(x) else float(x).hex() for x in w.ravel()))
    return "\n".join(parts) + "\n"


def _build(d, src, name, extra):
    exe = d / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcrat_amd", "csrc"), str(src), "-o", str(exe)] + extra,
                   check=True)
    return exe


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the rules' driver")
    d = tmp_path_factory.mktemp("fit_plan")
    src = d / "driver.cpp"
    cases = "\n".join('    plan("%s", [](FitArgs &a, double *edges, double *log_e) { (void)a; (void)edges; (void)log_e; %s });' % (name, spoil) for name, (spoil, _) in PLANS.items())
    src.write_text(DRIVER.replace("@CASES@", cases).replace("@LAST@", str(BAD_N_SPEC)))
    inputs = d / "inputs.txt"
    inputs.write_text(_input_text())
    return d, src, inputs


@pytest.fixture(scope="module")
def text(built):
    d, src, inputs = built
    return subprocess.run([str(_build(d, src, "driver", ["-O2"])), str(inputs)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def out(text):
    res = {}
    for line in text.splitlines():
        key, _, vals = line.partition(":")
        res[key] = vals if key.startswith("text_") else [int(v) for v in vals.split()]
    return res


def _bits(a):
    return [int(b) for b in np.asarray(a, dtype=np.float64).view(np.uint64).ravel()]


def layout_rule(n_spec, n_e):
    up = lambda x: -(-x // 256) * 256
    at = 0
    edges = at; at = up(at + 8 * (n_e + 1))
    log_e = at; at = up(at + 8 * n_e)
    count = at; at = up(at + 8 * n_spec * n_e)
    w = at; at = up(at + 8 * n_spec * n_e)
    f8, f8_pitch = at, up(8 * n_spec); at += 5 * f8_pitch
    i4, i4_pitch = at, up(4 * n_spec); at += 3 * i4_pitch
    return [edges, log_e, count, w, f8, f8, f8_pitch, i4, i4_pitch, at]


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan(out, name):
    want = PLANS[name][1]
    assert out["plan_" + name] == [want], (name, out["plan_" + name])
    assert ("planv_" + name in out) == (want == OK)


def test_layouts_and_grids(out):
    assert out["planv_good"] == [F.BAND, 2, 3, 16, 16, 8, 10] + layout_rule(2, 3) + [1]
    assert out["planv_comp"][:7] == [F.COMP, 2, 3, 16, 16, 1, 10]
    assert out["planv_comp_grid_beta_not_counted"][3:6] == [1024, 1024, 1]
    assert out["planv_most_bins"][7:17] == layout_rule(0, 512)
    n = 2 ** 31 - 1
    assert out["planv_most_spectra"][7:17] == layout_rule(n, 3) and out["planv_most_spectra"][-1] == 65536
    assert out["grid"] == [1, 1, 1, 2, 65536, 65536, 65536]
    assert out["constants"] == [F.MAX_BINS, F.WAVE, F.WAVES, 256, 65536, F.MAX_COARSE, F.MAX_ROUNDS, 4, 8, 256, 5, 3]
    assert 3 * 8 * F.MAX_BINS * F.WAVES <= 64 * 1024                          # (L, y, g) of four spectra fit the LDS of a workgroup
    assert out["nan"] == _bits([F.NAN, np.inf])


def test_every_refusal_is_reached_and_the_order_is_the_documented_one(out):
    assert {why for _, why in PLANS.values()} - {OK} == set(TEXTS)
    order = ["model_before_null", "null_before_n_e", "n_e_before_edges", "finite_before_ascending", "ascending_before_positive", "positive_before_log_e",
             "log_e_before_pivot", "pivot_before_bounds", "not_finite_before_empty", "empty_before_no_candidate", "no_candidate_before_grid", "grid_before_too_large",
             "too_large_before_rounds", "rounds_before_shrink", "shrink_before_min_count", "min_count_before_n_spec"]
    assert [PLANS[k][1] for k in order] == list(range(BAD_MODEL, BAD_N_SPEC))    # every neighbouring pair of the order has a case with both faults


def test_refusal_texts(out):
    assert out["text_0"] == ""
    for k, t in TEXTS.items():
        assert out["text_%d" % k] == t and t.startswith("fit_spectra: ")
    assert len(set(TEXTS.values())) == len(TEXTS)


def test_exp_and_log_have_the_checkers_bits(out):
    assert out["exp"] == _bits(F.fit_exp(exp_inputs()))
    got, want = out["log"], _bits(F.fit_log(log_inputs()))
    assert got == want
    assert F.fit_exp(np.array([-1e300, -746.0000001]))[1] == 0.0 and F.fit_exp(np.array([709.7800001]))[0] == np.inf


def test_a_candidates_chi2_has_the_checkers_bits(out):
    n, L, y, g, model, alpha, lam, beta = chi2_inputs()
    assert N_EXP + N_LOG + N_CHI2 == 10 ** 4
    got = out["chi2"]
    finite = 0
    for m in (F.COMP, F.BAND):
        sel = np.nonzero(model == m)[0]
        chi, amp = F.chi2(m, np.array([n]), L[None, :], y[None, :], g[None, :], F.candidate(m, alpha[None, sel], lam[None, sel], beta[None, sel]))
        for j, c, a in zip(sel, chi[0], amp[0]):
            assert got[2 * j] == _bits([c])[0], (m, j)
            if np.isfinite(c):
                assert got[2 * j + 1] == _bits([a])[0], (m, j)
                finite += 1
    assert N_CHI2 // 2 < finite < N_CHI2 - N_CHI2 // 20                    # both the rule's +inf and finite values are compared
    assert got[2 * 5] == _bits([np.inf])[0]                                # 2 + alpha == 0


def test_whole_fits_on_the_host_equal_the_checkers(out):
    seen = 0
    for f, (model, bounds, grid, n_rounds, shrink, min_count, edges, log_e, count, w) in enumerate(fit_inputs()):
        want = F.fit(count, w, edges, log_e, model, bounds, grid=grid, n_rounds=n_rounds, shrink=shrink, min_count=min_count)
        for s in range(count.shape[0]):
            got = out["fit_%d_%d" % (f, s)]
            assert got[:5] == [_bits([want[k][s]])[0] for k in ("alpha", "beta", "e_peak", "amplitude", "chi2")], (f, s)
            assert got[5:] == [int(want[k][s]) for k in ("n_used", "dof", "status")], (f, s)
            seen |= int(want["status"][s]) | (32 if want["status"][s] == 0 else 0)
    assert seen & F.TOO_FEW_BINS and seen & 32 and seen & F.AT_BOUND_BETA
    # the unconstrained beta resolves to the lowest index: with round 0 alone beta is the centre of the first of the four beta cells, exactly
    last = F.fit(*[fit_inputs()[-1][k] for k in (8, 9, 6, 7, 0, 1)], grid=(4, 4, 4), n_rounds=0, shrink=0.6)
    assert last["beta"][0] == -6.0 + 0.5 * ((-2.05 - -6.0) / 4.0) and last["status"][0] & F.AT_BOUND_BETA and np.isfinite(last["chi2"][0])


def test_driver_is_clean_under_the_sanitizers(built, text):
    """the same driver as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer: nothing reported, the same output"""
    d, src, inputs = built
    exe = _build(d, src, "driver_san", ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([str(exe), str(inputs)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "" and r.stdout == text
