// fit_plan.hpp -- the host's rules for the spectral fit (mcrat_hip_fit_spectra): the refusals and their texts, the layout of the block on the device,
// which bins are used, the two models, exp and log as fixed sequences of IEEE operations, a candidate's chi^2 with the amplitude profiled out, the
// boxes of the search and the search itself -- written once here and used by the kernel (fit.hip).  Plain inline C++ -- no HIP call, no context, no
// allocation -- so that a CPU test can drive them (tests/test_fit_plan_cpu.py).
//
// Definitions.  A spectrum is a row of n_e bins (count_i, W_i); bin i has the edges e_edges[i], e_edges[i + 1] (erg).
//     dE_i = e_edges[i + 1] - e_edges[i],   L_i = ln(E_i / E_piv) at the geometric centre E_i -- an input array, log_e[n_e] --,
//     y_i = W_i / dE_i,   g_i = (double)count_i / (y_i * y_i)        (sigma_i = y_i / sqrt(count_i))
// A bin is used iff count_i >= min_count, W_i is finite and W_i > 0; the used bins are compacted in bin order.  With fewer used bins than
// parameters + 1 the status is TOO_FEW_BINS, the double outputs are NaN and no search runs.
//
// Models.  The search runs in u = (alpha, lambda, beta), lambda = ln(E_pk / E_piv).  With a2 = 2 + alpha, amb = alpha - beta and
// x_i = a2 * fit_exp(L_i - lambda):
//     COMP   ln m_i = alpha * L_i - x_i                                                                              (2 parameters; beta is not read)
//     BAND   the same where x_i < amb; elsewhere ln m_i = c0 + beta * L_i,  c0 = amb * (((fit_log(amb) - fit_log(a2)) + lambda) - 1)
// and m_i = fit_exp(ln m_i).  A candidate with a2 <= 0 or (BAND) amb <= 0 has chi^2 = +inf.
//
// Amplitude.  Pass one over the used bins, in order:  gm = g_i * m_i,  Sym += gm * y_i,  Smm += gm * m_i;  A = Sym / Smm.  Pass two:
// r = y_i - A * m_i,  chi^2 += g_i * (r * r).  Smm zero or not finite: chi^2 = +inf; a chi^2 that is not a finite number is +inf.
//
// Search.  The bounds are lo[k] < hi[k], k = alpha, lambda, beta.  Round 0: the cell centres of a grid of g_alpha x g_lambda x g_beta cells over
// the bounds (COMP: g_beta counts as 1), in index order, alpha fastest.  Rounds 1 .. n_rounds: 4 x 4 x 4 (BAND) or 8 x 8 (COMP) cell centres of a
// box whose side is the previous round's side times shrink (round 0's side is hi - lo), centred on the best candidate so far and shifted, not
// clipped, to stay inside the bounds.  Best: the lowest chi^2 over all rounds so far; among equals the earliest round, then the lowest index.  No
// candidate with a finite chi^2: NO_FINITE_CANDIDATE, double outputs NaN but chi2 = +inf.  AT_BOUND_*: the result lies within one cell of the
// last round of that bound.  The kernel takes the candidates of a round 64 at a time, a lane each; the serial loop below gives the same bits.
#pragma once
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MCRAT_FIT_HD __host__ __device__
#else
#define MCRAT_FIT_HD
#endif

namespace mcrat {

enum FitModel { FIT_COMP = 0, FIT_BAND = 1 };
enum FitStatus { FIT_TOO_FEW_BINS = 1, FIT_AT_BOUND_ALPHA = 2, FIT_AT_BOUND_LAMBDA = 4, FIT_AT_BOUND_BETA = 8, FIT_NO_FINITE_CANDIDATE = 16 };

constexpr int FIT_MAX_BINS = 512;                // (L, y, g) of one spectrum in LDS: 12 KB a wavefront, 48 KB a workgroup
constexpr int FIT_WAVE = 64;
constexpr int FIT_WAVES = 4;                     // spectra per workgroup, a wavefront each
constexpr int FIT_BLOCK = FIT_WAVE * FIT_WAVES;
constexpr int FIT_MAX_GRID = 65536;              // workgroups: a grid-stride loop over the spectra
constexpr int FIT_MAX_COARSE = 1 << 20;          // candidates of round 0
constexpr int FIT_MAX_ROUNDS = 4096;
constexpr int FIT_REFINE_BAND = 4;               // cells per axis of a refinement round: 4 x 4 x 4
constexpr int FIT_REFINE_COMP = 8;               // ... and 8 x 8: FIT_WAVE candidates either way
static_assert(FIT_REFINE_BAND * FIT_REFINE_BAND * FIT_REFINE_BAND == FIT_WAVE && FIT_REFINE_COMP * FIT_REFINE_COMP == FIT_WAVE, "one candidate per lane");
constexpr size_t FIT_ALIGN = 256;

// ------------------------------------------------------------------ refusals and their texts
// In the order they are checked.
enum FitRefusal {
    FIT_OK = 0,
    FIT_BAD_MODEL,
    FIT_NULL_ARRAY,
    FIT_BAD_N_E,
    FIT_EDGES_NOT_FINITE,
    FIT_EDGES_NOT_ASCENDING,
    FIT_EDGES_NOT_POSITIVE,
    FIT_LOG_E_NOT_FINITE,
    FIT_BAD_PIVOT,
    FIT_BOUNDS_NOT_FINITE,
    FIT_BOUNDS_EMPTY,
    FIT_BOUNDS_NO_CANDIDATE,
    FIT_BAD_GRID,
    FIT_GRID_TOO_LARGE,
    FIT_BAD_ROUNDS,
    FIT_BAD_SHRINK,
    FIT_BAD_MIN_COUNT,
    FIT_BAD_N_SPEC
};
inline const char *fit_refusal_text(FitRefusal why)
{
    switch (why) {
    case FIT_OK: return "";
    case FIT_BAD_MODEL: return "fit_spectra: model must be MCRAT_HIP_FIT_COMP or MCRAT_HIP_FIT_BAND";
    case FIT_NULL_ARRAY: return "fit_spectra: count, w, e_edges and log_e must not be NULL";
    case FIT_BAD_N_E: return "fit_spectra: n_e must be between 1 and 512";
    case FIT_EDGES_NOT_FINITE: return "fit_spectra: an energy edge is not finite";
    case FIT_EDGES_NOT_ASCENDING: return "fit_spectra: the energy edges must ascend strictly";
    case FIT_EDGES_NOT_POSITIVE: return "fit_spectra: the energy edges must be positive";
    case FIT_LOG_E_NOT_FINITE: return "fit_spectra: a value of log_e is not finite";
    case FIT_BAD_PIVOT: return "fit_spectra: e_piv must be positive and finite";
    case FIT_BOUNDS_NOT_FINITE: return "fit_spectra: a bound of the search is not finite";
    case FIT_BOUNDS_EMPTY: return "fit_spectra: the bounds need lo < hi for alpha, lambda and (Band) beta";
    case FIT_BOUNDS_NO_CANDIDATE: return "fit_spectra: the bounds allow no candidate with 2 + alpha > 0 and (Band) alpha > beta";
    case FIT_BAD_GRID: return "fit_spectra: g_alpha, g_lambda and g_beta must be at least 1";
    case FIT_GRID_TOO_LARGE: return "fit_spectra: the coarse grid has more than 1048576 candidates";
    case FIT_BAD_ROUNDS: return "fit_spectra: n_rounds must be between 0 and 4096";
    case FIT_BAD_SHRINK: return "fit_spectra: shrink must lie in (0.25, 1)";
    case FIT_BAD_MIN_COUNT: return "fit_spectra: min_count must be at least 1";
    case FIT_BAD_N_SPEC: return "fit_spectra: n_spec must be between 0 and INT_MAX";
    }
    return "";
}

// ------------------------------------------------------------------ exp and log (host and device)
// Only + - * / and rint, frexp, ldexp: with -ffp-contract=off the same bits on the device, in g++ and in NumPy.  Within 4 ulp of the true value
// for exp on [-745, 50] and log on [1e-12, 1e12] (tests/test_fit_checker_cpu.py, against 200-bit arithmetic).
constexpr double FIT_LN2_HI = 6.93147180369123816490e-01;        // the upper 32 bits of ln 2: k * FIT_LN2_HI is exact for |k| < 2^20
constexpr double FIT_LN2_LO = 1.90821492927058770002e-10;        // ln 2 - FIT_LN2_HI
constexpr double FIT_INV_LN2 = 1.44269504088896338700e+00;
constexpr double FIT_SQRT_HALF = 7.07106781186547524401e-01;
MCRAT_FIT_HD inline double fit_nan()
{
    const uint64_t bits = 0x7ff8000000000000ull;                 // the one NaN the outputs hold
    double x;
    memcpy(&x, &bits, sizeof x);
    return x;
}
MCRAT_FIT_HD inline double fit_inf() { return HUGE_VAL; }
// exp(x): x = k ln 2 + r with k = rint(x / ln 2), |r| <= 0.35; the Taylor polynomial of degree 13 by Horner; times 2^k.  Below -746: 0; above
// 709.78: +inf; a result below 2^-1000 takes its one rounding in a multiplication.
MCRAT_FIT_HD inline double fit_exp(double x)
{
    if (x != x) return x;
    if (x < -746.0) return 0.0;
    if (x > 709.78) return fit_inf();
    const double kd = rint(x * FIT_INV_LN2);
    const double r = (x - kd * FIT_LN2_HI) - kd * FIT_LN2_LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const int k = (int)kd;
    if (k < -1000) return ldexp(p, k + 1000) * 0x1p-1000;
    return ldexp(p, k);
}
// ln(x), x positive and finite (anything else: NaN): x = m 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1),
// ln m = 2 s (1 + s^2 / 3 + s^4 / 5 + ... + s^22 / 23) by Horner in s^2, and e ln 2 in two parts.
MCRAT_FIT_HD inline double fit_log(double x)
{
    if (!(x > 0.0) || !(x <= DBL_MAX)) return fit_nan();
    int e;
    double m = frexp(x, &e);
    if (m < FIT_SQRT_HALF) { m = m * 2.0; e = e - 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    const double ed = (double)e;
    return ed * FIT_LN2_HI + ((2.0 * s) * p + ed * FIT_LN2_LO);
}

// ------------------------------------------------------------------ the data (host and device)
// whether bin (count, w) is used, and its y and g
MCRAT_FIT_HD inline bool fit_bin_used(long long count, double w, long long min_count) { return count >= min_count && w > 0.0 && w <= DBL_MAX; }
MCRAT_FIT_HD inline void fit_bin(long long count, double w, double e_lo, double e_hi, double &y, double &g)
{
    y = w / (e_hi - e_lo);
    g = (double)count / (y * y);
}

// ------------------------------------------------------------------ a candidate and its chi^2 (host and device)
MCRAT_FIT_HD inline int fit_parameters(int model) { return model == FIT_BAND ? 3 : 2; }
struct FitCandidate {
    double alpha, lambda, beta;
    double a2, amb, c0;
    bool valid;
};
MCRAT_FIT_HD inline FitCandidate fit_candidate(int model, double alpha, double lambda, double beta)
{
    FitCandidate c;
    c.alpha = alpha; c.lambda = lambda; c.beta = beta;
    c.a2 = 2.0 + alpha;
    c.amb = alpha - beta;
    c.valid = c.a2 > 0.0 && (model != FIT_BAND || c.amb > 0.0);
    c.c0 = 0.0;
    if (c.valid && model == FIT_BAND) c.c0 = c.amb * (((fit_log(c.amb) - fit_log(c.a2)) + lambda) - 1.0);
    return c;
}
// m_i of a valid candidate at L
MCRAT_FIT_HD inline double fit_model(int model, const FitCandidate &c, double L)
{
    const double x = c.a2 * fit_exp(L - c.lambda);
    double ln_m = c.alpha * L - x;
    if (model == FIT_BAND && !(x < c.amb)) ln_m = c.c0 + c.beta * L;
    return fit_exp(ln_m);
}
// -> chi^2 of the candidate on the n compacted bins, *A its amplitude (not set when chi^2 is +inf by rule)
MCRAT_FIT_HD inline double fit_chi2(int model, int n, const double *L, const double *y, const double *g, const FitCandidate &c, double *A)
{
    if (!c.valid) return fit_inf();
    double sym = 0.0, smm = 0.0;
    for (int i = 0; i < n; ++i) {
        const double m = fit_model(model, c, L[i]);
        const double gm = g[i] * m;
        sym = sym + gm * y[i];
        smm = smm + gm * m;
    }
    if (!(smm > 0.0) || !(smm <= DBL_MAX)) return fit_inf();
    const double amp = sym / smm;
    double chi2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const double m = fit_model(model, c, L[i]);
        const double r = y[i] - amp * m;
        chi2 = chi2 + g[i] * (r * r);
    }
    *A = amp;
    if (!(chi2 <= DBL_MAX)) return fit_inf();
    return chi2;
}

// ------------------------------------------------------------------ the search (host and device)
// what the caller chose, as the kernel takes it
struct FitSearch {
    int model;
    double lo0, lo1, lo2, hi0, hi1, hi2;         // alpha, lambda, beta
    int g0, g1, g2;                              // the coarse grid (g2 == 1 for COMP)
    int n_rounds;
    double shrink, e_piv;
    long long min_count;
};
// the cells of one round: n0 * n1 * n2 of them, cell k along axis a centred at lo_a + (k + 0.5) * cell_a
struct FitBox {
    double lo0, lo1, lo2, cell0, cell1, cell2, side0, side1, side2;
    int n0, n1, n2;
};
MCRAT_FIT_HD inline int fit_box_candidates(const FitBox &b) { return b.n0 * b.n1 * b.n2; }
MCRAT_FIT_HD inline FitBox fit_coarse_box(const FitSearch &s)
{
    FitBox b;
    b.n0 = s.g0; b.n1 = s.g1; b.n2 = s.model == FIT_BAND ? s.g2 : 1;
    b.lo0 = s.lo0; b.lo1 = s.lo1; b.lo2 = s.lo2;
    b.side0 = s.hi0 - s.lo0; b.side1 = s.hi1 - s.lo1; b.side2 = s.hi2 - s.lo2;
    b.cell0 = b.side0 / (double)b.n0; b.cell1 = b.side1 / (double)b.n1; b.cell2 = b.side2 / (double)b.n2;
    return b;
}
// one axis of a refinement box: the side, centred on c, shifted into [lo, hi]
MCRAT_FIT_HD inline double fit_axis_lo(double c, double side, double lo, double hi)
{
    double at = c - 0.5 * side;
    if (at < lo) at = lo;
    if (at + side > hi) at = hi - side;
    return at;
}
MCRAT_FIT_HD inline FitBox fit_refine_box(const FitSearch &s, const FitBox &prev, double alpha, double lambda, double beta)
{
    const int n = s.model == FIT_BAND ? FIT_REFINE_BAND : FIT_REFINE_COMP;
    FitBox b;
    b.n0 = n; b.n1 = n; b.n2 = s.model == FIT_BAND ? n : 1;
    b.side0 = prev.side0 * s.shrink; b.side1 = prev.side1 * s.shrink; b.side2 = prev.side2 * s.shrink;
    b.lo0 = fit_axis_lo(alpha, b.side0, s.lo0, s.hi0);
    b.lo1 = fit_axis_lo(lambda, b.side1, s.lo1, s.hi1);
    b.lo2 = fit_axis_lo(beta, b.side2, s.lo2, s.hi2);
    b.cell0 = b.side0 / (double)b.n0; b.cell1 = b.side1 / (double)b.n1; b.cell2 = b.side2 / (double)b.n2;
    return b;
}
// candidate idx of a box, alpha fastest
MCRAT_FIT_HD inline void fit_box_point(const FitBox &b, int idx, double &alpha, double &lambda, double &beta)
{
    const int i0 = idx % b.n0, rest = idx / b.n0;
    const int i1 = rest % b.n1, i2 = rest / b.n1;
    alpha = b.lo0 + ((double)i0 + 0.5) * b.cell0;
    lambda = b.lo1 + ((double)i1 + 0.5) * b.cell1;
    beta = b.lo2 + ((double)i2 + 0.5) * b.cell2;
}
// the best candidate so far; where the search starts: the middle of the bounds, chi^2 = +inf
struct FitBest { double alpha, lambda, beta, amplitude, chi2; };
MCRAT_FIT_HD inline FitBest fit_start(const FitSearch &s)
{
    FitBest b;
    b.alpha = s.lo0 + 0.5 * (s.hi0 - s.lo0); b.lambda = s.lo1 + 0.5 * (s.hi1 - s.lo1); b.beta = s.lo2 + 0.5 * (s.hi2 - s.lo2);
    b.amplitude = fit_nan(); b.chi2 = fit_inf();
    return b;
}
// one spectrum's outputs
struct FitRow { double alpha, beta, e_peak, amplitude, chi2; int n_used, dof, status; };
MCRAT_FIT_HD inline FitRow fit_too_few(int model, int n_used)
{
    FitRow r;
    r.alpha = r.beta = r.e_peak = r.amplitude = r.chi2 = fit_nan();
    r.n_used = n_used; r.dof = n_used - fit_parameters(model); r.status = FIT_TOO_FEW_BINS;
    return r;
}
MCRAT_FIT_HD inline bool fit_near(double x, double lo, double hi, double cell) { return x - lo <= cell || hi - x <= cell; }
// the outputs from the best candidate and the last round's box
MCRAT_FIT_HD inline FitRow fit_finish(const FitSearch &s, const FitBest &best, const FitBox &last, int n_used)
{
    FitRow r;
    r.n_used = n_used; r.dof = n_used - fit_parameters(s.model); r.status = 0;
    r.chi2 = best.chi2;
    if (!(best.chi2 <= DBL_MAX)) {
        r.alpha = r.beta = r.e_peak = r.amplitude = fit_nan();
        r.status = FIT_NO_FINITE_CANDIDATE;
        return r;
    }
    r.alpha = best.alpha;
    r.beta = s.model == FIT_BAND ? best.beta : fit_nan();
    r.e_peak = s.e_piv * fit_exp(best.lambda);
    r.amplitude = best.amplitude;
    if (fit_near(best.alpha, s.lo0, s.hi0, last.cell0)) r.status |= FIT_AT_BOUND_ALPHA;
    if (fit_near(best.lambda, s.lo1, s.hi1, last.cell1)) r.status |= FIT_AT_BOUND_LAMBDA;
    if (s.model == FIT_BAND && fit_near(best.beta, s.lo2, s.hi2, last.cell2)) r.status |= FIT_AT_BOUND_BETA;
    return r;
}
// The whole fit of one spectrum, one candidate after another: L, y, g are scratch for n_e values each.  The kernel runs the same rounds with the
// candidates of a round 64 at a time and a wavefront reduction on (chi^2, lane) in place of the inner loop.
inline FitRow fit_spectrum(const FitSearch &s, int n_e, const long long *count, const double *w, const double *e_edges, const double *log_e, double *L, double *y, double *g)
{
    int n_used = 0;
    for (int i = 0; i < n_e; ++i)
        if (fit_bin_used(count[i], w[i], s.min_count)) {
            L[n_used] = log_e[i];
            fit_bin(count[i], w[i], e_edges[i], e_edges[i + 1], y[n_used], g[n_used]);
            ++n_used;
        }
    if (n_used < fit_parameters(s.model) + 1) return fit_too_few(s.model, n_used);
    FitBest best = fit_start(s);
    FitBox box = fit_coarse_box(s);
    for (int round = 0; round <= s.n_rounds; ++round) {
        if (round > 0) box = fit_refine_box(s, box, best.alpha, best.lambda, best.beta);
        const int n = fit_box_candidates(box);
        for (int idx = 0; idx < n; ++idx) {
            double alpha, lambda, beta, amp = 0.0;
            fit_box_point(box, idx, alpha, lambda, beta);
            const double chi2 = fit_chi2(s.model, n_used, L, y, g, fit_candidate(s.model, alpha, lambda, beta), &amp);
            if (chi2 < best.chi2) { best.alpha = alpha; best.lambda = lambda; best.beta = beta; best.amplitude = amp; best.chi2 = chi2; }
        }
    }
    return fit_finish(s, best, box, n_used);
}

// ------------------------------------------------------------------ the arguments, the plan and the block
// the caller's arguments as the checks read them (host pointers)
struct FitArgs {
    int model;
    long long n_spec;
    int n_e;
    const long long *count;                      // [n_spec][n_e]
    const double *w;                             // [n_spec][n_e]
    const double *e_edges, *log_e;               // [n_e + 1], [n_e]
    double e_piv;
    double alpha_lo, alpha_hi, lambda_lo, lambda_hi, beta_lo, beta_hi;
    int g_alpha, g_lambda, g_beta, n_rounds;
    double shrink;
    long long min_count;
};
// The block: e_edges [n_e + 1]; log_e [n_e]; count [n_spec][n_e] (8 bytes each); w [n_spec][n_e]; then the outputs, alpha, beta, e_peak,
// amplitude, chi2 (double [n_spec] each) and n_used, dof, status (int [n_spec] each).  Every part starts on a multiple of FIT_ALIGN bytes.
constexpr int FIT_F8_COLUMNS = 5, FIT_I4_COLUMNS = 3;
struct FitPlan {
    FitSearch search;
    int n_spec, n_e;
    size_t edges_offset, log_e_offset, count_offset, w_offset;
    size_t f8_offset, f8_pitch, i4_offset, i4_pitch;             // column k of the doubles at f8_offset + k * f8_pitch; likewise the ints
    size_t input_bytes;                                          // what is uploaded: everything before f8_offset
    size_t total_bytes;
};
inline size_t fit_align(size_t x) { return (x + FIT_ALIGN - 1) / FIT_ALIGN * FIT_ALIGN; }
inline bool fit_finite(double x) { return x >= -DBL_MAX && x <= DBL_MAX; }

// The checks, in this order: the model; a NULL array; n_e; the edges -- finite, then ascending, then positive --; log_e finite; e_piv; the bounds --
// finite, then lo < hi, then a candidate allowed (alpha_hi > -2 and, Band, alpha_hi > beta_lo) --; the grid counts at least 1, then their product;
// n_rounds; shrink; min_count; n_spec.  COMP reads neither beta's bounds nor, beyond g_beta >= 1, its grid count.  *plan is filled when FIT_OK.
inline FitRefusal fit_plan(const FitArgs &a, FitPlan *plan)
{
    if (a.model != FIT_COMP && a.model != FIT_BAND) return FIT_BAD_MODEL;
    if (!a.count || !a.w || !a.e_edges || !a.log_e) return FIT_NULL_ARRAY;
    if (a.n_e < 1 || a.n_e > FIT_MAX_BINS) return FIT_BAD_N_E;
    for (int i = 0; i <= a.n_e; ++i)
        if (!fit_finite(a.e_edges[i])) return FIT_EDGES_NOT_FINITE;
    for (int i = 0; i < a.n_e; ++i)
        if (!(a.e_edges[i] < a.e_edges[i + 1])) return FIT_EDGES_NOT_ASCENDING;
    if (!(a.e_edges[0] > 0.0)) return FIT_EDGES_NOT_POSITIVE;
    for (int i = 0; i < a.n_e; ++i)
        if (!fit_finite(a.log_e[i])) return FIT_LOG_E_NOT_FINITE;
    if (!(a.e_piv > 0.0) || !fit_finite(a.e_piv)) return FIT_BAD_PIVOT;
    const bool band = a.model == FIT_BAND;
    if (!fit_finite(a.alpha_lo) || !fit_finite(a.alpha_hi) || !fit_finite(a.lambda_lo) || !fit_finite(a.lambda_hi)) return FIT_BOUNDS_NOT_FINITE;
    if (band && (!fit_finite(a.beta_lo) || !fit_finite(a.beta_hi))) return FIT_BOUNDS_NOT_FINITE;
    if (!(a.alpha_lo < a.alpha_hi) || !(a.lambda_lo < a.lambda_hi) || (band && !(a.beta_lo < a.beta_hi))) return FIT_BOUNDS_EMPTY;
    if (!(a.alpha_hi > -2.0) || (band && !(a.alpha_hi > a.beta_lo))) return FIT_BOUNDS_NO_CANDIDATE;
    if (a.g_alpha < 1 || a.g_lambda < 1 || a.g_beta < 1) return FIT_BAD_GRID;
    if ((long long)a.g_alpha * (long long)a.g_lambda > FIT_MAX_COARSE || (long long)a.g_alpha * (long long)a.g_lambda * (long long)(band ? a.g_beta : 1) > FIT_MAX_COARSE)
        return FIT_GRID_TOO_LARGE;
    if (a.n_rounds < 0 || a.n_rounds > FIT_MAX_ROUNDS) return FIT_BAD_ROUNDS;
    if (!(a.shrink > 0.25) || !(a.shrink < 1.0)) return FIT_BAD_SHRINK;
    if (a.min_count < 1) return FIT_BAD_MIN_COUNT;
    if (a.n_spec < 0 || a.n_spec > (long long)INT_MAX) return FIT_BAD_N_SPEC;
    FitPlan p{};
    FitSearch &s = p.search;
    s.model = a.model;
    s.lo0 = a.alpha_lo; s.hi0 = a.alpha_hi; s.lo1 = a.lambda_lo; s.hi1 = a.lambda_hi;
    s.lo2 = band ? a.beta_lo : 0.0; s.hi2 = band ? a.beta_hi : 0.0;
    s.g0 = a.g_alpha; s.g1 = a.g_lambda; s.g2 = band ? a.g_beta : 1;
    s.n_rounds = a.n_rounds; s.shrink = a.shrink; s.e_piv = a.e_piv; s.min_count = a.min_count;
    p.n_spec = (int)a.n_spec; p.n_e = a.n_e;
    const size_t cells = (size_t)p.n_spec * (size_t)p.n_e, rows = (size_t)p.n_spec;
    size_t at = 0;
    p.edges_offset = at; at = fit_align(at + 8 * ((size_t)p.n_e + 1));
    p.log_e_offset = at; at = fit_align(at + 8 * (size_t)p.n_e);
    p.count_offset = at; at = fit_align(at + 8 * cells);
    p.w_offset = at; at = fit_align(at + 8 * cells);
    p.input_bytes = at;
    p.f8_pitch = fit_align(8 * rows);
    p.f8_offset = at; at += p.f8_pitch * (size_t)FIT_F8_COLUMNS;
    p.i4_pitch = fit_align(4 * rows);
    p.i4_offset = at; at += p.i4_pitch * (size_t)FIT_I4_COLUMNS;
    p.total_bytes = at;
    *plan = p;
    return FIT_OK;
}
// what the kernel takes: the search and the block's parts (device pointers)
struct FitDev {
    FitSearch search;
    int n_spec, n_e;
    const double *e_edges, *log_e;               // [n_e + 1], [n_e]
    const long long *count;                      // [n_spec][n_e]
    const double *w;                             // [n_spec][n_e]
    double *alpha, *beta, *e_peak, *amplitude, *chi2;            // [n_spec]
    int *n_used, *dof, *status;                  // [n_spec]
};
// workgroups for n_spec spectra
inline int fit_grid(int n_spec)
{
    const long long groups = ((long long)n_spec + FIT_WAVES - 1) / FIT_WAVES;
    return (int)(groups < 1 ? 1 : (groups > FIT_MAX_GRID ? FIT_MAX_GRID : groups));
}

}  // namespace mcrat
