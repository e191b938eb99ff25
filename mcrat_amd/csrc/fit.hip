// fit.hip -- the spectral fit (mcrat_hip_fit_spectra): every row of a [n_spec][n_e] pair (count, W) fitted to a cutoff power law or a Band function
// by the deterministic, derivative-free chi^2 search of fit_plan.hpp.  One kernel:
//   one wavefront per spectrum, FIT_WAVES spectra per workgroup, a grid-stride loop over the spectra.  The wavefront compacts the used bins into
//   its part of LDS as (L, y, g) -- 64 bins a trip, a ballot and the popcount of the lanes below keep the bin order --, then every lane carries one
//   candidate of the round through both passes of fit_chi2 (all lanes read the same LDS word: a broadcast), and a butterfly of __shfl_xor on
//   (chi^2, lane) finds the round's best, the lowest lane among equals.  The candidates of round 0 are taken 64 at a time in index order and a batch
//   replaces the best so far only with a lower chi^2, so that equal candidates resolve to the lowest index as in fit_spectrum's serial loop.
// No atomics, no global scratch, no inline assembly; a wavefront touches its own part of LDS only, so no workgroup barrier and no wait on another
// workgroup; every loop is bounded by the bins, the candidates, the rounds or the spectra.  The arithmetic is fit_plan.hpp's, called, not restated:
// the outputs have the bits of the host's serial loop and of the NumPy checker.
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "launch.hpp"
#include "fit_plan.hpp"

namespace mcrat {

namespace {

__device__ __forceinline__ unsigned long long fit_lanes_below(int lane) { return (1ull << lane) - 1ull; }

__global__ __launch_bounds__(FIT_BLOCK) void fit_kernel(FitDev a)
{
    __shared__ double lds_L[FIT_WAVES][FIT_MAX_BINS], lds_y[FIT_WAVES][FIT_MAX_BINS], lds_g[FIT_WAVES][FIT_MAX_BINS];
    const int lane = (int)(threadIdx.x & (FIT_WAVE - 1)), wave = (int)(threadIdx.x / FIT_WAVE);
    double *L = lds_L[wave], *y = lds_y[wave], *g = lds_g[wave];
    const FitSearch s = a.search;
    const int n_e = a.n_e < FIT_MAX_BINS ? a.n_e : FIT_MAX_BINS;           // (fit_plan refuses more: the LDS rows hold FIT_MAX_BINS)
    const long long stride = (long long)gridDim.x * FIT_WAVES;
    for (long long spec = (long long)blockIdx.x * FIT_WAVES + wave; spec < (long long)a.n_spec; spec += stride) {
        const long long *count = a.count + spec * (long long)a.n_e;
        const double *w = a.w + spec * (long long)a.n_e;
        // the used bins, compacted in bin order
        int n_used = 0;
        for (int base = 0; base < n_e; base += FIT_WAVE) {
            const int i = base + lane;
            bool used = false;
            long long c = 0;
            double wi = 0.0;
            if (i < n_e) { c = count[i]; wi = w[i]; used = fit_bin_used(c, wi, s.min_count); }
            const unsigned long long mask = __ballot(used);
            if (used) {
                const int at = n_used + __popcll(mask & fit_lanes_below(lane));   // < n_e: one place per used bin before this one
                double yi, gi;
                fit_bin(c, wi, a.e_edges[i], a.e_edges[i + 1], yi, gi);
                L[at] = a.log_e[i]; y[at] = yi; g[at] = gi;
            }
            n_used += __popcll(mask);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        FitRow row;
        if (n_used < fit_parameters(s.model) + 1) {
            row = fit_too_few(s.model, n_used);
        } else {
            FitBest best = fit_start(s);
            FitBox box = fit_coarse_box(s);
            for (int round = 0; round <= s.n_rounds; ++round) {
                if (round > 0) box = fit_refine_box(s, box, best.alpha, best.lambda, best.beta);
                const int n = fit_box_candidates(box);
                for (int base = 0; base < n; base += FIT_WAVE) {
                    const int idx = base + lane;
                    double chi2 = fit_inf(), amp = 0.0;
                    if (idx < n) {
                        double alpha, lambda, beta;
                        fit_box_point(box, idx, alpha, lambda, beta);
                        chi2 = fit_chi2(s.model, n_used, L, y, g, fit_candidate(s.model, alpha, lambda, beta), &amp);
                    }
                    // the batch's best: the lowest chi^2, the lowest lane among equals (chi^2 is never NaN: fit_chi2)
                    double c = chi2;
                    int l = lane;
                    for (int m = FIT_WAVE / 2; m >= 1; m >>= 1) {
                        const double oc = __shfl_xor(c, m, FIT_WAVE);
                        const int ol = __shfl_xor(l, m, FIT_WAVE);
                        if (oc < c || (oc == c && ol < l)) { c = oc; l = ol; }
                    }
                    const double amp_best = __shfl(amp, l, FIT_WAVE);
                    if (c < best.chi2) {
                        fit_box_point(box, base + l, best.alpha, best.lambda, best.beta);
                        best.amplitude = amp_best; best.chi2 = c;
                    }
                }
            }
            row = fit_finish(s, best, box, n_used);
        }
        if (lane == 0) {
            a.alpha[spec] = row.alpha; a.beta[spec] = row.beta; a.e_peak[spec] = row.e_peak; a.amplitude[spec] = row.amplitude; a.chi2[spec] = row.chi2;
            a.n_used[spec] = row.n_used; a.dof[spec] = row.dof; a.status[spec] = row.status;
        }
        __builtin_amdgcn_wave_barrier();                                   // the next spectrum's bins go where this one's were read
    }
}

}  // namespace

// The caller has copied the inputs into the block (fit_plan.hpp).
hipError_t launch_fit(const FitDev &a, const FitPlan &plan, hipStream_t stream)
{
    if (a.n_spec != plan.n_spec || a.n_e != plan.n_e || a.n_e < 1 || a.n_e > FIT_MAX_BINS || a.n_spec < 0) return hipErrorInvalidValue;
    if (a.n_spec == 0) return hipSuccess;
    hipLaunchKernelGGL(fit_kernel, dim3(fit_grid(a.n_spec)), dim3(FIT_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mcrat
