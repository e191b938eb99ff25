// list_plan.hpp -- the host's rules for what changes a photon list's length: photon injection, cyclo-synchrotron pool emission and rebinning.
// Every rule here is used by the one-list path and by the rank pool's path of engine.hip alike, which is what makes a list of a pool come out bit
// for bit as the same list run alone.  Plain inline C++ -- no HIP call, no context, no allocation -- so that a CPU test can drive them
// (tests/test_list_plan_cpu.py).  Line numbers are the reference's.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "device_types.hpp"

// the rules the kernels of inject.hip apply too (weight search, list growth) are host and device functions under hipcc, plain inline ones elsewhere
#if defined(__HIPCC__)
#define MCRAT_LIST_HD __host__ __device__
#else
#define MCRAT_LIST_HD
#endif

namespace mcrat {

// ------------------------------------------------------------------ what the kernels and the host share
struct RebinRange {            // collect_photon_statistics :273-322, one per workgroup, finished on the host
    double p0_min, p0_max, theta_min, theta_max, phi_min, phi_max;
    int valid, synch;
};
struct RebinAxes {             // the three uniform histograms' ranges (:360-391) and the bin counts (:324-347)
    double e_lo, e_hi, t_lo, t_hi, p_lo, p_hi;
    int num_bins, num_bins_theta, num_bins_phi, total_bins, three;
};

// ------------------------------------------------------------------ refusals and their texts
// Where the reference refuses, exits or loops for ever, the engine returns an error code and says why (last_error).  One text per reason, whichever
// path met it.  (EMIT_NOT_CONVERGED names the number of cells: emit_not_converged_text.)
enum ListRefusal {
    LIST_OK = 0,
    REBIN_NO_VALID_PHOTONS,          // mc_cyclosynch.c:640-645
    REBIN_TOO_MANY_BINS,             // :649-654
    REBIN_BAD_DIMENSIONS,            // allocate_histograms :351-358
    REBIN_BIN_OUT_OF_RANGE,          // a photon outside the histograms: the reference's exit(1)
    REBIN_NO_NULL_SLOTS,             // addToPhotonList, photons.c:108-208
    REBIN_FEWER_PHOTONS_THAN_BINS,   // :676-681
    EMIT_NO_WEIGHT,                  // the weight loop of :1244-1296 did not end
    EMIT_NO_NULL_SLOTS,              // addToPhotonList
    EMIT_NOT_CONVERGED,              // gsl_integration_qags (:1276)
    INJECT_NO_WEIGHT,                // the weight loop of mclib.c:87-136 did not end
    INJECT_NO_PHOTONS
};
inline const char *list_refusal_text(ListRefusal why)
{
    switch (why) {
    case LIST_OK: return "";
    case REBIN_NO_VALID_PHOTONS: return "rebinning: no valid photons found for rebinning";
    case REBIN_TOO_MANY_BINS: return "rebinning would create more photons than max_photons";
    case REBIN_BAD_DIMENSIONS: return "rebinning: invalid histogram dimensions";
    case REBIN_BIN_OUT_OF_RANGE: return "rebinning: a photon maps to an invalid bin index (the reference exits)";
    case REBIN_NO_NULL_SLOTS: return "rebinning: fewer null slots than rebinned photons (the reference exits with \"Adding to the photon list has failed\")";
    case REBIN_FEWER_PHOTONS_THAN_BINS: return "rebinning: fewer photons in the list than bins after the rebinning";
    case EMIT_NO_WEIGHT: return "cyclo-synchrotron emission: no weight gives between 1 and rebin_e_perc * maximum_photons photons";
    case EMIT_NO_NULL_SLOTS: return "cyclo-synchrotron emission: fewer null slots than photons to add (the reference exits with \"Adding to the photon list has failed\")";
    case EMIT_NOT_CONVERGED: return "cyclo-synchrotron emission: the photon-density integral of %u cell(s) did not converge within the device's interval limit";
    case INJECT_NO_WEIGHT: return "photon injection: no weight puts the photon count between min_photons and max_photons";
    case INJECT_NO_PHOTONS: return "photon injection: no photons (no cell of the frame touches the injection slab?)";
    }
    return "";
}
// EMIT_NOT_CONVERGED's text for `cells` cells whose integral ran out of intervals (inject.hip, qags_planck), into buf; returns buf
inline const char *emit_not_converged_text(char *buf, size_t len, unsigned cells)
{
    snprintf(buf, len, list_refusal_text(EMIT_NOT_CONVERGED), cells);
    return buf;
}

// ------------------------------------------------------------------ rebinning (mc_cyclosynch.c:246-712)
// collect_photon_statistics :273-322 finished: the per-workgroup partials part[0 .. n), n >= 1, as one range.  A workgroup without a valid photon
// (valid == 0) leaves p0_min = DBL_MAX and p0_max = 0, neutral for photon energies, so it takes part like any other.
inline RebinRange rebin_range_merge(const RebinRange *part, int n)
{
    RebinRange q = part[0];
    for (int k = 1; k < n; ++k) {
        q.p0_min = fmin(q.p0_min, part[k].p0_min); q.p0_max = fmax(q.p0_max, part[k].p0_max);
        q.theta_min = fmin(q.theta_min, part[k].theta_min); q.theta_max = fmax(q.theta_max, part[k].theta_max);
        q.phi_min = fmin(q.phi_min, part[k].phi_min); q.phi_max = fmax(q.phi_max, part[k].phi_max);
        q.valid += part[k].valid; q.synch += part[k].synch;
    }
    return q;
}

// calculate_binning_params :324-347 and allocate_histograms :351-391: the histograms' axes from a list's range, or why the reference would not
// rebin (then *ax is not to be used).  The energy axis is log10(p0) (0 .. 1 when a p0 is not positive); angles per bin come in degrees for theta
// and in the histogram's own unit for phi; every upper edge is widened by a millionth of its range so that the largest value falls inside.  The
// checks in the reference's order: no valid photon, more bins than max_photons, an axis without bins.
inline ListRefusal rebin_axes(const RebinRange &q, double rebin_e_perc, double rebin_ang, double rebin_ang_phi, int max_photons, int three, RebinAxes *ax)
{
    if (q.valid == 0) return REBIN_NO_VALID_PHOTONS;
    const double log_p0_min = (q.p0_min > 0 && q.p0_max > 0) ? log10(q.p0_min) : 0.0, log_p0_max = (q.p0_min > 0 && q.p0_max > 0) ? log10(q.p0_max) : 1.0;
    *ax = RebinAxes{};
    ax->three = three;
    ax->num_bins = (int)(rebin_e_perc * max_photons);
    ax->num_bins_theta = (int)ceil((q.theta_max - q.theta_min) / (rebin_ang * (M_PI / 180.0)));
    ax->num_bins_phi = three ? (int)ceil((q.phi_max - q.phi_min) / rebin_ang_phi) : 1;
    const long long total_ll = (long long)ax->num_bins_theta * ax->num_bins * (three ? ax->num_bins_phi : 1);
    if (total_ll > max_photons) return REBIN_TOO_MANY_BINS;
    if (ax->num_bins <= 0 || ax->num_bins_theta <= 0 || ax->num_bins_phi <= 0) return REBIN_BAD_DIMENSIONS;
    ax->total_bins = (int)total_ll;
    ax->e_lo = log_p0_min; ax->e_hi = log_p0_max + (log_p0_max - log_p0_min) * 1e-6;
    ax->t_lo = q.theta_min; ax->t_hi = q.theta_max + (q.theta_max - q.theta_min) * 1e-6;
    ax->p_lo = q.phi_min; ax->p_hi = q.phi_max + (q.phi_max - q.phi_min) * 1e-6;
    return LIST_OK;
}

// After the rebinned photons are in the list (:676-690): a list of n slots of which n_null were null when the total_bins records went in,
// empty_bins of them empty; synch = the range's count of pool photons ('p'), which stay.  Refused when fewer photons are left than there are bins.
struct RebinCounts { int empty_bins, scatt_cyclosynch_num_ph, num_cyclosynch_ph_emit; };
inline ListRefusal rebin_after(long long n, long long n_null, int total_bins, int empty_bins, int synch, RebinCounts *out)
{
    if (n - n_null + (total_bins - empty_bins) < total_bins) return REBIN_FEWER_PHOTONS_THAN_BINS;      // :676-681
    out->empty_bins = empty_bins;
    out->scatt_cyclosynch_num_ph = total_bins - empty_bins;                                             // :689-690
    out->num_cyclosynch_ph_emit = total_bins + synch - empty_bins;
    return LIST_OK;
}

// ------------------------------------------------------------------ injection and emission
struct RadialRange { double rmin, rmax; };
// An injection slab or an emission shell with its angle range (wien: the slab's spectrum, 0 for a shell).  The lists of a pool are grouped by it --
// the cells of a region are found once for all lists that share it: region_group gives the first of groups[0 .. *n) that equals x in every member,
// or appends x (the caller keeps room for one more) and gives the new group.
struct Region { double rmin, rmax, tmin, tmax; int wien; };
inline int region_group(Region *groups, int *n, const Region &x)
{
    for (int k = 0; k < *n; ++k)
        if (groups[k].rmin == x.rmin && groups[k].rmax == x.rmax && groups[k].tmin == x.tmin && groups[k].tmax == x.tmax && groups[k].wien == x.wien) return k;
    groups[*n] = x;
    return (*n)++;
}
// the injection slab: one frame's light travel around r_inj (mclib.c:34-35)
inline RadialRange inject_slab_radii(double r_inj, double fps)
{
    return RadialRange{r_inj - 0.5 * C_LIGHT / fps, r_inj + 0.5 * C_LIGHT / fps};
}
// the photon number density's coefficient, a float in the reference (mclib.c:17,23-32): Wien or black-body spectrum
inline double inject_num_dens_coeff(bool wien) { return wien ? (double)8.44f : (double)20.29f; }
// the emission shell: where the photons injected inj_frame_number have got to by scatt_frame_number (calcCyclosynchRLimits, mc_cyclosynch.c:225-244)
inline RadialRange emit_shell_radii(double r_inj, int scatt_frame_number, int inj_frame_number, double fps)
{
    return RadialRange{r_inj + (C_LIGHT * (scatt_frame_number - inj_frame_number) / fps - 0.5 * C_LIGHT / fps),
                       r_inj + (C_LIGHT * (scatt_frame_number - inj_frame_number) / fps + 0.5 * C_LIGHT / fps)};
}

// One step of the weight search of mclib.c:87-136 and mc_cyclosynch.c:1244-1296: `total` photons were drawn with *weight.  More than max_photons:
// the weight x 10; fewer than min_photons (>= 0): x 0.5; otherwise the weight is accepted (true).  The caller draws again, up to its own limit.
MCRAT_LIST_HD inline bool weight_search_step(unsigned long long total, int min_photons, double max_photons, double *weight)
{
    if ((double)total > max_photons) *weight *= 10;
    else if (total < (unsigned long long)min_photons) *weight *= 0.5;
    else return true;
    return false;
}

// addToPhotonList (photons.c:112-121) when the list of `cap` slots has no null slot for the n_add photons: twice the slots if that is room enough,
// else cap * (n_add / cap) -- the reference's integer division, as it is.
MCRAT_LIST_HD inline long long list_capacity_grown(long long cap, long long n_add)
{
    return (cap * 2 > cap + n_add) ? cap * 2 : cap * (n_add / cap);
}

}  // namespace mcrat
