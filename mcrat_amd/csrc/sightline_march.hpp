// sightline_march.hpp -- one step of a sightline's march, device code, written once: sightline_kernel (sightline.hip) and escape_march_kernel
// (escape.hip) call it and nothing else does.  The per-ray rules -- step length, midpoint, advance -- are sightline_plan.hpp's, the cell look-up
// and the optical depth are the loop's own (physics.hpp).  A step is two dependent gathers -- the bucket's record (16 B), then one bucket-list
// entry (128 B), which holds everything the step needs from the cell (TABLE adds the cell's temperature) -- and some forty f64 operations between
// them.  Both callers get the same tau, path and positions bit for bit: the expressions and their order are these, whoever calls.
#pragma once
#include <hip/hip_runtime.h>
#include "device_types.hpp"
#include "physics.hpp"
#include "sightline_plan.hpp"

namespace mcrat {

// The step from (x, y, z) along (nx, ny, nz) for the photon momentum p: the midpoint, its hydro coordinates, the domain test, the bucket look-up,
// the azimuth, beta, (TABLE) the cross-section look-up, kappa, and the adds to tau, path and the position.
// -> -1: the step was counted (the caller adds 1 to its k and asks for tau_stop); SIGHTLINE_LEFT_MESH, SIGHTLINE_OFF_TABLE: the march ends before
// this step, nothing was added.
template <int DIMS, int GEOM, bool TABLE>
__device__ __forceinline__ int sightline_step(const HydroDev &hy, const double (&p)[4], double step_frac, double h_min, double nx, double ny, double nz,
                                              double &x, double &y, double &z, double &tau, double &path)
{
    const double h = sightline_step_length(x, y, z, step_frac, h_min);
    double mx, my, mz, a0, a1, a2;
    sightline_midpoint(x, y, z, h, nx, ny, nz, mx, my, mz);
    phys::hydro_coords<DIMS, GEOM>(mx, my, mz, a0, a1, a2);
    FatCell hit;
    hit.cell = -1;
    if (phys::in_domain<DIMS>(hy, a0, a1, a2))
        phys::find_in_bucket<DIMS>(hy, phys::grid_bucket_of<DIMS>(hy.grid, a0, a1, a2), a0, a1, a2, hit);
    if (hit.cell < 0) return SIGHTLINE_LEFT_MESH;
    double cphi, sphi, beta[3], norm = 1.0;
    phys::relocation_azimuth<DIMS, GEOM>(mx, my, a0, cphi, sphi);
    phys::beta_from_record<DIMS>(hit.a, hit.b, hit.c, cphi, sphi, beta);
    bool off_table = false;
    if constexpr (TABLE) {
        double comv[4], eps, theta;
        phys::boost_with<false>(beta, hit.gam, phys::kf_of_gamma(hit.gam), p, comv);
        off_table = phys::thermal_cross_section_lookup(hy, comv[0], hy.temp[hit.cell], norm, eps, theta);
    }
    if (off_table) return SIGHTLINE_OFF_TABLE;
    const double kappa = phys::optical_depth_staged(beta, hit.w, hit.nsig, p[1], p[2], p[3], norm);
    tau += kappa * h;
    path += h;
    sightline_advance(x, y, z, h, nx, ny, nz);
    return -1;
}

}  // namespace mcrat
