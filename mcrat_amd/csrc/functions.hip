// functions.hip -- the device functions of physics.hpp evaluated one by one on arrays (mcrat_hip_eval_function): the entry the
// function-level parity tests use (tests/test_gpu_functions.py).  The loop kernels reach these functions only
// along trajectories; here every one of them meets its edge cases directly -- both sides of the Klein-Nishina seam at 1e-3, a fluid at
// rest, gamma = 100, photon directions along the flow or along z, both sides of the 1e7 K switch of the electron sampler,
// unpolarised light -- against the oracle's restatement of the reference function.  Not used by the loop.
// The entries from RCP_NR on evaluate the loop's OWN arithmetic forms (cell_staged_operands, kf_of_gamma, boost_with, optical_depth_staged,
// the Newton reciprocal / reciprocal root, the azimuth selects, hydro_coords, the table look-up) -- each case calls the function the loop
// calls, never a copy of its body -- for tests/test_gpu_loop_arithmetic.py, which compares them with extended precision.
// Two more of physics.hpp's functions on arrays live here, used by the engine itself: exp(x) K_2(x) per hydro cell (k2e_kernel) and the cell
// look-up of given coordinates (lookup_kernel; mcrat_hip_lookup_cell).
#include <hip/hip_runtime.h>
#include "../../include/mcrat_hip.h"
#include "device_types.hpp"
#include "launch.hpp"
#include "physics.hpp"
#include "rng.hpp"

namespace mcrat {

namespace {

// the event stream of item i: what the oracle gets from orc_rng_init(seed, stream); orc_rng_set_iteration(i); orc_rng_event_begin(0)
__device__ __forceinline__ EventStream item_stream(uint64_t seed, uint32_t stream, int i) { return event_stream(seed, (uint64_t)i, 0u, stream); }

__device__ __forceinline__ double k2e_of(double temp)
{
    return temp >= 1e7 ? phys::bessel_k2_scaled((M_EL * C_LIGHT * C_LIGHT) / (K_B * temp)) : 0.0;     // k2e_kernel, below
}

// hydro_coords<DIMS, GEOM> for the context's switches: a run-time switch over the pairs the engine accepts (engine.hip, geometry_supported)
__device__ __forceinline__ void hydro_coords_of(int dims, int geom, double x, double y, double z, double &a0, double &a1, double &a2)
{
    a0 = a1 = a2 = -1;
    const int pair = dims * 4 + geom;
    switch (pair) {
    case DIM_TWO * 4 + GEOM_CARTESIAN: phys::hydro_coords<DIM_TWO, GEOM_CARTESIAN>(x, y, z, a0, a1, a2); break;
    case DIM_TWO * 4 + GEOM_CYLINDRICAL: phys::hydro_coords<DIM_TWO, GEOM_CYLINDRICAL>(x, y, z, a0, a1, a2); break;
    case DIM_TWO * 4 + GEOM_SPHERICAL: phys::hydro_coords<DIM_TWO, GEOM_SPHERICAL>(x, y, z, a0, a1, a2); break;
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CARTESIAN: phys::hydro_coords<DIM_TWO_POINT_FIVE, GEOM_CARTESIAN>(x, y, z, a0, a1, a2); break;
    case DIM_TWO_POINT_FIVE * 4 + GEOM_CYLINDRICAL: phys::hydro_coords<DIM_TWO_POINT_FIVE, GEOM_CYLINDRICAL>(x, y, z, a0, a1, a2); break;
    case DIM_TWO_POINT_FIVE * 4 + GEOM_SPHERICAL: phys::hydro_coords<DIM_TWO_POINT_FIVE, GEOM_SPHERICAL>(x, y, z, a0, a1, a2); break;
    case DIM_THREE * 4 + GEOM_CARTESIAN: phys::hydro_coords<DIM_THREE, GEOM_CARTESIAN>(x, y, z, a0, a1, a2); break;
    case DIM_THREE * 4 + GEOM_SPHERICAL: phys::hydro_coords<DIM_THREE, GEOM_SPHERICAL>(x, y, z, a0, a1, a2); break;
    case DIM_THREE * 4 + GEOM_POLAR: phys::hydro_coords<DIM_THREE, GEOM_POLAR>(x, y, z, a0, a1, a2); break;
    default: break;
    }
}

template <bool STOKES>
__global__ __launch_bounds__(64) void eval_kernel(int fn, int n, const double *__restrict__ in, double *__restrict__ out, uint64_t seed, uint32_t stream,
                                                  HydroDev hy, int dims, int geom)
{
    // one wavefront per item for the wave-wide sampler (all 64 lanes the same item), one lane per item otherwise
    const bool wave_items = fn == MCRAT_HIP_FN_THERMAL_ELECTRON_WAVE;
    const int i = wave_items ? (int)blockIdx.x : (int)(blockIdx.x * 64 + threadIdx.x);
    if (i >= n) return;
    switch (fn) {
    case MCRAT_HIP_FN_KN_CROSS_SECTION:
        out[i] = phys::kn_cross_section(in[i]);
        break;
    case MCRAT_HIP_FN_LORENTZ_BOOST_PHOTON:
    case MCRAT_HIP_FN_LORENTZ_BOOST_ELECTRON: {
        const double *r = in + (size_t)7 * i;
        const double b[3] = {r[0], r[1], r[2]}, p[4] = {r[3], r[4], r[5], r[6]};
        double res[4];
        phys::lorentz_boost(b, p, res, fn == MCRAT_HIP_FN_LORENTZ_BOOST_PHOTON);
        for (int k = 0; k < 4; ++k) out[(size_t)4 * i + k] = res[k];
        break;
    }
    case MCRAT_HIP_FN_STOKES_ROTATION: {
        const double *r = in + (size_t)13 * i;
        const double v[3] = {r[0], r[1], r[2]}, k1[3] = {r[3], r[4], r[5]}, k2[3] = {r[6], r[7], r[8]};
        double s[4] = {r[9], r[10], r[11], r[12]};
        phys::stokes_rotation(v, k1, k2, s);
        for (int k = 0; k < 4; ++k) out[(size_t)4 * i + k] = s[k];
        break;
    }
    case MCRAT_HIP_FN_THERMAL_ELECTRON:
    case MCRAT_HIP_FN_THERMAL_ELECTRON_WAVE: {
        const double *r = in + (size_t)5 * i;
        const double ph[4] = {r[1], r[2], r[3], r[4]};
        EventStream rng = item_stream(seed, stream, i);
        double el[4];
        if (wave_items) phys::single_thermal_electron<true>(el, r[0], k2e_of(r[0]), ph, rng);
        else phys::single_thermal_electron<false>(el, r[0], k2e_of(r[0]), ph, rng);
        if (!wave_items || threadIdx.x == 0)
            for (int k = 0; k < 4; ++k) out[(size_t)4 * i + k] = el[k];
        break;
    }
    case MCRAT_HIP_FN_ELECTRON_AND_SCATTER: {
        const double *r = in + (size_t)9 * i;
        double ph[4] = {r[1], r[2], r[3], r[4]}, s[4] = {r[5], r[6], r[7], r[8]};
        EventStream rng = item_stream(seed, stream, i);
        double el[4];
        phys::single_thermal_electron<false>(el, r[0], k2e_of(r[0]), ph, rng);
        const bool ok = phys::single_scatter<STOKES>(el, ph, s, rng);
        double *o = out + (size_t)13 * i;
        for (int k = 0; k < 4; ++k) { o[k] = el[k]; o[4 + k] = ph[k]; o[8 + k] = s[k]; }
        o[12] = ok ? 1.0 : 0.0;
        break;
    }
    case MCRAT_HIP_FN_RCP_NR:
        out[i] = phys::rcp_nr(in[i]);
        break;
    case MCRAT_HIP_FN_RSQRT_NR:
        out[i] = phys::rsqrt_nr(in[i]);
        break;
    case MCRAT_HIP_FN_SQRT_NR:
        out[i] = phys::sqrt_nr(in[i]);
        break;
    case MCRAT_HIP_FN_CELL_OPERANDS: {
        const double *r = in + (size_t)5 * i;
        CellFluid f;
        cell_staged_operands(r[0], r[1], r[2], r[3], r[4], f);                       // as stage_cells_kernel (ingest.hip) calls it
        double *o = out + (size_t)5 * i;
        o[0] = f.w; o[1] = f.nsig; o[2] = f.gam; o[3] = f.kf; o[4] = phys::kf_of_gamma(f.gam);
        break;
    }
    case MCRAT_HIP_FN_BOOST_WITH_PHOTON:
    case MCRAT_HIP_FN_BOOST_WITH_ELECTRON: {
        const double *r = in + (size_t)9 * i;
        const double b[3] = {r[0], r[1], r[2]}, p[4] = {r[5], r[6], r[7], r[8]};
        double res[4];
        if (fn == MCRAT_HIP_FN_BOOST_WITH_PHOTON) phys::boost_with<true>(b, r[3], r[4], p, res);
        else phys::boost_with<false>(b, r[3], r[4], p, res);
        for (int k = 0; k < 4; ++k) out[(size_t)4 * i + k] = res[k];
        break;
    }
    case MCRAT_HIP_FN_BOOST_STAGED_PHOTON: {                                         // slow_one's re-location (kernels.hip): gam of the staged record, kf recomputed
        const double *r = in + (size_t)7 * i;
        const double b[3] = {r[0], r[1], r[2]}, p[4] = {r[3], r[4], r[5], r[6]};
        CellFluid f;
        cell_staged_operands(b[0], b[1], b[2], 1.0, 1.0, f);
        double res[4];
        phys::boost_with<true>(b, f.gam, phys::kf_of_gamma(f.gam), p, res);
        for (int k = 0; k < 4; ++k) out[(size_t)4 * i + k] = res[k];
        break;
    }
    case MCRAT_HIP_FN_OPTICAL_DEPTH_STAGED: {
        const double *r = in + (size_t)9 * i;
        const double b[3] = {r[0], r[1], r[2]};
        CellFluid f;
        cell_staged_operands(b[0], b[1], b[2], r[3], r[4], f);
        const double tau = phys::optical_depth_staged(b, f.w, f.nsig, r[5], r[6], r[7], r[8]);
        out[(size_t)2 * i] = tau;
        out[(size_t)2 * i + 1] = -phys::rcp_nr(tau);
        break;
    }
    case MCRAT_HIP_FN_AZIMUTH: {
        const double x = in[(size_t)2 * i], y = in[(size_t)2 * i + 1];
        double a0, a1, a2;
        phys::hydro_coords<DIM_TWO, GEOM_CYLINDRICAL>(x, y, 0.0, a0, a1, a2);     // a0 = sqrt(x*x + y*y): the hypotenuse relocation_azimuth hands over
        double *o = out + (size_t)4 * i;
        phys::cos_sin_of_atan2(y, x, o[0], o[1]);
        phys::cos_sin_with_hypot(y, x, a0, o[2], o[3]);
        break;
    }
    case MCRAT_HIP_FN_HYDRO_COORDS: {
        const double *r = in + (size_t)3 * i;
        double *o = out + (size_t)3 * i;
        hydro_coords_of(dims, geom, r[0], r[1], r[2], o[0], o[1], o[2]);
        break;
    }
    case MCRAT_HIP_FN_THERMAL_CROSS_SECTION: {
        double norm = 1.0, eps = 0.0, theta = 0.0;
        const bool fallback = phys::thermal_cross_section_lookup(hy, in[(size_t)2 * i], in[(size_t)2 * i + 1], norm, eps, theta);
        double *o = out + (size_t)4 * i;
        o[0] = norm; o[1] = fallback ? 1.0 : 0.0; o[2] = fallback ? eps : 0.0; o[3] = fallback ? theta : 0.0;
        break;
    }
    case MCRAT_HIP_FN_KN_CROSS_SECTION_IEEE:
        out[i] = phys::kn_cross_section_ieee(in[i]);
        break;
    default:
        break;
    }
}

// ------------------------------------------------------------------ per-cell exp(x) K_2(x)
__global__ void k2e_kernel(const double *__restrict__ temp, double *__restrict__ k2e, int M)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M) return;
    const double T = temp[c];
    double v = 0.0;
    if (T >= 1e7) v = phys::bessel_k2_scaled((M_EL * C_LIGHT * C_LIGHT) / (K_B * T));
    k2e[c] = v;
}

// ------------------------------------------------------------------ cell lookup (A/B of findContainingBlock)
template <int DIMS>
__global__ void lookup_kernel(HydroDev hy, int n, const double *a0, const double *a1, const double *a2, int *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = phys::find_containing_block<DIMS>(hy, a0[i], a1[i], (DIMS == DIM_THREE) ? a2[i] : 0.0);
}

}  // namespace

hipError_t launch_k2e(const double *temp, double *k2e, int M, hipStream_t stream)
{
    hipLaunchKernelGGL(k2e_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, temp, k2e, M);
    return hipGetLastError();
}

hipError_t launch_lookup(const KernelConfig &kc, const HydroDev &hy, int n, const double *a0, const double *a1,
                         const double *a2, int *out, hipStream_t stream)
{
    const int blocks = (n + 255) / 256;
    if (kc.dimensions == DIM_THREE)
        hipLaunchKernelGGL((lookup_kernel<DIM_THREE>), dim3(blocks), dim3(256), 0, stream, hy, n, a0, a1, a2, out);
    else
        hipLaunchKernelGGL((lookup_kernel<DIM_TWO>), dim3(blocks), dim3(256), 0, stream, hy, n, a0, a1, a2, out);
    return hipGetLastError();
}

hipError_t launch_eval_function(const KernelConfig &kc, const HydroDev &hy, int fn, int n, const double *in, double *out, uint64_t seed, uint32_t stream_id,
                                hipStream_t stream)
{
    const int blocks = (fn == MCRAT_HIP_FN_THERMAL_ELECTRON_WAVE) ? n : (n + 63) / 64;
    if (kc.stokes) eval_kernel<true><<<dim3(blocks), dim3(64), 0, stream>>>(fn, n, in, out, seed, stream_id, hy, kc.dimensions, kc.geometry);
    else eval_kernel<false><<<dim3(blocks), dim3(64), 0, stream>>>(fn, n, in, out, seed, stream_id, hy, kc.dimensions, kc.geometry);
    return hipGetLastError();
}

}  // namespace mcrat
