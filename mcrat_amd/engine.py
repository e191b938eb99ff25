"""ctypes binding of libmcrat_hip.so (include/mcrat_hip.h) -- the product path.

There is no CPU fallback here: if the shared library is missing or no MI355X is
visible, construction raises.  Nothing under oracle/ is imported by this package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmcrat_hip.so")

ABI_VERSION = 1
CARTESIAN, SPHERICAL, CYLINDRICAL, POLAR = 0, 1, 2, 3
TWO, TWO_POINT_FIVE, THREE = 0, 1, 2
TAU_DIRECT = 1
TAU_TABLE = 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

# struct photon of Src/mcrat.h:142-171 (thermal-only build), 176 bytes
PHOTON_DTYPE = np.dtype(
    [("type", "S1"),
     ("p0", "f8"), ("p1", "f8"), ("p2", "f8"), ("p3", "f8"),
     ("comv_p0", "f8"), ("comv_p1", "f8"), ("comv_p2", "f8"), ("comv_p3", "f8"),
     ("r0", "f8"), ("r1", "f8"), ("r2", "f8"),
     ("s0", "f8"), ("s1", "f8"), ("s2", "f8"), ("s3", "f8"),
     ("num_scatt", "f8"),
     ("recalc_properties", "i4"),
     ("weight", "f8"),
     ("nearest_block_index", "i4"),
     ("time_to_scatter", "f8"),
     ("total_optical_depth", "f8")],
    align=True,
)
assert PHOTON_DTYPE.itemsize == 176

F8_COLUMNS = ("p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3", "r0", "r1", "r2",
              "s0", "s1", "s2", "s3", "num_scatt", "weight", "time_to_scatter", "total_optical_depth")


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int), ("dimensions", C.c_int), ("geometry", C.c_int),
                ("stokes_switch", C.c_int), ("tau_calculation", C.c_int), ("cyclosynchrotron_switch", C.c_int),
                ("device", C.c_int), ("stream", C.c_void_p), ("rng_stream", C.c_uint32),
                ("iterations_per_sync", C.c_int), ("use_graph", C.c_int), ("profile", C.c_int),
                ("virtual_rank_photons", C.c_int)]


class PhotonList(C.Structure):
    _fields_ = [("photons", C.c_void_p), ("sorted_indexes", _ip),
                ("num_photons", C.c_int), ("num_null_photons", C.c_int), ("list_capacity", C.c_int)]


class PhotonSoA(C.Structure):
    _fields_ = [("n", C.c_int), ("type", C.c_char_p),
                ("p0", _dp), ("p1", _dp), ("p2", _dp), ("p3", _dp),
                ("comv_p0", _dp), ("comv_p1", _dp), ("comv_p2", _dp), ("comv_p3", _dp),
                ("r0", _dp), ("r1", _dp), ("r2", _dp),
                ("s0", _dp), ("s1", _dp), ("s2", _dp), ("s3", _dp),
                ("num_scatt", _dp), ("recalc_properties", _ip), ("weight", _dp),
                ("nearest_block_index", _ip), ("time_to_scatter", _dp), ("total_optical_depth", _dp)]


class Hydro(C.Structure):
    _fields_ = [("num_elements", C.c_int),
                ("r0", _dp), ("r1", _dp), ("r2", _dp),
                ("r0_size", _dp), ("r1_size", _dp), ("r2_size", _dp),
                ("v0", _dp), ("v1", _dp), ("v2", _dp),
                ("dens_lab", _dp), ("temp", _dp), ("gamma", _dp),
                ("r0_domain", C.c_double * 2), ("r1_domain", C.c_double * 2), ("r2_domain", C.c_double * 2),
                ("fps", C.c_double)]


class FrameStats(C.Structure):
    _fields_ = [("iterations", C.c_longlong), ("photon_steps", C.c_longlong), ("frame_scatt_cnt", C.c_longlong),
                ("num_photons_find_new_element", C.c_longlong), ("not_found", C.c_longlong),
                ("kn_rejections", C.c_longlong), ("rescans", C.c_longlong),
                ("last_scattered_index", C.c_int), ("last_scattered_temp", C.c_double),
                ("last_time_step", C.c_double), ("remaining_time", C.c_double), ("time_now", C.c_double),
                ("step_kernel_ms", C.c_double), ("step_kernel_launches", C.c_longlong), ("event_kernel_ms", C.c_double),
                ("table_fallbacks", C.c_longlong), ("slot_steps", C.c_longlong)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FramePlan(C.Structure):
    """mcrat_hip_frame_plan: several hydro frames of every list of a pool in one launch (the frame queue)"""
    _fields_ = [("n_frames", C.c_int), ("chain_clock", C.c_int), ("restore_each_frame", C.c_int), ("capture_frames", C.c_int),
                ("open", C.POINTER(C.c_int)), ("seeds", C.POINTER(C.c_uint64)), ("time_now", _dp), ("remaining_time", _dp), ("frame_end", _dp),
                ("hydro", C.POINTER(C.c_void_p))]


class Slab(C.Structure):
    """mcrat_hip_slab: the selecting arguments of getHydroData (mcrat_io.h:26) + fps and the hydro domains"""
    _fields_ = [("r_inj", C.c_double), ("ph_inj_switch", C.c_int), ("min_r", C.c_double), ("max_r", C.c_double),
                ("min_theta", C.c_double), ("max_theta", C.c_double), ("fps", C.c_double),
                ("r0_domain", C.c_double * 2), ("r1_domain", C.c_double * 2), ("r2_domain", C.c_double * 2)]


class FlashBlocks(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("coord_stride", C.c_int), ("bsize_stride", C.c_int),
                ("coordinates", _dp), ("block_size", _dp), ("node_type", _ip),
                ("velx", _dp), ("vely", _dp), ("dens", _dp), ("pres", _dp),
                ("l_scale", C.c_double), ("d_scale", C.c_double), ("p_scale", C.c_double)]


class PlutoGrid(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int)] + \
               [(f, _dp) for f in ("x1", "dx1", "x2", "dx2", "x3", "dx3", "rho", "vx1", "vx2", "vx3", "prs")] + \
               [("l_scale", C.c_double), ("d_scale", C.c_double), ("p_scale", C.c_double)]


class ChomboLevel(C.Structure):
    _fields_ = [("n_boxes", C.c_int), ("boxes", _ip), ("box_offsets", _ip), ("data_len", C.c_longlong),
                ("prob_domain", C.c_int * 6), ("ref_ratio", C.c_int), ("logr", C.c_int),
                ("dx", C.c_double), ("dombeg1", C.c_double), ("dombeg2", C.c_double), ("dombeg3", C.c_double),
                ("g_x2stretch", C.c_double), ("g_x3stretch", C.c_double)]


class Chombo(C.Structure):
    _fields_ = [("num_levels", C.c_int), ("num_vars", C.c_int), ("levels", C.POINTER(ChomboLevel)), ("var_names", C.POINTER(C.c_char_p)),
                ("data", _dp), ("l_scale", C.c_double), ("d_scale", C.c_double), ("p_scale", C.c_double)]


class Cyclosynch(C.Structure):
    """mcrat_hip_cyclosynch: B_FIELD_CALC (0 INTERNAL_E, 1 TOTAL_E, 2 SIMULATION), EPSILON_B and the rebinning / frame fields"""
    _fields_ = [("b_field_calc", C.c_int), ("epsilon_b", C.c_double), ("rebin_e_perc", C.c_double), ("rebin_ang", C.c_double),
                ("rebin_ang_phi", C.c_double), ("scatt_frame_number", C.c_int), ("inj_frame_number", C.c_int)]


class CyclosynchCounts(C.Structure):
    """mcrat_hip_cyclosynch_counts: the counters of mcrat.c:735-878 for one scatter frame"""
    _fields_ = [("num_cyclosynch_ph_emit", C.c_int), ("scatt_cyclosynch_num_ph", C.c_int), ("frame_abs_cnt", C.c_int), ("rebins", C.c_int),
                ("integrals_not_converged", C.c_int), ("pad", C.c_int), ("n_comptonized", C.c_double), ("pool_weight", C.c_double)]


class Outflow(C.Structure):
    _fields_ = [("simulation_type", C.c_int), ("gamma_infinity", C.c_double), ("lumi", C.c_double), ("r00", C.c_double),
                ("t_comov", C.c_double), ("ddensity", C.c_double), ("theta_j", C.c_double), ("p", C.c_double)]


class IngestResult(C.Structure):
    _fields_ = [("num_elements", C.c_int), ("elem_factor", C.c_int), ("cells_read", C.c_longlong)]


HYDRO_COLUMNS = ("r0", "r1", "r2", "r0_size", "r1_size", "r2_size", "v0", "v1", "v2", "dens", "dens_lab", "pres", "temp", "gamma", "r", "theta")


class HydroColumns(C.Structure):
    _fields_ = [("num_elements", C.c_int)] + [(f, _dp) for f in HYDRO_COLUMNS]


OUTPUT_COLUMNS = ("p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3", "r0", "r1", "r2", "s0", "s1", "s2", "s3", "num_scatt", "weight")


class OutputColumns(C.Structure):
    _fields_ = [("count", C.c_int)] + [(f, _dp) for f in OUTPUT_COLUMNS] + [("type", C.c_char_p)]


class PoolInjectList(C.Structure):
    """mcrat_hip_pool_inject_list"""
    _fields_ = [("inject", C.c_int), ("spect", C.c_char), ("min_photons", C.c_int), ("max_photons", C.c_int),
                ("r_inj", C.c_double), ("ph_weight", C.c_double), ("theta_min", C.c_double), ("theta_max", C.c_double),
                ("seed", C.c_uint64), ("num_photons", C.c_int), ("ph_weight_adjusted", C.c_double), ("status", C.c_int)]


class RankSummary(C.Structure):
    """mcrat_hip_rank_summary: the per-frame reductions and printPhotons' count of one list of a rank pool"""
    _fields_ = [("min_r", C.c_double), ("max_r", C.c_double), ("min_theta", C.c_double), ("max_theta", C.c_double),
                ("avg_scatt", C.c_double), ("avg_r", C.c_double), ("avg_energy", C.c_double),
                ("max_scatt", C.c_int), ("min_scatt", C.c_int), ("num_output", C.c_int), ("list_capacity", C.c_int)]


class PoolCsList(C.Structure):
    """mcrat_hip_pool_cs_list: one list's arguments of a cyclo-synchrotron scatter frame of a rank pool"""
    _fields_ = [("open", C.c_int), ("emit_pool", C.c_int), ("scatt_frame_number", C.c_int), ("inj_frame_number", C.c_int), ("seed", C.c_uint64),
                ("time_now", C.c_double), ("remaining_time", C.c_double), ("r_inj", C.c_double), ("ph_weight_suggest", C.c_double),
                ("theta_min", C.c_double), ("theta_max", C.c_double)]


class Observer(C.Structure):
    """mcrat_hip_observer: the observers' directions and cones and the bin edges of a mock observation"""
    _fields_ = [("n_obs", C.c_int), ("cos_obs", _dp), ("sin_obs", _dp), ("cos_lo", _dp), ("cos_hi", _dp),
                ("n_t", C.c_int), ("t_edges", _dp), ("n_e", C.c_int), ("e_edges", _dp)]


class Observation(C.Structure):
    """mcrat_hip_observation: the cube's planes, each [n_obs * n_t * n_e], and the per-observer counters"""
    _fields_ = [("count", C.POINTER(C.c_longlong)), ("w", _dp), ("we", _dp), ("i", _dp), ("q", _dp), ("u", _dp), ("v", _dp),
                ("n_accepted", C.POINTER(C.c_longlong)), ("n_outside", C.POINTER(C.c_longlong))]


OBSERVE_PATH_LDS, OBSERVE_PATH_GLOBAL = 1, 2      # mcrat_hip_observe_path


class SkyObserver(C.Structure):
    """mcrat_hip_sky_observer: the observers' directions, cones and sky-plane vectors and the bin edges of a sky observation"""
    _fields_ = [("n_obs", C.c_int), ("n0", _dp), ("n1", _dp), ("n2", _dp), ("cos_acc", _dp),
                ("x0", _dp), ("x1", _dp), ("x2", _dp), ("y0", _dp), ("y1", _dp), ("y2", _dp),
                ("n_t", C.c_int), ("t_edges", _dp), ("n_e", C.c_int), ("e_edges", _dp),
                ("n_x", C.c_int), ("x_edges", _dp), ("n_y", C.c_int), ("y_edges", _dp)]


class SkyObservation(C.Structure):
    """mcrat_hip_sky_observation: the cube's planes, each [n_obs * n_t * n_e * n_y * n_x], and the per-observer counters"""
    _fields_ = [("count", C.POINTER(C.c_longlong)), ("w", _dp), ("we", _dp), ("i", _dp), ("q", _dp), ("u", _dp), ("v", _dp),
                ("n_accepted", C.POINTER(C.c_longlong)), ("n_outside", C.POINTER(C.c_longlong))]


SKY_PATH_LDS, SKY_PATH_GLOBAL = 1, 2              # mcrat_hip_observe_sky_path


class SightlineParams(C.Structure):
    """mcrat_hip_sightline_params: how a sightline is stepped and where it stops"""
    _fields_ = [("step_frac", C.c_double), ("h_min", C.c_double), ("max_steps", C.c_int), ("tau_stop", C.c_double), ("surface_level", C.c_double)]


class Sightlines(C.Structure):
    """mcrat_hip_sightlines: the per-ray outputs, each [n], and the rays per status"""
    _fields_ = [("tau", _dp), ("path", _dp), ("steps", _ip), ("status", _ip), ("surface_step", _ip),
                ("surface_r0", _dp), ("surface_r1", _dp), ("surface_r2", _dp), ("n_status", C.c_longlong * 5)]


# a sightline's status (mcrat_hip_sightlines.status)
SIGHTLINE_SKIPPED, SIGHTLINE_LEFT_MESH, SIGHTLINE_OPAQUE, SIGHTLINE_STEP_CAP, SIGHTLINE_OFF_TABLE = 0, 1, 2, 3, 4


class EscapeObserver(C.Structure):
    """mcrat_hip_escape_observer: a sky observation's inputs, the optical-depth edges and how the accepted photons are marched"""
    _fields_ = [("sky", SkyObserver), ("n_tau", C.c_int), ("tau_edges", _dp), ("march", SightlineParams)]


ESCAPE_SUMS = ("w", "we", "i", "q", "u", "v", "wx", "wex")
ESCAPE_COUNTERS = ("n_accepted", "n_outside", "n_opaque", "n_unresolved")


class EscapeObservation(C.Structure):
    """mcrat_hip_escape_observation: the cube's nine planes, each [n_obs * n_tau * n_t * n_e * n_y * n_x], the per-observer counters and the
    call's counters"""
    _fields_ = ([("count", C.POINTER(C.c_longlong))] + [(k, _dp) for k in ESCAPE_SUMS] + [(k, C.POINTER(C.c_longlong)) for k in ESCAPE_COUNTERS] +
                [("n_observable", C.c_longlong), ("n_selected", C.c_longlong), ("n_status", C.c_longlong * 5)])


ESCAPE_PATH_LDS, ESCAPE_PATH_GLOBAL = 1, 2        # mcrat_hip_observe_escaping_path


def escape_fraction(res):
    """WX / W of an escape-weighted observation: the share of each bin's signal that is already streaming out; 0 / 0 -> NaN"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(res["w"] != 0, res["wx"] / res["w"], np.nan)


class ResampleObserver(C.Structure):
    """mcrat_hip_resample_observer: a sky observation's inputs, the resampling mode with its replicas and seed, and the Stokes frame"""
    _fields_ = [("sky", SkyObserver), ("mode", C.c_int), ("n_rep", C.c_int), ("stokes_frame", C.c_int), ("seed", C.c_uint64)]


RESAMPLE_COUNTERS = ("n_accepted", "n_outside", "n_frame_undefined")


class ResampleObservation(C.Structure):
    """mcrat_hip_resample_observation: the cube's seven planes, each [n_obs * n_rep * n_t * n_e * n_y * n_x], and the per-observer counters"""
    _fields_ = ([("count", C.POINTER(C.c_longlong))] + [(k, _dp) for k in ("w", "we", "i", "q", "u", "v")] +
                [(k, C.POINTER(C.c_longlong)) for k in RESAMPLE_COUNTERS])


RESAMPLE_NONE, RESAMPLE_JACKKNIFE, RESAMPLE_BOOTSTRAP = 0, 1, 2       # mcrat_hip_resample_observer.mode
STOKES_AS_STORED, STOKES_SKY_PLANE = 0, 1                             # mcrat_hip_resample_observer.stokes_frame
RESAMPLE_PATH_LDS, RESAMPLE_PATH_GLOBAL, RESAMPLE_PATH_SLICED = 1, 2, 3      # mcrat_hip_observe_sky_resampled_path


class EventsObserver(C.Structure):
    """mcrat_hip_events_observer: the observers' directions, cones and optional sky-plane vectors, the window, the order, the Stokes frame and the
    rows there is room for"""
    _fields_ = [("n_obs", C.c_int), ("n0", _dp), ("n1", _dp), ("n2", _dp), ("cos_acc", _dp),
                ("x0", _dp), ("x1", _dp), ("x2", _dp), ("y0", _dp), ("y1", _dp), ("y2", _dp),
                ("t_lo", C.c_double), ("t_hi", C.c_double), ("e_lo", C.c_double), ("e_hi", C.c_double),
                ("order", C.c_int), ("stokes_frame", C.c_int), ("capacity", C.c_longlong)]


EVENTS_F8_COLUMNS = ("t", "e", "w", "s0", "s1", "s2", "s3", "X", "Y", "num_scatt")
EVENTS_COUNTERS = ("n_events", "n_accepted", "n_outside", "n_frame_undefined")


class Events(C.Structure):
    """mcrat_hip_events: the row columns, each [capacity], offsets [n_obs + 1], the per-observer counters and the call's figures"""
    _fields_ = ([("rank", _ip), ("slot", _ip)] + [(k, _dp) for k in EVENTS_F8_COLUMNS] + [("type", C.c_char_p), ("offsets", C.POINTER(C.c_longlong))] +
                [(k, C.POINTER(C.c_longlong)) for k in EVENTS_COUNTERS] +
                [("n_total", C.c_longlong), ("key_or", C.c_ulonglong), ("key_and", C.c_ulonglong), ("sort_passes_run", C.c_int), ("sort_passes_skipped", C.c_int)])


EVENTS_BY_PHOTON, EVENTS_BY_TIME = 0, 1                               # mcrat_hip_events_observer.order


def bin_events(res, t_edges, e_edges, x_edges=None, y_edges=None):
    """An event list (Engine.observe_events) binned on the host -> dict with the seven planes count, w, we, i, q, u, v, each (n_obs, n_t, n_e) or with
    x_edges and y_edges (n_obs, n_t, n_e, n_y, n_x), and n_outside (n_obs,), as Engine.observe_sky gives them: bin k of an axis holds
    edges[k] <= x < edges[k + 1]; n_outside counts the accepted pairs in no bin -- those outside the list's window and the rows outside an axis."""
    def find(edges, x):
        edges = np.asarray(edges, dtype=np.float64)
        k = np.searchsorted(edges, x, side="right") - 1
        return np.where((k >= 0) & (k < len(edges) - 1) & (x == x), k, -1), len(edges) - 1
    image = x_edges is not None
    if image != (y_edges is not None):
        raise ValueError("bin_events: x_edges and y_edges come together")
    if image and "X" not in res:
        raise ValueError("bin_events: the list has no X and Y columns (observe_events without ex and ey)")
    offsets = np.asarray(res["offsets"])
    n_obs, n = len(offsets) - 1, int(offsets[-1])
    (it, n_t), (ie, n_e) = find(t_edges, res["t"][:n]), find(e_edges, res["e"][:n])
    (ix, n_x), (iy, n_y) = (find(x_edges, res["X"][:n]), find(y_edges, res["Y"][:n])) if image else ((np.zeros(n, dtype=np.int64), 1), (np.zeros(n, dtype=np.int64), 1))
    o = np.repeat(np.arange(n_obs), np.diff(offsets))
    inside = (it >= 0) & (ie >= 0) & (ix >= 0) & (iy >= 0)
    per_obs = n_t * n_e * n_y * n_x
    flat = (o * per_obs + ((it * n_e + ie) * n_y + iy) * n_x + ix)[inside]
    shape = (n_obs, n_t, n_e, n_y, n_x) if image else (n_obs, n_t, n_e)
    w = np.asarray(res["w"][:n], dtype=np.float64)
    out = {"count": np.bincount(flat, minlength=n_obs * per_obs).astype(np.int64).reshape(shape)}
    for k, term in (("w", w), ("we", w * res["e"][:n]), ("i", w * res["s0"][:n]), ("q", w * res["s1"][:n]), ("u", w * res["s2"][:n]), ("v", w * res["s3"][:n])):
        out[k] = np.bincount(flat, weights=term[inside], minlength=n_obs * per_obs).reshape(shape)
    out["n_outside"] = np.asarray(res["n_outside"], dtype=np.int64) + np.bincount(o[~inside], minlength=n_obs).astype(np.int64)
    return out


def event_durations(res, fractions=(0.05, 0.95), weight="we"):
    """Per observer of an event list the detection times at which the cumulative weight reaches the given fractions of its total -- T90 is the
    difference of the pair for (0.05, 0.95), T50 that for (0.25, 0.75).  weight: "we" the fluence w * e, "w" the photon number, "count" the rows.
    The rows are taken in the order of (t, row); the time for fraction f is that of the first row at which the running sum is >= f * total.
    -> a list with one array (len(fractions),) per observer, None for an observer without events."""
    if weight not in ("we", "w", "count"):
        raise ValueError("event_durations: weight takes we, w and count, not %r" % (weight,))
    offsets = np.asarray(res["offsets"])
    out = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        if b == a:
            out.append(None)
            continue
        t = np.asarray(res["t"][a:b], dtype=np.float64)
        order = np.argsort(t, kind="stable")
        term = np.ones(b - a) if weight == "count" else np.asarray(res["w"][a:b], dtype=np.float64) * (res["e"][a:b] if weight == "we" else 1.0)
        run = np.cumsum(term[order])
        first = np.minimum(np.searchsorted(run, np.asarray(fractions, dtype=np.float64) * run[-1], side="left"), b - a - 1)
        out.append(t[order][first])
    return out


def _wrap_half_pi(d):
    """an angle difference into (-pi/2, pi/2]: polarisation angles are defined modulo pi"""
    return d - np.pi * np.ceil((d - 0.5 * np.pi) / np.pi)


def resampled_estimates(res, mode, reduce=(), percentiles=None):
    """Estimates with errors from the cube of Engine.observe_sky_resampled.  res: its dict, arrays (n_obs, n_rep, n_t, n_e[, n_y, n_x]); mode: the
    mode it was made with; reduce: the axes summed first, any of "time" (spectra), "energy" (light curves) and "pixels".
    -> dict with w, we, e_mean = WE / W, pi = sqrt(Q^2 + U^2) / I and angle = atan2(U, Q) / 2, each a dict of value and stderr over
    (n_obs, the axes that are left); a bin without photons gives NaN.
    RESAMPLE_JACKKNIFE: entry g holds group g's own sums x_g.  With T = sum_g x_g the estimate is f(T), replicate g is f((T - x_g) G / (G - 1)) --
    the rescale makes totals unbiased when the number of photons is itself Poisson; it cancels in ratios -- and
    var = (G - 1) / G sum_g (theta_g - mean theta)^2.
    RESAMPLE_BOOTSTRAP: the estimate is f(entry 0), stderr the sample standard deviation (ddof = 1) of f over entries 1 .. B; percentiles = (lo, hi)
    in per cent adds the bounds lo and hi of f over those entries.
    RESAMPLE_NONE: the estimates alone, stderr NaN.
    The angle's differences are wrapped into (-pi/2, pi/2] about the estimate before they are averaged."""
    axes = {"time": (2,), "energy": (3,), "pixels": (4, 5)}
    names = (reduce,) if isinstance(reduce, str) else tuple(reduce)
    for k in names:
        if k not in axes:
            raise ValueError("resampled_estimates: reduce takes time, energy and pixels, not %r" % (k,))
    ndim = res["count"].ndim
    over = tuple(sorted(a for k in set(names) for a in axes[k] if a < ndim))
    x = {k: np.asarray(res[k], dtype=np.float64).sum(axis=over) for k in ("w", "we", "i", "q", "u")}      # (n_obs, n_rep, ...)
    count = np.asarray(res["count"]).sum(axis=over)
    n_rep = count.shape[1]

    def stats(s):
        with np.errstate(invalid="ignore", divide="ignore"):
            return {"w": s["w"], "we": s["we"], "e_mean": s["we"] / s["w"], "pi": np.sqrt(s["q"] * s["q"] + s["u"] * s["u"]) / s["i"],
                    "angle": 0.5 * np.arctan2(s["u"], s["q"])}

    if mode == RESAMPLE_JACKKNIFE:
        if n_rep < 2:
            raise ValueError("resampled_estimates: a jackknife needs at least two groups")
        total = {k: v.sum(axis=1) for k, v in x.items()}
        filled = count.sum(axis=1) > 0
        value = stats(total)
        scale = n_rep / (n_rep - 1.0)
        reps = stats({k: (total[k][:, None] - v) * scale for k, v in x.items()})
    elif mode == RESAMPLE_BOOTSTRAP:
        if n_rep < 3:
            raise ValueError("resampled_estimates: a bootstrap error needs at least two replicas beside the sample")
        filled = count[:, 0] > 0
        value = stats({k: v[:, 0] for k, v in x.items()})
        reps = stats({k: v[:, 1:] for k, v in x.items()})
    elif mode == RESAMPLE_NONE:
        filled = count[:, 0] > 0
        value = stats({k: v[:, 0] for k, v in x.items()})
        reps = None
    else:
        raise ValueError("resampled_estimates: mode must be RESAMPLE_NONE, RESAMPLE_JACKKNIFE or RESAMPLE_BOOTSTRAP")
    out = {}
    for k, val in value.items():
        val = np.where(filled, val, np.nan)
        est = {"value": val, "stderr": np.full(val.shape, np.nan)}
        if reps is not None:
            with np.errstate(invalid="ignore"):
                dev = reps[k] - val[:, None]
                if k == "angle":
                    dev = _wrap_half_pi(dev)
                if mode == RESAMPLE_JACKKNIFE:
                    var = (n_rep - 1.0) / n_rep * ((dev - dev.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
                else:
                    var = dev.var(axis=1, ddof=1)
                    if percentiles is not None:
                        lo, hi = np.percentile(dev, list(percentiles), axis=1)
                        est["lo"], est["hi"] = np.where(filled, val + lo, np.nan), np.where(filled, val + hi, np.nan)
                est["stderr"] = np.where(filled, np.sqrt(var), np.nan)
        out[k] = est
    return out


class FitArgs(C.Structure):
    """mcrat_hip_fit_args: the spectra (count, w), the edges and log_e, the pivot, the bounds, the coarse grid, the rounds, shrink and min_count"""
    _fields_ = [("model", C.c_int), ("n_spec", C.c_longlong), ("n_e", C.c_int), ("count", C.POINTER(C.c_longlong)), ("w", _dp), ("e_edges", _dp), ("log_e", _dp),
                ("e_piv", C.c_double), ("alpha_lo", C.c_double), ("alpha_hi", C.c_double), ("lambda_lo", C.c_double), ("lambda_hi", C.c_double),
                ("beta_lo", C.c_double), ("beta_hi", C.c_double), ("g_alpha", C.c_int), ("g_lambda", C.c_int), ("g_beta", C.c_int), ("n_rounds", C.c_int),
                ("shrink", C.c_double), ("min_count", C.c_longlong)]


FIT_F8_COLUMNS = ("alpha", "beta", "e_peak", "amplitude", "chi2")
FIT_I4_COLUMNS = ("n_used", "dof", "status")


class FitResult(C.Structure):
    """mcrat_hip_fit_result: the output columns, each [n_spec]"""
    _fields_ = [(k, _dp) for k in FIT_F8_COLUMNS] + [(k, _ip) for k in FIT_I4_COLUMNS]


FIT_COMP, FIT_BAND = 0, 1                                              # mcrat_hip_fit_args.model
FIT_TOO_FEW_BINS, FIT_AT_BOUND_ALPHA, FIT_AT_BOUND_LAMBDA, FIT_AT_BOUND_BETA, FIT_NO_FINITE_CANDIDATE = 1, 2, 4, 8, 16      # bits of status
FIT_E_PIV = 100.0 * 1.602176634e-9                                     # 100 keV in erg
# The defaults of Engine.fit_spectra.  shrink, n_rounds and the coarse grid are chosen so that the NumPy restatement recovers 24 noise-free spectra
# to 1e-6 (tests/test_fit_checker_cpu.py): a faster shrink (0.9 and below) loses the minimum in the narrow valleys of Band fits.
FIT_DEFAULTS = dict(alpha=(-1.9, 2.0), beta=(-6.0, -2.05), grid=(16, 16, 8), n_rounds=320, shrink=0.95, min_count=1)


def spectra_from(res, mode, reduce=()):
    """The (count, w) spectra of a dict from Engine.observe, observe_sky or observe_sky_resampled, ready for Engine.fit_spectra.  reduce: the axes
    summed first, "time" and "pixels" (not "energy": it is the spectrum's axis).  Whether the cube has a replica axis behind the observer is read from its
    rank -- (n_obs, n_t, n_e[, n_y, n_x]) from observe and observe_sky, (n_obs, n_rep, n_t, n_e[, n_y, n_x]) from observe_sky_resampled.  mode:
    RESAMPLE_NONE leaves every entry as it stands; RESAMPLE_BOOTSTRAP leaves the entries as they are (entry 0 the sample);
    RESAMPLE_JACKKNIFE turns the G groups into G + 1 entries: entry 0 the total, entries 1 .. G the leave-one-out spectra -- the counts subtracted
    exactly, w scaled by G / (G - 1) as resampled_estimates scales it.  -> (count int64, w float64), energy as the last axis."""
    names = (reduce,) if isinstance(reduce, str) else tuple(reduce)
    for k in names:
        if k not in ("time", "pixels"):
            raise ValueError("spectra_from: reduce takes time and pixels, not %r" % (k,))
    count, w = np.asarray(res["count"], dtype=np.int64), np.asarray(res["w"], dtype=np.float64)
    if mode not in (RESAMPLE_NONE, RESAMPLE_JACKKNIFE, RESAMPLE_BOOTSTRAP):
        raise ValueError("spectra_from: mode must be RESAMPLE_NONE, RESAMPLE_JACKKNIFE or RESAMPLE_BOOTSTRAP")
    if count.shape != w.shape or count.ndim not in (3, 4, 5, 6):
        raise ValueError("spectra_from: count and w need one shape, (n_obs[, n_rep], n_t, n_e[, n_y, n_x])")
    replicas = count.ndim in (4, 6)                                    # (n_obs, n_rep, n_t, n_e[, n_y, n_x]): a replica axis behind the observer
    if mode != RESAMPLE_NONE and not replicas:
        raise ValueError("spectra_from: a jackknife or bootstrap cube has a replica axis, (n_obs, n_rep, n_t, n_e[, n_y, n_x])")
    lead = 2 if replicas else 1                                        # (n_obs[, n_rep]), then n_t, n_e[, n_y, n_x]
    if count.ndim > lead + 2:                                          # energy last
        count, w = np.moveaxis(count, lead + 1, -1), np.moveaxis(w, lead + 1, -1)
        if "pixels" in names:
            count, w = count.sum(axis=(-3, -2)), w.sum(axis=(-3, -2))
    if "time" in names:
        count, w = count.sum(axis=lead), w.sum(axis=lead)
    if mode == RESAMPLE_JACKKNIFE:
        G = count.shape[1]
        if G < 2:
            raise ValueError("spectra_from: a jackknife needs at least two groups")
        total_c, total_w = count.sum(axis=1, keepdims=True), w.sum(axis=1, keepdims=True)
        count = np.concatenate([total_c, total_c - count], axis=1)
        w = np.concatenate([total_w, (total_w - w) * (G / (G - 1.0))], axis=1)
    return np.ascontiguousarray(count), np.ascontiguousarray(w)


def fitted_estimates(fit, mode, percentiles=None):
    """Value, stderr and percentile bounds of alpha, beta, e_peak and ln_e_peak over the replica axis (axis 1) of a dict from Engine.fit_spectra on
    spectra_from's spectra, by the formulas of resampled_estimates.  RESAMPLE_JACKKNIFE: value is entry 0 (the total's fit), the replicates are
    entries 1 .. G, var = (G - 1) / G sum_g (theta_g - mean theta)^2.  RESAMPLE_BOOTSTRAP: value is entry 0, stderr the sample standard deviation
    (ddof = 1) over entries 1 .. B; percentiles = (lo, hi) in per cent adds the bounds.  RESAMPLE_NONE: the values alone, stderr NaN.  A replicate
    without a fit (TOO_FEW_BINS, NO_FINITE_CANDIDATE) is NaN and makes its stderr NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        x = {"alpha": np.asarray(fit["alpha"]), "beta": np.asarray(fit["beta"]), "e_peak": np.asarray(fit["e_peak"]), "ln_e_peak": np.log(np.asarray(fit["e_peak"]))}
    if mode not in (RESAMPLE_NONE, RESAMPLE_JACKKNIFE, RESAMPLE_BOOTSTRAP):
        raise ValueError("fitted_estimates: mode must be RESAMPLE_NONE, RESAMPLE_JACKKNIFE or RESAMPLE_BOOTSTRAP")
    out = {}
    for k, v in x.items():
        if mode == RESAMPLE_NONE:
            out[k] = {"value": v, "stderr": np.full(v.shape, np.nan)}
            continue
        if v.ndim < 2 or v.shape[1] < 3:
            raise ValueError("fitted_estimates: the replica axis needs the estimate and at least two replicates")
        val, reps = v[:, 0], v[:, 1:]
        n = reps.shape[1]
        est = {"value": val}
        with np.errstate(invalid="ignore"):
            dev = reps - val[:, None]
            if mode == RESAMPLE_JACKKNIFE:
                var = (n - 1.0) / n * ((dev - dev.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
            else:
                var = dev.var(axis=1, ddof=1)
                if percentiles is not None:
                    lo, hi = np.percentile(dev, list(percentiles), axis=1)
                    est["lo"], est["hi"] = val + lo, val + hi
            est["stderr"] = np.sqrt(var)
        out[k] = est
    return out


class RadfieldBins(C.Structure):
    """mcrat_hip_radfield_bins: the binning of a radiation field -- the hydro cells, or (r, mu) shells with their edges"""
    _fields_ = [("mode", C.c_int), ("n_r", C.c_int), ("r_edges", _dp), ("n_mu", C.c_int), ("mu_edges", _dp)]


class Radfield(C.Structure):
    """mcrat_hip_radfield: the six planes, each [n_bins], and the three counters"""
    _fields_ = [("count", C.POINTER(C.c_longlong)), ("w", _dp), ("we_lab", _dp), ("we_comv", _dp), ("w_nscatt", _dp), ("w_temp", _dp),
                ("n_observable", C.c_longlong), ("n_unlocated", C.c_longlong), ("n_outside", C.c_longlong)]


RADFIELD_CELLS, RADFIELD_SHELLS = 0, 1            # mcrat_hip_radfield_bins.mode
RADFIELD_PATH_LDS, RADFIELD_PATH_GLOBAL = 1, 2    # mcrat_hip_radiation_field_path
RADFIELD_PLANES = ("w", "we_lab", "we_comv", "w_nscatt", "w_temp")


class ComovingBins(C.Structure):
    """mcrat_hip_comoving_bins: the binning of a comoving field -- the hydro cells or (r, mu) shells, fluid-frame energy and fluid-frame cosine"""
    _fields_ = [("mode", C.c_int), ("n_r", C.c_int), ("r_edges", _dp), ("n_mu", C.c_int), ("mu_edges", _dp), ("n_e", C.c_int), ("e_edges", _dp),
                ("n_a", C.c_int), ("a_edges", _dp)]


class Comoving(C.Structure):
    """mcrat_hip_comoving: the eight planes, each [n_bins], and the three counters"""
    _fields_ = [("count", C.POINTER(C.c_longlong)), ("w", _dp), ("we", _dp), ("wea", _dp), ("weaa", _dp), ("we_lab", _dp), ("wem", _dp), ("wemm", _dp),
                ("n_observable", C.c_longlong), ("n_unlocated", C.c_longlong), ("n_outside", C.c_longlong)]


COMOVING_CELLS, COMOVING_SHELLS = 0, 1            # mcrat_hip_comoving_bins.mode
COMOVING_PATH_LDS, COMOVING_PATH_GLOBAL = 1, 2    # mcrat_hip_comoving_field_path
COMOVING_PLANES = ("w", "we", "wea", "weaa", "we_lab", "wem", "wemm")

SCIENCE, CYLINDRICAL_OUTFLOW, SPHERICAL_OUTFLOW, STRUCTURED_SPHERICAL_OUTFLOW = 0, 1, 2, 3    # SIMULATION_TYPE, mcrat.h:30-33

# every symbol include/mcrat_hip.h declares: (restype, argtypes)
_ctx = C.c_void_p
MODE_EXACT, MODE_FAST = 0, 1
SYMBOLS = {
    "mcrat_hip_init": (C.c_int, [C.POINTER(_ctx), C.POINTER(Config)]),
    "mcrat_hip_destroy": (None, [_ctx]),
    "mcrat_hip_version": (C.c_char_p, []),
    "mcrat_hip_strerror": (C.c_char_p, [C.c_int]),
    "mcrat_hip_last_error": (C.c_char_p, [_ctx]),
    "mcrat_hip_set_hydro": (C.c_int, [_ctx, C.POINTER(Hydro)]),
    "mcrat_hip_outflow_defaults": (None, [C.c_int, C.POINTER(Outflow)]),
    "mcrat_hip_ingest_flash": (C.c_int, [_ctx, C.POINTER(FlashBlocks), C.POINTER(Slab), C.POINTER(Outflow), C.POINTER(IngestResult)]),
    "mcrat_hip_ingest_pluto": (C.c_int, [_ctx, C.POINTER(PlutoGrid), C.POINTER(Slab), C.POINTER(Outflow), C.POINTER(IngestResult)]),
    "mcrat_hip_ingest_chombo": (C.c_int, [_ctx, C.POINTER(Chombo), C.POINTER(Slab), C.POINTER(Outflow), C.POINTER(IngestResult)]),
    "mcrat_hip_set_hydro_extras": (C.c_int, [_ctx, _dp, _dp, _dp, _dp]),
    "mcrat_hip_emit_cyclosynch_pool": (C.c_int, [_ctx, C.POINTER(Cyclosynch), C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                                 C.c_uint64, _ip, _dp, _ip]),
    "mcrat_hip_rebin_cyclosynch": (C.c_int, [_ctx, C.POINTER(Cyclosynch), C.c_int, _ip, _ip, _ip]),
    "mcrat_hip_scatter_frame_cyclosynch": (C.c_int, [_ctx, C.POINTER(Cyclosynch), _dp, C.c_double, C.c_uint64, C.c_double, C.c_double, C.c_int,
                                                     C.c_double, C.c_double, C.c_double, C.c_int, C.c_longlong, C.POINTER(FrameStats),
                                                     C.POINTER(CyclosynchCounts)]),
    "mcrat_hip_num_photon_slots": (C.c_int, [_ctx]),
    "mcrat_hip_absorb_cyclosynch": (C.c_int, [_ctx, C.POINTER(Cyclosynch), _ip, _ip, _dp]),
    "mcrat_hip_get_hydro": (C.c_int, [_ctx, C.POINTER(HydroColumns)]),
    "mcrat_hip_get_output": (C.c_int, [_ctx, C.POINTER(OutputColumns)]),
    "mcrat_hip_convert_comptonized": (C.c_int, [_ctx, _ip]),
    "mcrat_hip_get_photons_range": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_void_p]),
    "mcrat_hip_inject_photons": (C.c_int, [_ctx, C.c_double, C.c_double, C.c_int, C.c_int, C.c_char, C.c_double, C.c_double, C.c_double,
                                           C.c_uint64, _ip, _dp]),
    "mcrat_hip_set_hot_cross_section": (C.c_int, [_ctx, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "mcrat_hip_table_fallback_calls": (C.c_int, [_ctx, C.c_int]),
    "mcrat_hip_pool_select_frame": (C.c_int, [_ctx, C.c_int]),
    "mcrat_hip_create_hot_cross_section": (C.c_int, [_ctx, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_longlong,
                                                     C.c_uint64]),
    "mcrat_hip_set_photons": (C.c_int, [_ctx, C.POINTER(PhotonList)]),
    "mcrat_hip_register_host": (C.c_int, [_ctx, C.c_void_p, C.c_size_t]),
    "mcrat_hip_unregister_host": (C.c_int, [_ctx, C.c_void_p]),
    "mcrat_hip_get_photons": (C.c_int, [_ctx, C.POINTER(PhotonList)]),
    "mcrat_hip_set_photons_soa": (C.c_int, [_ctx, C.POINTER(PhotonSoA)]),
    "mcrat_hip_get_photons_soa": (C.c_int, [_ctx, C.POINTER(PhotonSoA)]),
    "mcrat_hip_num_photon_slots": (C.c_int, [_ctx]),
    "mcrat_hip_pool_inject_photons": (C.c_int, [_ctx, C.c_double, C.POINTER(PoolInjectList)]),
    "mcrat_hip_pool_set_photons": (C.c_int, [_ctx, C.c_int, _ip, C.c_void_p]),
    "mcrat_hip_profile_totals": (C.c_int, [_ctx, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "mcrat_hip_outbox_create": (C.c_int, [_ctx, C.POINTER(C.c_void_p)]),
    "mcrat_hip_outbox_destroy": (None, [C.c_void_p]),
    "mcrat_hip_outbox_post": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int]),
    "mcrat_hip_outbox_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p]),
    "mcrat_hip_bind_thread": (C.c_int, [_ctx]),
    "mcrat_hip_share_hydro": (C.c_int, [_ctx, _ctx]),
    "mcrat_hip_propagate_frame": (C.c_int, [_ctx, _dp, C.c_double, C.c_uint64, C.POINTER(FrameStats)]),
    "mcrat_hip_propagate_frame_mode": (C.c_int, [_ctx, _dp, C.c_double, C.c_uint64, C.c_int, C.c_int, C.POINTER(FrameStats)]),
    "mcrat_hip_fast_cadence": (C.c_int, [_ctx, C.c_int]),
    "mcrat_hip_pool_propagate_frames_fast": (C.c_int, [_ctx, C.POINTER(C.c_int), C.POINTER(C.c_uint64), _dp, _dp, C.c_int, C.POINTER(FrameStats)]),
    "mcrat_hip_begin_frame": (C.c_int, [_ctx, C.c_uint64, C.c_double, C.c_double]),
    "mcrat_hip_run": (C.c_int, [_ctx, C.c_longlong, C.POINTER(FrameStats)]),
    "mcrat_hip_snapshot_photons": (C.c_int, [_ctx]),
    "mcrat_hip_restore_photons": (C.c_int, [_ctx]),
    "mcrat_hip_num_virtual_ranks": (C.c_int, [_ctx]),
    "mcrat_hip_rank_stats": (C.c_int, [_ctx, C.c_int, C.POINTER(FrameStats)]),
    "mcrat_hip_pool_create": (C.c_int, [_ctx, C.c_int, C.c_int]),
    "mcrat_hip_pool_rank": (C.c_int, [_ctx, C.c_int, C.c_uint32, C.POINTER(_ctx)]),
    "mcrat_hip_pool_summaries": (C.c_int, [_ctx, C.POINTER(RankSummary)]),
    "mcrat_hip_pool_scatter_frames_cyclosynch": (C.c_int, [_ctx, C.POINTER(Cyclosynch), C.c_int, C.c_double, C.POINTER(PoolCsList), C.POINTER(FrameStats),
                                                           C.POINTER(CyclosynchCounts)]),
    "mcrat_hip_pool_begin_frames": (C.c_int, [_ctx, _ip, C.POINTER(C.c_uint64), _dp, _dp]),
    "mcrat_hip_pool_frame_stats": (C.c_int, [_ctx, C.POINTER(FrameStats)]),
    "mcrat_hip_pool_layout": (C.c_int, [_ctx, _ip, _ip]),
    "mcrat_hip_pool_run_frames": (C.c_int, [_ctx, C.POINTER(FramePlan), C.POINTER(FrameStats)]),
    "mcrat_hip_step_locate_sample": (C.c_int, [_ctx, C.c_int]),
    "mcrat_hip_step_event": (C.c_int, [_ctx, C.POINTER(FrameStats)]),
    "mcrat_hip_update_photon_position": (C.c_int, [_ctx, C.c_double]),
    "mcrat_hip_frame_statistics": (C.c_int, [_ctx, C.POINTER(FrameStats)]),
    "mcrat_hip_shared_clock_bytes_per_rank": (C.c_size_t, []),
    "mcrat_hip_shared_clock_attach": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]),
    "mcrat_hip_shared_clock_attach_device": (C.c_int, [_ctx, C.c_int, C.c_int, C.c_longlong]),
    "mcrat_hip_shared_clock_peer_buffers": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "mcrat_hip_shared_clock_set_peers": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mcrat_hip_shared_clock_exchange_push": (C.c_int, [_ctx]),
    "mcrat_hip_shared_clock_exchange_wait": (C.c_int, [_ctx]),
    "mcrat_hip_set_rng_tape": (C.c_int, [_ctx, _dp, C.c_longlong]),
    "mcrat_hip_rng_tape_position": (C.c_int, [_ctx, C.POINTER(C.c_longlong), _ip]),
    "mcrat_hip_pool_set_rng_tapes": (C.c_int, [_ctx, C.POINTER(_dp), C.POINTER(C.c_longlong)]),
    "mcrat_hip_pool_rng_tape_positions": (C.c_int, [_ctx, C.POINTER(C.c_longlong), _ip]),
    "mcrat_hip_shared_clock_exchange": (C.c_int, [_ctx]),
    "mcrat_hip_shared_clock_reset_exchange": (C.c_int, [_ctx]),
    "mcrat_hip_shared_clock_buffers": (C.c_int, [_ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "mcrat_hip_shared_clock_propose": (C.c_int, [_ctx]),
    "mcrat_hip_shared_clock_resolve": (C.c_int, [_ctx]),
    "mcrat_hip_shared_clock_poll": (C.c_int, [_ctx, _ip, C.POINTER(FrameStats)]),
    "mcrat_hip_shared_clock_finish": (C.c_int, [_ctx, C.POINTER(FrameStats)]),
    "mcrat_hip_ph_minmax": (C.c_int, [_ctx, _dp, _dp, _dp, _dp]),
    "mcrat_hip_scatt_stats": (C.c_int, [_ctx, _ip, _ip, _dp, _dp]),
    "mcrat_hip_avg_energy": (C.c_int, [_ctx, _dp]),
    "mcrat_hip_observe": (C.c_int, [_ctx, C.POINTER(Observer), C.c_double, C.POINTER(Observation)]),
    "mcrat_hip_pool_observe": (C.c_int, [_ctx, C.POINTER(Observer), _dp, C.POINTER(Observation)]),
    "mcrat_hip_observe_path": (C.c_int, [_ctx]),
    "mcrat_hip_sightline_rays": (C.c_int, [_ctx, _ctx, C.POINTER(SightlineParams), C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(Sightlines)]),
    "mcrat_hip_sightline_photons": (C.c_int, [_ctx, _ctx, C.POINTER(SightlineParams), C.POINTER(Sightlines)]),
    "mcrat_hip_pool_sightline_photons": (C.c_int, [_ctx, _ctx, C.POINTER(SightlineParams), C.POINTER(Sightlines)]),
    "mcrat_hip_radiation_field_bins": (C.c_int, [_ctx, _ctx, C.POINTER(RadfieldBins), _ip]),
    "mcrat_hip_radiation_field": (C.c_int, [_ctx, _ctx, C.POINTER(RadfieldBins), C.POINTER(Radfield)]),
    "mcrat_hip_pool_radiation_field": (C.c_int, [_ctx, _ctx, C.POINTER(RadfieldBins), C.POINTER(Radfield)]),
    "mcrat_hip_radiation_field_path": (C.c_int, [_ctx]),
    "mcrat_hip_comoving_field_bins": (C.c_int, [_ctx, _ctx, C.POINTER(ComovingBins), _ip]),
    "mcrat_hip_comoving_field": (C.c_int, [_ctx, _ctx, C.POINTER(ComovingBins), C.POINTER(Comoving)]),
    "mcrat_hip_pool_comoving_field": (C.c_int, [_ctx, _ctx, C.POINTER(ComovingBins), C.POINTER(Comoving)]),
    "mcrat_hip_comoving_field_path": (C.c_int, [_ctx]),
    "mcrat_hip_observe_sky": (C.c_int, [_ctx, C.POINTER(SkyObserver), C.c_double, C.POINTER(SkyObservation)]),
    "mcrat_hip_pool_observe_sky": (C.c_int, [_ctx, C.POINTER(SkyObserver), _dp, C.POINTER(SkyObservation)]),
    "mcrat_hip_observe_sky_path": (C.c_int, [_ctx]),
    "mcrat_hip_observe_escaping": (C.c_int, [_ctx, _ctx, C.POINTER(EscapeObserver), C.c_double, C.POINTER(EscapeObservation)]),
    "mcrat_hip_pool_observe_escaping": (C.c_int, [_ctx, _ctx, C.POINTER(EscapeObserver), _dp, C.POINTER(EscapeObservation)]),
    "mcrat_hip_observe_escaping_path": (C.c_int, [_ctx]),
    "mcrat_hip_observe_sky_resampled": (C.c_int, [_ctx, C.POINTER(ResampleObserver), C.c_double, C.POINTER(ResampleObservation)]),
    "mcrat_hip_pool_observe_sky_resampled": (C.c_int, [_ctx, C.POINTER(ResampleObserver), _dp, C.POINTER(ResampleObservation)]),
    "mcrat_hip_observe_sky_resampled_path": (C.c_int, [_ctx]),
    "mcrat_hip_observe_events": (C.c_int, [_ctx, C.POINTER(EventsObserver), C.c_double, C.POINTER(Events)]),
    "mcrat_hip_pool_observe_events": (C.c_int, [_ctx, C.POINTER(EventsObserver), _dp, C.POINTER(Events)]),
    "mcrat_hip_fit_spectra": (C.c_int, [_ctx, C.POINTER(FitArgs), C.POINTER(FitResult)]),
    "mcrat_hip_synchronize": (C.c_int, [_ctx]),
    "mcrat_hip_device_bytes": (C.c_size_t, [_ctx]),
    "mcrat_hip_eval_function": (C.c_int, [_ctx, C.c_int, C.c_int, _dp, _dp, C.c_uint64]),
    "mcrat_hip_lookup_cell": (C.c_int, [_ctx, C.c_int, _dp, _dp, _dp, _ip]),
    "mcrat_hip_covered_octants": (C.c_longlong, [_ctx, _ip, C.c_longlong]),
}

_lib = None


def load_library():
    """dlopen libmcrat_hip.so and bind every symbol; raises if the library was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libmcrat_hip.so is missing (%s): build it with `python -m mcrat_amd.build`; "
                "there is no CPU fallback for the photon loop" % LIB_PATH)
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64, and torch finds no GPU if the
        # system copy was mapped first.  Loading torch first makes this library bind to the copy torch uses, so that
        # torch streams / tensors / collectives and the engine share one runtime (shared_clock.py, bench.py).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(os.environ.get("MCRAT_HIP_LIB", LIB_PATH))     # MCRAT_HIP_LIB: another build of the same ABI (A/B timing)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args
        _lib = lib
    return _lib


class McratHipError(RuntimeError):
    pass


def _f8(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def observer_angles(theta_obs_deg, dtheta_deg):
    """observers at polar angles theta_obs_deg [degrees from the r2 axis], each accepting photons whose direction lies within its cone of full width
    dtheta_deg: theta_obs - dtheta / 2 < theta <= theta_obs + dtheta / 2, cut at the axis  ->  (cos_obs, sin_obs, cos_lo, cos_hi) for
    Engine.observe.  The lower edge is closed at the axis (cos_lo just above 1), so that a photon along the axis is seen by an observer there."""
    th = np.radians(np.atleast_1d(_f8(theta_obs_deg)))
    half = 0.5 * np.radians(np.broadcast_to(_f8(dtheta_deg), th.shape))
    lo, hi = th - half, th + half
    cos_lo = np.where(lo <= 0.0, np.nextafter(1.0, 2.0), np.cos(np.maximum(lo, 0.0)))
    cos_hi = np.where(hi >= np.pi, -np.nextafter(1.0, 2.0), np.cos(np.minimum(hi, np.pi)))
    return np.cos(th), np.sin(th), cos_lo, cos_hi


def sky_observers(theta, phi, half_angle):
    """observers at polar angle theta and azimuth phi [radians], each accepting photons whose direction lies within half_angle [radians] of the
    direction towards it  ->  (n, cos_acc, ex, ey) for Engine.observe_sky: n, ex, ey are (3, n_obs) and cos_acc (n_obs,), with
    n = (sin theta cos phi, sin theta sin phi, cos theta), ex = theta_hat = (cos theta cos phi, cos theta sin phi, -sin theta),
    ey = phi_hat = (-sin phi, cos phi, 0): ex x ey = n, and for an observer on the r2 axis at phi = 0 ex and ey are the r0 and r1 axes."""
    th, ph, half = np.broadcast_arrays(np.atleast_1d(_f8(theta)), np.atleast_1d(_f8(phi)), np.atleast_1d(_f8(half_angle)))
    ct, st, cp, sp = np.cos(th), np.sin(th), np.cos(ph), np.sin(ph)
    n = np.stack([st * cp, st * sp, ct])
    ex = np.stack([ct * cp, ct * sp, -st])
    ey = np.stack([-sp, cp, np.zeros_like(sp)])
    return n, np.cos(half), ex, ey


def shell_edges(r_edges, theta_edges_deg):
    """(r_edges, mu_edges) for Engine.radiation_field(RADFIELD_SHELLS, ...) from radial edges [cm] and polar-angle edges [degrees from the r2 axis,
    ascending]: mu = cos(theta) ascending, so shell column j holds theta_edges_deg[n - j - 1] >= theta > theta_edges_deg[n - j].  Where the top
    edge would be 1 (an angle edge of 0) it lies just above 1, as observer_angles closes its cones at the axis: a photon on the axis is counted."""
    th = np.radians(_f8(theta_edges_deg).ravel())
    mu = np.cos(th)[::-1].copy()
    if len(mu) and mu[-1] >= 1.0:
        mu[-1] = np.nextafter(1.0, 2.0)
    return _f8(r_edges).ravel().copy(), mu


def cosine_edges(n):
    """n equal bins over [-1, 1] for the a axis of Engine.comoving_field, the top edge just above 1, as shell_edges closes its axis: a photon
    along the flow (a == 1) is counted"""
    a = np.linspace(-1.0, 1.0, int(n) + 1)
    a[-1] = np.nextafter(1.0, 2.0)
    return a


def eddington_moments(res):
    """the moment hierarchy per position bin of a comoving field (Engine.comoving_field's dict): J, H, K = we, wea, weaa summed over the energy and
    cosine axes, the Eddington factor K / J and the mean cosine H / J in the fluid frame about the flow, and the lab analogues about the radial
    direction J_lab, H_lab, K_lab, K_lab / J_lab, H_lab / J_lab from we_lab, wem, wemm.  NaN where a bin holds no energy."""
    out = {}
    for tag, planes in (("", ("we", "wea", "weaa")), ("_lab", ("we_lab", "wem", "wemm"))):
        j, h, k = (_f8(res[p]).sum(axis=(-2, -1)) for p in planes)
        out["J" + tag], out["H" + tag], out["K" + tag] = j, h, k
        for name, num in (("K_over_J", k), ("H_over_J", h)):
            q = np.full(j.shape, np.nan)
            np.divide(num, j, out=q, where=j != 0)
            out[name + tag] = q
    return out


K_B = 1.380658e-16        # erg / K, the reference's value (mclib.c)


def photon_temperature(res, spect="b"):
    """the photon temperature per bin of a radiation field: we_comv / (w * K_B * xbar), xbar = 2.701 for a black body ('b'), 3 for a Wien spectrum
    ('w'): the mean comoving photon energy over xbar k_B.  NaN where the bin holds no weight."""
    xbar = {"b": 2.701, "w": 3.0}[spect.decode() if isinstance(spect, bytes) else spect]
    w, we = _f8(res["w"]), _f8(res["we_comv"])
    out = np.full(w.shape, np.nan)
    np.divide(we, w * K_B * xbar, out=out, where=w != 0)
    return out


class Engine:
    """One context of the HIP photon-loop engine (one per rank / GPU)."""

    def __init__(self, dimensions, geometry, stokes=0, device=0, stream=None, rng_stream=0,
                 iterations_per_sync=0, use_graph=False, profile=False, virtual_rank_photons=0, tau_calculation=TAU_DIRECT,
                 cyclosynchrotron=0):
        self.lib = load_library()
        self.cfg = Config(ABI_VERSION, int(dimensions), int(geometry), int(bool(stokes)), int(tau_calculation), int(cyclosynchrotron),
                          int(device), C.c_void_p(stream) if stream else None, int(rng_stream),
                          int(iterations_per_sync), int(bool(use_graph)), int(bool(profile)), int(virtual_rank_photons))
        self.ctx = _ctx()
        rc = self.lib.mcrat_hip_init(C.byref(self.ctx), C.byref(self.cfg))
        if rc != 0:
            self.ctx = _ctx()
            raise McratHipError("mcrat_hip_init: %s" % self.lib.mcrat_hip_strerror(rc).decode())
        self.n = 0

    def close(self):
        if getattr(self, "ctx", None):
            if getattr(self, "pool", None) is None:      # a view goes with its pool
                self.lib.mcrat_hip_destroy(self.ctx)
            self.ctx = _ctx()
            for v in getattr(self, "views", {}).values():
                v.ctx = _ctx()

    # ---- rank pool: R independent lists (the reference's MPI ranks) in one context
    def pool_create(self, n_ranks, slots_per_rank):
        self._check(self.lib.mcrat_hip_pool_create(self.ctx, int(n_ranks), int(slots_per_rank)), "pool_create")
        for v in getattr(self, "views", {}).values():
            v.ctx = _ctx()
        self.views = {}
        self.n_pool_ranks = int(n_ranks)
        self.n = int(self.lib.mcrat_hip_num_photon_slots(self.ctx))

    def pool_rank(self, rank, rng_stream=0):
        """the view of list `rank`: an Engine whose photons, clock and loop state are that list's"""
        ctx = _ctx()
        self._check(self.lib.mcrat_hip_pool_rank(self.ctx, int(rank), int(rng_stream), C.byref(ctx)), "pool_rank")
        if not hasattr(self, "views"):
            self.views = {}                                      # the pool was laid out from C (mcrat_host_run_ranks)
        v = self.views.get(rank)
        if v is None or v.ctx.value != ctx.value:
            v = Engine.__new__(Engine)
            v.lib, v.cfg, v.ctx, v.n, v.pool = self.lib, self.cfg, ctx, 0, self
            self.views[rank] = v
        v.n = int(self.lib.mcrat_hip_num_photon_slots(ctx))      # the list may have been set from C (mcrat_host_run_ranks)
        if getattr(self, "num_elements", None) is not None:
            v.num_elements = self.num_elements
        return v

    def pool_set_photons(self, ranks, records):
        """mcrat_hip_pool_set_photons: records[j] (numpy arrays of PHOTON_DTYPE, the reference's struct photon) becomes the list of pool rank
        ranks[j] -- one copy over PCIe and one launch for all of them (the views must exist: pool_rank)"""
        n = len(ranks)
        arrs = [np.ascontiguousarray(a, dtype=PHOTON_DTYPE) for a in records]
        lists = (PhotonList * n)()
        for j, a in enumerate(arrs):
            nulls = int(np.count_nonzero(a["type"] == b"N"))
            lists[j] = PhotonList(a.ctypes.data, None, len(a) - nulls, nulls, len(a))
        rk = np.ascontiguousarray(ranks, dtype=np.int32)
        self._check(self.lib.mcrat_hip_pool_set_photons(self.ctx, n, rk.ctypes.data_as(_ip), C.cast(lists, C.c_void_p)), "pool_set_photons")
        for r in ranks:
            if hasattr(self, "views") and r in self.views:
                self.views[r].n = int(self.lib.mcrat_hip_num_photon_slots(self.views[r].ctx))

    def pool_scatter_frames_cyclosynch(self, lists, max_photons, fps, b_field_calc=1, epsilon_b=0.5, rebin_e_perc=0.1, rebin_ang=0.5, rebin_ang_phi=10.0):
        """lists: one dict per list (None: the list sits the frame out) with seed, time_now, remaining_time, r_inj, ph_weight_suggest, theta_min,
        theta_max, emit_pool, scatt_frame_number, inj_frame_number -> ([FrameStats], [CyclosynchCounts])"""
        R = self.n_pool_ranks
        arr = (PoolCsList * R)()
        for r, d in enumerate(lists):
            if d is None:
                continue
            arr[r] = PoolCsList(1, int(d.get("emit_pool", 1)), int(d.get("scatt_frame_number", 0)), int(d.get("inj_frame_number", 0)), int(d["seed"]),
                                float(d["time_now"]), float(d["remaining_time"]), float(d["r_inj"]), float(d["ph_weight_suggest"]), float(d["theta_min"]),
                                float(d["theta_max"]))
        cs = Cyclosynch(int(b_field_calc), float(epsilon_b), float(rebin_e_perc), float(rebin_ang), float(rebin_ang_phi), 0, 0)
        st, cnt = (FrameStats * R)(), (CyclosynchCounts * R)()
        for r, d in enumerate(lists):
            if d is not None:
                cnt[r].scatt_cyclosynch_num_ph = int(d.get("scatt_cyclosynch_num_ph", 0))
        self._check(self.lib.mcrat_hip_pool_scatter_frames_cyclosynch(self.ctx, C.byref(cs), int(max_photons), float(fps), arr, st, cnt),
                    "pool_scatter_frames_cyclosynch")
        return list(st), list(cnt)

    def pool_inject_photons(self, fps, lists):
        """lists: one dict per list (None: no injection) with r_inj, ph_weight, min_photons, max_photons, spect, theta_min, theta_max, seed
        -> [(num_photons, ph_weight_adjusted) or None]"""
        R = self.n_pool_ranks
        arr = (PoolInjectList * R)()
        for r, q in enumerate(lists):
            if q is None:
                continue
            a = arr[r]
            a.inject, a.spect = 1, q["spect"].encode() if isinstance(q["spect"], str) else q["spect"]
            a.min_photons, a.max_photons = int(q["min_photons"]), int(q["max_photons"])
            a.r_inj, a.ph_weight, a.theta_min, a.theta_max, a.seed = float(q["r_inj"]), float(q["ph_weight"]), float(q["theta_min"]), float(q["theta_max"]), int(q["seed"])
        self._check(self.lib.mcrat_hip_pool_inject_photons(self.ctx, float(fps), arr), "pool_inject_photons")
        out = []
        for r, q in enumerate(lists):
            if q is None:
                out.append(None)
                continue
            v = self.views.get(r) if hasattr(self, "views") else None
            if v is not None:
                v.n = int(arr[r].num_photons)
            out.append((int(arr[r].num_photons), float(arr[r].ph_weight_adjusted)))
        return out

    def pool_summaries(self):
        out = (RankSummary * self.n_pool_ranks)()
        self._check(self.lib.mcrat_hip_pool_summaries(self.ctx, out), "pool_summaries")
        return list(out)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise McratHipError("%s: %s (%s)" % (what, self.lib.mcrat_hip_strerror(rc).decode(),
                                                 self.lib.mcrat_hip_last_error(self.ctx).decode()))

    # ---- staging
    def set_hot_cross_section(self, thermal_table, grid=(-12.0, 6.0, -4.0, 4.0)):
        """thermal_table: (N_PH_E + 1, N_T + 1) log10(sigma / sigma_T); grid: LOG_PH_E_MIN/MAX, LOG_T_MIN/MAX (hot_x_section.h:2-10)"""
        t = np.ascontiguousarray(thermal_table, dtype=np.float64)
        self._check(self.lib.mcrat_hip_set_hot_cross_section(self.ctx, t.ctypes.data_as(_dp), t.shape[0] - 1, t.shape[1] - 1,
                                                             float(grid[0]), float(grid[1]), float(grid[2]), float(grid[3])),
                    "set_hot_cross_section")

    def table_fallback_calls(self, calls=0):
        """samples of the integral a look-up off the table takes (hot_x_section.c:348: 500000); calls > 0 sets it"""
        return int(self.lib.mcrat_hip_table_fallback_calls(self.ctx, int(calls)))

    def create_hot_cross_section(self, n_ph_e=220, n_t=80, grid=(-12.0, 6.0, -4.0, 4.0), calls=500000, seed=1):
        """createHotCrossSection (hot_x_section.c:82-133) on the device -> (n_ph_e + 1, n_t + 1) array of log10(sigma / sigma_T)"""
        t = np.empty((n_ph_e + 1, n_t + 1))
        self._check(self.lib.mcrat_hip_create_hot_cross_section(self.ctx, t.ctypes.data_as(_dp), int(n_ph_e), int(n_t), float(grid[0]),
                                                                float(grid[1]), float(grid[2]), float(grid[3]), int(calls), int(seed)),
                    "create_hot_cross_section")
        return t

    def inject_photons(self, r_inj, ph_weight, min_photons, max_photons, spect, theta_min, theta_max, fps, seed):
        """photonInjection (mclib.c:9-300) on the device; returns (number of photons, adjusted weight)"""
        n, w = C.c_int(0), C.c_double(0)
        self._check(self.lib.mcrat_hip_inject_photons(self.ctx, float(r_inj), float(ph_weight), int(min_photons), int(max_photons),
                                                      spect.encode() if isinstance(spect, str) else spect, float(theta_min), float(theta_max),
                                                      float(fps), int(seed), C.byref(n), C.byref(w)), "inject_photons")
        self.n = n.value
        return n.value, w.value

    @staticmethod
    def outflow(simulation_type, **overrides):
        """the constants analytic_outflows.c hard-codes for this SIMULATION_TYPE, optionally overridden"""
        o = Outflow()
        load_library().mcrat_hip_outflow_defaults(int(simulation_type), C.byref(o))
        for k, v in overrides.items():
            setattr(o, k, float(v))
        return o

    @staticmethod
    def _slab(slab):
        s = Slab(float(slab["r_inj"]), int(slab["ph_inj_switch"]), float(slab["min_r"]), float(slab["max_r"]),
                 float(slab["min_theta"]), float(slab["max_theta"]), float(slab["fps"]))
        for k in ("r0_domain", "r1_domain", "r2_domain"):
            dom = slab.get(k, (0.0, 0.0))
            getattr(s, k)[0], getattr(s, k)[1] = float(dom[0]), float(dom[1])
        return s

    def ingest(self, raw, slab, outflow=None):
        """getHydroData (mcrat_io.c:1898-1990) on the device from a reader's buffers: raw["kind"] "flash" (coordinates,
        block_size, node_type, velx, vely, dens, pres) or "pluto" (nx, ny, nz, x1..dx3, rho, vx1, vx2, vx3, prs), with
        l_scale, d_scale, p_scale; slab: r_inj, ph_inj_switch, min_r, max_r, min_theta, max_theta, fps, r*_domain.
        The selected frame is staged for the loop; returns (num_elements, elem_factor, cells_read)."""
        keep, res, s = [], IngestResult(), self._slab(slab)

        def ptr(a, dtype=np.float64, ctype=C.c_double):
            arr = np.ascontiguousarray(a, dtype=dtype)
            keep.append(arr)
            return arr.ctypes.data_as(C.POINTER(ctype))
        op = C.byref(outflow) if outflow is not None else None
        if raw["kind"] == "flash":
            coords, bsize = _f8(raw["coordinates"]), _f8(raw["block_size"])
            b = FlashBlocks(coords.shape[0], coords.shape[1], bsize.shape[1], ptr(coords), ptr(bsize), ptr(raw["node_type"], np.int32, C.c_int),
                            ptr(raw["velx"]), ptr(raw["vely"]), ptr(raw["dens"]), ptr(raw["pres"]),
                            float(raw.get("l_scale", 1.0)), float(raw.get("d_scale", 1.0)), float(raw.get("p_scale", 1.0)))
            self._check(self.lib.mcrat_hip_ingest_flash(self.ctx, C.byref(b), C.byref(s), op, C.byref(res)), "ingest_flash")
        elif raw["kind"] == "chombo":
            nl = len(raw["levels"])
            levels = (ChomboLevel * nl)()
            for i, lv in enumerate(raw["levels"]):
                boxes = np.ascontiguousarray(lv["boxes"], dtype=np.int32)
                L = levels[i]
                L.n_boxes, L.boxes, L.box_offsets = boxes.shape[0], ptr(boxes, np.int32, C.c_int), ptr(lv["box_offsets"], np.int32, C.c_int)
                L.data_len = int(len(lv["data"]))
                for k in range(6):
                    L.prob_domain[k] = int(lv["prob_domain"][k]) if k < len(lv["prob_domain"]) else 0
                L.ref_ratio, L.logr = int(lv["ref_ratio"]), int(lv["logr"])
                for k in ("dx", "dombeg1", "dombeg2", "dombeg3", "g_x2stretch", "g_x3stretch"):
                    setattr(L, k, float(lv.get(k, 0.0)))
            names = (C.c_char_p * len(raw["var_names"]))(*[v.encode() for v in raw["var_names"]])
            keep += [levels, names]
            h = Chombo(nl, len(raw["var_names"]), levels, names, ptr(np.concatenate([_f8(lv["data"]) for lv in raw["levels"]])),
                       float(raw.get("l_scale", 1.0)), float(raw.get("d_scale", 1.0)), float(raw.get("p_scale", 1.0)))
            self._check(self.lib.mcrat_hip_ingest_chombo(self.ctx, C.byref(h), C.byref(s), op, C.byref(res)), "ingest_chombo")
        else:
            g = PlutoGrid()
            g.nx, g.ny, g.nz = int(raw["nx"]), int(raw["ny"]), int(raw.get("nz", 1))
            for k in ("x1", "dx1", "x2", "dx2", "x3", "dx3", "rho", "vx1", "vx2", "vx3", "prs"):
                setattr(g, k, ptr(raw[k]) if raw.get(k) is not None else None)
            g.l_scale, g.d_scale, g.p_scale = float(raw.get("l_scale", 1.0)), float(raw.get("d_scale", 1.0)), float(raw.get("p_scale", 1.0))
            self._check(self.lib.mcrat_hip_ingest_pluto(self.ctx, C.byref(g), C.byref(s), op, C.byref(res)), "ingest_pluto")
        self.num_elements = res.num_elements
        return res.num_elements, res.elem_factor, res.cells_read

    def set_hydro_extras(self, dens=None, B0=None, B1=None, B2=None):
        keep = [None if a is None else _f8(a) for a in (dens, B0, B1, B2)]
        self._check(self.lib.mcrat_hip_set_hydro_extras(self.ctx, *[None if a is None else a.ctypes.data_as(_dp) for a in keep]), "set_hydro_extras")

    def emit_cyclosynch_pool(self, r_inj, ph_weight, maximum_photons, theta_min, theta_max, fps, seed, b_field_calc=1, epsilon_b=0.5,
                             rebin_e_perc=0.1, scatt_frame_number=0, inj_frame_number=0):
        """photonEmitCyclosynch, inject_single_switch = 0 (mc_cyclosynch.c:1200-1460) -> (photons emitted, adjusted weight, integrals not converged)"""
        cs = Cyclosynch(int(b_field_calc), float(epsilon_b), float(rebin_e_perc), 0.5, 10.0, int(scatt_frame_number), int(inj_frame_number))
        n, w, bad = C.c_int(), C.c_double(), C.c_int()
        self._check(self.lib.mcrat_hip_emit_cyclosynch_pool(self.ctx, C.byref(cs), float(r_inj), float(ph_weight), int(maximum_photons), float(theta_min),
                                                            float(theta_max), float(fps), int(seed), C.byref(n), C.byref(w), C.byref(bad)),
                    "emit_cyclosynch_pool")
        self.n = int(self.lib.mcrat_hip_num_photon_slots(self.ctx))          # the list doubles when the pool does not fit
        return n.value, w.value, bad.value

    def scatter_frame_cyclosynch(self, time_now, remaining_time, seed, r_inj, ph_weight_suggest, max_photons, theta_min, theta_max, fps, emit_pool=1,
                                 max_iterations=0, b_field_calc=1, epsilon_b=0.5, rebin_e_perc=0.1, rebin_ang=0.5, rebin_ang_phi=10.0,
                                 scatt_frame_number=0, inj_frame_number=0, scatt_cyclosynch_num_ph=0):
        """main()'s scatter-frame body with CYCLOSYNCHROTRON_SWITCH on (mcrat.c:706-878) -> (time_now, FrameStats, CyclosynchCounts)"""
        cs = Cyclosynch(int(b_field_calc), float(epsilon_b), float(rebin_e_perc), float(rebin_ang), float(rebin_ang_phi), int(scatt_frame_number),
                        int(inj_frame_number))
        st, cnt, tn = FrameStats(), CyclosynchCounts(), C.c_double(time_now)
        cnt.scatt_cyclosynch_num_ph = int(scatt_cyclosynch_num_ph)       # main()'s counter, carried from the previous frame
        self._check(self.lib.mcrat_hip_scatter_frame_cyclosynch(self.ctx, C.byref(cs), C.byref(tn), float(remaining_time), int(seed), float(r_inj),
                                                                float(ph_weight_suggest), int(max_photons), float(theta_min), float(theta_max), float(fps),
                                                                int(emit_pool), int(max_iterations), C.byref(st), C.byref(cnt)),
                    "scatter_frame_cyclosynch")
        self.n = int(self.lib.mcrat_hip_num_photon_slots(self.ctx))
        return tn.value, st, cnt

    def rebin_cyclosynch(self, max_photons, rebin_e_perc=0.1, rebin_ang=0.5, rebin_ang_phi=10.0):
        """rebinCyclosynchCompPhotons (mc_cyclosynch.c:246-712) -> (empty bins, num_cyclosynch_ph_emit, scatt_cyclosynch_num_ph)"""
        cs = Cyclosynch(1, 0.5, float(rebin_e_perc), float(rebin_ang), float(rebin_ang_phi), 0, 0)
        e, a, s = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.mcrat_hip_rebin_cyclosynch(self.ctx, C.byref(cs), int(max_photons), C.byref(e), C.byref(a), C.byref(s)), "rebin_cyclosynch")
        return e.value, a.value, s.value

    def absorb_cyclosynch(self, b_field_calc=1, epsilon_b=0.5):
        """phAbsCyclosynch (mc_cyclosynch.c:1571-1623) -> (num_abs_ph, scatt_cyclosynch_num_ph, absorbed weight)"""
        cs = Cyclosynch(int(b_field_calc), float(epsilon_b), 0.1, 0.5, 10.0, 0, 0)
        a, s, w = C.c_int(), C.c_int(), C.c_double()
        self._check(self.lib.mcrat_hip_absorb_cyclosynch(self.ctx, C.byref(cs), C.byref(a), C.byref(s), C.byref(w)), "absorb_cyclosynch")
        return a.value, s.value, w.value

    def get_hydro(self, num_elements=None):
        """the staged frame's columns (struct hydro_dataframe) as a dict of numpy arrays"""
        n = int(num_elements if num_elements is not None else self.num_elements)
        out, cols = HydroColumns(), {}
        out.num_elements = n
        for f in HYDRO_COLUMNS:
            cols[f] = np.empty(n)
            setattr(out, f, cols[f].ctypes.data_as(_dp))
        self._check(self.lib.mcrat_hip_get_hydro(self.ctx, C.byref(out)), "get_hydro")
        cols = {f: a[:out.num_elements] for f, a in cols.items()}
        cols["num_elements"] = out.num_elements
        return cols

    def set_hydro(self, frame):
        self.num_elements = int(frame["num_elements"])
        n = int(frame["num_elements"])
        keep, h = [], Hydro()
        h.num_elements = n
        for f in ("r0", "r1", "r2", "r0_size", "r1_size", "r2_size", "v0", "v1", "v2", "dens_lab", "temp", "gamma"):
            a = frame.get(f)
            if a is None:
                setattr(h, f, None)
                continue
            a = _f8(a)
            assert a.shape == (n,), f
            keep.append(a)
            setattr(h, f, a.ctypes.data_as(_dp))
        for k in ("r0_domain", "r1_domain", "r2_domain"):
            dom = frame.get(k, (0.0, 0.0))
            getattr(h, k)[0], getattr(h, k)[1] = float(dom[0]), float(dom[1])
        h.fps = float(frame.get("fps", 1.0))
        self._check(self.lib.mcrat_hip_set_hydro(self.ctx, C.byref(h)), "set_hydro")

    def set_photons(self, ph):
        """ph: dict of SoA columns (mcrat_amd.synth layout)."""
        n = int(len(ph["p0"]))
        keep, s = [], PhotonSoA()
        s.n = n
        for f in F8_COLUMNS:
            a = ph.get(f)
            if a is None:
                setattr(s, f, None)
                continue
            a = _f8(a)
            assert a.shape == (n,), f
            keep.append(a)
            setattr(s, f, a.ctypes.data_as(_dp))
        t = np.ascontiguousarray(ph["type"], dtype="S1")
        idx = np.ascontiguousarray(ph["nearest_block_index"], dtype=np.int32)
        rc_ = np.ascontiguousarray(ph["recalc_properties"], dtype=np.int32)
        keep += [t, idx, rc_]
        s.type = t.ctypes.data_as(C.c_char_p)
        s.nearest_block_index = idx.ctypes.data_as(_ip)
        s.recalc_properties = rc_.ctypes.data_as(_ip)
        self._check(self.lib.mcrat_hip_set_photons_soa(self.ctx, C.byref(s)), "set_photons_soa")
        self.n = n

    def get_photons(self):
        n = self.n
        out, s = {}, PhotonSoA()
        s.n = n
        for f in F8_COLUMNS:
            out[f] = np.empty(n, dtype=np.float64)
            setattr(s, f, out[f].ctypes.data_as(_dp))
        out["type"] = np.empty(n, dtype="S1")
        out["nearest_block_index"] = np.empty(n, dtype=np.int32)
        out["recalc_properties"] = np.empty(n, dtype=np.int32)
        s.type = out["type"].ctypes.data_as(C.c_char_p)
        s.nearest_block_index = out["nearest_block_index"].ctypes.data_as(_ip)
        s.recalc_properties = out["recalc_properties"].ctypes.data_as(_ip)
        self._check(self.lib.mcrat_hip_get_photons_soa(self.ctx, C.byref(s)), "get_photons_soa")
        return out

    def get_output(self):
        """printPhotons' arrays (mcrat_io.c:137-181): photons with weight != 0 in slot order, compacted on the device"""
        o = OutputColumns()
        self._check(self.lib.mcrat_hip_get_output(self.ctx, C.byref(o)), "get_output (count)")
        m = o.count
        out = {f: np.empty(m) for f in OUTPUT_COLUMNS}
        out["type"] = np.empty(m, dtype="S1")
        for f in OUTPUT_COLUMNS:
            setattr(o, f, out[f].ctypes.data_as(_dp))
        o.type = out["type"].ctypes.data_as(C.c_char_p)
        self._check(self.lib.mcrat_hip_get_output(self.ctx, C.byref(o)), "get_output")
        assert o.count == m
        return out

    def profile_totals(self):
        """(summed ms, launches) of the loop kernel since the context was created (profile=True contexts)"""
        ms, n = C.c_double(), C.c_longlong()
        self._check(self.lib.mcrat_hip_profile_totals(self.ctx, C.byref(ms), C.byref(n)), "profile_totals")
        return ms.value, n.value

    def outbox_create(self):
        """mcrat_hip_outbox_create: a staging area (device + pinned host) for the frame's records and output columns"""
        b = C.c_void_p()
        self._check(self.lib.mcrat_hip_outbox_create(self.ctx, C.byref(b)), "outbox_create")
        return b

    def outbox_post(self, box, records=True, output=True):
        """stage what saveCheckpoint / printPhotons read and start its copy to the host; the photons may change when this returns"""
        self._check(self.lib.mcrat_hip_outbox_post(self.ctx, box, int(records), int(output)), "outbox_post")

    def outbox_wait(self, box):
        """-> (records or None, output columns dict or None): copies of what has landed in the outbox's pinned memory"""
        rec, n, o = C.c_void_p(), C.c_int(), OutputColumns()
        self._check(self.lib.mcrat_hip_outbox_wait(box, C.byref(rec), C.byref(n), C.byref(o)), "outbox_wait")
        records = None
        if rec.value:
            # (the raw bytes first: numpy copies a structured array member by member and leaves the bytes between the members undefined)
            records = np.frombuffer(C.string_at(rec, PHOTON_DTYPE.itemsize * n.value), dtype=PHOTON_DTYPE) if n.value else np.zeros(0, dtype=PHOTON_DTYPE)
        m = o.count
        cols = {f: np.ctypeslib.as_array(getattr(o, f), shape=(m,)).copy() if m else np.empty(0) for f in OUTPUT_COLUMNS}
        # (the raw pointer: reading a c_char_p member gives a Python bytes COPY that ends at the first NUL, not the address)
        type_ptr = C.c_void_p.from_buffer(o, OutputColumns.type.offset).value
        cols["type"] = np.frombuffer(C.string_at(type_ptr, m), dtype="S1").copy() if m else np.empty(0, dtype="S1")
        return records, cols

    def outbox_destroy(self, box):
        self.lib.mcrat_hip_outbox_destroy(box)

    def convert_comptonized(self):
        """saveCheckpoint's 'k' -> 'c' conversion (mcrat_io.c:896-900) on the resident list; returns the number converted"""
        n = C.c_int()
        self._check(self.lib.mcrat_hip_convert_comptonized(self.ctx, C.byref(n)), "convert_comptonized")
        return n.value

    def get_photons_range(self, first, count):
        a = np.zeros(count, dtype=PHOTON_DTYPE)
        self._check(self.lib.mcrat_hip_get_photons_range(self.ctx, int(first), int(count), a.ctypes.data), "get_photons_range")
        return a

    def set_photons_aos(self, aos, num_null=None):
        """aos: numpy array of PHOTON_DTYPE (the reference's struct photon records); num_null: photon_list->num_null_photons if known"""
        a = np.ascontiguousarray(aos, dtype=PHOTON_DTYPE)
        nulls = int(np.count_nonzero(a["type"] == b"N")) if num_null is None else int(num_null)
        l = PhotonList(a.ctypes.data, None, len(a) - nulls, nulls, len(a))
        self._check(self.lib.mcrat_hip_set_photons(self.ctx, C.byref(l)), "set_photons")
        self.n = len(a)

    def get_photons_aos(self, out=None):
        a = np.zeros(self.n, dtype=PHOTON_DTYPE) if out is None else out
        l = PhotonList(a.ctypes.data, None, self.n, 0, self.n)
        self._check(self.lib.mcrat_hip_get_photons(self.ctx, C.byref(l)), "get_photons")
        return a

    def register_host(self, array):
        """page-lock a numpy array the caller hands to set_photons_aos / get_photons_aos(out=...) repeatedly"""
        self._check(self.lib.mcrat_hip_register_host(self.ctx, array.ctypes.data, array.nbytes), "register_host")

    def unregister_host(self, array):
        self._check(self.lib.mcrat_hip_unregister_host(self.ctx, array.ctypes.data), "unregister_host")

    # ---- the loop
    def set_rng_tape(self, uniforms):
        """the random stream as an input: a float64 array of uniforms in [0,1) consumed in the reference's call order (None: the keyed source)"""
        if uniforms is None:
            self._check(self.lib.mcrat_hip_set_rng_tape(self.ctx, None, 0), "set_rng_tape")
            return
        u = _f8(uniforms)
        self._check(self.lib.mcrat_hip_set_rng_tape(self.ctx, u.ctypes.data_as(_dp), int(u.size)), "set_rng_tape")

    def rng_tape_position(self):
        pos, out = C.c_longlong(0), C.c_int(0)
        self._check(self.lib.mcrat_hip_rng_tape_position(self.ctx, C.byref(pos), C.byref(out)), "rng_tape_position")
        return pos.value, bool(out.value)

    def pool_set_rng_tapes(self, tapes):
        """one recorded stream per list of the pool (float64 arrays of uniforms in [0,1), consumed as set_rng_tape consumes one); None for a
        list that keeps its keyed streams.  Replaces every list's tape and starts them at position 0; all None: the pool is keyed again"""
        tapes = list(tapes)
        R = getattr(self, "n_pool_ranks", len(tapes))        # (a view or a context without lists: the library refuses the call)
        if len(tapes) != R:
            raise ValueError("pool_set_rng_tapes: %d tapes for %d lists" % (len(tapes), R))
        arrs = [None if t is None else _f8(t).ravel() for t in tapes]
        ptrs = (_dp * R)(*[(a.ctypes.data_as(_dp) if a is not None and a.size else None) for a in arrs])
        n = (C.c_longlong * R)(*[(int(a.size) if a is not None else 0) for a in arrs])
        self._check(self.lib.mcrat_hip_pool_set_rng_tapes(self.ctx, ptrs, n), "pool_set_rng_tapes")

    def pool_rng_tape_positions(self):
        """-> (positions, ran_out): numpy arrays over the lists of the pool (entries read so far; whether a list needed more than its tape holds)"""
        R = getattr(self, "n_pool_ranks", 0)
        pos, out = np.zeros(max(R, 1), dtype=np.int64)[:R], np.zeros(max(R, 1), dtype=np.int32)[:R]
        self._check(self.lib.mcrat_hip_pool_rng_tape_positions(self.ctx, pos.ctypes.data_as(C.POINTER(C.c_longlong)), out.ctypes.data_as(_ip)),
                    "pool_rng_tape_positions")
        return pos, out.astype(bool)

    def begin_frame(self, seed, time_now, remaining_time):
        self._check(self.lib.mcrat_hip_begin_frame(self.ctx, int(seed), float(time_now), float(remaining_time)), "begin_frame")

    def run(self, max_iterations=0):
        st = FrameStats()
        self._check(self.lib.mcrat_hip_run(self.ctx, int(max_iterations), C.byref(st)), "run")
        return st

    def propagate_frame(self, time_now, remaining_time, seed):
        st = FrameStats()
        tn = C.c_double(time_now)
        self._check(self.lib.mcrat_hip_propagate_frame(self.ctx, C.byref(tn), float(remaining_time), int(seed), C.byref(st)),
                    "propagate_frame")
        return tn.value, st

    def bind_thread(self):
        """select this engine's device in the calling host thread (HIP's current device is per thread)"""
        self._check(self.lib.mcrat_hip_bind_thread(self.ctx), "bind_thread")

    def share_hydro(self, owner):
        """read `owner`'s staged frame (one copy for several contexts in the same hydro frame); the owner must keep it while shared"""
        self._check(self.lib.mcrat_hip_share_hydro(self.ctx, owner.ctx), "share_hydro")
        self._hydro_owner = owner          # keeps the owner alive as long as this engine

    def propagate_frame_fast(self, time_now, remaining_time, seed, windows=0):
        """MCRAT_HIP_MODE_FAST: every photon through the frame on its own clock (statistically, not sequence-, equivalent)"""
        st = FrameStats()
        tn = C.c_double(time_now)
        self._check(self.lib.mcrat_hip_propagate_frame_mode(self.ctx, C.byref(tn), float(remaining_time), int(seed), MODE_FAST, int(windows),
                                                            C.byref(st)), "propagate_frame_mode")
        return tn.value, st

    def fast_cadence(self, set_windows=0):
        """the list's learnt FAST refresh cadence (windows per frame); set_windows > 0 sets it (a restarted run hands the value back)"""
        return int(self.lib.mcrat_hip_fast_cadence(self.ctx, int(set_windows)))

    def pool_propagate_frames_fast(self, open_, seeds, time_now, remaining_time, windows=0):
        """FAST mode for the lists of the pool, each with its own seed and frame time -> per-list FrameStats"""
        R = self.n_pool_ranks
        o = (C.c_int * R)(*[int(x) for x in open_])
        sd = (C.c_uint64 * R)(*[int(x) for x in seeds])
        t = (C.c_double * R)(*[float(x) for x in time_now])
        rem = (C.c_double * R)(*[float(x) for x in remaining_time])
        st = (FrameStats * R)()
        self._check(self.lib.mcrat_hip_pool_propagate_frames_fast(self.ctx, o, sd, t, rem, int(windows), st), "pool_propagate_frames_fast")
        return list(st)

    def frame_plan(self, open_, seeds, time_now, remaining_time, frame_end=None, chain_clock=False, restore_each_frame=False, hydro=None, capture=False):
        """a mcrat_hip_frame_plan from [n_frames][n_ranks] arrays -> (plan, stats array, the arrays the plan points into);
        hydro: per frame None (the pool's own staged frame) or an Engine holding that frame's staged hydro frame"""
        R = self.n_pool_ranks
        o = np.ascontiguousarray(open_, dtype=np.int32).reshape(-1, R)
        F = o.shape[0]
        sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(F, R)
        t = np.ascontiguousarray(time_now, dtype=np.float64).reshape(F, R)
        rem = np.ascontiguousarray(remaining_time, dtype=np.float64).reshape(F, R)
        fe = None if frame_end is None else np.ascontiguousarray(frame_end, dtype=np.float64).reshape(F, R)
        plan = FramePlan(F, int(bool(chain_clock)), int(bool(restore_each_frame)), int(bool(capture)), o.ctypes.data_as(C.POINTER(C.c_int)),
                         sd.ctypes.data_as(C.POINTER(C.c_uint64)), t.ctypes.data_as(_dp), rem.ctypes.data_as(_dp),
                         fe.ctypes.data_as(_dp) if fe is not None else None, None)
        hy = None
        if hydro is not None:
            hy = (C.c_void_p * F)(*[(h.ctx if h is not None else None) for h in hydro])
            plan.hydro = C.cast(hy, C.POINTER(C.c_void_p))
        return plan, (FrameStats * (F * R))(), (o, sd, t, rem, fe, hy, hydro)

    def pool_run_plan(self, plan, stats):
        """mcrat_hip_pool_run_frames on a prepared plan; stats (frame_plan's array) receives item f * n_ranks + r"""
        self._check(self.lib.mcrat_hip_pool_run_frames(self.ctx, C.byref(plan), stats), "pool_run_frames")

    def pool_run_frames(self, open_, seeds, time_now, remaining_time, frame_end=None, chain_clock=False, restore_each_frame=False, hydro=None, capture=False):
        """mcrat_hip_pool_run_frames: the arrays are [n_frames][n_ranks]; every open list through its frames in ONE launch (the frame queue:
        a list that is through frame f starts f + 1 while others are still in f) -> FrameStats [n_frames][n_ranks]"""
        plan, st, keep = self.frame_plan(open_, seeds, time_now, remaining_time, frame_end, chain_clock, restore_each_frame, hydro, capture)
        self.pool_run_plan(plan, st)
        R, F = self.n_pool_ranks, plan.n_frames
        return [[st[f * R + r] for r in range(R)] for f in range(F)]

    def pool_select_frame(self, frame):
        """the pool's read calls (pool_summaries, get_photons_range, get_output, outbox) on the lists as frame `frame` of the last plan with
        capture=True left them; -1: the live lists again"""
        self._check(self.lib.mcrat_hip_pool_select_frame(self.ctx, int(frame)), "pool_select_frame")

    def snapshot_photons(self):
        self._check(self.lib.mcrat_hip_snapshot_photons(self.ctx), "snapshot_photons")

    def restore_photons(self):
        self._check(self.lib.mcrat_hip_restore_photons(self.ctx), "restore_photons")

    def num_virtual_ranks(self):
        return int(self.lib.mcrat_hip_num_virtual_ranks(self.ctx))

    def rank_stats(self, rank):
        st = FrameStats()
        self._check(self.lib.mcrat_hip_rank_stats(self.ctx, int(rank), C.byref(st)), "rank_stats")
        return st

    def step_locate_sample(self, find_nearest_block_switch):
        self._check(self.lib.mcrat_hip_step_locate_sample(self.ctx, int(find_nearest_block_switch)), "step_locate_sample")

    def frame_statistics(self):
        st = FrameStats()
        self._check(self.lib.mcrat_hip_frame_statistics(self.ctx, C.byref(st)), "frame_statistics")
        return st

    def update_photon_position(self, t):
        self._check(self.lib.mcrat_hip_update_photon_position(self.ctx, float(t)), "update_photon_position")

    def step_event(self):
        st = FrameStats()
        self._check(self.lib.mcrat_hip_step_event(self.ctx, C.byref(st)), "step_event")
        return st

    # ---- one list over several GPUs, one clock (mcrat_amd/shared_clock.py drives these)
    def shared_clock_bytes_per_rank(self):
        return int(self.lib.mcrat_hip_shared_clock_bytes_per_rank())

    def shared_clock_attach(self, world, rank, slot_base, send_ptr=None, recv_ptr=None):
        self._check(self.lib.mcrat_hip_shared_clock_attach(self.ctx, int(world), int(rank), int(slot_base),
                                                           C.c_void_p(send_ptr) if send_ptr else None,
                                                           C.c_void_p(recv_ptr) if recv_ptr else None), "shared_clock_attach")

    def shared_clock_attach_device(self, world, rank, slot_base):
        """device-initiated exchange: library-owned fine-grained buffers -> (recv address, recv bytes, flags address, flags bytes)"""
        self._check(self.lib.mcrat_hip_shared_clock_attach_device(self.ctx, int(world), int(rank), int(slot_base)), "shared_clock_attach_device")
        r, f, rb, fb = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.mcrat_hip_shared_clock_peer_buffers(self.ctx, C.byref(r), C.byref(rb), C.byref(f), C.byref(fb)), "shared_clock_peer_buffers")
        return r.value, rb.value, f.value, fb.value

    def shared_clock_set_peers(self, peer_recv, peer_flags):
        n = len(peer_recv)
        a = (C.c_void_p * n)(*[C.c_void_p(x) for x in peer_recv])
        b = (C.c_void_p * n)(*[C.c_void_p(x) for x in peer_flags])
        self._check(self.lib.mcrat_hip_shared_clock_set_peers(self.ctx, a, b), "shared_clock_set_peers")

    def shared_clock_exchange_push(self):
        self._check(self.lib.mcrat_hip_shared_clock_exchange_push(self.ctx), "shared_clock_exchange_push")

    def shared_clock_exchange_wait(self):
        self._check(self.lib.mcrat_hip_shared_clock_exchange_wait(self.ctx), "shared_clock_exchange_wait")

    def shared_clock_reset_exchange(self):
        self._check(self.lib.mcrat_hip_shared_clock_reset_exchange(self.ctx), "shared_clock_reset_exchange")

    def shared_clock_propose(self):
        self._check(self.lib.mcrat_hip_shared_clock_propose(self.ctx), "shared_clock_propose")

    def shared_clock_resolve(self):
        self._check(self.lib.mcrat_hip_shared_clock_resolve(self.ctx), "shared_clock_resolve")

    def shared_clock_poll(self):
        st = FrameStats()
        done = C.c_int(0)
        self._check(self.lib.mcrat_hip_shared_clock_poll(self.ctx, C.byref(done), C.byref(st)), "shared_clock_poll")
        return bool(done.value), st

    def shared_clock_finish(self):
        st = FrameStats()
        self._check(self.lib.mcrat_hip_shared_clock_finish(self.ctx, C.byref(st)), "shared_clock_finish")
        return st

    # ---- reductions
    def ph_minmax(self):
        v = [C.c_double() for _ in range(4)]
        self._check(self.lib.mcrat_hip_ph_minmax(self.ctx, *[C.byref(x) for x in v]), "ph_minmax")
        return tuple(x.value for x in v)          # min_r, max_r, min_theta, max_theta

    def scatt_stats(self):
        mx, mn, avg, ravg = C.c_int(), C.c_int(), C.c_double(), C.c_double()
        self._check(self.lib.mcrat_hip_scatt_stats(self.ctx, C.byref(mx), C.byref(mn), C.byref(avg), C.byref(ravg)), "scatt_stats")
        return mx.value, mn.value, avg.value, ravg.value

    def avg_energy(self):
        e = C.c_double()
        self._check(self.lib.mcrat_hip_avg_energy(self.ctx, C.byref(e)), "avg_energy")
        return e.value

    def _pool_clocks(self, what, time_now):
        """time_now of a pool call, one clock per list, as the float64 array the ABI reads (the caller keeps it alive for the call)"""
        tn = _f8(time_now).ravel()
        if len(tn) != self.n_pool_ranks:
            raise ValueError("%s: time_now needs one clock per rank of the pool" % what)
        return tn

    @staticmethod
    def _cube_result(shape, struct, sums=("w", "we", "i", "q", "u", "v"), counters=("n_accepted", "n_outside")):
        """the count plane and the `sums` planes of a product's cube of `shape` (with counters: observer first) and the per-observer `counters`,
        zeroed, and the ABI's output struct (Observation, SkyObservation, EscapeObservation, ..., Radfield, Comoving) that points at them"""
        res = {"count": np.zeros(shape, dtype=np.int64)}
        res.update({k: np.zeros(shape) for k in sums})
        res.update({k: np.zeros(shape[0], dtype=np.int64) for k in counters})
        ll = C.POINTER(C.c_longlong)
        return res, struct(res["count"].ctypes.data_as(ll), *([res[k].ctypes.data_as(_dp) for k in sums] + [res[k].ctypes.data_as(ll) for k in counters]))

    # ---- mock observations: the resident photons binned by observer, detection time and energy (include/mcrat_hip.h)
    def _observe(self, call, what, cos_obs, sin_obs, cos_lo, cos_hi, t_edges, e_edges, time_now):
        co, so, cl, ch, te, ee = (_f8(a).ravel() for a in (cos_obs, sin_obs, cos_lo, cos_hi, t_edges, e_edges))
        n_obs, n_t, n_e = len(co), len(te) - 1, len(ee) - 1
        if not (len(so) == len(cl) == len(ch) == n_obs):
            raise ValueError("%s: cos_obs, sin_obs, cos_lo and cos_hi must have one entry per observer" % what)
        obs = Observer(n_obs, co.ctypes.data_as(_dp), so.ctypes.data_as(_dp), cl.ctypes.data_as(_dp), ch.ctypes.data_as(_dp),
                       n_t, te.ctypes.data_as(_dp), n_e, ee.ctypes.data_as(_dp))
        res, out = self._cube_result((max(n_obs, 0), max(n_t, 0), max(n_e, 0)), Observation)
        self._check(call(self.ctx, C.byref(obs), time_now, C.byref(out)), what)
        return res

    def observe(self, cos_obs, sin_obs, cos_lo, cos_hi, t_edges, e_edges, time_now):
        """this list's photons as the observers see them at the list's clock time_now -> dict of (n_obs, n_t, n_e) arrays count, w, we, i, q, u, v
        and the per-observer n_accepted, n_outside (mcrat_hip_observe; observer_angles gives the four cosine arrays)"""
        return self._observe(self.lib.mcrat_hip_observe, "observe", cos_obs, sin_obs, cos_lo, cos_hi, t_edges, e_edges, float(time_now))

    def pool_observe(self, cos_obs, sin_obs, cos_lo, cos_hi, t_edges, e_edges, time_now):
        """every list of the pool in one launch, list r at its own clock time_now[r] (mcrat_hip_pool_observe)"""
        tn = self._pool_clocks("pool_observe", time_now)
        return self._observe(self.lib.mcrat_hip_pool_observe, "pool_observe", cos_obs, sin_obs, cos_lo, cos_hi, t_edges, e_edges, tn.ctypes.data_as(_dp))

    def observe_path(self):
        """how the last observation of this context was accumulated: OBSERVE_PATH_LDS, OBSERVE_PATH_GLOBAL, 0: none yet"""
        return int(self.lib.mcrat_hip_observe_path(self.ctx))

    # ---- sky observers: mock observations from any direction, with images (include/mcrat_hip.h)
    @staticmethod
    def _sky_observer(what, n, cos_acc, t_edges, e_edges, ex, ey, x_edges, y_edges):
        """-> the ABI's SkyObserver for these arguments, the arrays it points at (to be kept alive for the call), the cube's shape with the
        observers first, and whether there are image axes"""
        def vec(a, name):
            a = _f8(a)
            if a.ndim == 1 and a.shape[0] == 3:
                a = a.reshape(3, 1)
            if a.ndim != 2 or a.shape[0] != 3:
                raise ValueError("%s: %s must be three components per observer, shape (3, n_obs)" % (what, name))
            return np.ascontiguousarray(a)
        nv, ca, te, ee = vec(n, "n"), _f8(cos_acc).ravel(), _f8(t_edges).ravel(), _f8(e_edges).ravel()
        n_obs, n_t, n_e = nv.shape[1], len(te) - 1, len(ee) - 1
        if len(ca) != n_obs:
            raise ValueError("%s: cos_acc must have one entry per observer" % what)
        if (x_edges is None) != (y_edges is None):
            raise ValueError("%s: x_edges and y_edges come together" % what)
        image = x_edges is not None
        xe, ye = (_f8(x_edges).ravel(), _f8(y_edges).ravel()) if image else (None, None)
        n_x, n_y = (len(xe) - 1, len(ye) - 1) if image else (0, 0)
        xv, yv = (vec(ex, "ex") if ex is not None else None), (vec(ey, "ey") if ey is not None else None)
        for a, name in ((xv, "ex"), (yv, "ey")):
            if a is not None and a.shape[1] != n_obs:
                raise ValueError("%s: %s must have one vector per observer" % (what, name))
        ptr = lambda a: a.ctypes.data_as(_dp) if a is not None else None
        row = lambda a, k: ptr(a[k]) if a is not None else None
        obs = SkyObserver(n_obs, row(nv, 0), row(nv, 1), row(nv, 2), ptr(ca), row(xv, 0), row(xv, 1), row(xv, 2), row(yv, 0), row(yv, 1), row(yv, 2),
                          n_t, ptr(te), n_e, ptr(ee), n_x, ptr(xe), n_y, ptr(ye))
        return obs, (nv, ca, te, ee, xe, ye, xv, yv), tuple(max(m, 0) for m in ((n_obs, n_t, n_e, n_y, n_x) if image else (n_obs, n_t, n_e))), image

    def _observe_sky(self, call, what, n, cos_acc, t_edges, e_edges, time_now, ex, ey, x_edges, y_edges):
        obs, _alive, shape, _ = self._sky_observer(what, n, cos_acc, t_edges, e_edges, ex, ey, x_edges, y_edges)
        res, out = self._cube_result(shape, SkyObservation)
        self._check(call(self.ctx, C.byref(obs), time_now, C.byref(out)), what)
        return res

    def observe_sky(self, n, cos_acc, t_edges, e_edges, time_now, ex=None, ey=None, x_edges=None, y_edges=None):
        """this list's photons as observers anywhere on the sky see them at the list's clock time_now (mcrat_hip_observe_sky; sky_observers gives
        n, cos_acc, ex, ey from angles).  n, ex, ey: (3, n_obs).  Without x_edges and y_edges -> dict of (n_obs, n_t, n_e) arrays count, w, we, i,
        q, u, v and the per-observer n_accepted, n_outside; with them the arrays are images, (n_obs, n_t, n_e, n_y, n_x) over the sky-plane
        coordinates X = r.ex, Y = r.ey [cm]."""
        return self._observe_sky(self.lib.mcrat_hip_observe_sky, "observe_sky", n, cos_acc, t_edges, e_edges, float(time_now), ex, ey, x_edges, y_edges)

    def pool_observe_sky(self, n, cos_acc, t_edges, e_edges, time_now, ex=None, ey=None, x_edges=None, y_edges=None):
        """every list of the pool in one launch, list r at its own clock time_now[r] (mcrat_hip_pool_observe_sky)"""
        tn = self._pool_clocks("pool_observe_sky", time_now)
        return self._observe_sky(self.lib.mcrat_hip_pool_observe_sky, "pool_observe_sky", n, cos_acc, t_edges, e_edges, tn.ctypes.data_as(_dp), ex, ey,
                                 x_edges, y_edges)

    def observe_sky_path(self):
        """how the last sky observation of this context was accumulated: SKY_PATH_LDS, SKY_PATH_GLOBAL, 0: none yet"""
        return int(self.lib.mcrat_hip_observe_sky_path(self.ctx))

    # ---- escape-weighted sky observations: optical depth as an axis of the cube (include/mcrat_hip.h)
    def _observe_escaping(self, call, what, n, cos_acc, t_edges, e_edges, tau_edges, time_now, step_frac, h_min, max_steps, tau_stop, hydro, ex, ey,
                          x_edges, y_edges):
        sky, _alive, sky_shape, _ = self._sky_observer(what, n, cos_acc, t_edges, e_edges, ex, ey, x_edges, y_edges)
        tau = _f8(tau_edges).ravel()
        n_tau = len(tau) - 1
        obs = EscapeObserver(sky, n_tau, tau.ctypes.data_as(_dp), SightlineParams(float(step_frac), float(h_min), int(max_steps), float(tau_stop), -1.0))
        res, out = self._cube_result((sky_shape[0], max(n_tau, 0)) + sky_shape[1:], EscapeObservation, ESCAPE_SUMS, ESCAPE_COUNTERS)
        self._check(call(self.ctx, hydro.ctx if hydro is not None else None, C.byref(obs), time_now, C.byref(out)), what)
        res.update(n_observable=int(out.n_observable), n_selected=int(out.n_selected), n_status=np.array(list(out.n_status), dtype=np.int64))
        return res

    def observe_escaping(self, n, cos_acc, t_edges, e_edges, tau_edges, time_now, step_frac, h_min, max_steps, tau_stop=np.inf, hydro=None, ex=None, ey=None,
                         x_edges=None, y_edges=None):
        """this list's photons as observe_sky bins them, with their optical depth to the edge of the staged frame as one more axis and the sums
        weighted with exp(-tau) beside the raw ones (mcrat_hip_observe_escaping).  Only the photons that an observer accepts are marched, as
        sightline_photons marches them (step_frac, h_min, max_steps, tau_stop); hydro: another Engine whose staged frame they cross (None: this
        one's).  -> dict of (n_obs, n_tau, n_t, n_e[, n_y, n_x]) arrays count, w, we, i, q, u, v, wx, wex; the per-observer n_accepted, n_outside,
        n_opaque, n_unresolved; n_observable, n_selected and n_status (5,).  escape_fraction(res) gives wx / w."""
        return self._observe_escaping(self.lib.mcrat_hip_observe_escaping, "observe_escaping", n, cos_acc, t_edges, e_edges, tau_edges, float(time_now),
                                      step_frac, h_min, max_steps, tau_stop, hydro, ex, ey, x_edges, y_edges)

    def pool_observe_escaping(self, n, cos_acc, t_edges, e_edges, tau_edges, time_now, step_frac, h_min, max_steps, tau_stop=np.inf, hydro=None, ex=None,
                              ey=None, x_edges=None, y_edges=None):
        """every list of the pool at once, list r at its own clock time_now[r] (mcrat_hip_pool_observe_escaping)"""
        tn = self._pool_clocks("pool_observe_escaping", time_now)
        return self._observe_escaping(self.lib.mcrat_hip_pool_observe_escaping, "pool_observe_escaping", n, cos_acc, t_edges, e_edges, tau_edges,
                                      tn.ctypes.data_as(_dp), step_frac, h_min, max_steps, tau_stop, hydro, ex, ey, x_edges, y_edges)

    def observe_escaping_path(self):
        """how the last escape-weighted observation of this context was accumulated: ESCAPE_PATH_LDS, ESCAPE_PATH_GLOBAL, 0: none yet"""
        return int(self.lib.mcrat_hip_observe_escaping_path(self.ctx))

    # ---- sky polarimetry: observer-frame Stokes sums and a resampling axis (include/mcrat_hip.h)
    def _observe_sky_resampled(self, call, what, n, cos_acc, t_edges, e_edges, time_now, mode, n_rep, stokes_frame, seed, ex, ey, x_edges, y_edges):
        sky, _alive, sky_shape, _ = self._sky_observer(what, n, cos_acc, t_edges, e_edges, ex, ey, x_edges, y_edges)
        obs = ResampleObserver(sky, int(mode), int(n_rep), int(stokes_frame), int(seed) & 0xFFFFFFFFFFFFFFFF)
        res, out = self._cube_result((sky_shape[0], max(int(n_rep), 0)) + sky_shape[1:], ResampleObservation, counters=RESAMPLE_COUNTERS)
        self._check(call(self.ctx, C.byref(obs), time_now, C.byref(out)), what)
        return res

    def observe_sky_resampled(self, n, cos_acc, t_edges, e_edges, time_now, mode=RESAMPLE_JACKKNIFE, n_rep=32, stokes_frame=STOKES_AS_STORED, seed=0,
                              ex=None, ey=None, x_edges=None, y_edges=None):
        """this list's photons as observe_sky bins them, with a replica axis behind the observer -- RESAMPLE_JACKKNIFE: n_rep disjoint groups;
        RESAMPLE_BOOTSTRAP: the sample and n_rep - 1 Poisson(1) resamples; RESAMPLE_NONE: n_rep = 1 -- and, with STOKES_SKY_PLANE, Q and U carried
        into the observer's frame (ex, ey) before they are summed (mcrat_hip_observe_sky_resampled).  -> dict of (n_obs, n_rep, n_t, n_e[, n_y, n_x])
        arrays count, w, we, i, q, u, v and the per-observer n_accepted, n_outside, n_frame_undefined.  resampled_estimates(res, mode) turns it into
        estimates with errors."""
        return self._observe_sky_resampled(self.lib.mcrat_hip_observe_sky_resampled, "observe_sky_resampled", n, cos_acc, t_edges, e_edges, float(time_now),
                                           mode, n_rep, stokes_frame, seed, ex, ey, x_edges, y_edges)

    def pool_observe_sky_resampled(self, n, cos_acc, t_edges, e_edges, time_now, mode=RESAMPLE_JACKKNIFE, n_rep=32, stokes_frame=STOKES_AS_STORED, seed=0,
                                   ex=None, ey=None, x_edges=None, y_edges=None):
        """every list of the pool in one launch, list r at its own clock time_now[r] (mcrat_hip_pool_observe_sky_resampled)"""
        tn = self._pool_clocks("pool_observe_sky_resampled", time_now)
        return self._observe_sky_resampled(self.lib.mcrat_hip_pool_observe_sky_resampled, "pool_observe_sky_resampled", n, cos_acc, t_edges, e_edges,
                                           tn.ctypes.data_as(_dp), mode, n_rep, stokes_frame, seed, ex, ey, x_edges, y_edges)

    def observe_sky_resampled_path(self):
        """how the last resampled sky observation of this context was accumulated: RESAMPLE_PATH_LDS, RESAMPLE_PATH_SLICED, RESAMPLE_PATH_GLOBAL,
        0: none yet"""
        return int(self.lib.mcrat_hip_observe_sky_resampled_path(self.ctx))

    # ---- detected-photon event lists: time-ordered rows per observer (include/mcrat_hip.h)
    def _observe_events(self, call, what, n, cos_acc, time_now, order, stokes_frame, ex, ey, t_window, e_window, capacity):
        t_window, e_window = (t_window or (-np.inf, np.inf)), (e_window or (-np.inf, np.inf))
        sky, _alive, _, _ = self._sky_observer(what, n, cos_acc, [0.0, 1.0], [0.0, 1.0], ex, ey, None, None)
        axes = ex is not None and ey is not None
        obs = EventsObserver(sky.n_obs, sky.n0, sky.n1, sky.n2, sky.cos_acc, sky.x0, sky.x1, sky.x2, sky.y0, sky.y1, sky.y2,
                             float(t_window[0]), float(t_window[1]), float(e_window[0]), float(e_window[1]), int(order), int(stokes_frame), 0)
        n_obs = max(sky.n_obs, 0)

        def one(cap, rows):
            obs.capacity = cap
            res = {"offsets": np.zeros(n_obs + 1, dtype=np.int64)}
            for k in EVENTS_COUNTERS:
                res[k] = np.zeros(n_obs, dtype=np.int64)
            out = Events()
            ll = C.POINTER(C.c_longlong)
            out.offsets = res["offsets"].ctypes.data_as(ll)
            for k in EVENTS_COUNTERS:
                setattr(out, k, res[k].ctypes.data_as(ll))
            if rows:
                m = max(int(cap), 0)
                res["rank"], res["slot"] = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
                out.rank, out.slot = res["rank"].ctypes.data_as(_ip), res["slot"].ctypes.data_as(_ip)
                for k in EVENTS_F8_COLUMNS:
                    if k in ("X", "Y") and not axes:
                        continue
                    res[k] = np.zeros(m)
                    setattr(out, k, res[k].ctypes.data_as(_dp))
                res["type"] = np.zeros(m, dtype="S1")
                out.type = C.cast(res["type"].ctypes.data, C.c_char_p)
            rc = call(self.ctx, C.byref(obs), time_now, C.byref(out))
            res.update(n_total=int(out.n_total), key_or=int(out.key_or), key_and=int(out.key_and), sort_passes_run=int(out.sort_passes_run),
                       sort_passes_skipped=int(out.sort_passes_skipped))
            return rc, res

        if capacity is None:
            rc, counted = one(0, False)
            self._check(rc, what)
            capacity = counted["n_total"]
        rc, res = one(int(capacity), True)
        self.last_events = res                   # (a refused call's counters are exact: kept for the caller that catches the error)
        self._check(rc, what)
        for k in ("rank", "slot", "type") + EVENTS_F8_COLUMNS:
            if k in res:
                res[k] = res[k][:res["n_total"]]
        return res

    def observe_events(self, n, cos_acc, time_now, order=EVENTS_BY_TIME, stokes_frame=STOKES_AS_STORED, ex=None, ey=None, t_window=None, e_window=None,
                       capacity=None):
        """the photons each observer detects as rows (mcrat_hip_observe_events): every accepted (photon, observer) pair with
        t_window[0] <= t_det < t_window[1] and e_window[0] <= e < e_window[1] (None: no bound), observer o's rows at [offsets[o], offsets[o + 1]),
        ordered by (rank, slot) -- EVENTS_BY_PHOTON -- or by (t_det, rank, slot) -- EVENTS_BY_TIME.  n, ex, ey: (3, n_obs) as for observe_sky; with
        ex and ey the rows have X and Y, and STOKES_SKY_PLANE carries s1, s2 into the observer's frame.  capacity: the rows there is room for; None
        asks the device for the count first.  -> dict of the columns rank, slot, t, e, w, s0 .. s3, [X, Y,] num_scatt, type (n_total rows each),
        offsets (n_obs + 1,), the per-observer n_events, n_accepted, n_outside, n_frame_undefined, and n_total, key_or, key_and, sort_passes_run,
        sort_passes_skipped.  A list beyond `capacity` raises McratHipError; its exact counters are in self.last_events.  bin_events and
        event_durations work on the result."""
        return self._observe_events(self.lib.mcrat_hip_observe_events, "observe_events", n, cos_acc, float(time_now), order, stokes_frame, ex, ey, t_window,
                                    e_window, capacity)

    def pool_observe_events(self, n, cos_acc, time_now, order=EVENTS_BY_TIME, stokes_frame=STOKES_AS_STORED, ex=None, ey=None, t_window=None, e_window=None,
                            capacity=None):
        """every list of the pool as one event list, list r at its own clock time_now[r] (mcrat_hip_pool_observe_events)"""
        tn = self._pool_clocks("pool_observe_events", time_now)
        return self._observe_events(self.lib.mcrat_hip_pool_observe_events, "pool_observe_events", n, cos_acc, tn.ctypes.data_as(_dp), order, stokes_frame, ex, ey,
                                    t_window, e_window, capacity)

    # ---- spectral fits: Band function and cutoff power law (include/mcrat_hip.h)
    def fit_spectra(self, count, w, e_edges, model=FIT_BAND, e_piv=FIT_E_PIV, alpha=FIT_DEFAULTS["alpha"], lam=None, beta=FIT_DEFAULTS["beta"],
                    grid=FIT_DEFAULTS["grid"], n_rounds=FIT_DEFAULTS["n_rounds"], shrink=FIT_DEFAULTS["shrink"], min_count=FIT_DEFAULTS["min_count"], log_e=None):
        """every spectrum of (count, w) -- arrays (..., n_e), e_edges (n_e + 1,) in erg -- fitted to FIT_BAND or FIT_COMP on the device
        (mcrat_hip_fit_spectra).  alpha, lam, beta: the (lo, hi) bounds of the search in alpha, lambda = ln(E_pk / e_piv) and beta; lam=None takes
        the edges' range.  grid: the coarse grid's cells (alpha, lambda, beta).  log_e: ln(E_i / e_piv) at the bins' geometric centres, computed here
        with NumPy when None.  -> dict of alpha, beta (NaN for FIT_COMP), e_peak (erg), amplitude, chi2 (float64) and n_used, dof, status (int32),
        each with the input's leading shape.  spectra_from makes the input from an observation, fitted_estimates the error bars from the output."""
        count, w = np.ascontiguousarray(count, dtype=np.int64), _f8(w)
        edges = _f8(e_edges).ravel()
        if count.shape != w.shape or count.ndim < 1:
            raise ValueError("fit_spectra: count and w need the same shape (..., n_e)")
        n_e = count.shape[-1]
        if len(edges) != n_e + 1:
            raise ValueError("fit_spectra: e_edges needs n_e + 1 values")
        with np.errstate(all="ignore"):
            if log_e is None:
                log_e = np.log(np.sqrt(edges[:-1] * edges[1:]) / e_piv)
            if lam is None:
                lam = (np.log(edges[0] / e_piv), np.log(edges[-1] / e_piv))
        log_e = _f8(log_e).ravel()
        if len(log_e) != n_e:
            raise ValueError("fit_spectra: log_e needs n_e values")
        lead = count.shape[:-1]
        n_spec = int(np.prod(lead, dtype=np.int64))
        args = FitArgs(int(model), n_spec, n_e, count.ctypes.data_as(C.POINTER(C.c_longlong)), w.ctypes.data_as(_dp), edges.ctypes.data_as(_dp),
                       log_e.ctypes.data_as(_dp), float(e_piv), float(alpha[0]), float(alpha[1]), float(lam[0]), float(lam[1]), float(beta[0]), float(beta[1]),
                       int(grid[0]), int(grid[1]), int(grid[2]), int(n_rounds), float(shrink), int(min_count))
        res = {k: np.zeros(n_spec) for k in FIT_F8_COLUMNS}
        res.update({k: np.zeros(n_spec, dtype=np.int32) for k in FIT_I4_COLUMNS})
        out = FitResult(*([res[k].ctypes.data_as(_dp) for k in FIT_F8_COLUMNS] + [res[k].ctypes.data_as(_ip) for k in FIT_I4_COLUMNS]))
        self._check(self.lib.mcrat_hip_fit_spectra(self.ctx, C.byref(args), C.byref(out)), "fit_spectra")
        return {k: v.reshape(lead) for k, v in res.items()}

    # ---- line-of-sight optical depths and photospheres (include/mcrat_hip.h)
    def _sightlines(self, what, n, call, step_frac, h_min, max_steps, tau_stop, surface_level):
        par = SightlineParams(float(step_frac), float(h_min), int(max_steps), float(tau_stop), float(surface_level))
        m = max(int(n), 0)
        res = {"tau": np.zeros(m), "path": np.zeros(m), "steps": np.zeros(m, dtype=np.int32), "status": np.zeros(m, dtype=np.int32),
               "surface_step": np.zeros(m, dtype=np.int32), "surface_r": np.zeros((3, m))}
        out = Sightlines(res["tau"].ctypes.data_as(_dp), res["path"].ctypes.data_as(_dp), res["steps"].ctypes.data_as(_ip),
                         res["status"].ctypes.data_as(_ip), res["surface_step"].ctypes.data_as(_ip),
                         *[res["surface_r"][k].ctypes.data_as(_dp) for k in range(3)])
        self._check(call(C.byref(par), C.byref(out)), what)
        res["n_status"] = np.array(list(out.n_status), dtype=np.int64)
        return res

    def sightline_rays(self, r, p, step_frac, h_min, max_steps, tau_stop=np.inf, surface_level=-1.0, hydro=None):
        """optical depth along straight rays through the staged frame (mcrat_hip_sightline_rays).  r: the starting points (r0, r1, r2), p: the
        4-momenta (p0, p1, p2, p3), each a sequence of arrays of one length.  hydro: another Engine whose staged frame the rays cross (None: this
        one's).  -> dict of per-ray arrays tau, path, steps, status (SIGHTLINE_*), surface_step, surface_r (3, n) and n_status (5,)"""
        cols = [_f8(a).ravel() for a in list(r) + list(p)]
        if len(cols) != 7 or any(len(a) != len(cols[0]) for a in cols):
            raise ValueError("sightline_rays: r needs three and p four arrays of one length")
        n, h = len(cols[0]), hydro.ctx if hydro is not None else None
        ptrs = [a.ctypes.data_as(_dp) for a in cols]
        return self._sightlines("sightline_rays", n, lambda par, out: self.lib.mcrat_hip_sightline_rays(self.ctx, h, par, n, *ptrs, out),
                                step_frac, h_min, max_steps, tau_stop, surface_level)

    def sightline_photons(self, step_frac, h_min, max_steps, tau_stop=np.inf, surface_level=-1.0, hydro=None):
        """the same for this list's resident photons, one entry per slot; slots that are not observable come back SIGHTLINE_SKIPPED
        (mcrat_hip_sightline_photons)"""
        h = hydro.ctx if hydro is not None else None
        n = int(self.lib.mcrat_hip_num_photon_slots(self.ctx))
        return self._sightlines("sightline_photons", n, lambda par, out: self.lib.mcrat_hip_sightline_photons(self.ctx, h, par, out),
                                step_frac, h_min, max_steps, tau_stop, surface_level)

    def pool_sightline_photons(self, step_frac, h_min, max_steps, tau_stop=np.inf, surface_level=-1.0, hydro=None):
        """every slot of the pool in one launch, list r from r * (slots per list) on (mcrat_hip_pool_sightline_photons)"""
        h = hydro.ctx if hydro is not None else None
        n = int(self.lib.mcrat_hip_num_photon_slots(self.ctx))
        return self._sightlines("pool_sightline_photons", n, lambda par, out: self.lib.mcrat_hip_pool_sightline_photons(self.ctx, h, par, out),
                                step_frac, h_min, max_steps, tau_stop, surface_level)

    # ---- the radiation field on the hydro mesh: per-cell and per-shell photon moments (include/mcrat_hip.h)
    def _radiation_field(self, call, what, mode, r_edges, mu_edges, hydro):
        h = hydro.ctx if hydro is not None else None
        re_ = _f8(r_edges).ravel() if r_edges is not None else None
        mu = _f8(mu_edges).ravel() if mu_edges is not None else None
        n_r, n_mu = (len(re_) - 1 if re_ is not None else 0), (len(mu) - 1 if mu is not None else 0)
        bins = RadfieldBins(int(mode), n_r, re_.ctypes.data_as(_dp) if re_ is not None else None, n_mu, mu.ctypes.data_as(_dp) if mu is not None else None)
        n_bins = C.c_int(0)
        self._check(self.lib.mcrat_hip_radiation_field_bins(self.ctx, h, C.byref(bins), C.byref(n_bins)), what)
        shape = (n_r, n_mu) if int(mode) == RADFIELD_SHELLS else (n_bins.value,)
        res, out = self._cube_result(shape, Radfield, RADFIELD_PLANES, ())
        self._check(call(self.ctx, h, C.byref(bins), C.byref(out)), what)
        res.update(n_observable=int(out.n_observable), n_unlocated=int(out.n_unlocated), n_outside=int(out.n_outside))
        return res

    def radiation_field(self, mode, r_edges=None, mu_edges=None, hydro=None):
        """this list's photons located in the staged frame (hydro: another Engine's) and summed per hydro cell (RADFIELD_CELLS) or per (r, mu) shell
        (RADFIELD_SHELLS; shell_edges gives mu_edges from polar angles) -> dict of arrays count, w, we_lab, we_comv, w_nscatt, w_temp -- (M,) for
        CELLS, (n_r, n_mu) for SHELLS -- and the counters n_observable, n_unlocated, n_outside (mcrat_hip_radiation_field)"""
        return self._radiation_field(self.lib.mcrat_hip_radiation_field, "radiation_field", mode, r_edges, mu_edges, hydro)

    def pool_radiation_field(self, mode, r_edges=None, mu_edges=None, hydro=None):
        """every list of the pool in one launch (mcrat_hip_pool_radiation_field)"""
        return self._radiation_field(self.lib.mcrat_hip_pool_radiation_field, "pool_radiation_field", mode, r_edges, mu_edges, hydro)

    def radiation_field_path(self):
        """how the last radiation field of this context was accumulated: RADFIELD_PATH_LDS, RADFIELD_PATH_GLOBAL, 0: none yet"""
        return int(self.lib.mcrat_hip_radiation_field_path(self.ctx))

    # ---- the comoving radiation field: fluid-frame spectra, beaming and Eddington moments (include/mcrat_hip.h)
    def _comoving_field(self, call, what, mode, e_edges, a_edges, r_edges, mu_edges, hydro):
        h = hydro.ctx if hydro is not None else None
        axes = [_f8(x).ravel() if x is not None else None for x in (r_edges, mu_edges, e_edges, a_edges)]
        n_ax = [len(x) - 1 if x is not None else 0 for x in axes]
        ptr = [x.ctypes.data_as(_dp) if x is not None else None for x in axes]
        bins = ComovingBins(int(mode), n_ax[0], ptr[0], n_ax[1], ptr[1], n_ax[2], ptr[2], n_ax[3], ptr[3])
        n_bins = C.c_int(0)
        self._check(self.lib.mcrat_hip_comoving_field_bins(self.ctx, h, C.byref(bins), C.byref(n_bins)), what)
        per_s = n_ax[2] * n_ax[3]
        shape = (n_ax[0], n_ax[1], n_ax[2], n_ax[3]) if int(mode) == COMOVING_SHELLS else (n_bins.value // per_s, n_ax[2], n_ax[3])
        res, out = self._cube_result(shape, Comoving, COMOVING_PLANES, ())
        self._check(call(self.ctx, h, C.byref(bins), C.byref(out)), what)
        res.update(n_observable=int(out.n_observable), n_unlocated=int(out.n_unlocated), n_outside=int(out.n_outside))
        return res

    def comoving_field(self, mode, e_edges, a_edges, r_edges=None, mu_edges=None, hydro=None):
        """this list's photons located in the staged frame (hydro: another Engine's), boosted into their cell's frame and binned by position --
        hydro cell (COMOVING_CELLS) or (r, mu) shell (COMOVING_SHELLS) --, fluid-frame energy [erg] and fluid-frame cosine about the flow
        (cosine_edges gives a_edges) -> dict of arrays count, w, we, wea, weaa, we_lab, wem, wemm -- (M, n_e, n_a) for CELLS, (n_r, n_mu, n_e, n_a)
        for SHELLS -- and the counters n_observable, n_unlocated, n_outside (mcrat_hip_comoving_field); eddington_moments takes the dict"""
        return self._comoving_field(self.lib.mcrat_hip_comoving_field, "comoving_field", mode, e_edges, a_edges, r_edges, mu_edges, hydro)

    def pool_comoving_field(self, mode, e_edges, a_edges, r_edges=None, mu_edges=None, hydro=None):
        """every list of the pool in one launch (mcrat_hip_pool_comoving_field)"""
        return self._comoving_field(self.lib.mcrat_hip_pool_comoving_field, "pool_comoving_field", mode, e_edges, a_edges, r_edges, mu_edges, hydro)

    def comoving_field_path(self):
        """how the last comoving field of this context was accumulated: COMOVING_PATH_LDS, COMOVING_PATH_GLOBAL, 0: none yet"""
        return int(self.lib.mcrat_hip_comoving_field_path(self.ctx))

    def synchronize(self):
        self._check(self.lib.mcrat_hip_synchronize(self.ctx), "synchronize")

    def device_bytes(self):
        return int(self.lib.mcrat_hip_device_bytes(self.ctx))

    FN = dict(kn_cross_section=(1, 1, 1), lorentz_boost_photon=(2, 7, 4), lorentz_boost_electron=(3, 7, 4), stokes_rotation=(4, 13, 4),
              thermal_electron=(5, 5, 4), thermal_electron_wave=(6, 5, 4), electron_and_scatter=(7, 9, 13),
              # the loop's own arithmetic forms (include/mcrat_hip.h; tests/test_gpu_loop_arithmetic.py)
              rcp_nr=(8, 1, 1), rsqrt_nr=(9, 1, 1), sqrt_nr=(10, 1, 1), cell_operands=(11, 5, 5), boost_with_photon=(12, 9, 4),
              boost_with_electron=(13, 9, 4), boost_staged_photon=(14, 7, 4), optical_depth_staged=(15, 9, 2), azimuth=(16, 2, 4),
              hydro_coords=(17, 3, 3), thermal_cross_section=(18, 2, 4), kn_cross_section_ieee=(19, 1, 1))

    def eval_function(self, name, rows, seed=0):
        """one device function of physics.hpp on an array of argument rows (mcrat_hip_eval_function); returns the result rows"""
        fn, wi, wo = self.FN[name]
        a = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, wi)
        out = np.empty((a.shape[0], wo))
        self._check(self.lib.mcrat_hip_eval_function(self.ctx, fn, a.shape[0], a.ctypes.data_as(_dp), out.ctypes.data_as(_dp), int(seed)), "eval_function")
        return out

    def covered_octants(self):
        """the staged frame's covered-octant table, one int32 per lookup bucket and octant (cell index or -1); empty: the frame's grid has none"""
        n = int(self.lib.mcrat_hip_covered_octants(self.ctx, None, 0))
        self._check(min(n, 0), "covered_octants")
        out = np.empty(n, dtype=np.int32)
        if n:
            self._check(min(int(self.lib.mcrat_hip_covered_octants(self.ctx, out.ctypes.data_as(_ip), n)), 0), "covered_octants")
        return out

    def lookup_cell(self, a0, a1, a2=None):
        a0, a1 = _f8(a0), _f8(a1)
        a2p = _f8(a2) if a2 is not None else None
        out = np.empty(len(a0), dtype=np.int32)
        self._check(self.lib.mcrat_hip_lookup_cell(self.ctx, len(a0), a0.ctypes.data_as(_dp), a1.ctypes.data_as(_dp),
                                                   a2p.ctypes.data_as(_dp) if a2p is not None else None,
                                                   out.ctypes.data_as(_ip)), "lookup_cell")
        return out
