"""An independent NumPy restatement of the escape-weighted sky observation (include/mcrat_hip.h), for tests/test_gpu_escape.py,
tests/test_escape_checker_cpu.py and tests/test_escape_plan_cpu.py.  Built on the two checkers that exist -- tests/sky_checker.py for acceptance,
detection time, energy and sky-plane position, tests/sightline_checker.py for the march, its error bound and its fragile marks -- and not a copy of
the kernels: whole-array expressions in the definitions' order, bins from np.searchsorted, per-bin sums with math.fsum and sum|term| beside them.

Bounds, derived, not measured:
    raw sums (W, WE, I, Q, U, V)     |device - fsum| <= (m + 2) 2^-53 sum|term|                      (m terms in the bin; tests/sky_checker.py)
    WX, WEX                          ... + sum_k |term_k| (bound_k + 3 2^-53)
bound_k is the sightline checker's bound on photon k's tau: exp turns an absolute error of tau into a relative error of exp(-tau); 3 2^-53 covers the
two exp implementations and the product.

fragile: a marched photon that the sightline checker marks, or a LEFT_MESH photon whose tau lies within its bound of a tau edge -- the device's tau may
fall on the other side.  tau == 0 with bound 0 (a photon that starts outside the frame) is not fragile: the device must give exactly 0."""
import math

import numpy as np

from tests import sightline_checker as sc
from tests import sky_checker as S

U = S.U
RAW = tuple(k for k, _ in S.PLANES)                 # w, we, i, q, u, v
WEIGHTED = ("wx", "wex")
PLANES = RAW + WEIGHTED
COUNTERS = ("n_accepted", "n_outside", "n_opaque", "n_unresolved")
TAU_EDGES = np.array([0.0, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0])


def rays_of(ph):
    """the photons' positions (3, n) and momenta (4, n), as the sightline checker takes rays"""
    return np.stack([ph["r0"], ph["r1"], ph["r2"]]), np.stack([ph["p0"], ph["p1"], ph["p2"], ph["p3"]])


def observation(ph, marched, n, cos_acc, t_edges, e_edges, tau_edges, time_now, ex=None, ey=None, x_edges=None, y_edges=None, stokes=True):
    """ph: a synth photon dict; marched: sightline_checker.march's answer for rays_of(ph) with the call's four march parameters (its surface outputs
    are not read; what it says of photons that nobody accepts is not read either).
    -> dict: count, the eight sums, abs_<sum> (sum|term|) and, for wx and wex, tol_<sum> (sum |term| (bound + 3u)), each (n_obs, n_tau, n_t, n_e[, n_y,
    n_x]); the four per-observer counters; n_observable, n_selected, n_status (5,); per photon: selected, tau, status, bound, fragile; bin: the flat
    bin per (observer, photon) within the observer's part of the cube, -1 where there is none"""
    q = S.per_photon(ph, n, cos_acc, t_edges, e_edges, time_now, ex, ey, x_edges, y_edges)
    tau_edges = np.asarray(tau_edges, dtype=np.float64)
    image = x_edges is not None
    acc = q["accepted"]
    n_obs, n_ph = acc.shape
    n_tau, n_t, n_e = len(tau_edges) - 1, len(t_edges) - 1, len(e_edges) - 1
    n_x, n_y = (len(x_edges) - 1, len(y_edges) - 1) if image else (1, 1)
    shape = (n_obs, n_tau, n_t, n_e, n_y, n_x) if image else (n_obs, n_tau, n_t, n_e)
    per_obs = n_tau * n_t * n_e * n_y * n_x

    w = np.asarray(ph["weight"], dtype=np.float64)
    typ = np.asarray(ph["type"], dtype="S1")
    observable = (w != 0) & (typ != b"p") & (typ != b"N")
    selected = acc.any(axis=0)
    tau = np.where(selected, marched["tau"], np.nan)
    status = np.where(selected, marched["status"], sc.SKIPPED)
    bound = np.where(selected, marched["bound"], 0.0)
    left = status == sc.LEFT_MESH
    itau = S.find_bin(tau_edges, tau)
    with np.errstate(invalid="ignore"):
        near_edge = (np.abs(tau[None, :] - tau_edges[:, None]) <= bound[None, :]).any(axis=0) & ~((tau == 0) & (bound == 0))
    fragile = selected & (np.asarray(marched["fragile"], dtype=bool) | (left & near_edge))

    inside = q["inside"] & left[None, :] & (itau >= 0)[None, :]
    flat = np.where(inside, (((itau[None, :] * n_t + q["it"]) * n_e + q["ie"]) * n_y + q["iy"]) * n_x + q["ix"], -1)
    want = {"n_accepted": acc.sum(axis=1).astype(np.int64), "n_outside": (acc & left[None, :] & ~inside).sum(axis=1).astype(np.int64),
            "n_opaque": (acc & (status == sc.OPAQUE)[None, :]).sum(axis=1).astype(np.int64),
            "n_unresolved": (acc & ((status == sc.STEP_CAP) | (status == sc.OFF_TABLE))[None, :]).sum(axis=1).astype(np.int64),
            "n_observable": int(observable.sum()), "n_selected": int(selected.sum()),
            "n_status": np.bincount(status[selected], minlength=5).astype(np.int64),
            "selected": selected, "tau": tau, "status": status, "bound": bound, "fragile": fragile, "bin": flat,
            "count": np.zeros((n_obs, per_obs), dtype=np.int64)}
    with np.errstate(invalid="ignore"):
        x = np.exp(-tau)
    terms = {"w": w, "we": w * q["e"][0]}
    for k, c in S.PLANES[2:]:
        terms[k] = w * np.asarray(ph[c], dtype=np.float64) if stokes else np.zeros_like(w)
    terms["wx"] = w * x
    terms["wex"] = (w * q["e"][0]) * x
    for k in PLANES:
        want[k] = np.zeros((n_obs, per_obs))
        want["abs_" + k] = np.zeros((n_obs, per_obs))
    for k in WEIGHTED:
        want["tol_" + k] = np.zeros((n_obs, per_obs))
    for o in range(n_obs):
        idx = np.nonzero(inside[o])[0]
        idx = idx[np.argsort(flat[o, idx], kind="stable")]
        b = flat[o, idx]
        starts = np.nonzero(np.diff(b, prepend=-1))[0]
        for s, t in zip(starts, list(starts[1:]) + [len(b)]):
            members = idx[s:t]
            want["count"][o, b[s]] = t - s
            for k in PLANES:
                want[k][o, b[s]] = math.fsum(terms[k][members])
                want["abs_" + k][o, b[s]] = math.fsum(np.abs(terms[k][members]))
            for k in WEIGHTED:
                want["tol_" + k][o, b[s]] = math.fsum(np.abs(terms[k][members]) * (bound[members] + 3 * U))
    for k in ["count"] + list(PLANES) + ["abs_" + p for p in PLANES] + ["tol_" + p for p in WEIGHTED]:
        want[k] = want[k].reshape(shape)
    return want


def identities(res, label=""):
    """per observer: the bins' counts and the three other fates add up to the accepted; per call: the marched rays per status add up to the selected"""
    n_obs = len(res["n_accepted"])
    assert np.array_equal(res["count"].reshape(n_obs, -1).sum(axis=1) + res["n_outside"] + res["n_opaque"] + res["n_unresolved"], res["n_accepted"]), label
    assert res["n_status"][0] == 0 and res["n_status"][1:].sum() == res["n_selected"] <= res["n_observable"], label


def compare(res, want, label="", exact_only=False):
    """the issue's assertions: every counter and the count plane exact for photons that are not fragile -- with f <= 1 fragile photons the count cubes
    may differ in at most 2 f entries by 1 each --, both identities, raw sums within (m + 2) u sum|term|, WX and WEX within that plus
    sum |term| (bound + 3u); the largest error / bound is printed"""
    f = int(want["fragile"].sum())
    assert f <= 1, (label, f)
    identities(res, label)
    identities(want, label)
    for k in ("n_observable", "n_selected"):
        assert res[k] == want[k], (label, k, res[k], want[k])
    assert np.array_equal(res["n_accepted"], want["n_accepted"]), (label, "n_accepted")
    assert res["count"].shape == want["count"].shape, (label, res["count"].shape, want["count"].shape)
    diff = res["count"] - want["count"]
    if f == 0:
        assert not diff.any(), (label, "count", int(res["count"].sum()), int(want["count"].sum()))
        for k in COUNTERS + ("n_status",):
            assert np.array_equal(res[k], want[k]), (label, k, res[k], want[k])
    else:
        # a fragile photon's tau may fall on the other side of a tau edge: it moves between two neighbouring tau bins of the same (o, t, e[, y, x]),
        # so at most 2 f entries differ, by 1 each, and the counts summed over tau are still exact; the other counters can differ by at most f
        assert (diff != 0).sum() <= 2 * f and np.abs(diff).max(initial=0) <= 1, (label, "count with a fragile photon")
        assert np.array_equal(res["count"].sum(axis=1), want["count"].sum(axis=1)), (label, "tau-summed counts with a fragile photon")
        for k in ("n_outside", "n_opaque", "n_unresolved", "n_status"):
            assert np.abs(res[k] - want[k]).max(initial=0) <= f, (label, k, res[k], want[k])
    if exact_only:
        return
    m = want["count"].astype(np.float64)
    same = diff == 0
    for k in PLANES:
        bound = (m + 2.0) * U * want["abs_" + k] + (want["tol_" + k] if k in WEIGHTED else 0.0)
        err = np.where(same, np.abs(res[k] - want[k]), 0.0)
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
        print("%s %s: largest error / bound = %.3g over %d bins in use" % (label, k, worst, int((m > 0).sum())))
        assert (err <= bound).all(), (label, k, worst)


# ---------------------------------------------------------------------------------------------- the cases of the CPU and the GPU test
# The sightline checker's cases (16 x 16 and 8 x 8 x 8 meshes around r = 1e12 cm on the polar axis), their rays placed as resident photons.  Three
# observers: the polar axis and two directions within 0.15 rad of it, with cones of 0.15 to 0.5 rad, so that a real fraction of the photons -- which
# head within 0.5 rad of their radial direction, one in ten anywhere -- is accepted by none, by one and by several.  The lists' clock is 40 s; the
# photons sit at r.n / c = 33 .. 39 s, so they are detected between 1 and 7 s: ten 1-s bins from 0 s hold them (T_EDGES), and ten from 30 s hold none
# (T_EDGES_LATE: every LEFT_MESH photon an observer accepts is then outside).  Energies: p0 c of p0 = 1e-20 .. 1e-16 g cm/s lies within 1e-10 .. 1e-5
# erg; the TABLE cases' softer photons lie partly below.
TIME_NOW = 40.0
T_EDGES = np.arange(0.0, 11.0)
T_EDGES_LATE = np.arange(30.0, 41.0)
E_EDGES = 10.0 ** np.linspace(-10.0, -5.0, 6)
X_EDGES = np.linspace(-2.0e11, 2.0e11, 9)
Y_EDGES = np.linspace(-2.0e11, 2.0e11, 7)
GPU_CASES = (["uniform_n%d" % n for n in (1, 63, 65, 1000)] + ["pair_%d_%d" % pair for pair in sc.PAIRS] +
             ["gap", "opaque", "cap_1", "cap_7", "photons", "larger_frame", "table_in", "table_off", "table_cold"])


def observers():
    """(n, cos_acc, ex, ey): the polar axis with a cone of 0.15 rad, and two directions 0.1 and 0.14 rad off it with cones of 0.3 and 0.5 rad"""
    return S.observers([0.0, 0.1, 0.14], [0.0, 0.7, 3.5], [0.15, 0.3, 0.5])


def march_params(params):
    """a sightline case's parameters without the surface level, which this product does not read"""
    return {k: v for k, v in params.items() if k != "surface_level"}


def photons_of(c, seed, first=0, count=None, exclusions=True):
    """the rays [first, first + count) of a sightline case as a synth photon dict (weights over three decades, Stokes components of both signs); with
    exclusions about three in ten are slots that do not count: weight 0, type 'p', type 'N'"""
    sl = slice(first, None if count is None else first + count)
    ph = S.photon_list(c["r"][:, sl], c["p"][:, sl], seed)
    if exclusions:
        kind = np.random.default_rng(seed + 77).integers(0, 10, len(ph["weight"]))
        ph["weight"][kind == 0] = 0.0
        ph["type"][kind == 1] = b"p"
        ph["type"][kind == 2] = b"N"
        ph["type"][kind == 3] = b"c"                   # other types count
    return ph


def marched_slice(want, first=0, count=None):
    sl = slice(first, None if count is None else first + count)
    return {k: want[k][sl] for k in ("tau", "status", "bound", "fragile")}


_CASES = {}


def case(name, exclusions=True):
    """the sightline case `name` as resident photons and the checker's answer for the three observers without image axes, computed once per process:
    dict(c = the sightline case, ph, want)"""
    key = (name, exclusions)
    if key not in _CASES:
        c = sc.case(name)
        ph = photons_of(c, 7000 + len(name), exclusions=exclusions)
        n, cos_acc, _, _ = observers()
        want = observation(ph, marched_slice(c["want"]), n, cos_acc, T_EDGES, E_EDGES, TAU_EDGES, TIME_NOW)
        _CASES[key] = dict(c=c, ph=ph, want=want)
    return _CASES[key]


def add(results):
    """several observations of one binning added up: counts, sums, their bounds' terms and the counters (per-photon entries are dropped)"""
    per_photon = ("selected", "tau", "status", "bound", "fragile", "bin")
    out = {k: sum(r[k] for r in results[1:]) + v for k, v in results[0].items() if k not in per_photon}
    out["fragile"] = np.concatenate([r["fragile"] for r in results])
    return out
