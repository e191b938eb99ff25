"""An independent NumPy restatement of the sky observers (include/mcrat_hip.h), for tests/test_gpu_sky.py and
tests/test_sky_checker_cpu.py.  Not a copy of the kernel: the per-photon quantities are whole-array expressions in the definitions' order (so that
what decides a bin is comparable bit for bit), the bins come from np.searchsorted, and the per-bin sums are taken with math.fsum -- exact sums,
correctly rounded -- with sum|term| kept beside them for the bound

    |device sum - fsum| <= (m + 2) * 2**-53 * sum|term|        (m terms in the bin)

the worst case of adding m equal-bits terms in any order (m - 1 roundings of partial sums no larger than sum|term|) plus room for the final
roundings; derived, not measured."""
import math

import numpy as np

C_LIGHT = 2.99792458e10
U = 2.0 ** -53
PLANES = (("w", None), ("we", "e"), ("i", "s0"), ("q", "s1"), ("u", "s2"), ("v", "s3"))


def observers(theta, phi, half_angle):
    """(n, cos_acc, ex, ey) of observers at (theta, phi) [radians] with cones of half_angle: n towards the observer, ex = theta_hat, ey = phi_hat"""
    th, ph, half = np.broadcast_arrays(*(np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (theta, phi, half_angle)))
    n = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    ex = np.stack([np.cos(th) * np.cos(ph), np.cos(th) * np.sin(ph), -np.sin(th)])
    ey = np.stack([-np.sin(ph), np.cos(ph), 0.0 * ph])
    return n, np.cos(half), ex, ey


def find_bin(edges, x):
    """edges[k] <= x < edges[k + 1], else -1 (a NaN is in no bin)"""
    edges = np.asarray(edges, dtype=np.float64)
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1) & (x == x), k, -1)


def per_photon(ph, n, cos_acc, t_edges, e_edges, time_now, ex=None, ey=None, x_edges=None, y_edges=None):
    """-> dict of (n_obs, n_photons) arrays: accepted, t, e, X, Y (NaN without image axes), it, ie, ix, iy (0 without image axes), inside"""
    col = lambda k: np.asarray(ph[k], dtype=np.float64)[None, :]
    p0, p1, p2, p3, r0, r1, r2, w = (col(k) for k in ("p0", "p1", "p2", "p3", "r0", "r1", "r2", "weight"))
    typ = np.asarray(ph["type"], dtype="S1")[None, :]
    n = np.asarray(n, dtype=np.float64).reshape(3, -1)
    n0, n1, n2 = (n[k][:, None] for k in range(3))
    ca = np.asarray(cos_acc, dtype=np.float64).ravel()[:, None]
    tn = np.broadcast_to(np.asarray(time_now, dtype=np.float64), p0.shape[1:])[None, :]
    observable = (w != 0) & (typ != b"p") & (typ != b"N")
    with np.errstate(invalid="ignore", over="ignore"):
        acc = observable & (((p1 * n0 + p2 * n1) + p3 * n2) >= p0 * ca)
        e = np.broadcast_to(p0 * C_LIGHT, acc.shape)
        t = tn - (((r0 * n0 + r1 * n1) + r2 * n2) / C_LIGHT)
        out = dict(accepted=acc, t=t, e=e, it=find_bin(t_edges, t), ie=find_bin(e_edges, e))
        if x_edges is not None:
            ex, ey = np.asarray(ex, dtype=np.float64).reshape(3, -1), np.asarray(ey, dtype=np.float64).reshape(3, -1)
            X = (r0 * ex[0][:, None] + r1 * ex[1][:, None]) + r2 * ex[2][:, None]
            Y = (r0 * ey[0][:, None] + r1 * ey[1][:, None]) + r2 * ey[2][:, None]
            out.update(X=X, Y=Y, ix=find_bin(x_edges, X), iy=find_bin(y_edges, Y))
        else:
            out.update(X=np.full(acc.shape, np.nan), Y=np.full(acc.shape, np.nan), ix=np.zeros(acc.shape, dtype=np.int64), iy=np.zeros(acc.shape, dtype=np.int64))
    out["inside"] = acc & (out["it"] >= 0) & (out["ie"] >= 0) & (out["ix"] >= 0) & (out["iy"] >= 0)
    return out


def observation(ph, n, cos_acc, t_edges, e_edges, time_now, ex=None, ey=None, x_edges=None, y_edges=None, stokes=True):
    """-> dict: count, the six sums and abs_<sum> (sum|term|), each (n_obs, n_t, n_e[, n_y, n_x]); n_accepted, n_outside (n_obs,); bin, the flat bin
    per (observer, photon) within the observer's part of the cube, -1 where there is none"""
    q = per_photon(ph, n, cos_acc, t_edges, e_edges, time_now, ex, ey, x_edges, y_edges)
    image = x_edges is not None
    n_obs, n_t, n_e = q["accepted"].shape[0], len(t_edges) - 1, len(e_edges) - 1
    n_x, n_y = (len(x_edges) - 1, len(y_edges) - 1) if image else (1, 1)
    shape = (n_obs, n_t, n_e, n_y, n_x) if image else (n_obs, n_t, n_e)
    per_obs = n_t * n_e * n_y * n_x
    flat = np.where(q["inside"], ((q["it"] * n_e + q["ie"]) * n_y + q["iy"]) * n_x + q["ix"], -1)
    want = {"n_accepted": q["accepted"].sum(axis=1).astype(np.int64), "n_outside": (q["accepted"] & ~q["inside"]).sum(axis=1).astype(np.int64),
            "count": np.zeros((n_obs, per_obs), dtype=np.int64), "bin": flat}
    w = np.asarray(ph["weight"], dtype=np.float64)
    terms = {"w": w, "we": w * q["e"][0]}
    for k, c in PLANES[2:]:
        terms[k] = w * np.asarray(ph[c], dtype=np.float64) if stokes else np.zeros_like(w)
    for k, _ in PLANES:
        want[k] = np.zeros((n_obs, per_obs))
        want["abs_" + k] = np.zeros((n_obs, per_obs))
    for o in range(n_obs):
        idx = np.nonzero(q["inside"][o])[0]
        order = np.argsort(flat[o, idx], kind="stable")
        idx = idx[order]
        b = flat[o, idx]
        starts = np.nonzero(np.diff(b, prepend=-1))[0]
        for s, t in zip(starts, list(starts[1:]) + [len(b)]):
            members = idx[s:t]
            want["count"][o, b[s]] = t - s
            for k, _ in PLANES:
                want[k][o, b[s]] = math.fsum(terms[k][members])
                want["abs_" + k][o, b[s]] = math.fsum(np.abs(terms[k][members]))
    for k in ["count"] + [p for p, _ in PLANES] + ["abs_" + p for p, _ in PLANES]:
        want[k] = want[k].reshape(shape)
    return want


def compare(res, want, label="", exact_only=False):
    """counts and counters exactly; each sum within (m + 2) * 2**-53 * sum|term| of the checker's (an empty bin: the device's plane must hold 0)"""
    for k in ("n_accepted", "n_outside", "count"):
        assert res[k].shape == want[k].shape, (label, k, res[k].shape, want[k].shape)
        assert np.array_equal(res[k], want[k]), (label, k, int(res[k].sum()), int(want[k].sum()))
    assert np.array_equal(want["count"].reshape(len(want["n_accepted"]), -1).sum(axis=1), want["n_accepted"] - want["n_outside"])
    if exact_only:
        return
    m = want["count"].astype(np.float64)
    for k, _ in PLANES:
        bound = (m + 2.0) * U * want["abs_" + k]
        err = np.abs(res[k] - want[k])
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
        print("%s %s: largest error / bound = %.3g over %d bins in use" % (label, k, worst, int((m > 0).sum())))
        assert (err <= bound).all(), (label, k, worst)


def add(results):
    """several observations of one binning added up: counts, sums, sum|term| and counters (the per-photon `bin` is dropped)"""
    return {k: sum(r[k] for r in results[1:]) + v for k, v in results[0].items() if k != "bin"}


# ---------------------------------------------------------------------------------------------- photons
def photon_list(r, p, seed):
    """a synth photon dict at the positions r (3, n) with the momenta p (4, n): weights over three decades, Stokes components of both signs"""
    n = r.shape[1]
    g = np.random.default_rng(seed)
    ph = {"r0": r[0].copy(), "r1": r[1].copy(), "r2": r[2].copy(), "p0": p[0].copy(), "p1": p[1].copy(), "p2": p[2].copy(), "p3": p[3].copy(),
          "s0": np.ones(n), "s1": g.uniform(-1.0, 1.0, n), "s2": g.uniform(-1.0, 1.0, n), "s3": g.uniform(-1.0, 1.0, n),
          "weight": 10.0 ** g.uniform(48.0, 51.0, n), "num_scatt": np.floor(g.uniform(0.0, 30.0, n)),
          "time_to_scatter": np.zeros(n), "total_optical_depth": np.ones(n),
          "type": np.full(n, b"i", dtype="S1"), "nearest_block_index": np.zeros(n, dtype=np.int32), "recalc_properties": np.ones(n, dtype=np.int32)}
    for k in ("comv_p0", "comv_p1", "comv_p2", "comv_p3"):
        ph[k] = ph[k[5:]].copy()
    return ph


def jet_photons(seed, n, opening=0.5):
    """a 3-D outflow about the r2 axis that is not axisymmetric: r ~ 1e12 .. 1e13 cm within `opening` of the axis, twice as many photons at
    azimuths near 0 as near pi, each moving within ~0.15 rad of its own radial direction, p0 log-uniform over six decades"""
    g = np.random.default_rng(seed)
    r = 10.0 ** g.uniform(12.0, 13.0, n)
    th = opening * np.sqrt(g.uniform(0.0, 1.0, n))
    phi = np.where(g.uniform(0, 1, n) < 2.0 / 3.0, g.normal(0.0, 1.0, n), g.uniform(0.0, 2 * np.pi, n))
    rhat = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)])
    d = rhat + 0.1 * g.standard_normal((3, n))
    d /= np.sqrt((d * d).sum(axis=0))
    p0 = 10.0 ** g.uniform(-20.0, -14.0, n)
    pv = p0 * d
    return photon_list(r * rhat, np.stack([np.sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]), pv[0], pv[1], pv[2]]), seed + 1)


def concatenate(lists):
    return {k: np.concatenate([ph[k] for ph in lists]) for k in lists[0]}
