"""An independent NumPy restatement of the resampled sky observation (include/mcrat_hip.h), for tests/test_gpu_resample.py,
tests/test_resample_plan_cpu.py and tests/test_resample_checker_cpu.py: Philox4x32-10 and the keyed block, the multiplicities of the three modes,
the Stokes rotation into the observer's frame, and the binning with the replica axis.  Acceptance, t_det, e, (X, Y) and the bins within one
(observer, replica) are tests/sky_checker.py's.  Not a copy of the kernel: whole-array expressions in the definitions' order, so that what decides a
count is comparable exactly and a term bit for bit; the per-bin sums are math.fsum's of the terms k * term, with sum|k * term| beside them for

    |device sum - fsum| <= (m + 2) * 2**-53 * sum|k * term|        (m terms k * term with k > 0 in the bin)

the bound of tests/sky_checker.py, derived there."""
import math

import numpy as np

from tests import sky_checker as S

NONE, JACKKNIFE, BOOTSTRAP = 0, 1, 2
AS_STORED, SKY_PLANE = 0, 1
RNG_RESAMPLE = 2
U = S.U
PLANES = S.PLANES
# T_m = floor(2**32 * sum_{i <= m} exp(-1) / i!), m = 0 .. 11 (tests/test_resample_checker_cpu.py recomputes them with 50 digits)
THRESHOLDS = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463, 4294966817, 4294967252,
              4294967292)
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------- Philox4x32-10 (Salmon et al., SC'11)
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """counter words and key words as arrays (or scalars) below 2**32 -> four arrays of uint64 below 2**32"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        prod0, prod1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2           # 32 x 32 bits: no wrap in 64
        c0, c1, c2, c3 = (prod1 >> np.uint64(32)) ^ c1 ^ k0, prod1 & M32, (prod0 >> np.uint64(32)) ^ c3 ^ k1, prod0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def block(seed, rank, slot, number, mode):
    """the four words of keyed_block(seed, slot | rank << 32, number, RNG_RESAMPLE, mode)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10(slot, rank, number, RNG_RESAMPLE | (int(mode) << 8), seed & 0xFFFFFFFF, seed >> 32)


def group(seed, rank, slot, G):
    """the jackknife group of each photon: (w[0] * G) >> 32 of block 0"""
    return ((block(seed, rank, slot, 0, JACKKNIFE)[0] * np.uint64(G)) >> np.uint64(32)).astype(np.int64)


def poisson(word):
    """k = #{m : word >= T_m}"""
    word = np.asarray(word, dtype=np.uint64)
    return sum((word >= np.uint64(t)).astype(np.int64) for t in THRESHOLDS)


def multiplicities(mode, seed, rank, slot, n_rep):
    """k[rho, photon], (n_rep, n) integers"""
    rank, slot = np.broadcast_arrays(np.asarray(rank, dtype=np.uint64), np.asarray(slot, dtype=np.uint64))
    n = slot.shape[0]
    if mode == NONE:
        assert n_rep == 1
        return np.ones((1, n), dtype=np.int64)
    if mode == JACKKNIFE:
        return (group(seed, rank, slot, n_rep)[None, :] == np.arange(n_rep)[:, None]).astype(np.int64)
    assert mode == BOOTSTRAP
    k = np.ones((n_rep, n), dtype=np.int64)
    for rho in range(1, n_rep):
        j = rho - 1
        k[rho] = poisson(block(seed, rank, slot, j >> 2, BOOTSTRAP)[j & 3])
    return k


# ---------------------------------------------------------------------------------------------- the Stokes rotation
def rotation(p1, p2, p3, ey0, ey1, ey2, Q, Uq):
    """(Q', U', undefined): the photon's (Q, U) in the observer's frame, the operations in the header's order; where h is 0 or not finite the pair is
    returned as stored and flagged"""
    p1, p2, p3, ey0, ey1, ey2, Q, Uq = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (p1, p2, p3, ey0, ey1, ey2, Q, Uq)))
    with np.errstate(all="ignore"):
        rho2 = p1 * p1 + p2 * p2
        pn = np.sqrt(rho2 + p3 * p3)
        d = p2 * ey0 - p1 * ey1
        s = (rho2 * ey2 - p3 * (p1 * ey0 + p2 * ey1)) / pn
        h = np.sqrt(d * d + s * s)
        undefined = ~((h > 0.0) & np.isfinite(h))
        c, sg = d / h, s / h
        c2 = c * c - sg * sg
        s2 = (-2.0 * sg) * c
        q = Q * c2 - Uq * s2
        u = Q * s2 + Uq * c2
    return np.where(undefined, Q, q), np.where(undefined, Uq, u), undefined


# ---------------------------------------------------------------------------------------------- the observation
def observation(ph, n, cos_acc, t_edges, e_edges, time_now, mode, n_rep, frame=AS_STORED, seed=0, rank=0, slot=None, ex=None, ey=None, x_edges=None,
                y_edges=None, stokes=True):
    """-> dict: count, the six sums, abs_<sum> (sum|k * term|) and terms (the bin's contributions with k > 0), each (n_obs, n_rep, n_t, n_e[, n_y,
    n_x]); n_accepted, n_outside, n_frame_undefined (n_obs,).  rank, slot: the photons' identities (slot None: their index)."""
    image = x_edges is not None
    q = S.per_photon(ph, n, cos_acc, t_edges, e_edges, time_now, ex if image else None, ey if image else None, x_edges, y_edges)
    n_obs, n_ph = q["accepted"].shape
    n_t, n_e = len(t_edges) - 1, len(e_edges) - 1
    n_x, n_y = (len(x_edges) - 1, len(y_edges) - 1) if image else (1, 1)
    shape = (n_obs, n_rep, n_t, n_e, n_y, n_x) if image else (n_obs, n_rep, n_t, n_e)
    per_rep = n_t * n_e * n_y * n_x
    flat = np.where(q["inside"], ((q["it"] * n_e + q["ie"]) * n_y + q["iy"]) * n_x + q["ix"], -1)
    slot = np.arange(n_ph) if slot is None else np.asarray(slot)
    k = multiplicities(mode, seed, np.broadcast_to(np.asarray(rank), (n_ph,)), slot, n_rep)
    w = np.asarray(ph["weight"], dtype=np.float64)
    s = [np.asarray(ph[c], dtype=np.float64) for c in ("s0", "s1", "s2", "s3")]
    undefined = np.zeros((n_obs, n_ph), dtype=bool)
    qq, uu = np.broadcast_to(s[1], (n_obs, n_ph)), np.broadcast_to(s[2], (n_obs, n_ph))
    if frame == SKY_PLANE and stokes:
        eyv = np.asarray(ey, dtype=np.float64).reshape(3, -1)
        p1, p2, p3 = (np.asarray(ph[c], dtype=np.float64)[None, :] for c in ("p1", "p2", "p3"))
        qq, uu, undefined = rotation(p1, p2, p3, eyv[0][:, None], eyv[1][:, None], eyv[2][:, None], s[1][None, :], s[2][None, :])
        undefined = undefined & q["accepted"]
    zero = np.zeros((n_obs, n_ph))
    both = lambda a: np.broadcast_to(a, (n_obs, n_ph))
    terms = {"w": both(w), "we": both(w * q["e"][0])}
    terms.update({"i": both(w * s[0]), "q": w[None, :] * qq, "u": w[None, :] * uu, "v": both(w * s[3])} if stokes else {c: zero for c in "iquv"})
    want = {"n_accepted": q["accepted"].sum(axis=1).astype(np.int64), "n_outside": (q["accepted"] & ~q["inside"]).sum(axis=1).astype(np.int64),
            "n_frame_undefined": undefined.sum(axis=1).astype(np.int64), "count": np.zeros((n_obs, n_rep, per_rep), dtype=np.int64),
            "terms": np.zeros((n_obs, n_rep, per_rep), dtype=np.int64), "k": k, "bin": flat}
    for name, _ in PLANES:
        want[name] = np.zeros((n_obs, n_rep, per_rep))
        want["abs_" + name] = np.zeros((n_obs, n_rep, per_rep))
    for o in range(n_obs):
        for rho in range(n_rep):
            idx = np.nonzero(q["inside"][o] & (k[rho] > 0))[0]
            idx = idx[np.argsort(flat[o, idx], kind="stable")]
            b = flat[o, idx]
            starts = np.nonzero(np.diff(b, prepend=-1))[0]
            for a, z in zip(starts, list(starts[1:]) + [len(b)]):
                members = idx[a:z]
                kk = k[rho, members]
                want["count"][o, rho, b[a]] = kk.sum()
                want["terms"][o, rho, b[a]] = z - a
                for name, _ in PLANES:
                    t = kk.astype(np.float64) * terms[name][o, members]
                    want[name][o, rho, b[a]] = math.fsum(t)
                    want["abs_" + name][o, rho, b[a]] = math.fsum(np.abs(t))
    for name in ["count", "terms"] + [p for p, _ in PLANES] + ["abs_" + p for p, _ in PLANES]:
        want[name] = want[name].reshape(shape)
    return want


COUNTERS = ("n_accepted", "n_outside", "n_frame_undefined")


def compare(res, want, label="", exact_only=False, factor=1.0):
    """counts and counters exactly; each sum within factor * (m + 2) * 2**-53 * sum|k * term| of the checker's"""
    for name in COUNTERS + ("count",):
        assert res[name].shape == want[name].shape, (label, name, res[name].shape, want[name].shape)
        assert np.array_equal(res[name], want[name]), (label, name, int(res[name].sum()), int(want[name].sum()))
    if exact_only:
        return
    m = want["terms"].astype(np.float64)
    for name, _ in PLANES:
        bound = factor * (m + 2.0) * U * want["abs_" + name]
        err = np.abs(res[name] - want[name])
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
        print("%s %s: largest error / bound = %.3g over %d bins in use" % (label, name, worst, int((m > 0).sum())))
        assert (err <= bound).all(), (label, name, worst)


# ---------------------------------------------------------------------------------------------- photons for the closed forms
def ring_photons(alpha, azimuths, Q=1.0, Uq=0.0, weight=None):
    """photons at polar angle alpha about the r2 axis at the given azimuths, moving along their own radial direction from r = 3e12 cm, with the
    stored Stokes vector (1, Q, U, 0); weights 1 unless given"""
    az = np.asarray(azimuths, dtype=np.float64)
    d = np.stack([np.sin(alpha) * np.cos(az), np.sin(alpha) * np.sin(az), np.cos(alpha) * np.ones_like(az)])
    p0 = 2.0 ** -60
    pv = p0 * d
    ph = S.photon_list(3.0e12 * d, np.stack([np.sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]), pv[0], pv[1], pv[2]]), 5)
    n = len(az)
    ph["s1"], ph["s2"], ph["s3"] = np.full(n, float(Q)), np.full(n, float(Uq)), np.zeros(n)
    ph["weight"] = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64)
    return ph
