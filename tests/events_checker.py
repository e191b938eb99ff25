"""An independent NumPy restatement of the detected-photon event list (include/mcrat_hip.h), for tests/test_gpu_events.py,
tests/test_events_plan_cpu.py and tests/test_events_checker_cpu.py.  Acceptance, t_det, e and (X, Y) of every (observer, photon) pair are
tests/sky_checker.py's per_photon, the Stokes rotation is tests/resample_checker.py's; the key of a detection time, the window, both orders -- one
np.lexsort on (slot, rank, key, observer) -- and the host helpers bin_events and event_durations are restated here, not imported from
mcrat_amd/engine.py.  Every value of a row is one of the documented IEEE expressions evaluated in the documented order, and the order of the rows is
fully specified: a device list is compared with np.array_equal, column by column, with no tolerance."""
import math

import numpy as np

from tests import resample_checker as R
from tests import sky_checker as S

BY_PHOTON, BY_TIME = 0, 1
AS_STORED, SKY_PLANE = R.AS_STORED, R.SKY_PLANE
F8_COLUMNS = ("t", "e", "w", "s0", "s1", "s2", "s3", "X", "Y", "num_scatt")
COLUMNS = ("rank", "slot") + F8_COLUMNS + ("type",)
COUNTERS = ("n_events", "n_accepted", "n_outside", "n_frame_undefined")
SIGN = np.uint64(1 << 63)
UNIT = [0.0, 1.0]                                 # edges that per_photon wants and nothing here looks at


def key(t):
    """the order-preserving map of a double's bits to a uint64: with the sign bit set all bits are inverted, otherwise the sign bit is set"""
    bits = np.ascontiguousarray(t, dtype=np.float64).view(np.uint64)
    return np.where((bits & SIGN) != 0, ~bits, bits | SIGN)


def events(ph, n, cos_acc, time_now, order=BY_TIME, frame=AS_STORED, ex=None, ey=None, t_window=None, e_window=None, rank=0, slot=None, stokes=True):
    """-> dict: the columns (n_total rows each; X and Y with ex and ey only), offsets (n_obs + 1,), the per-observer counters, n_total, key_or, key_and.
    time_now: one clock, or one per photon.  rank, slot: the photons' identities (slot None: their index)."""
    axes = ex is not None and ey is not None
    t_lo, t_hi = t_window or (-np.inf, np.inf)
    e_lo, e_hi = e_window or (-np.inf, np.inf)
    q = S.per_photon(ph, n, cos_acc, UNIT, UNIT, time_now, ex if axes else None, ey if axes else None, UNIT if axes else None, UNIT if axes else None)
    acc, t, e = q["accepted"], q["t"], q["e"]
    n_obs, n_ph = acc.shape
    with np.errstate(invalid="ignore"):
        inside = acc & (t >= t_lo) & (t < t_hi) & (e >= e_lo) & (e < e_hi)
    slot = np.arange(n_ph) if slot is None else np.asarray(slot)
    rank = np.broadcast_to(np.asarray(rank), (n_ph,))
    col = lambda k: np.asarray(ph[k], dtype=np.float64)
    s1, s2 = np.broadcast_to(col("s1"), (n_obs, n_ph)), np.broadcast_to(col("s2"), (n_obs, n_ph))
    undefined = np.zeros((n_obs, n_ph), dtype=bool)
    if frame == SKY_PLANE and stokes:
        eyv = np.asarray(ey, dtype=np.float64).reshape(3, -1)
        s1, s2, undefined = R.rotation(col("p1")[None, :], col("p2")[None, :], col("p3")[None, :], eyv[0][:, None], eyv[1][:, None], eyv[2][:, None],
                                       col("s1")[None, :], col("s2")[None, :])
        undefined = undefined & acc
    o, p = np.nonzero(inside)
    k = key(t[o, p])
    by = np.lexsort((slot[p], rank[p], o)) if order == BY_PHOTON else np.lexsort((slot[p], rank[p], k, o))
    o, p, k = o[by], p[by], k[by]
    zero = np.zeros(len(p))
    res = {"rank": rank[p].astype(np.int32), "slot": slot[p].astype(np.int32), "t": t[o, p], "e": e[o, p], "w": col("weight")[p],
           "s0": col("s0")[p] if stokes else zero, "s1": s1[o, p] if stokes else zero, "s2": s2[o, p] if stokes else zero,
           "s3": col("s3")[p] if stokes else zero, "num_scatt": col("num_scatt")[p], "type": np.asarray(ph["type"], dtype="S1")[p]}
    if axes:
        res["X"], res["Y"] = q["X"][o, p], q["Y"][o, p]
    res["n_events"] = inside.sum(axis=1).astype(np.int64)
    res["n_accepted"] = acc.sum(axis=1).astype(np.int64)
    res["n_outside"] = (acc & ~inside).sum(axis=1).astype(np.int64)
    res["n_frame_undefined"] = undefined.sum(axis=1).astype(np.int64)
    res["offsets"] = np.concatenate([[0], np.cumsum(res["n_events"])]).astype(np.int64)
    res["n_total"] = int(res["offsets"][-1])
    res["key_or"] = int(np.bitwise_or.reduce(k)) if len(k) else 0
    res["key_and"] = int(np.bitwise_and.reduce(k)) if len(k) else 2 ** 64 - 1
    res["keys"] = k
    res["observer"] = o
    return res


def compare(got, want, label=""):
    """every column, offsets and every counter: equal, bit for bit"""
    assert got["n_total"] == want["n_total"], (label, got["n_total"], want["n_total"])
    for name in COUNTERS + ("offsets",):
        assert np.array_equal(got[name], want[name]), (label, name, got[name], want[name])
    for name in COLUMNS:
        assert (name in got) == (name in want), (label, name)
        if name not in want:
            continue
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, name, a.shape, b.shape, a.dtype, b.dtype)
        same = a.view(np.uint64) == b.view(np.uint64) if a.dtype == np.float64 else a == b      # bits: -0.0 is not +0.0 here
        assert same.all(), (label, name, int((~same).sum()), np.nonzero(~same)[0][:5])
    assert np.array_equal(want["n_events"] + want["n_outside"], want["n_accepted"])
    for name in ("key_or", "key_and"):
        if name in got:
            assert got[name] == want[name], (label, name, hex(got[name]), hex(want[name]))


def bin_events(res, t_edges, e_edges, x_edges=None, y_edges=None):
    """the list binned as a sky observation: count, the six sums by math.fsum and abs_<sum> (sum|term|) beside them, each (n_obs, n_t, n_e[, n_y,
    n_x]), and n_outside (n_obs,)"""
    image = x_edges is not None
    offsets = res["offsets"]
    n_obs, n_t, n_e = len(offsets) - 1, len(t_edges) - 1, len(e_edges) - 1
    n_x, n_y = (len(x_edges) - 1, len(y_edges) - 1) if image else (1, 1)
    shape = (n_obs, n_t, n_e, n_y, n_x) if image else (n_obs, n_t, n_e)
    terms = {"w": res["w"], "we": res["w"] * res["e"], "i": res["w"] * res["s0"], "q": res["w"] * res["s1"], "u": res["w"] * res["s2"], "v": res["w"] * res["s3"]}
    out = {"count": np.zeros(shape, dtype=np.int64), "n_outside": np.array(res["n_outside"], dtype=np.int64)}
    members = {}
    for o in range(n_obs):
        for row in range(offsets[o], offsets[o + 1]):
            where = [S.find_bin(t_edges, res["t"][row]), S.find_bin(e_edges, res["e"][row])]
            if image:
                where += [S.find_bin(y_edges, res["Y"][row]), S.find_bin(x_edges, res["X"][row])]
            if min(int(b) for b in where) < 0:
                out["n_outside"][o] += 1
            else:
                members.setdefault((o,) + tuple(int(b) for b in where), []).append(row)
    for name in terms:
        out[name], out["abs_" + name] = np.zeros(shape), np.zeros(shape)
    for at, rows in members.items():
        out["count"][at] = len(rows)
        for name, term in terms.items():
            out[name][at] = math.fsum(term[rows])
            out["abs_" + name][at] = math.fsum(np.abs(term[rows]))
    return out


def event_durations(res, fractions=(0.05, 0.95), weight="we"):
    """per observer the times at which the running sum of the weight over the rows in time order first reaches f * total; None without events"""
    out = []
    for o in range(len(res["offsets"]) - 1):
        rows = sorted(range(res["offsets"][o], res["offsets"][o + 1]), key=lambda r: (res["t"][r], r))
        if not rows:
            out.append(None)
            continue
        term = [1.0 if weight == "count" else (res["w"][r] * res["e"][r] if weight == "we" else res["w"][r]) for r in rows]
        total, times = float(np.cumsum(term)[-1]), []
        for f in fractions:
            run = 0.0
            for r, x in zip(rows, term):
                run += x
                if run >= f * total:
                    break
            times.append(res["t"][r])
        out.append(np.array(times))
    return out
