"""Sky observers on the device (mcrat_hip_observe_sky, mcrat_hip_pool_observe_sky; mcrat_amd/csrc/sky.hip): the resident photons binned by observer
direction, detection time, energy and sky-plane position, against the NumPy restatement of the definitions in tests/sky_checker.py (itself checked
against hand-built photons in tests/test_sky_checker_cpu.py).

count, n_accepted and n_outside must be EXACTLY equal, every photon included: each expression that decides a bin is written in one fixed order and
evaluated without contraction, so it is bit-identical on the device and in the checker.  Each of the six sums of a bin with m photons must be within
(m + 2) * 2**-53 * sum|term| of the checker's fsum (sky_checker.compare; the bound is derived there)."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from mcrat_amd import synth
from tests import sky_checker as S
from tests.test_sky_plan_cpu import TEXTS, match_hash
from tests import test_sky_plan_cpu as P

pytestmark = pytest.mark.gpu

PATHS = ("lds", "global")
TIME_NOW = 400.0
# one observer on the axis and two off it at different azimuths whose cones overlap
OBSERVERS = S.observers([0.0, 0.25, 0.3], [0.0, 0.3, 1.2], [0.3, 0.25, 0.25])
T_EDGES = np.linspace(100.0, 360.0, 5)                 # t_det = 400 - r.n / c lies between ~65 and ~370 s: some photons fall outside
E_EDGES = 10.0 ** np.linspace(-9.0, -4.0, 9)           # e = p0 c lies between 3e-10 and 3e-4 erg: some fall outside
X_EDGES = np.linspace(-3.0e12, 3.0e12, 6)              # the jet reaches |X|, |Y| ~ 5e12 cm: some fall outside
Y_EDGES = np.linspace(-2.0e12, 2.0e12, 4)
# observers with vectors of zeros and ones: a photon at r = R n + a ex + b ey has X = a, Y = b, t_det = time_now - R / c exactly
AXIS = (np.array([[0.0], [0.0], [1.0]]), np.array([0.5]), np.array([[1.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]]))


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def engine_with(hip, ph, stokes=1, dims=synth.TWO, geom=synth.CYLINDRICAL):
    e = hip.Engine(dims, geom, stokes)
    e.set_photons(ph)
    return e


def cut(ph, a, b=None):
    return {k: (v[a:b] if b is not None else v[:a]).copy() for k, v in ph.items()}


def image_of(e, obs, time_now, edges=None, pool=False):
    n, cos_acc, ex, ey = obs
    te, ee, xe, ye = edges or (T_EDGES, E_EDGES, X_EDGES, Y_EDGES)
    return (e.pool_observe_sky if pool else e.observe_sky)(n, cos_acc, te, ee, time_now, ex, ey, xe, ye)


def want_image(ph, obs, time_now, edges=None, stokes=True):
    n, cos_acc, ex, ey = obs
    te, ee, xe, ye = edges or (T_EDGES, E_EDGES, X_EDGES, Y_EDGES)
    return S.observation(ph, n, cos_acc, te, ee, time_now, ex, ey, xe, ye, stokes=stokes)


def expect_path(hip, e, path):
    assert e.observe_sky_path() == (hip.SKY_PATH_LDS if path == "lds" else hip.SKY_PATH_GLOBAL)


@functools.lru_cache(maxsize=None)
def base():
    """2000 photons of a jet that is not axisymmetric, and the checker's cube 3 x 4 x 8 x 3 x 5 for them (shared by the tests: do not change it)"""
    ph = S.jet_photons(101, 2000)
    return ph, want_image(ph, OBSERVERS, TIME_NOW)


# ---------------------------------------------------------------------------------------------- 1: three observers, both paths
@pytest.mark.parametrize("path", PATHS)
def test_three_observers_image(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    ph, want = base()
    e = engine_with(hip, ph)
    assert e.observe_sky_path() == 0
    res = image_of(e, OBSERVERS, TIME_NOW)
    expect_path(hip, e, path)
    assert res["count"].shape == (3, 4, 8, 3, 5) and res["q"].shape == (3, 4, 8, 3, 5) and res["n_accepted"].shape == (3,)
    S.compare(res, want, "three observers " + path)
    acc = S.per_photon(ph, OBSERVERS[0], OBSERVERS[1], T_EDGES, E_EDGES, TIME_NOW)["accepted"]
    assert (acc.sum(axis=1) > 100).all() and (acc[1] & acc[2]).sum() > 20                 # the off-axis cones overlap: those photons count twice
    assert want["n_accepted"].sum() > acc.any(axis=0).sum() + 20
    assert (want["n_outside"] > 0).all() and (want["count"] > 0).sum() > 150 and np.abs(res["u"]).sum() > 0
    assert not np.array_equal(want["count"][1], want["count"][2])                         # the azimuth matters
    e.close()


def test_the_rule_picks_the_path(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_SKY_PATH", raising=False)
    ph, want = base()
    e = engine_with(hip, ph)
    S.compare(image_of(e, OBSERVERS, TIME_NOW), want, "small image")
    assert e.observe_sky_path() == hip.SKY_PATH_LDS
    # 1 x 2 x 2 x 64 x 64 bins of 56 bytes: 917 KB, far beyond the 80 KiB a workgroup may use
    edges = (np.array([60.0, 250.0, 380.0]), np.array([1e-10, 1e-7, 1e-3]), np.linspace(-4e12, 4e12, 65), np.linspace(-4e12, 4e12, 65))
    obs = tuple(a[..., 1:2] for a in OBSERVERS)
    res = image_of(e, obs, TIME_NOW, edges)
    assert e.observe_sky_path() == hip.SKY_PATH_GLOBAL
    w = want_image(ph, obs, TIME_NOW, edges)
    S.compare(res, w, "64 x 64 image")
    assert (w["count"] > 0).sum() > 200
    e.close()


# ---------------------------------------------------------------------------------------------- 2: list lengths
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_list_lengths(hip, monkeypatch, n, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    ph = cut(base()[0], n)
    e = engine_with(hip, ph)
    res = image_of(e, OBSERVERS, TIME_NOW)
    expect_path(hip, e, path)
    S.compare(res, want_image(ph, OBSERVERS, TIME_NOW), "n=%d %s" % (n, path))
    e.close()


# ---------------------------------------------------------------------------------------------- 3: ties and non-numbers
def placed(R, a, b, p=None):
    """photons at (a, b, R) moving along the axis (or with the momenta p): the on-axis observer AXIS sees them at X = a, Y = b, t_det = 400 - R / c"""
    R, a, b = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (R, a, b)))
    p0 = np.full(R.shape, 2.0 ** -60)
    return S.photon_list(np.stack([a, b, R]).astype(np.float64), np.stack([p0, 0 * p0, 0 * p0, p0]) if p is None else p, 17)


@pytest.mark.parametrize("path", PATHS)
def test_ties_and_non_numbers(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    R = 100.0 * S.C_LIGHT                                                           # t_det = 300 exactly
    te, ee = np.array([200.0, 300.0, 400.0]), np.array([1e-12, 1e-3])
    xe, ye = np.array([-2.0, -1.0, 0.0, 1.0, 2.0]) * 1e10, np.array([-1.0, 0.0, 1.0]) * 1e10
    a = np.array([xe[2], xe[4], np.nextafter(xe[4], 0.0), xe[0], np.nextafter(xe[0], -1e300), 5e9, 5e9, 5e9, 5e9, 5e9])
    b = np.array([5e9, 5e9, 5e9, 5e9, 5e9, ye[1], ye[2], 5e9, 5e9, 5e9])
    ph = placed(R, a, b)
    p0 = ph["p0"][0]
    # acceptance at equality: p3 = 0.5 p0 with p0 a power of two and cos_acc = 0.5 -- accepted; one unit in the last place below -- not
    for k, p3 in ((7, 0.5 * p0), (8, np.nextafter(0.5 * p0, 0.0))):
        ph["p1"][k], ph["p3"][k] = p0 * math.sqrt(0.75), p3
    ph["r2"][9] = 50.0 * S.C_LIGHT                                                  # t_det = 350: the second time bin's inside
    nan, inf = cut(ph, 9, 10), cut(ph, 9, 10)
    nan["r0"][0] = np.nan
    inf["r1"][0] = np.inf
    ph = S.concatenate([ph, nan, inf])
    edges = (te, ee, xe, ye)
    want = want_image(ph, AXIS, TIME_NOW, edges)
    q = S.per_photon(ph, AXIS[0], AXIS[1], te, ee, TIME_NOW, AXIS[2], AXIS[3], xe, ye)
    assert q["accepted"][0].tolist() == [True] * 8 + [False] + [True] * 3
    assert q["ix"][0, :5].tolist() == [2, -1, 3, 0, -1] and q["iy"][0, 5:7].tolist() == [1, -1] and q["it"][0, :9].tolist() == [1] * 9      # on an edge: the upper bin; on the last: outside
    assert want["n_accepted"].tolist() == [11] and want["n_outside"].tolist() == [5] and want["count"][0, 1, 0, 1, 2] == 4
    e = engine_with(hip, ph)
    res = image_of(e, AXIS, TIME_NOW, edges)
    expect_path(hip, e, path)
    S.compare(res, want, "ties " + path)
    e.close()
    # ... and photon by photon, so that no other photon can make up for a wrong one
    for k in range(len(ph["p0"])):
        one = cut(ph, k, k + 1)
        e1 = engine_with(hip, one)
        S.compare(image_of(e1, AXIS, TIME_NOW, edges), want_image(one, AXIS, TIME_NOW, edges), "ties, photon %d, %s" % (k, path))
        e1.close()


# ---------------------------------------------------------------------------------------------- 4: bystanders
@pytest.mark.parametrize("path", PATHS)
def test_bystanders(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    n = 1000
    ph = cut(base()[0], n)
    kind = np.random.default_rng(8).integers(0, 10, n)
    ph["weight"][kind == 0] = 0.0
    ph["type"][kind == 1] = b"p"
    ph["type"][kind == 2] = b"N"
    ph["type"][kind == 3] = b"c"                       # other types count
    want = want_image(ph, OBSERVERS, TIME_NOW)
    acc_all = S.per_photon(cut(base()[0], n), OBSERVERS[0], OBSERVERS[1], T_EDGES, E_EDGES, TIME_NOW)["accepted"]
    acc = S.per_photon(ph, OBSERVERS[0], OBSERVERS[1], T_EDGES, E_EDGES, TIME_NOW)["accepted"]
    for k in (0, 1, 2):
        assert acc_all[:, kind == k].any(axis=0).sum() > 10 and not acc[:, kind == k].any()
    assert acc[:, kind == 3].any()
    e = engine_with(hip, ph)
    S.compare(image_of(e, OBSERVERS, TIME_NOW), want, "bystanders " + path)
    e.close()
    # slots beyond the list's length, and a list never created: a pool of two windows of 1500 slots holding this one list
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 1500)
    pool.pool_rank(1, 1).set_photons(ph)
    S.compare(image_of(pool, OBSERVERS, [0.0, TIME_NOW], pool=True), want, "bystanders, pool " + path)
    pool.close()


# ---------------------------------------------------------------------------------------------- 5: sharing on the global path
SIDE = 38                                              # 38 x 38 pixels: with the edges 81 616 of the 81 920 bytes, the largest square image that fits LDS too
SHARE_EDGES = (np.array([200.0, 400.0]), np.array([1e-12, 1e-3]), np.arange(SIDE + 1.0) * 1e10, np.arange(SIDE + 1.0) * 1e10)


def in_pixels(bins, seed):
    """photons in the pixels `bins` (iy * SIDE + ix) of SHARE_EDGES, at random places inside them"""
    bins = np.asarray(bins)
    g = np.random.default_rng(seed)
    a, b = (bins % SIDE + g.uniform(0.1, 0.9, len(bins))) * 1e10, (bins // SIDE + g.uniform(0.1, 0.9, len(bins))) * 1e10
    return placed(100.0 * S.C_LIGHT, a, b)


def colliding_pairs():
    """pairs of different pixels with the same entry in the match table (the header's hash, restated in tests/test_sky_plan_cpu.py)"""
    by_hash = {}
    for b in range(SIDE * SIDE):
        by_hash.setdefault(match_hash(b), []).append(b)
    return [v[:2] for v in by_hash.values() if len(v) >= 2]


def share_cases():
    g = np.random.default_rng(5)
    pairs = colliding_pairs()
    assert len(pairs) >= 16
    one = np.full(64, 37)
    different = g.permutation(SIDE * SIDE)[:64]
    collide = np.array([b for pair in pairs[:16] for b in pair] + [pairs[0][0]] * 8 + [pairs[0][1]] * 8 + list(g.permutation(SIDE * SIDE)[:16]))
    mix = np.concatenate([one, different, collide, g.integers(0, SIDE * SIDE, 64), g.integers(100, 104, 37)])
    return {"one_pixel": one, "all_different": different, "collisions": collide, "mix": mix}


@pytest.mark.parametrize("name", ["one_pixel", "all_different", "collisions", "mix"])
def test_sharing_on_the_global_path(hip, monkeypatch, name):
    bins = share_cases()[name]
    if name != "mix":
        assert len(bins) == 64                         # one wavefront
    if name == "collisions":
        assert len(set(bins)) > 32 and len({match_hash(b) for b in bins[:32]}) == 16
    ph = in_pixels(bins, 3)
    want = want_image(ph, AXIS, TIME_NOW, SHARE_EDGES)
    assert np.array_equal(want["count"][0, 0, 0].ravel(), np.bincount(bins, minlength=SIDE * SIDE)) and want["n_outside"].tolist() == [0]
    got = {}
    for path in PATHS:
        monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
        e = engine_with(hip, ph)
        got[path] = image_of(e, AXIS, TIME_NOW, SHARE_EDGES)
        expect_path(hip, e, path)
        S.compare(got[path], want, "%s %s" % (name, path))
        e.close()
    for k in ("count", "n_accepted", "n_outside"):
        assert np.array_equal(got["lds"][k], got["global"][k])


# ---------------------------------------------------------------------------------------------- 6: against Engine.observe on the axis
@pytest.mark.parametrize("path", PATHS)
def test_on_axis_light_curve_equals_observe(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    ph = base()[0]
    cos_acc = math.cos(0.3)
    assert not (ph["p3"] == ph["p0"] * cos_acc).any() and (ph["p3"] <= ph["p0"]).all()      # the points where the cone ring and the cone differ
    e = engine_with(hip, ph)
    res = e.observe_sky(AXIS[0], [cos_acc], T_EDGES, E_EDGES, TIME_NOW)
    expect_path(hip, e, path)
    assert res["count"].shape == (1, 4, 8)
    ring = e.observe([1.0], [0.0], [1.0], [cos_acc], T_EDGES, E_EDGES, TIME_NOW)
    for k in ("count", "n_accepted", "n_outside"):
        assert np.array_equal(res[k], ring[k]), k
    assert res["count"].sum() > 300
    S.compare(res, S.observation(ph, AXIS[0], [cos_acc], T_EDGES, E_EDGES, TIME_NOW), "no image " + path)
    e.close()


# ---------------------------------------------------------------------------------------------- 7: Stokes off
@pytest.mark.parametrize("path", PATHS)
def test_stokes_off(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    ph, want = base()
    off = engine_with(hip, ph, stokes=0)
    res = image_of(off, OBSERVERS, TIME_NOW)
    S.compare(res, want_image(ph, OBSERVERS, TIME_NOW, stokes=False), "stokes off " + path)
    for k in ("i", "q", "u", "v"):
        assert not res[k].any() and want[k].any()
    assert np.array_equal(res["count"], want["count"])
    off.close()


# ---------------------------------------------------------------------------------------------- 8: a pool, every list its own clock
@pytest.mark.parametrize("path", PATHS)
def test_pool_every_list_its_own_clock(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    lens, ranks = [1, 63, 65, 300], [0, 1, 3, 4]                  # rank 2 is never created
    clocks = np.array([400.0, 380.0, -1.0e9, 410.0, 395.5])
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(5, 320)
    starts = np.concatenate([[0], np.cumsum(lens)])
    lists = [cut(base()[0], int(a), int(b)) for a, b in zip(starts[:-1], starts[1:])]
    for r, ph in zip(ranks, lists):
        pool.pool_rank(r, r).set_photons(ph)
    res = image_of(pool, OBSERVERS, clocks, pool=True)
    expect_path(hip, pool, path)
    tn = np.concatenate([np.full(m, clocks[r]) for r, m in zip(ranks, lens)])
    want = want_image(S.concatenate(lists), OBSERVERS, tn)
    S.compare(res, want, "pool " + path)
    assert want["count"].sum() > 100
    assert not np.array_equal(want_image(S.concatenate(lists), OBSERVERS, 400.0)["count"], want["count"])      # the clocks matter
    # each view observed alone: that list, exactly; together they are the pool's counts
    alone = []
    for r, ph in zip(ranks, lists):
        v = pool.pool_rank(r, r)
        alone.append(image_of(v, OBSERVERS, clocks[r]))
        S.compare(alone[-1], want_image(ph, OBSERVERS, clocks[r]), "view %d %s" % (r, path))
    for k in ("count", "n_accepted", "n_outside"):
        assert np.array_equal(sum(a[k] for a in alone), res[k]), k
    pool.close()


# ---------------------------------------------------------------------------------------------- 9: photons are 3-D Cartesian in every geometry
def test_same_counts_in_every_geometry(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_SKY_PATH", raising=False)
    ph, want = base()
    got = []
    for dims, geom in ((synth.TWO, synth.CYLINDRICAL), (synth.THREE, synth.SPHERICAL)):
        e = engine_with(hip, ph, dims=dims, geom=geom)
        got.append(image_of(e, OBSERVERS, TIME_NOW))
        S.compare(got[-1], want, "dims %d geometry %d" % (dims, geom))
        e.close()
    for k in ("count", "n_accepted", "n_outside"):
        assert np.array_equal(got[0][k], got[1][k])


# ---------------------------------------------------------------------------------------------- 10: refusals and states through the ABI
def _abi_observer(hip, c, keep):
    """a mcrat_hip_sky_observer from a case of tests/test_sky_plan_cpu.py (keep: the arrays it points to)"""
    dp = C.POINTER(C.c_double)
    def arr(v, n):
        v = [float(k) for k in range(n + 1)] if v == "ramp" else ([float(-k) for k in range(n + 1)] if v == "ramp_descending" else list(v))
        a = np.array(v + [0.0], dtype=np.float64)                 # (never empty: a pointer to something)
        keep.append(a)
        return a.ctypes.data_as(dp)
    def vec(rows):
        if rows is None:
            return [None, None, None]
        return [arr([r[k] for r in rows], 0) for k in range(3)]
    return hip.SkyObserver(c["n_obs"], *vec(c["n"]), arr(c["cos_acc"], 0), *vec(c["ex"]), *vec(c["ey"]), c["n_t"], arr(c["te"], c["n_t"]),
                           c["n_e"], arr(c["ee"], c["n_e"]), c["n_x"], arr(c["xe"], c["n_x"]), c["n_y"], arr(c["ye"], c["n_y"]))


def test_refusals_reach_the_caller(hip, monkeypatch):
    e = engine_with(hip, cut(base()[0], 10))
    lib = e.lib
    for name, why in sorted(P.REFUSED.items()):
        c = P.PLANS[name]
        if c["env"] is None:
            monkeypatch.delenv("MCRAT_HIP_SKY_PATH", raising=False)
        else:
            monkeypatch.setenv("MCRAT_HIP_SKY_PATH", c["env"])
        keep = []
        obs, out = _abi_observer(hip, c, keep), hip.SkyObservation()
        assert lib.mcrat_hip_observe_sky(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == -1, name          # MCRAT_HIP_EINVAL
        assert lib.mcrat_hip_last_error(e.ctx).decode() == TEXTS[why], name
        assert e.observe_sky_path() == 0
    monkeypatch.delenv("MCRAT_HIP_SKY_PATH", raising=False)
    assert set(P.REFUSED.values()) == set(TEXTS)
    # through the Python interface
    with pytest.raises(hip.McratHipError, match="not a unit vector"):
        e.observe_sky([[0.0], [0.0], [2.0]], [0.5], T_EDGES, E_EDGES, TIME_NOW)
    with pytest.raises(hip.McratHipError, match="image axes need the sky-plane vectors"):
        e.observe_sky(AXIS[0], AXIS[1], T_EDGES, E_EDGES, TIME_NOW, x_edges=X_EDGES, y_edges=Y_EDGES)
    with pytest.raises(hip.McratHipError, match="both be 0"):
        e.observe_sky(AXIS[0], AXIS[1], T_EDGES, E_EDGES, TIME_NOW, AXIS[2], AXIS[3], x_edges=X_EDGES, y_edges=[0.0])
    # NULL output pointers: the call runs and writes nowhere; then only the counters
    keep = []
    obs, out = _abi_observer(hip, P.PLANS["image"], keep), hip.SkyObservation()
    assert lib.mcrat_hip_observe_sky(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == 0 and e.observe_sky_path() == hip.SKY_PATH_LDS
    n_acc = np.full(1, -1, dtype=np.int64)
    out.n_accepted = n_acc.ctypes.data_as(C.POINTER(C.c_longlong))
    assert lib.mcrat_hip_observe_sky(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == 0
    want = S.per_photon(cut(base()[0], 10), AXIS[0], [0.5], [0.0, 1.0], [0.0, 1.0], TIME_NOW)["accepted"].sum()
    assert n_acc[0] == want > 0
    assert lib.mcrat_hip_observe_sky(None, C.byref(obs), TIME_NOW, C.byref(out)) == -1 and lib.mcrat_hip_observe_sky(e.ctx, None, TIME_NOW, C.byref(out)) == -1
    assert lib.mcrat_hip_observe_sky(e.ctx, C.byref(obs), TIME_NOW, None) == -1 and lib.mcrat_hip_observe_sky_path(None) == 0
    obs.t_edges = None
    assert lib.mcrat_hip_observe_sky(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == -1
    assert lib.mcrat_hip_last_error(e.ctx).decode() == "observe_sky: a null array in mcrat_hip_sky_observer"
    # the wrong kind of context, and no photons: MCRAT_HIP_ESTATE
    keep = []
    obs, out = _abi_observer(hip, P.PLANS["image"], keep), hip.SkyObservation()
    clocks = np.array([TIME_NOW, TIME_NOW])
    dp = C.POINTER(C.c_double)
    ESTATE = -5
    assert lib.mcrat_hip_pool_observe_sky(e.ctx, C.byref(obs), clocks.ctypes.data_as(dp), C.byref(out)) == ESTATE
    assert lib.mcrat_hip_last_error(e.ctx).decode() == "pool_observe_sky: the context is no rank pool"
    assert lib.mcrat_hip_pool_observe_sky(e.ctx, C.byref(obs), None, C.byref(out)) == -1
    empty = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    assert lib.mcrat_hip_observe_sky(empty.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == ESTATE
    empty.close()
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 64)
    pool.pool_rank(0, 0).set_photons(cut(base()[0], 10))
    assert lib.mcrat_hip_observe_sky(pool.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == ESTATE
    assert "mcrat_hip_pool_observe_sky" in lib.mcrat_hip_last_error(pool.ctx).decode()
    assert lib.mcrat_hip_pool_observe_sky(pool.ctx, C.byref(obs), clocks.ctypes.data_as(dp), C.byref(out)) == 0
    with pytest.raises(ValueError):
        pool.pool_observe_sky(AXIS[0], AXIS[1], T_EDGES, E_EDGES, [TIME_NOW])      # one clock per list
    pool.close()
    e.close()


# ---------------------------------------------------------------------------------------------- 11: more slots than one sweep of the largest grid
@pytest.mark.parametrize("path", PATHS)
def test_more_slots_than_one_sweep_of_the_largest_grid(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
    header = open(os.path.join(P.ROOT, "mcrat_amd", "csrc", "sky_plan.hpp")).read()
    block, grid = (int(re.search(r"constexpr int %s = (\d+);" % k, header).group(1)) for k in ("SKY_BLOCK", "SKY_MAX_GRID"))
    n = block * grid + 300
    assert n == 524588
    ph = S.jet_photons(404, n)
    edges = (np.array([60.0, 250.0, 380.0]), np.array([1e-10, 1e-7, 1e-3]), np.array([-4e12, 0.0, 4e12]), np.array([-4e12, 0.0, 4e12]))
    obs = tuple(a[..., 1:2] for a in OBSERVERS)
    want = want_image(ph, obs, TIME_NOW, edges)
    last = want_image(cut(ph, block * grid, n), obs, TIME_NOW, edges)
    assert last["count"].sum() > 20                    # the slots past the first sweep hold photons that count
    e = engine_with(hip, ph)
    res = image_of(e, obs, TIME_NOW, edges)
    expect_path(hip, e, path)
    S.compare(res, want, "%d slots %s" % (n, path))
    e.close()


# ---------------------------------------------------------------------------------------------- 12: nothing changes
def test_photons_are_left_as_they_were(hip, monkeypatch):
    ph = base()[0]
    e = engine_with(hip, ph)
    before = e.get_photons()
    for path in PATHS:
        monkeypatch.setenv("MCRAT_HIP_SKY_PATH", path)
        image_of(e, OBSERVERS, TIME_NOW)
        e.observe_sky(OBSERVERS[0], OBSERVERS[1], T_EDGES, E_EDGES, TIME_NOW)
    after = e.get_photons()
    assert set(before) == set(after)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    e.close()
