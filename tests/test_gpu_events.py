"""Detected-photon event lists on the device (mcrat_hip_observe_events, mcrat_hip_pool_observe_events; mcrat_amd/csrc/events.hip) against the NumPy
restatement of the definitions in tests/events_checker.py (itself held to closed forms in tests/test_events_checker_cpu.py).

Every comparison of a list is events_checker.compare: every column, offsets and every counter np.array_equal -- doubles by their bits -- because the
definition leaves no tolerance: each value of a row is one documented IEEE expression and the order of the rows is fully specified.

One departure from the wording of the issue, in test_keys: with time_now = 0 a detection time is -(r . n) / c, and |r| <= DBL_MAX bounds it at 6e297;
the ladder of magnitudes therefore runs from 1e-300 to 3e297 s, not to 1e300.  And 0.0 - x is never -0.0, so the pair (-0.0, +0.0) comes from two
lists of a pool whose clocks are -0.0 and +0.0: both are time_now = 0."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from mcrat_amd import synth
from tests import events_checker as E
from tests import resample_checker as R
from tests import sky_checker as S
from tests import test_events_plan_cpu as EP
from tests.test_gpu_sky import cut

pytestmark = pytest.mark.gpu

TIME_NOW = 400.0
OBSERVERS = S.observers([0.25, 0.3], [0.3, 1.2], [0.25, 0.25])        # tests/test_gpu_resample.py's: two overlapping cones off the axis
T_EDGES = np.linspace(100.0, 360.0, 4)
E_EDGES = 10.0 ** np.linspace(-9.0, -4.0, 3)
X_EDGES = np.array([-3.0e12, 0.0, 3.0e12])
Y_EDGES = np.array([-2.0e12, 0.0, 2.0e12])
T_WINDOW, E_WINDOW = (100.0, 360.0), (1e-9, 1e-4)
AXIS = (np.array([[0.0], [0.0], [1.0]]), np.array([-1.0]), np.array([[1.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]]))      # along +r2, accepts all
T = EP.SORT_TILE                                                       # the pairs one workgroup ranks per pass
EINVAL, ESTATE, EREFUSED = -1, -5, -6


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def engine_with(hip, ph, stokes=1):
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, stokes)
    e.set_photons(ph)
    return e


@functools.lru_cache(maxsize=None)
def base():
    """257 photons of a jet that is not axisymmetric (shared by the tests: do not change it)"""
    return S.jet_photons(101, 257)


def observe(e, obs, time_now, order, frame=E.AS_STORED, axes=True, pool=False, **kw):
    n, cos_acc, ex, ey = obs
    f = e.pool_observe_events if pool else e.observe_events
    return f(n, cos_acc, time_now, order, frame, ex if axes else None, ey if axes else None, **kw)


def want_of(ph, obs, time_now, order, frame=E.AS_STORED, axes=True, **kw):
    n, cos_acc, ex, ey = obs
    return E.events(ph, n, cos_acc, time_now, order, frame, ex if axes else None, ey if axes else None, **kw)


def on_axis(r2, seed=3):
    """photons on the r2 axis at the heights r2, moving along it: AXIS sees them at t_det = time_now - r2 / c"""
    r2 = np.asarray(r2, dtype=np.float64)
    p0 = np.full(r2.shape, 2.0 ** -60)
    return S.photon_list(np.stack([0 * r2, 0 * r2, r2]), np.stack([p0, 0 * p0, 0 * p0, p0]), seed)


# ---------------------------------------------------------------------------------------------- 1: orders, frames, axes
@pytest.mark.parametrize("order", [E.BY_PHOTON, E.BY_TIME])
@pytest.mark.parametrize("frame,axes", [(E.AS_STORED, False), (E.AS_STORED, True), (E.SKY_PLANE, True)])
def test_orders_frames_and_axes(hip, order, frame, axes):
    ph = base()
    n, cos_acc, ex, ey = OBSERVERS
    want = want_of(ph, OBSERVERS, TIME_NOW, order, frame, axes, t_window=T_WINDOW, e_window=E_WINDOW)
    acc = S.per_photon(ph, n, cos_acc, T_EDGES, E_EDGES, TIME_NOW)["accepted"]
    assert (acc.sum(axis=1) > 20).all() and (acc[0] & acc[1]).sum() > 5 and (want["n_outside"] > 0).all() and (want["n_events"] > 10).all()
    e = engine_with(hip, ph)
    got = observe(e, OBSERVERS, TIME_NOW, order, frame, axes, t_window=T_WINDOW, e_window=E_WINDOW)
    E.compare(got, want, "order %d frame %d axes %d" % (order, frame, axes))
    assert ("X" in got) == axes
    if order == E.BY_TIME:
        assert got["sort_passes_run"] + got["sort_passes_skipped"] == 9 and got["sort_passes_skipped"] >= 1      # the sign and top exponent bits agree
        for o in range(2):
            assert (np.diff(got["t"][got["offsets"][o]:got["offsets"][o + 1]]) >= 0).all()
    else:
        assert got["sort_passes_run"] == 0 == got["sort_passes_skipped"]
    # the list, binned, is the sky observation of the same engine
    edges = (T_EDGES, E_EDGES, X_EDGES, Y_EDGES) if axes else (T_EDGES, E_EDGES)
    sky = e.observe_sky(n, cos_acc, T_EDGES, E_EDGES, TIME_NOW, *((ex, ey, X_EDGES, Y_EDGES) if axes else ()))
    sky_want = S.observation(ph, n, cos_acc, T_EDGES, E_EDGES, TIME_NOW, *((ex, ey, X_EDGES, Y_EDGES) if axes else ()))
    binned = hip.bin_events(got, *edges)
    assert np.array_equal(binned["count"], sky["count"]) and np.array_equal(binned["n_outside"], sky["n_outside"]) and sky["count"].sum() > 20
    if frame == E.AS_STORED:
        binned["n_accepted"] = got["n_accepted"]
        S.compare(binned, sky_want, "binned list")
    else:
        stored = want_of(ph, OBSERVERS, TIME_NOW, order, E.AS_STORED, axes, t_window=T_WINDOW, e_window=E_WINDOW)
        assert np.abs(got["s1"] - stored["s1"]).max() > 1e-3 * np.abs(got["s1"]).max() and np.array_equal(got["s0"], stored["s0"])
        assert (want["n_frame_undefined"] == 0).all()
    e.close()


# ---------------------------------------------------------------------------------------------- 2: list lengths
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_list_lengths(hip, n):
    ph = cut(base(), n)
    e = engine_with(hip, ph)
    for order in (E.BY_PHOTON, E.BY_TIME):
        E.compare(observe(e, OBSERVERS, TIME_NOW, order, E.SKY_PLANE), want_of(ph, OBSERVERS, TIME_NOW, order, E.SKY_PLANE), "n=%d order %d" % (n, order))
    e.close()


def test_no_accepted_photon(hip):
    ph = base()
    away = (-OBSERVERS[0], np.array([0.9, 0.9]), OBSERVERS[2], OBSERVERS[3])       # the jet moves the other way
    e = engine_with(hip, ph)
    for order in (E.BY_PHOTON, E.BY_TIME):
        got = observe(e, away, TIME_NOW, order)
        E.compare(got, want_of(ph, away, TIME_NOW, order), "nothing accepted")
        assert got["n_total"] == 0 and not got["offsets"].any() and not got["n_accepted"].any() and len(got["t"]) == 0
        got = observe(e, away, TIME_NOW, order, capacity=5)
        assert got["n_total"] == 0 and len(got["t"]) == 0
    e.close()


# ---------------------------------------------------------------------------------------------- 3: the sort's tile boundaries
@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1, 4099])
def test_sort_tile_boundaries(hip, n):
    ph = S.jet_photons(7, n)
    everything = (OBSERVERS[0], -np.ones(2), OBSERVERS[2], OBSERVERS[3])
    e = engine_with(hip, ph)
    got = observe(e, everything, TIME_NOW, E.BY_TIME)
    E.compare(got, want_of(ph, everything, TIME_NOW, E.BY_TIME), "n=%d" % n)
    assert got["n_total"] == 2 * n and np.array_equal(got["offsets"], [0, n, 2 * n])
    e.close()


# ---------------------------------------------------------------------------------------------- 4: stability
def test_equal_keys_keep_slot_order_and_then_rank_order(hip):
    ph = cut(base(), 100)
    both = S.concatenate([ph, ph])
    everything = (OBSERVERS[0], -np.ones(2), OBSERVERS[2], OBSERVERS[3])
    e = engine_with(hip, both)
    got = observe(e, everything, TIME_NOW, E.BY_TIME)
    E.compare(got, want_of(both, everything, TIME_NOW, E.BY_TIME), "duplicated list")
    for o in range(2):
        t, slot = (got[k][got["offsets"][o]:got["offsets"][o + 1]] for k in ("t", "slot"))
        assert np.array_equal(t[0::2], t[1::2]) and np.array_equal(slot[1::2], slot[0::2] + 100)
    e.close()
    # the same list in ranks 0 and 2 of a pool with equal clocks: ties break by rank
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(3, 128)
    for r in (2, 0):
        pool.pool_rank(r, r).set_photons(ph)
    got = observe(pool, everything, np.full(3, TIME_NOW), E.BY_TIME, pool=True)
    want = want_of(both, everything, TIME_NOW, E.BY_TIME, rank=np.repeat([0, 2], 100), slot=np.tile(np.arange(100), 2))
    E.compare(got, want, "two ranks")
    assert np.array_equal(got["rank"][0::2], np.zeros(200)) and np.array_equal(got["rank"][1::2], np.full(200, 2))
    assert np.array_equal(got["slot"][0::2], got["slot"][1::2])
    pool.close()


# ---------------------------------------------------------------------------------------------- 5: keys
def test_keys(hip):
    c = S.C_LIGHT
    mags = 10.0 ** np.arange(-290.0, 309.0, 13.0)                                  # r2: |t_det| from 3e-301 to 3e297 s
    ladder = np.concatenate([mags, -mags, [0.0, 5e-324, -5e-324]])
    lists = [on_axis(np.random.default_rng(4).permutation(ladder)), on_axis([0.0, 1.0, -1.0])]
    clocks = np.array([0.0, -0.0])                                                  # rank 1's photon at the origin arrives at -0.0, rank 0's at +0.0
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 128)
    for r, ph in enumerate(lists):
        pool.pool_rank(r, r).set_photons(ph)
    tn = np.concatenate([np.full(len(l["r2"]), clocks[r]) for r, l in enumerate(lists)])
    rank = np.concatenate([np.full(len(l["r2"]), r) for r, l in enumerate(lists)])
    slot = np.concatenate([np.arange(len(l["r2"])) for l in lists])
    for window in (None, (-np.inf, np.inf), (-np.inf, 0.0), (-0.0, np.inf)):
        got = observe(pool, AXIS, clocks, E.BY_TIME, pool=True, t_window=window)
        want = want_of(S.concatenate(lists), AXIS, tn, E.BY_TIME, rank=rank, slot=slot, t_window=window)
        E.compare(got, want, "ladder %r" % (window,))
    assert got["n_total"] > 40 and (np.diff(got["t"]) >= 0).all()
    zeros = np.nonzero(got["t"] == 0.0)[0]                                          # (-0.0, +0.0) is inside [-0.0, inf): comparisons only
    assert len(zeros) >= 3 and np.signbit(got["t"][zeros[0]]) and got["rank"][zeros[0]] == 1 and not np.signbit(got["t"][zeros[1:]]).any()
    full = observe(pool, AXIS, clocks, E.BY_TIME, pool=True)
    assert full["t"].min() < -1e297 and full["t"].max() > 1e297 and 0 < np.abs(full["t"][full["t"] != 0]).min() < 1e-300
    assert full["sort_passes_run"] == 8
    pool.close()
    # all at one position: every key is equal, every pass of the key is skipped, the rows stay in slot order
    same = on_axis(np.full(300, 7.0 * c))
    e = engine_with(hip, same)
    got = observe(e, AXIS, 0.0, E.BY_TIME)
    E.compare(got, want_of(same, AXIS, 0.0, E.BY_TIME), "equal keys")
    assert got["sort_passes_run"] == 0 and got["sort_passes_skipped"] == 8 and got["key_or"] == got["key_and"] and np.array_equal(got["slot"], np.arange(300))
    assert (got["t"] == -7.0).all()
    e.close()
    # keys that differ only in the exponent's top bits: t_det = 2^k with biased exponents 0x010, 0x110, 0x310, 0x710: one pass, the top byte
    k = np.array([0x310, 0x010, 0x710, 0x110, 0x310, 0x010]) - 1023
    top = on_axis(-c * 2.0 ** k)
    e = engine_with(hip, top)
    got = observe(e, AXIS, 0.0, E.BY_TIME)
    E.compare(got, want_of(top, AXIS, 0.0, E.BY_TIME), "top bits")
    assert np.array_equal(got["t"], 2.0 ** np.sort(k)) and np.array_equal(got["slot"], [1, 5, 3, 0, 4, 2])
    assert got["sort_passes_run"] == 1 and got["sort_passes_skipped"] == 7 and got["key_or"] ^ got["key_and"] == 0x7 << 60
    e.close()


# ---------------------------------------------------------------------------------------------- 6: many observers
def test_many_observers(hip):
    k = np.arange(257)
    n, cos_acc, ex, ey = S.observers(np.full(257, 0.3), 2 * math.pi * k / 257, np.full(257, 0.036))
    g = np.random.default_rng(12)
    d = n[:, 100][:, None] + 0.004 * g.standard_normal((3, 65))                     # 65 photons moving towards observer 100, within its neighbours' cones
    d /= np.sqrt((d * d).sum(axis=0))
    pv = 2.0 ** -60 * d
    ph = S.photon_list(10.0 ** g.uniform(12.0, 13.0, 65) * d, np.stack([np.sqrt((pv[0] * pv[0] + pv[1] * pv[1]) + pv[2] * pv[2]), pv[0], pv[1], pv[2]]), 13)
    obs = (n, cos_acc, ex, ey)
    want = want_of(ph, obs, TIME_NOW, E.BY_TIME, E.SKY_PLANE)
    seen = np.nonzero(want["n_events"])[0]
    assert 8 <= len(seen) <= 14 and seen.min() > 90 and seen.max() < 110 and (want["n_events"][seen] > 30).sum() >= 5 and want["n_total"] > 300
    e = engine_with(hip, ph)
    for order in (E.BY_PHOTON, E.BY_TIME):
        got = observe(e, obs, TIME_NOW, order, E.SKY_PLANE)
        E.compare(got, want_of(ph, obs, TIME_NOW, order, E.SKY_PLANE), "257 observers order %d" % order)
        assert len(got["offsets"]) == 258 and (np.diff(got["offsets"]) == 0).sum() == 257 - len(seen)
    assert got["sort_passes_skipped"] >= 1 and got["sort_passes_run"] >= 3         # two observer digits among them
    e.close()


# ---------------------------------------------------------------------------------------------- 7: capacity
def test_capacity(hip):
    ph = base()
    n, cos_acc, ex, ey = OBSERVERS
    want = want_of(ph, OBSERVERS, TIME_NOW, E.BY_TIME, t_window=T_WINDOW, e_window=E_WINDOW)
    total = want["n_total"]
    e = engine_with(hip, ph)
    for order in (E.BY_PHOTON, E.BY_TIME):
        want = want_of(ph, OBSERVERS, TIME_NOW, order, t_window=T_WINDOW, e_window=E_WINDOW)
        E.compare(observe(e, OBSERVERS, TIME_NOW, order, t_window=T_WINDOW, e_window=E_WINDOW, capacity=total), want, "capacity n_total")
        E.compare(observe(e, OBSERVERS, TIME_NOW, order, t_window=T_WINDOW, e_window=E_WINDOW), want, "capacity None")
        E.compare(observe(e, OBSERVERS, TIME_NOW, order, t_window=T_WINDOW, e_window=E_WINDOW, capacity=total + 1000), want, "room to spare")
        with pytest.raises(hip.McratHipError, match="observe_events: the list has %d rows, capacity is %d" % (total, total - 1)):
            observe(e, OBSERVERS, TIME_NOW, order, t_window=T_WINDOW, e_window=E_WINDOW, capacity=total - 1)
        refused = e.last_events
        assert refused["n_total"] == total
        for k in E.COUNTERS + ("offsets",):
            assert np.array_equal(refused[k], want[k]), k
    # through the ABI: the counting call returns 0 and its counters are exact; a refused call returns MCRAT_HIP_EREFUSED
    keep = [np.ascontiguousarray(a) for a in (n[0], n[1], n[2], cos_acc)]
    dp, ll = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    obs = hip.EventsObserver(2, *[a.ctypes.data_as(dp) for a in keep], None, None, None, None, None, None, T_WINDOW[0], T_WINDOW[1], E_WINDOW[0], E_WINDOW[1],
                             E.BY_TIME, E.AS_STORED, 0)
    out = hip.Events()
    n_events, offsets = np.full(2, -1, dtype=np.int64), np.full(3, -1, dtype=np.int64)
    out.n_events, out.offsets = n_events.ctypes.data_as(ll), offsets.ctypes.data_as(ll)
    assert e.lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == 0
    assert out.n_total == total and np.array_equal(n_events, want["n_events"]) and np.array_equal(offsets, want["offsets"])
    t = np.zeros(total)
    out.t = t.ctypes.data_as(dp)
    assert e.lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == EREFUSED       # capacity 0 with a row pointer: no counting call
    obs.capacity = total - 1
    assert e.lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == EREFUSED and out.n_total == total
    obs.capacity = total
    assert e.lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == 0 and np.array_equal(t, want["t"])
    e.close()


# ---------------------------------------------------------------------------------------------- 8: a pool of ragged lists and its views
def ragged_lists():
    lens = [65, 1, 191]
    starts = np.concatenate([[0], np.cumsum(lens)])
    lists = [cut(base(), int(a), int(b)) for a, b in zip(starts[:-1], starts[1:])]
    kind = np.random.default_rng(8).integers(0, 6, lens[2])
    lists[2]["weight"][kind == 0] = 0.0
    lists[2]["type"][kind == 1] = b"p"
    lists[2]["type"][kind == 2] = b"N"
    assert all((kind == k).sum() > 10 for k in (0, 1, 2))
    return lens, lists


@pytest.mark.parametrize("order", [E.BY_PHOTON, E.BY_TIME])
def test_pool_equals_the_checker_and_its_views(hip, order):
    lens, lists = ragged_lists()
    ranks, clocks = [0, 2, 3], np.array([400.0, -1.0e9, 380.0, 410.0])             # rank 1 is never created: an empty list
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(4, 200)
    for r, ph in zip(ranks, lists):
        pool.pool_rank(r, r).set_photons(ph)
    everything = S.concatenate(lists)
    tn = np.concatenate([np.full(m, clocks[r]) for r, m in zip(ranks, lens)])
    rank = np.concatenate([np.full(m, r) for r, m in zip(ranks, lens)])
    slot = np.concatenate([np.arange(m) for m in lens])
    got = observe(pool, OBSERVERS, clocks, order, E.SKY_PLANE, pool=True, t_window=T_WINDOW)
    want = want_of(everything, OBSERVERS, tn, order, E.SKY_PLANE, rank=rank, slot=slot, t_window=T_WINDOW)
    E.compare(got, want, "pool order %d" % order)
    assert want["n_total"] > 50 and len(set(want["rank"])) >= 2 and not np.isin(want["type"], [b"p", b"N"]).any() and (want["w"] != 0).all()
    # a view's list is that rank's rows of the pool's list
    for r, ph in zip(ranks, lists):
        alone = observe(pool.pool_rank(r, r), OBSERVERS, clocks[r], order, E.SKY_PLANE, t_window=T_WINDOW)
        E.compare(alone, want_of(ph, OBSERVERS, clocks[r], order, E.SKY_PLANE, rank=r, t_window=T_WINDOW), "view %d" % r)
        mine = got["rank"] == r
        observer = np.repeat(np.arange(2), np.diff(got["offsets"]))
        assert np.array_equal(np.bincount(observer[mine], minlength=2), alone["n_events"])
        for k in E.COLUMNS:
            assert got[k][mine].tobytes() == alone[k].tobytes(), (r, k)
    pool.close()


# ---------------------------------------------------------------------------------------------- 9: Stokes off, undefined frames
def test_stokes_off_and_undefined_frames(hip):
    ph = base()
    off = engine_with(hip, ph, stokes=0)
    for frame in (E.AS_STORED, E.SKY_PLANE):
        got = observe(off, OBSERVERS, TIME_NOW, E.BY_TIME, frame)
        E.compare(got, want_of(ph, OBSERVERS, TIME_NOW, E.BY_TIME, frame, stokes=False), "stokes off frame %d" % frame)
        assert got["n_total"] > 40 and not got["n_frame_undefined"].any() and got["w"].all()
        for k in ("s0", "s1", "s2", "s3"):
            assert not got[k].any()
    off.close()
    # along the polar axis the photon's own frame is undefined: counted, and stored as is
    ph = S.concatenate([R.ring_photons(0.0, [0.0, 1.0, 2.0], Q=0.25, Uq=-0.5), R.ring_photons(0.05, [0.7, 2.9], Q=0.25, Uq=-0.5)])
    ph["p3"][1] = -ph["p3"][1]                                                      # along -z_hat: undefined too, but nobody accepts it
    obs = (AXIS[0], np.array([math.cos(0.1)]), AXIS[2], AXIS[3])
    want = want_of(ph, obs, TIME_NOW, E.BY_PHOTON, E.SKY_PLANE)
    assert want["n_frame_undefined"].tolist() == [2] and want["n_events"].tolist() == [4]
    e = engine_with(hip, ph)
    got = observe(e, obs, TIME_NOW, E.BY_PHOTON, E.SKY_PLANE)
    E.compare(got, want, "undefined frames")
    assert np.array_equal(got["slot"], [0, 2, 3, 4]) and got["s1"][:2].tolist() == [0.25, 0.25] and got["s2"][:2].tolist() == [-0.5, -0.5]
    assert got["s1"][2] != 0.25 and got["s1"][3] != 0.25
    late = observe(e, obs, TIME_NOW, E.BY_PHOTON, E.SKY_PLANE, t_window=(1e9, np.inf))       # outside the window they are counted all the same
    assert late["n_total"] == 0 and late["n_frame_undefined"].tolist() == [2] and late["n_outside"].tolist() == [4]
    e.close()


# ---------------------------------------------------------------------------------------------- 10: reproducibility, and nothing changes
def test_the_same_call_twice_gives_the_same_bytes(hip):
    ph = S.jet_photons(31, 3000)
    everything = (OBSERVERS[0], np.array([0.5, -1.0]), OBSERVERS[2], OBSERVERS[3])
    e = engine_with(hip, ph)
    before = e.get_photons()
    for order in (E.BY_PHOTON, E.BY_TIME):
        a, b = (observe(e, everything, TIME_NOW, order, E.SKY_PLANE) for _ in range(2))
        assert a["n_total"] > 3000
        for k in E.COLUMNS + E.COUNTERS + ("offsets",):
            assert a[k].tobytes() == b[k].tobytes(), (order, k)
    after = e.get_photons()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    e.close()


# ---------------------------------------------------------------------------------------------- 11: refusals and states through the ABI
def _abi_observer(hip, c, keep):
    """a mcrat_hip_events_observer from a case of tests/test_events_plan_cpu.py (keep: the arrays it points to)"""
    dp = C.POINTER(C.c_double)
    def arr(v):
        a = np.array(list(v) + [0.0], dtype=np.float64)           # (never empty: a pointer to something)
        keep.append(a)
        return a.ctypes.data_as(dp)
    def vec(rows):
        return [None, None, None] if rows is None else [arr([r[k] for r in rows]) for k in range(3)]
    return hip.EventsObserver(c["n_obs"], *vec(c["n"]), arr(c["cos_acc"]), *vec(c["ex"]), *vec(c["ey"]), *c["window"], c["order"], c["frame"], c["capacity"])


def test_refusals_reach_the_caller(hip):
    e = engine_with(hip, cut(base(), 10))
    lib = e.lib
    dp = C.POINTER(C.c_double)
    room = np.zeros(1000)
    def call(c, ctx=e):
        keep = []
        obs = _abi_observer(hip, c, keep)
        out = hip.Events()
        if c["want_xy"]:
            out.X = room.ctypes.data_as(dp)
        return lib.mcrat_hip_observe_events(ctx.ctx, C.byref(obs), TIME_NOW, C.byref(out)), obs, out, keep
    for name, why in sorted(EP.REFUSED.items()):
        assert call(EP.PLANS[name])[0] == EINVAL, name
        assert lib.mcrat_hip_last_error(e.ctx).decode() == EP.TEXTS[why], name
    assert set(EP.TEXTS) == set(EP.REFUSED.values())
    # through the Python interface
    with pytest.raises(hip.McratHipError, match="needs the sky-plane vectors"):
        e.observe_events(AXIS[0], AXIS[1], TIME_NOW, stokes_frame=hip.STOKES_SKY_PLANE)
    with pytest.raises(hip.McratHipError, match="the window needs"):
        e.observe_events(AXIS[0], AXIS[1], TIME_NOW, t_window=(5.0, 5.0))
    # NULL pointers
    rc, obs, out, keep = call(EP.PLANS["counting"])
    assert rc == 0 and out.n_total == S.per_photon(cut(base(), 10), AXIS[0], [0.5], [0.0, 1.0], [0.0, 1.0], TIME_NOW)["accepted"].sum() > 0
    assert lib.mcrat_hip_observe_events(None, C.byref(obs), TIME_NOW, C.byref(out)) == EINVAL
    assert lib.mcrat_hip_observe_events(e.ctx, None, TIME_NOW, C.byref(out)) == EINVAL
    assert lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, None) == EINVAL
    obs.cos_acc = None
    assert lib.mcrat_hip_observe_events(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == EINVAL
    assert lib.mcrat_hip_last_error(e.ctx).decode() == "observe_events: a null array in mcrat_hip_events_observer"
    # the wrong kind of context, and no photons: MCRAT_HIP_ESTATE
    rc, obs, out, keep = call(EP.PLANS["counting"])
    clocks = np.array([TIME_NOW, TIME_NOW])
    assert lib.mcrat_hip_pool_observe_events(e.ctx, C.byref(obs), clocks.ctypes.data_as(dp), C.byref(out)) == ESTATE
    assert lib.mcrat_hip_last_error(e.ctx).decode() == "pool_observe_events: the context is no rank pool"
    assert lib.mcrat_hip_pool_observe_events(e.ctx, C.byref(obs), None, C.byref(out)) == EINVAL
    empty = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    assert lib.mcrat_hip_observe_events(empty.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == ESTATE
    empty.close()
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 64)
    pool.pool_rank(0, 0).set_photons(cut(base(), 10))
    assert lib.mcrat_hip_observe_events(pool.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == ESTATE
    assert "mcrat_hip_pool_observe_events" in lib.mcrat_hip_last_error(pool.ctx).decode()
    assert lib.mcrat_hip_pool_observe_events(pool.ctx, C.byref(obs), clocks.ctypes.data_as(dp), C.byref(out)) == 0 and out.n_total > 0
    with pytest.raises(ValueError):
        pool.pool_observe_events(AXIS[0], AXIS[1], [TIME_NOW])                       # one clock per list
    pool.close()
    e.close()
