"""tests/events_checker.py held to closed forms: the key of a detection time is monotone and injective over a hand-written ladder; three photons
whose arrival order is known; a duplicated list has every key twice, in slot order; the checker's list, binned, is the sky checker's observation
for the resample tests' fixture (counts exactly, sums within sky_checker.compare's bound); the durations of a list with equal weights and known
times.  mcrat_amd.engine's host helpers bin_events and event_durations are held to the same cases (importing the module does not load the
library)."""
import numpy as np

from tests import events_checker as E
from tests import sky_checker as S

INF = float("inf")
LADDER = [-INF, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, INF]
TIME_NOW = 400.0
OBSERVERS = S.observers([0.25, 0.3], [0.3, 1.2], [0.25, 0.25])      # tests/test_gpu_resample.py's: two overlapping cones off the axis
T_EDGES = np.linspace(100.0, 360.0, 4)
E_EDGES = 10.0 ** np.linspace(-9.0, -4.0, 3)
X_EDGES = np.array([-3.0e12, 0.0, 3.0e12])
Y_EDGES = np.array([-2.0e12, 0.0, 2.0e12])
AXIS = (np.array([[0.0], [0.0], [1.0]]), np.array([-1.0]))          # one observer along +r2 that accepts everything


def on_axis(r2, seed=3):
    """photons on the r2 axis at the heights r2, moving along it: the observer along +r2 sees them at t_det = time_now - r2 / c"""
    r2 = np.asarray(r2, dtype=np.float64)
    p0 = np.full(r2.shape, 2.0 ** -60)
    return S.photon_list(np.stack([0 * r2, 0 * r2, r2]), np.stack([p0, 0 * p0, 0 * p0, p0]), seed)


def test_key_is_monotone_and_injective():
    k = E.key(np.array(LADDER))
    assert k.dtype == np.uint64 and (np.diff(k.astype(object)) > 0).all()
    assert len(set(int(v) for v in k)) == len(LADDER)
    assert int(k[4]) == 2 ** 63 - 1 and int(k[5]) == 2 ** 63                         # -0.0 sorts right before +0.0
    assert int(k[0]) == (2 ** 64 - 1) ^ 0xFFF0000000000000 and int(k[-1]) == 0xFFF0000000000000      # -inf and +inf are legal keys


def test_three_photons_arrive_in_the_known_order():
    c = S.C_LIGHT
    ph = on_axis([10.0 * c, 30.0 * c, 20.0 * c])                                      # t_det = -10, -30, -20 at time_now = 0
    by_time = E.events(ph, *AXIS, 0.0, E.BY_TIME)
    assert np.array_equal(by_time["slot"], [1, 2, 0]) and np.array_equal(by_time["t"], [-30.0, -20.0, -10.0])
    by_photon = E.events(ph, *AXIS, 0.0, E.BY_PHOTON)
    assert np.array_equal(by_photon["slot"], [0, 1, 2]) and np.array_equal(by_photon["t"], [-10.0, -30.0, -20.0])
    for res in (by_time, by_photon):
        assert np.array_equal(res["offsets"], [0, 3]) and res["n_total"] == 3 and np.array_equal(res["e"], ph["p0"] * S.C_LIGHT)
        assert np.array_equal(res["rank"], [0, 0, 0]) and "X" not in res
    # the window: t_lo <= t < t_hi
    cutoff = E.events(ph, *AXIS, 0.0, E.BY_TIME, t_window=(-30.0, -10.0))
    assert np.array_equal(cutoff["slot"], [1, 2]) and cutoff["n_outside"][0] == 1 and cutoff["n_accepted"][0] == 3
    nan = on_axis([10.0 * c, np.nan, 20.0 * c])
    res = E.events(nan, *AXIS, 0.0, E.BY_TIME)
    assert np.array_equal(res["slot"], [2, 0]) and res["n_outside"][0] == 1             # a NaN never reaches a row


def test_a_duplicated_list_has_every_key_twice_in_slot_order():
    ph = S.jet_photons(7, 40)
    both = S.concatenate([ph, ph])
    n, cos_acc, ex, ey = S.observers([0.0, 0.3], [0.0, 1.0], [3.0, 3.0])
    res = E.events(both, n, -np.ones(2), TIME_NOW, E.BY_TIME)
    assert res["n_total"] == 160
    for o in range(2):
        a, b = res["offsets"][o], res["offsets"][o + 1]
        keys, slots = res["keys"][a:b], res["slot"][a:b]
        assert np.array_equal(keys[0::2], keys[1::2]) and (np.diff(keys[0::2].astype(object)) > 0).all()
        assert np.array_equal(slots[1::2], slots[0::2] + 40)
    # ... and ties between ranks break by rank
    ranks = np.repeat([2, 0], 40)
    res = E.events(both, n, -np.ones(2), TIME_NOW, E.BY_TIME, rank=ranks, slot=np.tile(np.arange(40), 2))
    assert np.array_equal(res["rank"][0::2], np.zeros(80)) and np.array_equal(res["rank"][1::2], np.full(80, 2))
    assert np.array_equal(res["slot"][0::2], res["slot"][1::2])


def test_binned_list_is_the_sky_observation():
    from mcrat_amd import engine
    ph = S.jet_photons(101, 257)
    n, cos_acc, ex, ey = OBSERVERS
    acc = S.per_photon(ph, n, cos_acc, T_EDGES, E_EDGES, TIME_NOW)["accepted"]
    for image in (False, True):
        edges = (T_EDGES, E_EDGES, X_EDGES, Y_EDGES) if image else (T_EDGES, E_EDGES)
        want = S.observation(ph, n, cos_acc, T_EDGES, E_EDGES, TIME_NOW, *((ex, ey, X_EDGES, Y_EDGES) if image else ()))
        assert (acc.sum(axis=1) > 20).all() and (acc[0] & acc[1]).sum() > 5 and (want["n_outside"] > 0).all() and want["count"].sum() > 40
        for order in (E.BY_PHOTON, E.BY_TIME):
            for window in (None, (T_EDGES[0], T_EDGES[-1])):                          # outside the window or outside the edges: outside either way
                res = E.events(ph, n, cos_acc, TIME_NOW, order, ex=ex, ey=ey, t_window=window)
                assert np.array_equal(res["n_accepted"], want["n_accepted"]) and res["n_total"] > 40
                for binned in (E.bin_events(res, *edges), engine.bin_events(res, *edges)):
                    binned["n_accepted"] = want["n_accepted"]
                    S.compare(binned, want, "image %d order %d" % (image, order))


def test_durations_of_equal_weights_and_known_times():
    from mcrat_amd import engine
    c = S.C_LIGHT
    times = np.arange(1.0, 21.0)                                                      # t_det = 1 .. 20, shuffled over the slots
    ph = on_axis(-c * times[np.random.default_rng(5).permutation(20)])
    ph["weight"][:] = 2.0
    for order in (E.BY_PHOTON, E.BY_TIME):
        res = E.events(ph, *AXIS, 0.0, order)
        for helper in (E.event_durations, engine.event_durations):
            for weight in ("we", "w", "count"):
                (t90,) = helper(res, (0.05, 0.95), weight)                            # 1 of 20 is 5 per cent, 19 of 20 are 95
                (t50,) = helper(res, (0.25, 0.75), weight)
                assert np.array_equal(t90, [1.0, 19.0]) and np.array_equal(t50, [5.0, 15.0]), (order, weight, t90, t50)
    # an observer without events
    away = (np.array([[0.0, 0.0], [0.0, 0.0], [1.0, -1.0]]), np.array([0.9, 0.9]))
    res = E.events(ph, *away, 0.0, E.BY_TIME)
    for helper in (E.event_durations, engine.event_durations):
        got = helper(res)
        assert got[1] is None and np.array_equal(got[0], [1.0, 19.0])
