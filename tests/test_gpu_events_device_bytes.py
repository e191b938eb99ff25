"""mcrat_hip_device_bytes counts the device block of the eighth analysis product, the event list (include/mcrat_hip.h: "HBM held by the context"):
its first call allocates the block and the figure grows by at least what events_plan.hpp lays out for it; a call with an equal or smaller capacity
finds the block and leaves the figure alone, a larger one makes it grow by at least the difference; the block is counted on the pool, not on a
view.  The shape is the smallest that allocates: 3 photons, one observer.  The bytes are worked out here from the documented layout -- without the
padding between its parts, so they are a lower bound -- not read back from the library.  (The pattern of tests/test_gpu_resample_device_bytes.py.)"""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import sky_checker as S

pytestmark = pytest.mark.gpu

N_PHOTONS = 3
# the head: three counters, two offsets, two masks; the staged observer: n0, n1, n2, cos_acc; one chunk of one observer in the count table
FIXED = 8 * (3 + 2 + 2) + 8 * 4 + 8
# a row without X and Y: rank, slot, eight doubles, type; BY_TIME adds the slot behind the row, two keys and two row indices
ROW, SORT_ROW = 4 + 4 + 8 * 8 + 1, 4 + 2 * 8 + 2 * 4
SORT_TABLE = 4 * 256                            # one tile: a word per digit


def call(e, time_now=40.0, pool=False, order=1, capacity=N_PHOTONS):
    f = e.pool_observe_events if pool else e.observe_events
    return f([0.0, 0.0, 1.0], [-1.0], time_now, order, capacity=capacity)


def test_device_bytes_counts_the_events_block():
    from mcrat_amd import engine
    engine.load_library()
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    e.set_photons(S.jet_photons(3, N_PHOTONS))
    need = FIXED + N_PHOTONS * (ROW + SORT_ROW) + SORT_TABLE
    assert need == 96 + 3 * 101 + 1024
    before = e.device_bytes()
    res = call(e)
    after = e.device_bytes()
    print("observe_events: device_bytes %d -> %d, the block needs at least %d" % (before, after, need))
    assert res["n_total"] == N_PHOTONS == res["n_accepted"][0] and len(res["t"]) == N_PHOTONS
    assert after - before >= need
    call(e)
    assert e.device_bytes() == after
    sky = e.observe_sky([0.0, 0.0, 1.0], [-1.0], [-1e9, 1e9], [1e-300, 1e300], 40.0)       # a block of its own: observe_sky's does not shrink or replace it
    assert e.device_bytes() > after and sky["count"].sum() == N_PHOTONS
    grown = e.device_bytes()
    call(e)
    call(e, order=0)                                                                        # (smaller needs: the block stays)
    call(e, capacity=None)
    assert e.device_bytes() == grown
    call(e, capacity=N_PHOTONS + 5000)                                                      # a larger one: it grows by at least the difference
    assert e.device_bytes() - grown >= 5000 * (ROW + SORT_ROW) - 4096                       # (less the padding the small block held)
    e.close()


def test_the_block_is_counted_on_the_pool_not_on_a_view():
    from mcrat_amd import engine
    engine.load_library()
    pool = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 256)
    view = pool.pool_rank(0, 0)
    view.set_photons(S.jet_photons(3, N_PHOTONS))
    pool_before, view_before = pool.device_bytes(), view.device_bytes()
    res = call(view)
    assert res["n_total"] == N_PHOTONS
    assert view.device_bytes() == view_before
    assert pool.device_bytes() - pool_before >= FIXED + N_PHOTONS * (ROW + SORT_ROW) + SORT_TABLE
    whole = call(pool, time_now=np.array([40.0, 41.0]), pool=True)                          # with the two clocks and the pool's chunks: the block grows once more, on the pool
    assert whole["n_total"] == N_PHOTONS and view.device_bytes() == view_before
    for k in ("rank", "slot", "t", "e", "w", "type"):
        assert whole[k].tobytes() == res[k].tobytes(), k                                    # the view's photons are the pool's rows
    grown = pool.device_bytes()
    assert grown - pool_before >= FIXED + N_PHOTONS * (ROW + SORT_ROW) + SORT_TABLE + 8 * 2
    call(pool, time_now=np.array([40.0, 41.0]), pool=True)
    call(view)                                                                              # (a smaller need: the block stays)
    assert pool.device_bytes() == grown
    pool.close()
