"""mcrat_hip_device_bytes counts the device block of the seventh analysis product, the resampled sky observation (include/mcrat_hip.h: "HBM held by
the context"): its first call allocates the block and the figure grows by at least what resample_plan.hpp lays out for it; a second call of the same
size finds the block and leaves the figure alone; the block is counted on the pool, not on a view.  The shape is the smallest that allocates: 3
photons, one observer, one bin on every axis, four jackknife groups.  The bytes are worked out here from the documented layout, not read back from
the library.  (The pattern of tests/test_gpu_escape_device_bytes.py.)"""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import sky_checker as S

pytestmark = pytest.mark.gpu

N_PHOTONS, N_REP = 3, 4
# seven 8-byte planes of one bin per group and three per-observer counters; the staged inputs -- n0, n1, n2, cos_acc, two edges each for t and e
PLANES_COUNTERS = 7 * 8 * N_REP + 3 * 8
STAGED = 8 * (4 + 2 + 2)


def call(e, time_now=40.0, pool=False, n_rep=N_REP):
    from mcrat_amd import engine
    f = e.pool_observe_sky_resampled if pool else e.observe_sky_resampled
    return f([0.0, 0.0, 1.0], [-1.0], [-1e9, 1e9], [1e-300, 1e300], time_now, engine.RESAMPLE_JACKKNIFE, n_rep, engine.STOKES_AS_STORED, 5)


def test_device_bytes_counts_the_resample_block():
    from mcrat_amd import engine
    engine.load_library()
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    e.set_photons(S.jet_photons(3, N_PHOTONS))
    need = PLANES_COUNTERS + STAGED
    assert need == 248 + 64
    before = e.device_bytes()
    res = call(e)
    after = e.device_bytes()
    print("observe_sky_resampled: device_bytes %d -> %d, the block needs %d" % (before, after, need))
    assert res["count"].shape == (1, N_REP, 1, 1) and res["count"].sum() == N_PHOTONS == res["n_accepted"][0]
    assert after - before >= need
    call(e)
    assert e.device_bytes() == after
    sky = e.observe_sky([0.0, 0.0, 1.0], [-1.0], [-1e9, 1e9], [1e-300, 1e300], 40.0)      # a block of its own: observe_sky's does not shrink or replace it
    assert e.device_bytes() > after and sky["count"].sum() == N_PHOTONS
    grown = e.device_bytes()
    call(e)
    call(e, n_rep=2)                                                                        # (a smaller need: the block stays)
    assert e.device_bytes() == grown
    call(e, n_rep=64)                                                                       # a larger one: it grows by at least the difference
    assert e.device_bytes() - grown >= 7 * 8 * (64 - N_REP)
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
    assert res["count"].sum() == N_PHOTONS
    assert view.device_bytes() == view_before
    assert pool.device_bytes() - pool_before >= PLANES_COUNTERS + STAGED
    whole = call(pool, time_now=np.array([40.0, 41.0]), pool=True)                          # with the two clocks behind the staged inputs: the block grows once more, on the pool
    assert whole["count"].sum() == N_PHOTONS and view.device_bytes() == view_before
    assert np.array_equal(whole["count"], res["count"])                                     # the view's photons keep their groups in the pool's call
    grown = pool.device_bytes()
    assert grown - pool_before >= PLANES_COUNTERS + STAGED + 8 * 2
    call(pool, time_now=np.array([40.0, 41.0]), pool=True)
    call(view)                                                                              # (a smaller need: the block stays)
    assert pool.device_bytes() == grown
    pool.close()
