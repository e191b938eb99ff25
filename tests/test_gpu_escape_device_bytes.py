"""mcrat_hip_device_bytes counts the device block of the sixth analysis product, the escape-weighted sky observation (include/mcrat_hip.h: "HBM held
by the context"): its first call allocates the block and the figure grows by at least what escape_plan.hpp lays out for it; a second call of the
same size finds the block and leaves the figure alone; the block is counted on the pool, not on a view.  The shape is the smallest that allocates:
3 photons, a staged 2 x 2 frame, one observer, one bin on every axis.  The bytes are worked out here from the documented layout, not read back from
the library.  (The pattern of tests/test_gpu_comoving_device_bytes.py.)"""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import radfield_checker as rc
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

N_PHOTONS, N_CELLS = 3, 4
# nine 8-byte planes of one bin, four per-observer counters, the head of eight words; the staged inputs -- n0, n1, n2, cos_acc, two edges each for t, e
# and tau --; then per slot tau (8 bytes), index and status (4 each)
PLANES_COUNTERS_HEAD = 9 * 8 + 4 * 8 + 8 * 8
STAGED = 8 * (4 + 2 + 2 + 2)
PER_SLOT = 8 + 4 + 4


def frame_and_photons():
    frame = synth.uniform_mesh_2d(0.0, 1.6e11, 2, 1e12, 1.16e12, 2, synth.CYLINDRICAL, (0.0, 1.6e11), (1e12, 1.16e12), 5.0)
    frame["dimensions"] = synth.TWO
    frame = sc.random_fluid(frame, 4242)
    assert frame["num_elements"] == N_CELLS
    return frame, rc.photon_list(rc.points_in_cells(frame, [0, 1, 3], 4243), rc.momenta(4244, N_PHOTONS), 4245, exclusions=False)


def call(e, time_now=40.0, pool=False):
    f = e.pool_observe_escaping if pool else e.observe_escaping
    return f([0.0, 0.0, 1.0], [-1.0], [-1e9, 1e9], [1e-300, 1e300], [0.0, 1e300], time_now, 1e-3, 1e8, 4000)


def test_device_bytes_counts_the_escape_block():
    from mcrat_amd import engine
    engine.load_library()
    frame, ph = frame_and_photons()
    e = engine.Engine(frame["dimensions"], frame["geometry"], 0)
    e.set_hydro(frame)
    e.set_photons(ph)
    slots = len(e.sightline_photons(1e-3, 1e8, 4000)["tau"])
    need = PLANES_COUNTERS_HEAD + STAGED + PER_SLOT * slots
    assert PLANES_COUNTERS_HEAD == 168 and STAGED == 80 and slots >= N_PHOTONS
    before = e.device_bytes()
    res = call(e)
    after = e.device_bytes()
    print("observe_escaping: device_bytes %d -> %d, the block needs %d for %d slots" % (before, after, need, slots))
    assert res["count"].shape == (1, 1, 1, 1) and res["count"].sum() == N_PHOTONS == res["n_observable"] == res["n_selected"] == res["n_status"][1]
    assert after - before >= need
    call(e)
    assert e.device_bytes() == after
    sky = e.observe_sky([0.0, 0.0, 1.0], [-1.0], [-1e9, 1e9], [1e-300, 1e300], 40.0)      # a block of its own: observe_sky's does not shrink or replace it
    assert e.device_bytes() > after and sky["count"].sum() == N_PHOTONS
    grown = e.device_bytes()
    call(e)
    assert e.device_bytes() == grown
    e.close()


def test_the_block_is_counted_on_the_pool_not_on_a_view():
    from mcrat_amd import engine
    engine.load_library()
    frame, ph = frame_and_photons()
    pool = engine.Engine(frame["dimensions"], frame["geometry"], 0)
    pool.set_hydro(frame)
    pool.pool_create(2, 256)
    view = pool.pool_rank(0, 0)
    view.set_photons(ph)
    pool_before, view_before = pool.device_bytes(), view.device_bytes()
    res = call(view)
    assert res["count"].sum() == N_PHOTONS
    assert view.device_bytes() == view_before
    assert pool.device_bytes() - pool_before >= PLANES_COUNTERS_HEAD + STAGED + PER_SLOT * N_PHOTONS
    whole = call(pool, time_now=np.array([40.0, 41.0]), pool=True)                          # every slot of the pool: the block grows once more, on the pool
    assert whole["count"].sum() == N_PHOTONS and view.device_bytes() == view_before
    grown = pool.device_bytes()
    assert grown - pool_before >= PLANES_COUNTERS_HEAD + STAGED + 8 * 2 + PER_SLOT * 2 * 256
    call(pool, time_now=np.array([40.0, 41.0]), pool=True)
    call(view)                                                                              # (a smaller need: the block stays)
    assert pool.device_bytes() == grown
    pool.close()
