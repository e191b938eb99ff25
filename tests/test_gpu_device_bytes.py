"""mcrat_hip_device_bytes counts the device blocks of all four analysis products (include/mcrat_hip.h: "HBM held by the context"): the first call of
observe, observe_sky, sightline_photons and radiation_field each allocates its block, and the figure grows by at least what the product's plan
header lays out for it; a second identical call finds the block and leaves the figure alone.  The shapes are the smallest that allocate: one list of
3 photons, a staged 2 x 2 frame, one observer, 1 x 1 bins.  The bytes are worked out here from the documented layouts (observe_plan.hpp,
sky_plan.hpp, sightline_plan.hpp, radfield_plan.hpp), not read back from the library."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import radfield_checker as rc
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

N_PHOTONS, N_CELLS, N_OBS, N_T, N_E = 3, 4, 1, 1, 1


def align(x, a=256):
    return (x + a - 1) // a * a


def cube_block(vectors_per_observer):
    """seven 8-byte planes per bin, two 8-byte counters per observer, then the staged doubles: the observers' vectors, t_edges, e_edges (no clocks)"""
    n_bins = N_OBS * N_T * N_E
    return 7 * 8 * n_bins + 2 * 8 * N_OBS + 8 * (vectors_per_observer * N_OBS + (N_T + 1) + (N_E + 1))


# what each product's block holds at the least, in bytes: 136, 136, 256, 512
NEED = {
    "observe": cube_block(4),                                                 # cos_obs, sin_obs, cos_lo, cos_hi
    "observe_sky": cube_block(4),                                             # n0, n1, n2, cos_acc; no image axes
    # a head of eight 8-byte words, five double planes and three int planes of one entry per slot, padded to 256 B (the rays are the photons)
    "sightline_photons": align(8 * 8 + 5 * 8 * N_PHOTONS + 3 * 4 * N_PHOTONS),
    # CELLS: a 256-B head, six 8-byte words per cell (plane-major; a bin-major build holds more), padded to 256 B; no edges are staged
    "radiation_field": align(256 + 6 * 8 * N_CELLS),
}


def test_device_bytes_counts_every_analysis_block(hip_engine):
    e = hip_engine
    t_edges, e_edges = np.array([-1e30, 1e30]), np.array([1e-300, 1e300])
    calls = {
        "observe": lambda: e.observe([1.0], [0.0], [1.0], [-1.0], t_edges, e_edges, 0.0),
        "observe_sky": lambda: e.observe_sky(np.array([[0.0], [0.0], [1.0]]), [-1.0], t_edges, e_edges, 0.0),
        "sightline_photons": lambda: e.sightline_photons(0.5, 1e-6, 4),
        "radiation_field": lambda: e.radiation_field(rc.CELLS),
    }
    for name, call in calls.items():
        before = e.device_bytes()
        call()
        after = e.device_bytes()
        print("%s: device_bytes %d -> %d, the block needs %d" % (name, before, after, NEED[name]))
        assert after - before >= NEED[name], name
        call()
        assert e.device_bytes() == after, name


@pytest.fixture
def hip_engine():
    from mcrat_amd import engine
    engine.load_library()
    frame = synth.uniform_mesh_2d(0.0, 1.6e11, 2, 1e12, 1.16e12, 2, synth.CYLINDRICAL, (0.0, 1.6e11), (1e12, 1.16e12), 5.0)
    frame["dimensions"] = synth.TWO
    frame = sc.random_fluid(frame, 4242)
    assert frame["num_elements"] == N_CELLS
    ph = rc.photon_list(rc.points_in_cells(frame, [0, 1, 3], 4243), rc.momenta(4244, N_PHOTONS), 4245, exclusions=False)
    e = engine.Engine(frame["dimensions"], frame["geometry"], 0)
    e.set_hydro(frame)
    e.set_photons(ph)
    yield e
    e.close()
