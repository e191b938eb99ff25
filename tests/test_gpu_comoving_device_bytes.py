"""mcrat_hip_device_bytes counts the device block of the fifth analysis product, the comoving field (include/mcrat_hip.h: "HBM held by the
context"): its first call allocates the block and the figure grows by at least what comoving_plan.hpp lays out for it; a second identical call finds
the block and leaves the figure alone.  The shape is the smallest that allocates: one list of 3 photons, a staged 2 x 2 frame, 1 x 1 shells x 1
energy x 1 cosine.  The bytes are worked out here from the documented layout, not read back from the library.  (The four older blocks:
tests/test_gpu_device_bytes.py.)"""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import comoving_checker as cc
from tests import radfield_checker as rc
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

N_PHOTONS, N_CELLS = 3, 4
# a 256-B head, eight 8-byte planes of one bin, then the eight staged edges (two per axis): 256 + 64 + 64 bytes before padding
NEED = 256 + 8 * 8 * 1 + 8 * (2 + 2 + 2 + 2)


def test_device_bytes_counts_the_comoving_block():
    from mcrat_amd import engine
    engine.load_library()
    frame = synth.uniform_mesh_2d(0.0, 1.6e11, 2, 1e12, 1.16e12, 2, synth.CYLINDRICAL, (0.0, 1.6e11), (1e12, 1.16e12), 5.0)
    frame["dimensions"] = synth.TWO
    frame = sc.random_fluid(frame, 4242)
    assert frame["num_elements"] == N_CELLS and NEED == 384
    ph = rc.photon_list(rc.points_in_cells(frame, [0, 1, 3], 4243), rc.momenta(4244, N_PHOTONS), 4245, exclusions=False)
    e = engine.Engine(frame["dimensions"], frame["geometry"], 0)
    e.set_hydro(frame)
    e.set_photons(ph)
    call = lambda: e.comoving_field(cc.SHELLS, [1e-300, 1e300], [-1.0, 2.0], [1e11, 1e13], [-1.0, 2.0])
    before = e.device_bytes()
    res = call()
    after = e.device_bytes()
    print("comoving_field: device_bytes %d -> %d, the block needs %d" % (before, after, NEED))
    assert res["count"].shape == (1, 1, 1, 1) and res["count"].sum() == N_PHOTONS == res["n_observable"]
    assert after - before >= NEED
    call()
    assert e.device_bytes() == after
    rad = e.radiation_field(rc.CELLS)                          # a block of its own: the radiation field's does not shrink or replace it
    assert e.device_bytes() > after and rad["count"].sum() == N_PHOTONS
    grown = e.device_bytes()
    call()
    assert e.device_bytes() == grown
    e.close()
