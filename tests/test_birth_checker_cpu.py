"""tests/birth_checker.py on the CPU: its invariants hold on the oracle's photon injection and pool emission in all nine (DIMENSIONS, GEOMETRY) pairs,
and each of them FAILS on an input that is wrong in the way it is there to catch.  The inputs are those of tests/test_gpu_birth_geometries.py: the
frames of tests.test_gpu_instantiations._case, the slab laid around the case's own photons (birth_checker.slab_around), weight 1e42, 2000 - 6000
photons, seed 2024.  (With this seed and these opening angles every premise holds in every pair -- a photon total well inside [2000, 6000], so that the
weight loop's truncation of the Poisson total does not bias it; no photon on a cell face.  Were one to fail for another seed, the seed or the angle
is what to change, not a margin.)"""
import functools

import numpy as np
import pytest

from mcrat_amd import synth
from tests import birth_checker as B
from tests.test_gpu_cyclosynch import _oracle_pool
from tests.test_gpu_instantiations import GEOMS, NAMES, PAIRS, _case

PAIR_IDS = ["%s-%s" % (NAMES[d], GEOMS[g]) for d, g in PAIRS]
WEIGHT, MIN_PHOTONS, MAX_PHOTONS, SEED = 1e42, 2000, 6000, 2024


@functools.lru_cache(maxsize=None)
def _injected(dims, geom, spect):
    from oracle import oracle_py as oracle
    frame, ph, cfg = _case(dims, geom, 0)
    args = dict(B.slab_around(ph), spect=spect)
    ref, w = oracle.photon_injection(oracle.make_config(dims, geom, 0), oracle.OracleHydro(frame), args["r_inj"], WEIGHT, MIN_PHOTONS, MAX_PHOTONS, spect,
                                     args["theta_min"], args["theta_max"], seed=SEED)
    ref.setflags(write=False)
    return frame, cfg, args, ref, w


@pytest.mark.parametrize("spect", ["b", "w"])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_the_oracles_injection_passes(oracle, pair, spect):
    frame, cfg, args, ref, w = _injected(*pair, spect)
    assert MIN_PHOTONS <= len(ref) <= MAX_PHOTONS
    rep = B.check_injection(frame, cfg, ref, w, args)
    assert rep["photons"] == len(ref) and rep["cells_hit"] >= 6


@pytest.mark.parametrize("b_field_calc", [1])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_the_oracles_pool_emission_passes(oracle, pair, b_field_calc):
    frame, ph, cfg = _case(*pair, 1)
    args = dict(B.slab_around(ph), scatt_frame_number=200, inj_frame_number=200)
    aos = synth.photons_to_aos(ph, oracle.PHOTON_DTYPE)
    n, w, fb, before, after = _oracle_pool(oracle, frame, cfg, aos, range(1, len(aos), 2), np.ascontiguousarray(frame["dens"]), b_field_calc, 77, 1500,
                                           r_inj=args["r_inj"], theta_min=args["theta_min"], theta_max=args["theta_max"])
    new = np.flatnonzero((before["type"] == b"N") & (after["type"] != b"N"))
    assert 10 <= n == len(new) <= 150
    B.check_pool_emission(frame, cfg, after[new], w, args)
    # the shell a hundred frames later (100 c / fps further out: beyond the widest cell here) holds none of them
    with pytest.raises(AssertionError, match="outside the emission shell"):
        B.check_pool_emission(frame, cfg, after[new], w, dict(args, scatt_frame_number=300))


def _columns(ref):
    return {k: np.array(ref[k]) for k in ref.dtype.names}


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_swapped_axes_are_rejected(oracle, pair):
    frame, cfg, args, ref, w = _injected(*pair, "b")
    bad = _columns(ref)
    bad["r0"], bad["r2"] = bad["r2"], bad["r0"]
    with pytest.raises(AssertionError, match="lie in no cell|outside the injection slab"):
        B.check_injection(frame, cfg, bad, w, args)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_a_boost_with_the_wrong_sign_is_rejected(oracle, pair):
    frame, cfg, args, ref, w = _injected(*pair, "b")
    bad = _columns(ref)
    a = B.mcrat_to_hydro(*pair, bad["r0"], bad["r1"], bad["r2"])
    cell, _, _ = B.containing_cells(frame, *a, cells=B.cells_meeting_box(frame, *a))
    beta = synth.hydro_vector_to_cartesian(frame, cell, np.arctan2(bad["r1"], bad["r0"]))
    for sign in (-1.0, +1.0):
        p = synth.lorentz_boost(sign * beta, np.stack([bad["comv_p%d" % k] for k in range(4)], axis=-1))
        p[:, 1:] *= (p[:, 0] / np.sqrt(np.sum(p[:, 1:] ** 2, axis=-1)))[:, None]        # null again, as the reference's boost leaves it
        for k in range(4):
            bad["p%d" % k] = p[:, k].copy()
        if sign < 0:
            B.check_injection(frame, cfg, bad, w, args)                                  # the right sign, rebuilt the same way, passes
        else:
            with pytest.raises(AssertionError, match="p is not comv_p boosted"):
                B.check_injection(frame, cfg, bad, w, args)


# a formula of ANOTHER geometry that the same frame can be put through (it has the columns the formula reads)
OTHER_VOLUME = {(synth.TWO, synth.CARTESIAN): (synth.TWO, synth.SPHERICAL), (synth.TWO, synth.CYLINDRICAL): (synth.TWO, synth.SPHERICAL),
                (synth.TWO, synth.SPHERICAL): (synth.TWO, synth.CYLINDRICAL),
                (synth.TWO_POINT_FIVE, synth.CARTESIAN): (synth.TWO, synth.SPHERICAL), (synth.TWO_POINT_FIVE, synth.CYLINDRICAL): (synth.TWO, synth.SPHERICAL),
                (synth.TWO_POINT_FIVE, synth.SPHERICAL): (synth.TWO, synth.CYLINDRICAL),
                (synth.THREE, synth.CARTESIAN): (synth.THREE, synth.POLAR), (synth.THREE, synth.SPHERICAL): (synth.THREE, synth.POLAR),
                (synth.THREE, synth.POLAR): (synth.THREE, synth.CARTESIAN)}


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_a_volume_from_another_geometry_is_rejected(oracle, pair, monkeypatch):
    frame, cfg, args, ref, w = _injected(*pair, "b")
    right = B.cell_volume
    monkeypatch.setattr(B, "cell_volume", lambda frame, dims, geom, idx: right(frame, *OTHER_VOLUME[(dims, geom)], idx))
    with pytest.raises(AssertionError, match="photons where the slab's mean is"):
        B.check_injection(frame, cfg, ref, w, args)


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_a_thinned_list_is_rejected(oracle, pair):
    frame, cfg, args, ref, w = _injected(*pair, "b")
    keep = np.random.default_rng(3).random(len(ref)) < 0.8
    with pytest.raises(AssertionError, match="photons where the slab's mean is"):
        B.check_injection(frame, cfg, ref[keep], w, args)


@pytest.mark.parametrize("spect", ["b", "w"])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_scaled_energies_are_rejected(oracle, pair, spect):
    frame, cfg, args, ref, w = _injected(*pair, spect)
    bad = _columns(ref)
    for k in range(4):
        bad["p%d" % k] *= 1.1
        bad["comv_p%d" % k] *= 1.1
    with pytest.raises(AssertionError, match="<h nu / kT>"):
        B.check_injection(frame, cfg, bad, w, args)


def test_other_fields_are_checked(oracle):
    frame, cfg, args, ref, w = _injected(synth.TWO, synth.CARTESIAN, "b")
    for k, v in (("s1", 0.1), ("num_scatt", 1.0), ("weight", 2 * w), ("type", b"p")):
        bad = _columns(ref)
        bad[k][7] = v
        with pytest.raises(AssertionError, match=k):
            B.check_injection(frame, cfg, bad, w, args)


def test_the_restricted_scan_is_the_full_scan(oracle):
    """the 32768-cell mesh: scanning only the cells that meet the photons' bounding box finds the same cells as scanning all of them"""
    pair = (synth.TWO, synth.SPHERICAL)
    frame, cfg, args, ref, w = _injected(*pair, "b")
    assert frame["num_elements"] == 32768
    a = B.mcrat_to_hydro(*pair, ref["r0"], ref["r1"], ref["r2"])
    some = B.cells_meeting_box(frame, *a)
    assert 0 < some.size < frame["num_elements"] // 20
    full, part = B.containing_cells(frame, *a), B.containing_cells(frame, *a, cells=some)
    for f, p in zip(full, part):
        assert np.array_equal(f, p)


def test_cells_on_faces_and_outside():
    """closed intervals: a point on a shared face lies in both cells and belongs to the lower index; one outside the mesh lies in none"""
    frame = synth.uniform_mesh_2d(0.0, 4.0, 4, 0.0, 2.0, 2, synth.CARTESIAN, (0.0, 4.0), (0.0, 2.0), 5.0)
    a0, a1 = np.array([0.5, 1.0, 1.0, 5.0, 2.0]), np.array([0.5, 0.5, 1.0, 0.5, 1.5])
    cell, count, interior = B.containing_cells(frame, a0, a1, np.zeros(5))
    assert cell.tolist() == [0, 0, 0, -1, 5] and count.tolist() == [1, 2, 4, 0, 2] and interior.tolist() == [True, False, False, False, False]


def test_the_inverse_map_inverts_the_forward_map():
    """mcrat_to_hydro against the forward expressions of geometry.c:108-154, in all nine pairs, azimuths in all four quadrants"""
    g = np.random.default_rng(0)
    n = 200
    for dims, geom in PAIRS:
        phi = g.uniform(0, 2 * np.pi, n)
        if geom == synth.SPHERICAL:
            r, th = g.uniform(1e11, 1e12, n), g.uniform(0.01, 3.0, n)
            x, y, z = r * np.sin(th) * np.cos(phi), r * np.sin(th) * np.sin(phi), r * np.cos(th)
            want = (r, th, phi if dims == synth.THREE else 0 * phi)
        elif dims == synth.THREE and geom == synth.CARTESIAN:
            x, y, z = g.uniform(-1e11, 1e11, (3, n))
            want = (x, y, z)
        else:
            rho, zz = g.uniform(1e9, 1e11, n), g.uniform(-1e12, 1e12, n)
            x, y, z = rho * np.cos(phi), rho * np.sin(phi), zz
            want = (rho, phi, zz) if geom == synth.POLAR else (rho, zz, 0 * phi)
        got = B.mcrat_to_hydro(dims, geom, x, y, z)
        for a, b in zip(got, want):
            assert np.allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max()), (dims, geom)
