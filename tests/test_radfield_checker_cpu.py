"""tests/radfield_checker.py on its own: the conditions its committed cases must meet for the GPU test to be exact -- no photon within 1e-9 of a cell's
size of a face --, conservation, and closed-form answers of the restatement itself."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import radfield_checker as rc
from tests import sightline_checker as sc


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_no_committed_case_holds_a_fragile_photon(name):
    for mode in (rc.CELLS, rc.SHELLS):
        w = rc.want(name, mode)
        assert w["n_fragile"] == 0, (name, mode)
        assert int(w["count"].sum()) + w["n_unlocated"] + w["n_outside"] == w["n_observable"], (name, mode)
        assert w["n_observable"] > 0


@pytest.mark.parametrize("gamma_max", [10.0, 100.0])
def test_the_seeded_meshes_hold_no_fragile_photon_in_18000(gamma_max):
    """sightline_checker.mesh(dims, geom) with random_fluid(500 + k) and rays_in(1500 + k, 1000): all nine pairs, both Lorentz-factor ranges; and the
    largest conditioning bar of the comoving energy stays what the bound's derivation quotes"""
    worst = 0.0
    for k, (dims, geom) in enumerate(sc.PAIRS):
        frame = sc.random_fluid(sc.mesh(dims, geom), 500 + k, gamma_max)
        r, p = sc.rays_in(frame, 1500 + k, 1000)
        q = rc.per_photon(frame, rc.photon_list(r, p, 1, exclusions=False))
        assert not q["near"].any(), (dims, geom, np.nonzero(q["near"])[0])
        assert (q["cell"] >= 0).sum() > 800
        worst = max(worst, float(q["bar_e"].max()))
    print("gamma_max %g: largest bar_e = %.3g" % (gamma_max, worst))
    assert worst <= (2.6e-11 if gamma_max == 10.0 else 1.6e-8) * 1.05


def test_cases_exercise_what_they_are_named_for():
    w = rc.want("crowded_4", rc.CELLS)
    assert (w["count"] > 0).sum() == 4 and w["count"].sum() == 1000
    w = rc.want("crowded_1", rc.CELLS)
    assert (w["count"] > 0).sum() == 1 and w["count"].max() == 1000
    w = rc.want("spread", rc.CELLS)
    assert w["count"].max() == 1 and w["count"].sum() == 1000 and w["count"].shape == (1024,)
    assert np.array_equal(np.sort(np.nonzero(w["count"])[0]), np.sort(rc.case("spread")["cells"]))
    gap, c = rc.want("gap", rc.CELLS), rc.case("gap")
    whole = rc.field(c["whole"], c["ph"], rc.CELLS)
    assert gap["n_unlocated"] > whole["n_unlocated"] + 20 and whole["n_unlocated"] > 10       # the gap, and the photons beyond the domain
    sh = rc.want("shells", rc.SHELLS)
    assert sh["n_outside"] > 20 and (sh["count"] > 0).sum() > 12 and sh["count"].shape == (8, 4)
    ph = rc.case("shells")["ph"]
    assert sh["n_observable"] == int(((ph["weight"] != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")).sum()) < 800


def one_cell_frame(v0, v1, gamma):
    frame = sc.mesh(synth.TWO, synth.CYLINDRICAL)
    m = frame["num_elements"]
    frame.update(v0=np.full(m, v0), v1=np.full(m, v1), gamma=np.full(m, gamma), dens_lab=np.full(m, 1e-10), temp=np.full(m, 3e6))
    frame["dens"] = frame["dens_lab"] / gamma
    frame["pres"] = synth.A_RAD * frame["temp"] ** 4.0 / 3
    return frame


def test_a_cell_at_rest_gives_the_lab_energy_bit_for_bit():
    frame = one_cell_frame(0.0, 0.0, 1.0)
    r, p = sc.rays_in(frame, 7, 500)
    ph = rc.photon_list(r, p, 8)
    w = rc.field(frame, ph, rc.CELLS)
    assert w["count"].sum() > 300
    assert np.array_equal(w["we_comv"].view(np.int64), w["we_lab"].view(np.int64))
    q = w["q"]
    at = q["cell"] >= 0
    assert np.array_equal(q["e_comv"][at].view(np.int64), q["e_lab"][at].view(np.int64))


@pytest.mark.parametrize("gamma", [1.5, 10.0, 100.0])
def test_a_photon_along_the_flow_is_redshifted_by_gamma_one_minus_beta(gamma):
    """the flow along +z (v1 of a 2-D cylindrical cell), the photon along +z: e_comv = e_lab Gamma (1 - beta), within the bar"""
    beta = np.sqrt(1.0 - 1.0 / (gamma * gamma))
    frame = one_cell_frame(0.0, beta, gamma)
    n = 200
    r = rc.points_in_cells(frame, np.arange(n), 3)
    p0 = 10.0 ** np.random.default_rng(4).uniform(-20.0, -16.0, n)
    p = np.stack([p0, np.zeros(n), np.zeros(n), p0])
    q = rc.per_photon(frame, rc.photon_list(r, p, 5, exclusions=False))
    assert (q["cell"] == np.arange(n)).all()
    expect = q["e_lab"] * (gamma * (1.0 - beta))
    one_minus = 1.0 / (gamma * gamma * (1.0 + beta))            # 1 - beta without the cancellation
    exact = q["e_lab"] * (gamma * one_minus)
    assert (np.abs(q["e_comv"] - exact) <= q["bar_e"] * exact).all()
    assert np.allclose(expect, exact, rtol=1e-6 if gamma > 50 else 1e-10)
    assert (q["bar_e"] < 4e-16 * 8 * 2 * (1 + gamma ** 2) / one_minus).all()


def test_one_photon_per_cell_gives_a_count_of_ones():
    frame = sc.random_fluid(sc.mesh(synth.TWO, synth.CYLINDRICAL), 11)
    m = frame["num_elements"]
    r = rc.points_in_cells(frame, np.arange(m), 12)
    w = rc.field(frame, rc.photon_list(r, rc.momenta(13, m), 14, exclusions=False), rc.CELLS)
    assert np.array_equal(w["count"], np.ones(m, dtype=np.int64)) and w["n_unlocated"] == 0 and w["n_fragile"] == 0
    assert np.array_equal(w["w"], rc.photon_list(r, rc.momenta(13, m), 14, exclusions=False)["weight"])
    assert (w["bound_we_comv"] > w["bound_we_lab"]).all()


def test_find_bin_is_half_open():
    e = np.array([1.0, 2.0, 4.0])
    assert rc.find_bin(e, np.array([0.5, 1.0, 1.99, 2.0, 3.9, 4.0, np.nan, np.inf])).tolist() == [-1, 0, 0, 1, 1, -1, -1, -1]
