"""tests/escape_checker.py on the CPU: the checker against hand-built photons whose bin and tau are known in closed form -- a slab of uniform kappa
crossed along the axis, a photon outside the mesh, one that goes opaque, one at the step cap -- and the condition tests/test_gpu_escape.py relies on:
with the tau edges (0, 0.1, 0.3, 1, 3, 10, 30) no case has a fragile photon (the GPU test tolerates one), every tau bin is populated, several photons
land beyond 30 (n_outside), and the three observers accept a real fraction of the photons by none, by one and by several."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import escape_checker as ec
from tests import sightline_checker as sc
from tests import sky_checker as S

H = 1.03e9                          # the step: 155.3 of them cross the 16 x 16 mesh's 1.6e11 cm
GAMMA, DENS_LAB = 2.0, 2.5e-10
BETA = np.sqrt(1.0 - 1.0 / GAMMA ** 2)
KAPPA = (DENS_LAB / synth.M_P) * synth.THOM_X_SECT * (1.0 - BETA)           # a photon along the fluid's velocity: n sigma_T (1 - beta)


def slab():
    """the sightline checker's 2-D cylindrical mesh with one fluid everywhere, moving up the axis with Lorentz factor 2"""
    frame = sc.mesh(synth.TWO, synth.CYLINDRICAL)
    m = frame["num_elements"]
    frame.update(v0=np.zeros(m), v1=np.full(m, BETA), gamma=np.full(m, GAMMA), dens_lab=np.full(m, DENS_LAB), temp=np.full(m, 1e7))
    frame["dens"] = frame["dens_lab"] / GAMMA
    frame["pres"] = synth.A_RAD * frame["temp"] ** 4.0 / 3
    return frame


def hand_built():
    """five photons along +z at x = 1.5e10, the middle of a cell: from z = 1.10e12, 1.15e12 and 1.00e12 + 1 inside the mesh, one from beyond its far edge in r (outside),
    and one more from 1.10e12 that another call stops early"""
    z0 = np.array([1.10e12, 1.15e12, 1.0e12 + 1.0, 1.05e12, 1.10e12])
    x0 = np.array([1.5e10, 1.5e10, 1.5e10, 2.0e11, 1.5e10])
    r = np.stack([x0, np.zeros(5), z0])
    p0 = np.full(5, 1e-18)
    p = np.stack([p0, np.zeros(5), np.zeros(5), p0])
    return r, p, S.photon_list(r, p, 31)


def steps_to_edge(z0):
    """counted steps: the k with a midpoint z0 + (k + 1/2) h strictly below the domain's edge"""
    k = 0
    while z0 + (k + 0.5) * H < 1.16e12:
        k += 1
    return k


def test_uniform_slab_in_closed_form():
    frame = slab()
    r, p, ph = hand_built()
    marched = sc.march(frame, r, p, 0.0, H, 400)
    want_steps = np.array([steps_to_edge(z) for z in r[2]])
    want_steps[3] = 0
    assert np.array_equal(marched["steps"], want_steps) and (marched["status"] == sc.LEFT_MESH).all()
    want_tau = want_steps * KAPPA * H
    assert np.allclose(marched["tau"], want_tau, rtol=1e-12, atol=0.0) and marched["tau"][3] == 0.0 and marched["bound"][3] == 0.0
    assert 0.5 < want_tau[0] < 1.5 and want_tau[1] < 0.3 and want_tau[2] > 1.5          # the case spans three tau bins
    n, cos_acc = np.array([[0.0], [0.0], [1.0]]), np.array([np.cos(0.1)])
    tau_edges = [0.0, 0.3, 1.5, 100.0]
    t_edges, e_edges = [0.0, 40.0 - 1.10e12 / S.C_LIGHT, 10.0], [1e-10, 1e-5]
    want = ec.observation(ph, marched, n, cos_acc, t_edges, e_edges, tau_edges, 40.0)
    ec.identities(want)
    # the time bins: z0 < 1.10e12 is detected later than the edge 40 - 1.10e12 / c, z0 == 1.10e12 exactly at it (the bin it opens), z0 beyond earlier
    cube = np.zeros((1, 3, 2, 1), dtype=np.int64)
    cube[0, 1, 1, 0] = 2                 # photons 0 and 4: tau ~ 0.98, t_det on the edge
    cube[0, 0, 0, 0] = 1                 # photon 1: tau ~ 0.16, from 1.15e12
    cube[0, 0, 1, 0] = 1                 # photon 3 outside the mesh: tau = 0 in the bin that holds 0
    cube[0, 2, 1, 0] = 1                 # photon 2: the whole mesh
    assert np.array_equal(want["count"], cube)
    assert want["n_accepted"][0] == 5 and want["n_selected"] == 5 and not want["n_outside"].any() and not want["fragile"].any()
    w, e = ph["weight"], ph["p0"] * S.C_LIGHT
    assert np.isclose(want["wx"][0, 0, 0, 0], w[1] * np.exp(-want_tau[1]), rtol=1e-12) and want["wx"][0, 0, 1, 0] == w[3] == want["w"][0, 0, 1, 0]
    assert np.isclose(want["wex"][0, 2, 1, 0], w[2] * e[2] * np.exp(-want_tau[2]), rtol=1e-12)
    assert want["w"][0, 0, 0, 0] == w[1] and np.isclose(want["tol_wx"][0, 2, 1, 0], w[2] * np.exp(-want_tau[2]) * (marched["bound"][2] + 3 * ec.U))


def test_opaque_step_cap_and_outside_go_to_their_counters():
    frame = slab()
    r, p, ph = hand_built()
    n, cos_acc = np.array([[0.0], [0.0], [1.0]]), np.array([np.cos(0.1)])
    stopped = ec.observation(ph, sc.march(frame, r, p, 0.0, H, 400, tau_stop=1.5), n, cos_acc, [0.0, 10.0], [1e-10, 1e-5], ec.TAU_EDGES, 40.0)
    assert stopped["n_opaque"][0] == 1 and stopped["status"][2] == sc.OPAQUE and stopped["count"].sum() == 4 and stopped["n_status"][sc.OPAQUE] == 1
    capped = ec.observation(ph, sc.march(frame, r, p, 0.0, H, 20), n, cos_acc, [0.0, 10.0], [1e-10, 1e-5], ec.TAU_EDGES, 40.0)
    # 20 steps: photon 1 (10 steps to the edge) and photon 3 (outside) still leave
    assert capped["n_unresolved"][0] == 3 and capped["count"].sum() == 2 and capped["n_status"][sc.STEP_CAP] == 3
    for want in (stopped, capped):
        ec.identities(want)
        assert want["n_accepted"][0] == 5
    # nobody accepts: nothing is marched; a tau beyond the last edge is outside; a tau within its bound of an edge is fragile, tau = 0 at bound 0 is not
    away = ec.observation(ph, sc.march(frame, r, p, 0.0, H, 400), np.array([[1.0], [0.0], [0.0]]), np.array([0.9]), [0.0, 10.0], [1e-10, 1e-5], ec.TAU_EDGES, 40.0)
    assert away["n_selected"] == 0 and not away["n_status"].any() and away["n_observable"] == 5 and not away["count"].any()
    marched = sc.march(frame, r, p, 0.0, H, 400)
    beyond = ec.observation(ph, marched, n, cos_acc, [0.0, 10.0], [1e-10, 1e-5], [0.0, 0.5], 40.0)
    assert beyond["n_outside"][0] == 3 and beyond["count"].sum() == 2
    edge = ec.observation(ph, marched, n, cos_acc, [0.0, 10.0], [1e-10, 1e-5], [0.0, marched["tau"][0] + 0.5 * marched["bound"][0], 50.0], 40.0)
    assert np.array_equal(edge["fragile"], [True, False, False, False, True])


@pytest.mark.parametrize("name", ec.GPU_CASES)
def test_no_case_has_a_fragile_photon(name):
    k = ec.case(name)
    want, c = k["want"], k["c"]
    assert int(want["fragile"].sum()) == 0, (name, np.nonzero(want["fragile"])[0])
    assert int(c["want"]["fragile"].sum()) == 0, name                              # the sightline checker's own marks, of every ray
    left = want["selected"] & (want["status"] == sc.LEFT_MESH)
    near = (np.abs(want["tau"][left][None, :] - ec.TAU_EDGES[:, None]) <= want["bound"][left][None, :]).any(axis=0)
    assert not (near & ~((want["tau"][left] == 0) & (want["bound"][left] == 0))).any(), name
    ec.identities(want, name)


def test_cases_populate_every_tau_bin_and_every_counter():
    wants = {name: ec.case(name)["want"] for name in ec.GPU_CASES}
    per_tau = sum(w["count"].sum(axis=(0, 2, 3)) for w in wants.values())
    assert (per_tau > 0).all(), per_tau
    beyond = sum(int((w["selected"] & (w["status"] == sc.LEFT_MESH) & (w["tau"] >= 30.0)).sum()) for w in wants.values())
    assert beyond >= 3, beyond
    zero = sum(int((w["selected"] & (w["tau"] == 0) & (w["bound"] == 0) & (w["status"] == sc.LEFT_MESH)).sum()) for w in wants.values())
    assert zero >= 3, zero                                                          # photons that start outside the frame: tau = 0 exactly
    assert wants["opaque"]["n_opaque"].sum() > 50 and wants["cap_7"]["n_unresolved"].sum() > 50 and wants["table_off"]["n_unresolved"].sum() > 10
    assert wants["table_in"]["n_outside"].sum() > 0
    w = wants["pair_2_1"]
    assert w["n_selected"] < w["n_observable"] < 257 and (w["n_accepted"] > 10).all()
    n, cos_acc, _, _ = ec.observers()
    by = S.per_photon(ec.case("pair_2_1")["ph"], n, cos_acc, ec.T_EDGES, ec.E_EDGES, ec.TIME_NOW)["accepted"].sum(axis=0)
    assert (by == 0).sum() > 20 and (by == 1).sum() > 10 and (by >= 2).sum() > 10, np.bincount(by)
