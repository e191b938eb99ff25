"""Function-level parity on the device: every function of physics.hpp that restates a reference function is
evaluated on arrays through mcrat_hip_eval_function and compared with the oracle's restatement of that function -- on the committed
vectors of tests/golden/functions.npz and on the edge cases a trajectory reaches only by luck: both sides of the Klein-Nishina seam
(mcrat_scattering.c:610), a fluid at rest and gamma = 100 in lorentzBoost (mclib.c:302), photon directions along the flow and along
z in stokesRotation (mcrat_scattering.c:103), both sides of the 1e7 K switch of singleThermalElectron (electron.c:208), unpolarised
light in kleinNishinaScatter (mcrat_scattering.c:548).  Tolerances: no random numbers 1e-13; sampled quantities 1e-11 (the same
stream on both sides; the accepted sample is the same one, its value differs by libm's last ulps through a few boosts).
The arithmetic forms the loop kernels themselves call (boost_with, cell_staged_operands, optical_depth_staged, rcp_nr / rsqrt_nr / sqrt_nr, the
azimuth selects, hydro_coords, the table look-up) are in tests/test_gpu_loop_arithmetic.py, against extended precision."""
import ctypes as C
import os

import numpy as np
import pytest

from mcrat_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "functions.npz")
M_EL, C_LIGHT = synth.M_EL, synth.C_LIGHT


@pytest.fixture(scope="module")
def dev():
    from mcrat_amd import engine
    e = {s: engine.Engine(synth.TWO, synth.CYLINDRICAL, s) for s in (0, 1)}
    yield e
    for x in e.values():
        x.close()


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _rel(a, b, scale=None):
    a, b = np.asarray(a, float), np.asarray(b, float)
    s = np.maximum(np.abs(b), 1e-300) if scale is None else scale
    return float(np.max(np.abs(a - b) / s))


def _kn_tol(eps):
    """the exact branch (eps >= 1e-3, mcrat_scattering.c:610-615) subtracts terms of 2/eps^2 from one another down to O(1): an ulp of
    log(1 + 2 eps) -- where glibc and the device library may differ -- is worth 2/eps^2 ulps of the result"""
    eps = np.asarray(eps, float)
    return 1e-13 + np.where(eps >= 1e-3, 4e-16 * 2.0 / np.maximum(eps, 1e-3) ** 2, 0.0)


def test_klein_nishina_cross_section(dev, oracle):
    g = np.load(GOLD)
    got = dev[0].eval_function("kn_cross_section", g["kn_eps"])[:, 0]
    assert np.all(np.abs(got - g["kn_sigma"]) <= _kn_tol(g["kn_eps"]) * np.abs(g["kn_sigma"]))
    seam = np.array([1e-3, np.nextafter(1e-3, 0), np.nextafter(1e-3, 1), 0.0, 1e-300, 1e-6, 1.0, 50.0, 1e3, 1e6])
    got = dev[0].eval_function("kn_cross_section", seam)[:, 0]
    want = np.array([oracle.lib().orc_kleinNishinaCrossSection(float(e)) for e in seam])
    assert np.all(np.abs(got - want) <= _kn_tol(seam) * np.abs(want))
    # the 5e-6 step at the seam is reference behaviour (linear branch below 1e-3): it must be there on the device too
    assert got[1] == 1.0 - 2.0 * seam[1] and got[0] > got[1] and abs(got[0] - 0.99800519) < 1e-7 and got[3] == 1.0
    assert got[6] == pytest.approx(0.4307278419, abs=1e-9)


def test_lorentz_boost_photon_and_electron(dev, oracle):
    g = np.load(GOLD)
    rows = np.concatenate([g["boost_beta"], g["boost_p"]], axis=1)
    norm = np.abs(g["boost_out_photon"][:, :1])
    assert _rel(dev[0].eval_function("lorentz_boost_photon", rows), g["boost_out_photon"], norm) < 1e-13
    assert _rel(dev[0].eval_function("lorentz_boost_electron", rows), g["boost_out_electron"], np.abs(g["boost_out_electron"][:, :1])) < 1e-13
    # edge cases: a fluid at rest (the identity, mclib.c:313), gamma = 100 and 1000 head-on, tail-on and sideways, tiny speeds
    rng = np.random.default_rng(5)
    cases = []
    for gamma in (1.0, 1.0 + 1e-12, 1.0000001, 2.0, 100.0, 1000.0):
        b = np.sqrt(1.0 - 1.0 / gamma ** 2)
        for axis in range(3):
            for k_dir in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 1], list(rng.normal(size=3))):
                d = np.array(k_dir, float) / np.linalg.norm(k_dir)
                beta = np.zeros(3); beta[axis] = b
                e = 10 ** rng.uniform(-20, -15)
                cases.append([*beta, e, *(e * d)])
    cases = np.array(cases)
    want_p, want_e = np.zeros((len(cases), 4)), np.zeros((len(cases), 4))
    for i, r in enumerate(cases):
        b, p = np.ascontiguousarray(r[:3]), np.ascontiguousarray(r[3:])
        oracle.lib().orc_lorentzBoost(dp(b), dp(p), dp(want_p[i]), b"p")
        oracle.lib().orc_lorentzBoost(dp(b), dp(p), dp(want_e[i]), b"e")
    got_p, got_e = dev[0].eval_function("lorentz_boost_photon", cases), dev[0].eval_function("lorentz_boost_electron", cases)
    assert _rel(got_p, want_p, np.abs(want_p[:, :1])) < 1e-13 and _rel(got_e, want_e, np.abs(want_e[:, :1])) < 1e-13
    rest = cases[:, :3].max(axis=1) == 0
    assert rest.sum() == 15 and np.array_equal(got_e[rest], cases[rest, 3:])          # beta = 0: untouched
    assert np.allclose(np.linalg.norm(got_p[:, 1:], axis=1), got_p[:, 0], rtol=1e-15)  # 'p': null after zeroNorm


def test_stokes_rotation(dev, oracle):
    g = np.load(GOLD)
    rows = np.concatenate([g["stokes_v"], g["stokes_k"], g["stokes_kb"], g["stokes_in"]], axis=1)
    assert _rel(dev[1].eval_function("stokes_rotation", rows), g["stokes_out"], np.ones((len(rows), 1))) < 1e-13
    # near-parallel vectors: k almost along the boost v (findXY's cross product nearly vanishes), k almost along z (the other basis does)
    rng = np.random.default_rng(6)
    cases = []
    for eps in (1e-3, 1e-6, 1e-9):
        for _ in range(8):
            v = rng.normal(size=3) * 0.3
            k_par_v = v / np.linalg.norm(v) + eps * rng.normal(size=3)
            k_par_z = np.array([0, 0, 1.0]) + eps * rng.normal(size=3)
            kb = rng.normal(size=3)
            s = [1.0, *rng.uniform(-0.5, 0.5, 2), 0.0]
            cases.append([*v, *k_par_v, *kb, *s])
            cases.append([*v, *k_par_z, *kb, *s])
            cases.append([*v, *kb, *k_par_z, *s])
    cases = np.array(cases)
    want = cases[:, 9:].copy()
    for i, r in enumerate(cases):
        oracle.lib().orc_stokesRotation(dp(np.ascontiguousarray(r[0:3])), dp(np.ascontiguousarray(r[3:6])), dp(np.ascontiguousarray(r[6:9])), dp(want[i]))
    got = dev[1].eval_function("stokes_rotation", cases)
    # a near-degenerate basis amplifies rounding by 1/eps: the bar scales with it (1e-13 / eps of the Stokes fraction)
    eps_of = np.repeat([1e-3, 1e-6, 1e-9], 24)
    assert np.all(np.abs(got - want).max(axis=1) <= 4e-13 / eps_of)
    assert np.allclose(got[:, 1] ** 2 + got[:, 2] ** 2, cases[:, 10] ** 2 + cases[:, 11] ** 2, rtol=1e-6)   # a rotation: Q^2 + U^2 kept


@pytest.mark.parametrize("sampler", ["thermal_electron", "thermal_electron_wave"])
def test_single_thermal_electron_on_both_sides_of_the_switch(dev, oracle, sampler):
    rng = np.random.default_rng(7)
    temps = np.array([1e4, 1e5, 5e6, np.nextafter(1e7, 0), 1e7, 1.0000001e7, 3e7, 1e9, 4e9])
    n = 16 * len(temps)
    rows = np.zeros((n, 5))
    for i in range(n):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        e = 10 ** rng.uniform(-4, 0.5) * M_EL * C_LIGHT
        rows[i] = [temps[i % len(temps)], e, *(e * d)]
    rows[0, 2:] = [rows[0, 1], 0.0, 0.0]                     # photon along x: rotateElectron's angles degenerate (electron.c:141-146)
    rows[1, 2:] = [0.0, 0.0, rows[1, 1]]                     # ... along z
    seed = 11
    got = dev[0].eval_function(sampler, rows, seed=seed)
    r = oracle.Rng()
    oracle.lib().orc_rng_init(C.byref(r), seed, 0)
    want = np.zeros((n, 4))
    for i in range(n):
        oracle.lib().orc_rng_set_iteration(C.byref(r), i)
        oracle.lib().orc_rng_event_begin(C.byref(r), 0)
        oracle.lib().orc_singleThermalElectron(dp(want[i]), float(rows[i, 0]), dp(np.ascontiguousarray(rows[i, 1:])), C.byref(r))
    assert _rel(got, want, np.abs(want[:, :1])) < 1e-11
    gam = got[:, 0] / (M_EL * C_LIGHT)
    assert (gam >= 1).all() and gam[rows[:, 0] < 1e7].max() < 1.05 and gam[rows[:, 0] >= 1e9].mean() > 1.3


@pytest.mark.parametrize("stokes", [0, 1])
def test_electron_and_single_scatter(dev, oracle, stokes):
    g = np.load(GOLD)
    if stokes:                                               # the committed G6 vectors (STOKES on, seed 7)
        rows = np.concatenate([g["scatter_temp"][:, None], g["scatter_ph_in"], g["scatter_stokes_in"]], axis=1)
        got = dev[1].eval_function("electron_and_scatter", rows, seed=7)
        assert np.array_equal(got[:, 12].astype(np.int32), g["scatter_occurred"])
        ok = g["scatter_occurred"] == 1
        assert _rel(got[:, 0:4], g["scatter_electron"], np.abs(g["scatter_electron"][:, :1])) < 1e-11
        assert _rel(got[ok, 4:8], g["scatter_ph_out"][ok], np.abs(g["scatter_ph_out"][ok, :1])) < 1e-10
        assert _rel(got[ok, 8:12], g["scatter_stokes_out"][ok], np.ones((int(ok.sum()), 1))) < 1e-10
    # edge cases against the oracle: unpolarised light (uniform phi branch), fully polarised light, Thomson and deep Klein-Nishina
    # regimes (where the first draw rejects often), cold and hot electrons
    rng = np.random.default_rng(8 + stokes)
    rows = []
    for eps in (1e-7, 9.99e-4, 1.001e-3, 0.05, 1.0, 30.0):
        for temp in (1e5, 2e7, 2e9):
            for pol in ((0.0, 0.0), (1.0, 0.0), (-0.6, 0.8), (0.2, -0.1)):
                for _ in range(3):
                    d = rng.normal(size=3); d /= np.linalg.norm(d)
                    e = eps * M_EL * C_LIGHT
                    rows.append([temp, e, *(e * d), 1.0, pol[0], pol[1], 0.0])
    rows = np.array(rows)
    seed = 21
    got = dev[stokes].eval_function("electron_and_scatter", rows, seed=seed)
    cfg = oracle.make_config(oracle.TWO, oracle.CYLINDRICAL, stokes)
    r = oracle.Rng()
    oracle.lib().orc_rng_init(C.byref(r), seed, 0)
    n = len(rows)
    el, ph, st, occ = np.zeros((n, 4)), rows[:, 1:5].copy(), rows[:, 5:9].copy(), np.zeros(n, dtype=np.int32)
    for i in range(n):
        oracle.lib().orc_rng_set_iteration(C.byref(r), i)
        oracle.lib().orc_rng_event_begin(C.byref(r), 0)
        oracle.lib().orc_singleThermalElectron(dp(el[i]), float(rows[i, 0]), dp(ph[i]), C.byref(r))
        occ[i] = oracle.lib().orc_singleScatter(C.byref(cfg), dp(el[i].copy()), dp(ph[i]), dp(st[i]), C.byref(r))
    assert np.array_equal(got[:, 12].astype(np.int32), occ) and 0 < occ.sum() < n          # accepted and rejected draws both occur
    ok = occ == 1
    assert _rel(got[:, 0:4], el, np.abs(el[:, :1])) < 1e-11
    assert _rel(got[ok, 4:8], ph[ok], np.abs(ph[ok, :1])) < 1e-10
    if stokes:
        assert _rel(got[ok, 8:12], st[ok], np.ones((int(ok.sum()), 1))) < 1e-9
        assert (got[ok, 8] == 1.0).all() and (np.hypot(got[ok, 9], got[ok, 10]) <= 1 + 1e-9).all()
    else:
        assert np.array_equal(got[:, 8:12], rows[:, 5:9])                                  # STOKES off: s is not touched
    assert np.allclose(np.linalg.norm(got[ok, 5:8], axis=1), got[ok, 4], rtol=1e-14)        # null 4-momentum
