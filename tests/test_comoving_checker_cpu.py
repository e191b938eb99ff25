"""tests/comoving_checker.py on its own: hand-built photons whose answers are known without it -- each with an input that is wrong in the way the
check is there to catch, shown failing --, the conditions its committed cases must meet for the GPU test's counts to be exact (no fragile photon),
the closed form of a that the device evaluates against the textbook boost the checker uses, and the figures its docstring quotes."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import comoving_checker as cc
from tests import radfield_checker as rc
from tests import sightline_checker as sc

C_LIGHT = synth.C_LIGHT


def unit(g, n):
    d = g.standard_normal((n, 3))
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def flows(seed, n, gamma_max):
    """n velocities (n, 3) in random directions with Lorentz factors log-uniform in [1.05, gamma_max], and their sizes"""
    g = np.random.default_rng(seed)
    gamma = np.exp(g.uniform(np.log(1.05), np.log(gamma_max), n))
    b = np.sqrt(1.0 - 1.0 / (gamma * gamma))
    return b[:, None] * unit(g, n), b, gamma


def photons(d, seed):
    """momenta (4, n) along the unit vectors d (n, 3), p0 log-uniform over four decades"""
    p0 = 10.0 ** np.random.default_rng(seed).uniform(-20.0, -16.0, len(d))
    return np.stack([p0, p0 * d[:, 0], p0 * d[:, 1], p0 * d[:, 2]])


def positions(seed, n):
    return 1e12 * unit(np.random.default_rng(seed), n).T


def perpendicular(g, vhat):
    t = g.standard_normal(vhat.shape)
    t -= (t * vhat).sum(axis=1)[:, None] * vhat
    return t / np.sqrt((t * t).sum(axis=1))[:, None]


def closed_form(v, p):
    """a as the definition writes it: ((bp / b) - b p0) / (p0 - bp), clamped"""
    bp = (v[:, 0] * p[1] + v[:, 1] * p[2]) + v[:, 2] * p[3]
    b = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return cc.clamp(((bp / b) - b * p[0]) / (p[0] - bp))


# ---------------------------------------------------------------------------------------------- answers known without the checker
@pytest.mark.parametrize("gamma_max", [10.0, 100.0])
def test_along_and_against_the_flow(gamma_max):
    n = 500
    v, b, _ = flows(21, n, gamma_max)
    vhat = v / b[:, None]
    r = positions(22, n)
    for sign in (1.0, -1.0):
        m, a, bar = cc.cosines(v, photons(sign * vhat, 23), r)
        assert (np.abs(a - sign) <= bar).all() and (np.abs(a) <= 1.0).all()
    # shown failing: a photon 0.1 rad off the flow is not at the pole, by far more than the bar; one at right angles to the flow in the lab runs
    # backwards in the fluid frame, a = -beta
    g = np.random.default_rng(24)
    off = np.cos(0.1) * vhat + np.sin(0.1) * perpendicular(g, vhat)
    _, a_off, bar = cc.cosines(v, photons(off, 23), r)
    assert (np.abs(a_off - 1.0) > 1e3 * bar).all()
    _, a_side, bar = cc.cosines(v, photons(perpendicular(g, vhat), 23), r)
    assert (np.abs(a_side + b) <= bar).all()


def test_a_photon_at_lab_cosine_beta_is_at_right_angles_in_the_fluid_frame():
    n = 500
    v, b, _ = flows(31, n, 10.0)
    vhat = v / b[:, None]
    g = np.random.default_rng(32)
    d = b[:, None] * vhat + np.sqrt(1.0 - b * b)[:, None] * perpendicular(g, vhat)
    p, r = photons(d, 33), positions(34, n)
    _, a, bar = cc.cosines(v, p, r)
    assert (np.abs(a) <= bar).all() and bar.max() < 64 * cc.U * 101.0
    # shown failing: the lab cosine about the flow is beta, not 0; boosted with the wrong sign it is 2 beta / (1 + beta^2)
    lab = (d * vhat).sum(axis=1)
    assert (np.abs(lab - b) < 1e-14).all() and (np.abs(lab) > 1e9 * bar).all()
    pp = synth.lorentz_boost(-v, p.T.copy())
    wrong = (pp[:, 1:] * vhat).sum(axis=1) / pp[:, 0]
    assert (np.abs(wrong - 2 * b / (1 + b * b)) < 1e-12).all() and (np.abs(wrong) > 1e9 * bar).all()


def test_a_cell_at_rest_gives_the_radial_cosine_and_a_radial_photon_gives_one():
    n = 400
    g = np.random.default_rng(41)
    r = positions(42, n)
    d = unit(g, n)
    p = photons(d, 43)
    m, a, bar = cc.cosines(np.zeros((n, 3)), p, r)
    assert np.array_equal(a.view(np.int64), m.view(np.int64)) and not bar.any()
    rhat = (r / np.sqrt((r * r).sum(axis=0))).T
    assert (np.abs(m - (d * rhat).sum(axis=1)) < 1e-15).all() and m.min() < -0.9 and m.max() > 0.9
    m_rad, a_rad, _ = cc.cosines(np.zeros((n, 3)), photons(rhat, 43), r)
    assert (np.abs(m_rad - 1.0) <= 4 * cc.U).all() and (m_rad <= 1.0).all() and np.array_equal(a_rad, m_rad)
    m_in, _, _ = cc.cosines(np.zeros((n, 3)), photons(-rhat, 43), r)
    assert (np.abs(m_in + 1.0) <= 4 * cc.U).all() and (m_in >= -1.0).all()
    # shown failing: in a moving cell a is not m
    v, _, _ = flows(44, n, 10.0)
    m2, a2, bar2 = cc.cosines(v, p, r)
    assert np.array_equal(m2.view(np.int64), m.view(np.int64)) and (np.abs(a2 - m2) > 1e6 * bar2).sum() > n - 5


def test_not_a_number_stays_not_a_number_and_the_clamp_is_a_clamp():
    assert cc.clamp(np.array([-2.0, -1.0, 0.25, 1.0, 1.0 + 1e-15, np.inf])).tolist() == [-1.0, -1.0, 0.25, 1.0, 1.0, 1.0]
    assert np.isnan(cc.clamp(np.array([np.nan]))[0])
    v, _, _ = flows(51, 2, 10.0)
    p = np.array([[0.0, 1e-18], [0.0, 1e-18], [0.0, 0.0], [0.0, 0.0]])
    m, a, _ = cc.cosines(v, p, np.array([[1e12, 0.0], [0.0, 0.0], [0.0, 0.0]]))
    assert np.isnan(m[0]) and np.isnan(a[0]) and np.isnan(m[1]) and np.isfinite(a[1])      # p0 == 0; the origin


@pytest.mark.parametrize("gamma_max, tol", [(10.0, 4e-14), (100.0, None)])
def test_the_closed_form_of_a_agrees_with_the_textbook_boost(gamma_max, tol):
    """what the device evaluates against what the checker evaluates, both here on the CPU: within twice the derived bar for every photon, and to
    4e-14 for Lorentz factors up to 10"""
    n = 20000
    v, b, _ = flows(61, n, gamma_max)
    g = np.random.default_rng(62)
    d = unit(g, n)
    d[:2000] = (np.cos(0.02) * v / b[:, None] + np.sin(0.02) * perpendicular(g, v / b[:, None]))[:2000]      # some near the forward pole, where 1 - x is smallest
    p = photons(d, 63)
    _, a, bar = cc.cosines(v, p, positions(64, n))
    diff = np.abs(closed_form(v, p) - a)
    print("gamma <= %g: closed form against textbook boost: largest difference %.3g, largest difference / bar_a %.3g, largest bar_a %.3g"
          % (gamma_max, diff.max(), (diff / bar).max(), bar.max()))
    assert (diff <= 2 * bar).all()
    if tol is not None:                                        # the photons in random directions; those sent to the pole are the worst conditioned
        print("in random directions alone: %.3g" % diff[2000:].max())
        assert diff[2000:].max() <= tol


# ---------------------------------------------------------------------------------------------- the committed cases
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_no_committed_case_holds_a_fragile_photon(name):
    for mode in (cc.CELLS, cc.SHELLS):
        w = cc.want(name, mode)
        assert w["n_fragile"] == 0 and not w["fragile"].any(), (name, mode, np.nonzero(w["fragile"])[0])
        assert np.array_equal(w["count"], w["count_sure"])
        assert int(w["count"].sum()) + w["n_unlocated"] + w["n_outside"] == w["n_observable"], (name, mode)
        assert w["n_observable"] > 0
        radfield = rc.want(name, mode) if name in rc.CASES else None
        if radfield is not None:                                   # the same photons are counted, located and put into shells
            assert (w["n_observable"], w["n_unlocated"]) == (radfield["n_observable"], radfield["n_unlocated"])
            assert w["n_outside"] >= radfield["n_outside"]


def test_the_largest_bars_are_what_the_docstring_quotes():
    worst = {10.0: 0.0, 100.0: 0.0}
    for name in sorted(cc.CASES):
        q = cc.want(name, cc.CELLS)["q"]
        key = 100.0 if name == "gamma_100" else 10.0
        worst[key] = max(worst[key], float(q["bar_a"].max()))
    print("largest bar_a on the committed cases: %.3g (gamma <= 10), %.3g (gamma <= 100)" % (worst[10.0], worst[100.0]))
    assert 4.4e-13 * 0.95 <= worst[10.0] <= 4.5e-13 and 2.8e-13 * 0.95 <= worst[100.0] <= 2.9e-13


def test_cases_exercise_what_they_are_named_for():
    for name, cells in (("crowded_4", 4), ("crowded_1", 1), ("spread", 1000)):
        w = cc.want(name, cc.CELLS)
        in_use = int((w["count"].sum(axis=(1, 2)) > 0).sum())
        assert (in_use == cells if cells < 1000 else 900 < in_use <= cells) and w["count"].sum() + w["n_outside"] == 1000 and w["count"].sum() > 900
    w = cc.want("shells", cc.SHELLS)
    assert w["count"].shape == (8, 4, 6, 4) and (w["count"] > 0).sum() > 100 and w["n_outside"] > 20
    assert (w["count"].sum(axis=(0, 1, 3)) > 0).all() and (w["count"].sum(axis=(0, 1, 2)) > 0).all()      # every energy bin and every cosine bin is in use
    q = w["q"]
    inside = q["cell"] >= 0
    assert (cc.find_bin(cc.E_EDGES, q["e"][inside]) < 0).sum() > 5                       # ... and some energies lie outside
    rest = cc.want("rest", cc.CELLS)
    q, frame = rest["q"], cc.case("rest")["frame"]
    still = (q["cell"] >= 0) & (frame["gamma"][np.maximum(q["cell"], 0)] == 1.0)
    assert still.sum() > 150 and np.array_equal(q["a"][still].view(np.int64), q["m"][still].view(np.int64))
    assert np.array_equal(q["e"][still].view(np.int64), q["e_lab"][still].view(np.int64)) and not q["bar_a"][still].any()
    g100 = cc.want("gamma_100", cc.CELLS)
    assert cc.case("gamma_100")["frame"]["gamma"].max() > 80
    assert (g100["bound_wea"] >= g100["bound_we"] * 0).all() and (g100["bound_weaa"][g100["count"] > 0] > 0).all()


def test_planes_obey_their_inequalities_and_sum_to_the_radiation_field():
    c = cc.case("shells")
    w = cc.field(c["frame"], c["ph"], cc.SHELLS, [0.0, 1e300], [-1.0, 2.0], cc.SHELL_R, cc.SHELL_MU)       # edges that cover everything
    rf = rc.want("shells", rc.SHELLS)
    assert np.array_equal(w["count"][:, :, 0, 0], rf["count"]) and w["n_outside"] == rf["n_outside"]
    for k, kr in (("w", "w"), ("we", "we_comv"), ("we_lab", "we_lab")):
        assert np.array_equal(w[k][:, :, 0, 0], rf[kr]), k
    full = cc.want("shells", cc.SHELLS)
    for e, first, second in (("we", "wea", "weaa"), ("we_lab", "wem", "wemm")):
        assert (np.abs(full[first]) <= full[e]).all() and (full[second] >= 0).all() and (full[second] <= full[e]).all()
    mom = cc.moments(full)
    used = mom["J"] > 0
    assert used.sum() > 12 and np.isnan(mom["K_over_J"][~used]).all() and (np.abs(mom["H_over_J"][used]) <= 1).all()
    assert ((mom["K_over_J"][used] >= mom["H_over_J"][used] ** 2 - 1e-12) & (mom["K_over_J"][used] <= 1)).all()      # Cauchy-Schwarz


def test_isotropic_radiation_has_eddington_factor_one_third():
    """the construction of tests/test_gpu_comoving.py's isotropy test through the checker: H / J and K / J within 5 sigma of 0 and 1 / 3; the same
    photons measured about the flow in the lab frame are beamed -- far outside"""
    n = 4096
    iso = cc.isotropic(n)
    w = cc.field(iso["frame"], iso["ph"], cc.SHELLS, [1e-9, 1e-6], np.linspace(-1.0, 1.0, 9) + np.r_[np.zeros(8), 1e-15], [1.0e12, 1.2e12], [0.9, 1.01])
    assert w["count"].sum() == n and w["n_fragile"] == 0
    q = w["q"]
    assert (np.abs(q["a"] - iso["a_true"]) <= 2 * q["bar_a"] + 1e-14).all()              # the boost back recovers the cosines as drawn
    assert (np.abs(q["e"] / 3.1e-8 - 1.0) < 1e-12).all()
    mom = cc.moments(w)
    h, k = float(mom["H_over_J"][0, 0]), float(mom["K_over_J"][0, 0])
    s_h, s_k = 1.0 / np.sqrt(3.0 * n), np.sqrt(4.0 / (45.0 * n))
    print("isotropic in the fluid frame: H / J = %.4f (sigma %.4f), K / J = %.4f (sigma %.4f)" % (h, s_h, k, s_k))
    assert abs(h) <= 5 * s_h and abs(k - 1.0 / 3.0) <= 5 * s_k
    ph = iso["ph"]
    v = synth.hydro_vector_to_cartesian(iso["frame"], iso["cells"], np.arctan2(ph["r1"], ph["r0"]))
    lab = (v[:, 0] * ph["p1"] + v[:, 1] * ph["p2"] + v[:, 2] * ph["p3"]) / (np.sqrt((v * v).sum(axis=1)) * ph["p0"])
    e_lab = ph["p0"] * C_LIGHT
    h_lab, k_lab = float((e_lab * lab).sum() / e_lab.sum()), float((e_lab * lab * lab).sum() / e_lab.sum())
    print("the same photons about the flow in the lab frame: H / J = %.3f, K / J = %.3f" % (h_lab, k_lab))
    assert h_lab > 100 * s_h and k_lab - 1.0 / 3.0 > 100 * s_k
