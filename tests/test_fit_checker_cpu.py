"""The NumPy restatement of the spectral fit (tests/fit_checker.py) on its own: fit_exp and fit_log against 200-bit arithmetic (4 ulp), noise-free
spectra recovered to 1e-6 with the binding's default search, Poisson spectra -- the reduced chi^2 and the jackknife error of ln E_pk against the
scatter of independent samples --, the checker failing on a wrong model and on a wrong break side, and the host-side helpers of the binding
(spectra_from, fitted_estimates) on small arrays.  No GPU, no library."""
import functools

import mpmath
import numpy as np
import pytest

from mcrat_amd import engine as hip
from tests import fit_checker as F

# The noise-free spectra: 40 bins over three decades, 10 keV .. 10 MeV.  alpha and beta as the issue sets them; E_pk at four log-spaced values that
# leave a decade of bins (13 of the 40) on the far side of the peak at either end, so that both slopes are constrained by data: 100 .. 1000 keV.
ALPHAS, BETAS = (-1.5, -0.7, 0.3), (-2.3, -3.5)
E_PEAKS = tuple(10.0 ** np.linspace(2.0, 3.0, 4))
N_BINS, TOTAL = 40, 1e5


def edges40():
    return np.logspace(1.0, 4.0, N_BINS + 1) * F.KEV


@functools.lru_cache(maxsize=None)
def noise_free(model):
    """-> edges, count, w, truth [(alpha, beta or None, E_pk in erg)]: w_i = A m(E_i) dE_i exactly at the geometric centres, count_i the expected
    counts of TOTAL photons rounded to integers (a bin that rounds to 0 is not used)"""
    edges = edges40()
    cen = np.sqrt(edges[:-1] * edges[1:])
    truth = [(a, b, ep * F.KEV) for a in ALPHAS for b in (BETAS if model == F.BAND else (None,)) for ep in E_PEAKS]
    y = np.array([3.0e50 * F.band_shape(a, b, ep, cen) for a, b, ep in truth])
    w = y * np.diff(edges)
    count = np.rint(TOTAL * w / w.sum(axis=1, keepdims=True)).astype(np.int64)
    for a in (edges, count, w):
        a.setflags(write=False)
    return edges, count, w, truth


def recovery_errors(fit, truth, model):
    """the worst |error| of alpha, beta and ln E_pk over the spectra that are not flagged AT_BOUND; every spectrum must have a fit"""
    worst = 0.0
    for k, (a, b, ep) in enumerate(truth):
        assert fit["status"][k] & (F.TOO_FEW_BINS | F.NO_FINITE_CANDIDATE) == 0, k
        if fit["status"][k] & (F.AT_BOUND_ALPHA | F.AT_BOUND_LAMBDA | F.AT_BOUND_BETA):
            continue
        errs = [abs(fit["alpha"][k] - a), abs(np.log(fit["e_peak"][k] / ep))] + ([abs(fit["beta"][k] - b)] if model == F.BAND else [])
        worst = max(worst, *errs)
    return worst


def ulps(f, exact, xs):
    mpmath.mp.prec = 200
    got = f(np.asarray(xs, dtype=np.float64))
    worst = 0.0
    for x, v in zip(xs, got):
        t = exact(mpmath.mpf(float(x)))
        unit = float(np.spacing(abs(float(t)))) if float(t) != 0.0 else 5e-324
        worst = max(worst, float(abs(mpmath.mpf(float(v)) - t) / mpmath.mpf(unit)))
    return worst


def test_fit_exp_within_4_ulp():
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(-745.0, 50.0, 3000), rng.uniform(-745.0, -700.0, 500), rng.uniform(-1.0, 1.0, 500), (np.arange(-1074, 73) + 0.5) * np.log(2.0),
                         [-745.0, 50.0, 0.0]])
    xs = xs[(xs >= -745.0) & (xs <= 50.0)]
    worst = ulps(F.fit_exp, mpmath.exp, xs)
    print("fit_exp: worst error %.3f ulp over %d points" % (worst, len(xs)))
    assert worst <= 4.0


def test_fit_log_within_4_ulp():
    rng = np.random.default_rng(2)
    xs = np.concatenate([10.0 ** rng.uniform(-12.0, 12.0, 3000), rng.uniform(0.5, 2.0, 500), 1.0 + rng.uniform(-1e-3, 1e-3, 500), np.sqrt(0.5) * 2.0 ** np.arange(-39, 40),
                         [1e-12, 1e12, 1.0]])
    worst = ulps(F.fit_log, mpmath.log, xs)
    print("fit_log: worst error %.3f ulp over %d points" % (worst, len(xs)))
    assert worst <= 4.0
    assert F.fit_log(np.array([1.0]))[0] == 0.0 and np.isnan(F.fit_log(np.array([0.0, -1.0, np.inf, np.nan]))).all()


@functools.lru_cache(maxsize=None)
def default_fit(model):
    edges, count, w, _ = noise_free(model)
    return F.fit(count, w, edges, F.log_e_of(edges), model, F.default_bounds(edges))


@pytest.mark.parametrize("model", [F.BAND, F.COMP])
def test_noise_free_spectra_are_recovered_to_1e_6(model):
    """24 Band spectra and 12 cutoff power laws, the default search: alpha, beta and ln E_pk to 1e-6 wherever no AT_BOUND bit is raised"""
    truth = noise_free(model)[3]
    assert len(truth) == (24 if model == F.BAND else 12)
    fit = default_fit(model)
    worst = recovery_errors(fit, truth, model)
    flagged = int((fit["status"] != 0).sum())
    print("noise-free recovery, model %d: worst error %.3e, %d of %d flagged AT_BOUND, worst chi2 %.3e" % (model, worst, flagged, len(truth), fit["chi2"].max()))
    assert worst <= 1e-6
    assert flagged == 0                                                   # none of these lies near a bound: nothing may hide behind a flag
    assert hip.FIT_DEFAULTS == F.DEFAULTS


def test_the_checker_fails_on_a_wrong_break_side_and_on_a_wrong_model():
    edges, count, w, truth = noise_free(F.BAND)
    pick = [0, 9, 22]
    search = dict(grid=(16, 16, 8), n_rounds=60, shrink=0.85)
    args = (count[pick], w[pick], edges, F.log_e_of(edges))
    right = F.fit(*args, F.BAND, F.default_bounds(edges), **search)
    wrong_side = F.fit(*args, F.BAND, F.default_bounds(edges), wrong_break_side=True, **search)
    wrong_model = F.fit(*args, F.COMP, F.default_bounds(edges), **search)
    dof = right["dof"].astype(np.float64)
    assert (right["chi2"] / dof < 1e-2).all()
    # the power law below the break and the cutoff above it, or no high-energy power law at all: no parameters describe these spectra
    assert (wrong_side["chi2"] / dof > 10.0).all() and (wrong_model["chi2"] / wrong_model["dof"] > 10.0).all()
    for k, j in enumerate(pick):
        assert abs(right["alpha"][k] - truth[j][0]) < 1e-2 and abs(wrong_side["alpha"][k] - truth[j][0]) > 1e-2


# Poisson spectra: one Band shape, 64 independent samples of about 10^5 photons, and for sample 0 a jackknife over 16 groups of its photons.
POISSON_SEARCH = dict(grid=(16, 16, 8), n_rounds=100, shrink=0.9, min_count=10)      # (the statistical error is 1e-2: 1e-4 from the search is enough)
TRUE = (-0.7, -2.3, 300.0 * F.KEV)
SAMPLES, GROUPS = 64, 16


@functools.lru_cache(maxsize=None)
def poisson_fits():
    rng = np.random.default_rng(7)
    edges = edges40()
    cen = np.sqrt(edges[:-1] * edges[1:])
    shape = F.band_shape(*TRUE, cen) * np.diff(edges)
    mu = TOTAL * shape / shape.sum()
    count = rng.poisson(mu, size=(SAMPLES, N_BINS)).astype(np.int64)
    groups = rng.multinomial(count[0], np.full(GROUPS, 1.0 / GROUPS)).T.astype(np.int64)       # (GROUPS, N_BINS): sample 0's photons dealt to groups
    assert np.array_equal(groups.sum(axis=0), count[0])
    unit = 2.0e45                                                          # every photon has the same weight
    jack_c, jack_w = hip.spectra_from({"count": groups[None, :, None, :], "w": unit * groups[None, :, None, :]}, hip.RESAMPLE_JACKKNIFE, reduce="time")
    all_c = np.concatenate([count, jack_c[0]])
    all_w = np.concatenate([unit * count, jack_w[0]])
    fit = F.fit(all_c, all_w, edges, F.log_e_of(edges), F.BAND, F.default_bounds(edges), **POISSON_SEARCH)
    return {k: v[:SAMPLES] for k, v in fit.items()}, {k: v[None, SAMPLES:] for k, v in fit.items()}, (jack_c, jack_w, count)


def test_poisson_spectra_reduced_chi2():
    """With sigma_i = y_i / sqrt(count_i) from the data and count_i >= 10, chi^2 / dof of a sample has mean 1 within the bias of data-based
    weights (at most 1 / min_count = 10 %, upwards) and standard deviation sqrt(2 / dof) = 0.25 at dof ~ 33: the mean of 64 samples must lie in
    [0.9, 1.2] (three standard errors of 0.03 and the bias) and every sample in [0.2, 2.3] (five standard deviations and the bias)."""
    fit, _, _ = poisson_fits()
    red = fit["chi2"] / fit["dof"]
    print("reduced chi2 of %d samples: mean %.3f, min %.3f, max %.3f, dof %d .. %d" % (SAMPLES, red.mean(), red.min(), red.max(), fit["dof"].min(), fit["dof"].max()))
    assert (fit["status"] == 0).all() and (fit["dof"] >= 25).all()
    assert 0.9 <= red.mean() <= 1.2 and red.min() >= 0.2 and red.max() <= 2.3
    assert abs(fit["alpha"].mean() - TRUE[0]) < 0.05 and abs(np.log(fit["e_peak"] / TRUE[2]).mean()) < 0.05 and abs(fit["beta"].mean() - TRUE[1]) < 0.1


def test_jackknife_error_of_ln_e_peak_against_the_scatter_of_samples():
    fit, jack, (jack_c, jack_w, count) = poisson_fits()
    assert jack_c.shape == (1, GROUPS + 1, N_BINS) and np.array_equal(jack_c[0, 0], count[0])
    assert np.array_equal(jack_c[0, 1:].sum(axis=0), (GROUPS - 1) * count[0])                  # every photon is left out exactly once
    np.testing.assert_allclose(jack_w[0, 1:].sum(axis=0), GROUPS * jack_w[0, 0], rtol=1e-12)    # ... and w is scaled by G / (G - 1)
    est = hip.fitted_estimates(jack, hip.RESAMPLE_JACKKNIFE)
    scatter = np.log(fit["e_peak"]).std(ddof=1)
    stderr = est["ln_e_peak"]["stderr"][0]
    print("ln E_pk: jackknife stderr %.4f, scatter of %d samples %.4f" % (stderr, SAMPLES, scatter))
    assert est["ln_e_peak"]["value"][0] == np.log(jack["e_peak"][0, 0]) and jack["e_peak"][0, 0] == fit["e_peak"][0]
    assert 0.5 * scatter <= stderr <= 2.0 * scatter
    assert np.isfinite(est["alpha"]["stderr"][0]) and np.isfinite(est["beta"]["stderr"][0]) and est["e_peak"]["stderr"][0] > 0.0


def test_spectra_from_and_fitted_estimates_on_small_arrays():
    rng = np.random.default_rng(3)
    count = rng.integers(0, 9, (2, 3, 4, 5, 2, 2)).astype(np.int64)         # (n_obs, n_rep, n_t, n_e, n_y, n_x)
    w = rng.uniform(0.0, 1.0, count.shape)
    res = {"count": count, "w": w, "n_frame_undefined": np.zeros(2, dtype=np.int64)}
    c, x = hip.spectra_from(res, hip.RESAMPLE_BOOTSTRAP, reduce=("time", "pixels"))
    assert c.shape == (2, 3, 5) and np.array_equal(c, count.sum(axis=(2, 4, 5))) and np.allclose(x, w.sum(axis=(2, 4, 5)), rtol=1e-14)
    c, x = hip.spectra_from(res, hip.RESAMPLE_JACKKNIFE, reduce="pixels")
    assert c.shape == (2, 4, 4, 5) and np.array_equal(c[:, 0], count.sum(axis=(1, 4, 5))) and np.array_equal(c[:, 2], c[:, 0] - count[:, 1].sum(axis=(3, 4)))
    assert np.allclose(x[:, 3], (w.sum(axis=(1, 4, 5)) - w[:, 2].sum(axis=(3, 4))) * 1.5, rtol=1e-13)
    c, x = hip.spectra_from({"count": count[:, 0, :, :, 0, 0], "w": w[:, 0, :, :, 0, 0]}, hip.RESAMPLE_NONE)       # observe's cube: no replica axis
    assert c.shape == (2, 4, 5) and c.flags.c_contiguous and np.array_equal(c, count[:, 0, :, :, 0, 0])
    with pytest.raises(ValueError):
        hip.spectra_from(res, hip.RESAMPLE_NONE, reduce="energy")
    with pytest.raises(ValueError):                                        # a jackknife of a cube without a replica axis
        hip.spectra_from({"count": count[:, 0, :, :, 0, 0], "w": w[:, 0, :, :, 0, 0]}, hip.RESAMPLE_JACKKNIFE)
    with pytest.raises(ValueError):
        hip.fitted_estimates({"alpha": np.zeros((2, 6)), "beta": np.zeros((2, 6)), "e_peak": np.ones((2, 6))}, 7)
    c, x = hip.spectra_from({"count": count[:, :, :, :, 0, 0], "w": w[:, :, :, :, 0, 0]}, hip.RESAMPLE_NONE, reduce="time")     # a replica axis, taken as it is
    assert c.shape == (2, 3, 5) and np.array_equal(c, count[:, :, :, :, 0, 0].sum(axis=2))
    e_peak = np.exp(rng.normal(0.0, 0.1, (2, 6)))
    fit = {"alpha": rng.normal(-1.0, 0.1, (2, 6)), "beta": np.full((2, 6), np.nan), "e_peak": e_peak}
    boot = hip.fitted_estimates(fit, hip.RESAMPLE_BOOTSTRAP, percentiles=(16.0, 84.0))
    assert np.allclose(boot["alpha"]["stderr"], fit["alpha"][:, 1:].std(axis=1, ddof=1)) and np.array_equal(boot["alpha"]["value"], fit["alpha"][:, 0])
    assert (boot["ln_e_peak"]["lo"] <= boot["ln_e_peak"]["hi"]).all() and np.isnan(boot["beta"]["stderr"]).all()
    jack = hip.fitted_estimates(fit, hip.RESAMPLE_JACKKNIFE)
    dev = np.log(e_peak[:, 1:])
    assert np.allclose(jack["ln_e_peak"]["stderr"], np.sqrt(4.0 / 5.0 * ((dev - dev.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)))
    assert np.isnan(hip.fitted_estimates(fit, hip.RESAMPLE_NONE)["alpha"]["stderr"]).all()
