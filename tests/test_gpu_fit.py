"""mcrat_hip_fit_spectra on the device against the NumPy restatement (tests/fit_checker.py), bit for bit: every output column -- the doubles by their
bytes, n_used, dof and status exactly -- for both models, for bin counts around the wavefront's 64, spectrum counts around the workgroup's four, rows
without a used bin, rows with every bin used, rows whose used bins start behind bin 64, coarse grids around 64 candidates, no refinement and the
default search, exact ties, and bounds that put the result on a face.  Then the noise-free spectra of tests/test_fit_checker_cpu.py against their
true parameters, one run from a resampled pool observation to error bars, and every refusal through the ABI with its text."""
import ctypes as C
import functools

import numpy as np
import pytest

from mcrat_amd import synth
from tests import fit_checker as F
from tests import test_fit_checker_cpu as N
from tests import test_fit_plan_cpu as P

pytestmark = pytest.mark.gpu

F8, I4 = ("alpha", "beta", "e_peak", "amplitude", "chi2"), ("n_used", "dof", "status")
SMALL = dict(grid=(3, 3, 2), n_rounds=3, shrink=0.6)                      # a search the checker runs in milliseconds


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(scope="module")
def eng(hip):
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    yield e
    e.close()


def same(got, want, what):
    for k in F8:
        assert got[k].dtype == np.float64 and got[k].tobytes() == np.asarray(want[k], dtype=np.float64).tobytes(), (what, k, got[k], want[k])
    for k in I4:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def both(eng, model, edges, count, w, bounds=None, min_count=1, **search):
    """the device's and the checker's columns for the same arguments"""
    bounds = bounds or F.default_bounds(edges)
    log_e = F.log_e_of(edges)
    got = eng.fit_spectra(count, w, edges, model=model, alpha=bounds[0], lam=bounds[1], beta=bounds[2], log_e=log_e, min_count=min_count, **search)
    want = F.fit(count, w, edges, log_e, model, bounds, min_count=min_count, **search)
    return got, want


@functools.lru_cache(maxsize=None)
def spectra(model, n_spec, n_e, seed=0):
    """Poisson spectra with gaps; row 0 has every bin used when there are two rows or more; the last row of three or more has no used bin"""
    rng = np.random.default_rng(1000 * n_e + 10 * n_spec + model + seed)
    edges, _, count, w = P.synthetic(rng, model, n_spec, n_e, total=40.0 * n_e)
    w = np.where(count > 0, w, rng.choice([0.0, -1.0, np.nan], size=w.shape))      # an unused bin may hold anything
    if n_spec >= 2:
        count[0] = np.maximum(count[0], 1)
        w[0] = np.where(w[0] > 0, w[0], 1e50)
    if n_spec >= 3:
        count[-1] = 0
    for a in (count, w):
        a.setflags(write=False)
    return edges, count, w


@pytest.mark.parametrize("model", [F.BAND, F.COMP])
@pytest.mark.parametrize("n_e", [1, 3, 4, 63, 64, 65, 200])
def test_bin_counts(eng, model, n_e):
    edges, count, w = spectra(model, 5, n_e)
    got, want = both(eng, model, edges, count, w, **SMALL)
    same(got, want, "n_e %d" % n_e)
    assert want["n_used"][0] == n_e and want["n_used"][-1] == 0 and want["status"][-1] == F.TOO_FEW_BINS
    assert (want["status"][0] == F.TOO_FEW_BINS) == (n_e < F.n_par(model) + 1)
    assert np.isnan(got["beta"]).all() if model == F.COMP else True


@pytest.mark.parametrize("model", [F.BAND, F.COMP])
@pytest.mark.parametrize("n_spec", [1, 3, 4, 5, 257])
def test_spectrum_counts(eng, model, n_spec):
    edges, count, w = spectra(model, n_spec, 24)
    got, want = both(eng, model, edges, count, w, **SMALL)
    same(got, want, "n_spec %d" % n_spec)
    assert got["alpha"].shape == (n_spec,) and np.isfinite(want["chi2"]).sum() >= (n_spec + 1) // 2


def test_more_spectra_than_one_trip_of_the_grid(eng):
    """Beyond 4 * 65536 spectra a wavefront takes a second spectrum: its LDS rows, n_used and the best candidate start afresh.  262 150 spectra
    of four bins, rows of 50 different spectra in turn (50 does not divide 262 144, so a wavefront's second spectrum differs from its first),
    some with a bin missing -- TOO_FEW_BINS beside fits --, a search of 4 + 64 candidates; the checker fits the 50 and every row is compared."""
    n_spec, period = 4 * 65536 + 6, 50
    edges, count, w = spectra(F.COMP, period, 4, seed=9)
    rows = np.arange(n_spec) % period
    search = dict(grid=(2, 2, 1), n_rounds=1, shrink=0.5)
    bounds, log_e = F.default_bounds(edges), F.log_e_of(edges)
    got = eng.fit_spectra(count[rows], w[rows], edges, model=F.COMP, alpha=bounds[0], lam=bounds[1], beta=bounds[2], log_e=log_e, **search)
    want = F.fit(count, w, edges, log_e, F.COMP, bounds, **search)
    same(got, {k: v[rows] for k, v in want.items()}, "second trip")
    kinds = set(want["status"][rows[4 * 65536:]] == F.TOO_FEW_BINS) | set(want["n_used"][:6] != want["n_used"][rows[4 * 65536:]])
    assert kinds == {False, True} and (want["n_used"][:-1] >= 2).any()


def test_leading_shape_and_used_bins_behind_bin_64(eng):
    edges, count, w = spectra(F.BAND, 6, 200, seed=3)
    count = count.copy()
    count[1, :70] = 0                                                      # the first used bin is in the wavefront's second trip
    count[2, :130] = 0                                                     # ... and in its third
    count[3, 64:] = 0                                                      # only the first trip holds used bins
    got, want = both(eng, F.BAND, edges, count.reshape(2, 3, 200), w.reshape(2, 3, 200), min_count=2, **SMALL)
    assert got["chi2"].shape == (2, 3)
    same({k: v.ravel() for k, v in got.items()}, want, "behind bin 64")
    assert (want["n_used"][1:4] >= 4).all() and want["n_used"][1] < 130 and want["n_used"][2] < 70


@pytest.mark.parametrize("model,grid", [(F.BAND, (1, 1, 1)), (F.BAND, (7, 3, 3)), (F.BAND, (4, 4, 4)), (F.BAND, (5, 13, 1)), (F.BAND, (16, 8, 8)),
                                        (F.COMP, (1, 1, 5)), (F.COMP, (9, 7, 1)), (F.COMP, (8, 8, 2)), (F.COMP, (5, 13, 1)), (F.COMP, (32, 32, 1))])
def test_coarse_grids_alone(eng, model, grid):
    """1, 63, 64, 65 and 1024 candidates, n_rounds 0: whole batches, a batch with one lane idle, one with one lane busy"""
    assert grid[0] * grid[1] * (grid[2] if model == F.BAND else 1) in (1, 63, 64, 65, 1024)
    edges, count, w = spectra(model, 4, 40)
    got, want = both(eng, model, edges, count, w, grid=grid, n_rounds=0, shrink=0.5)
    same(got, want, "grid %s" % (grid,))
    assert np.isfinite(want["chi2"][:3]).all()


@pytest.mark.parametrize("model", [F.BAND, F.COMP])
def test_default_search(eng, hip, model):
    edges, count, w = spectra(model, 3, 40, seed=5)
    assert hip.FIT_DEFAULTS == F.DEFAULTS and hip.FIT_E_PIV == F.E_PIV and (hip.FIT_COMP, hip.FIT_BAND) == (F.COMP, F.BAND)
    log_e = F.log_e_of(edges)
    got = eng.fit_spectra(count, w, edges, model=model)                    # every argument left to the binding
    want = F.fit(count, w, edges, log_e, model, F.default_bounds(edges))
    same(got, want, "defaults")


def test_exact_ties_resolve_to_the_lowest_index(eng):
    """beta is not constrained -- every break the bounds allow lies above the last bin --: all betas of an (alpha, lambda) tie exactly"""
    model, bounds, grid, n_rounds, shrink, min_count, edges, log_e, count, w = P.fit_inputs()[-1]
    for rounds in (0, n_rounds):
        got, want = both(eng, model, edges, count, w, bounds=bounds, grid=grid, n_rounds=rounds, shrink=shrink)
        same(got, want, "ties, %d rounds" % rounds)
    got, _ = both(eng, model, edges, count, w, bounds=bounds, grid=grid, n_rounds=0, shrink=shrink)
    assert got["beta"][0] == -6.0 + 0.5 * ((-2.05 - -6.0) / 4.0) and got["status"][0] & F.AT_BOUND_BETA


def test_bounds_that_put_the_result_on_a_face(eng):
    """noise-free Band spectra with alpha = -1.5, beta = -3.5 and E_pk of 100 and 215 keV (25 bins and more above the peak), searched in boxes that exclude those values"""
    edges, count, w = N.noise_free(F.BAND)[:3]
    lam = F.default_bounds(edges)[1]
    for bounds, bit in ((((0.5, 2.0), lam, (-6.0, -2.05)), F.AT_BOUND_ALPHA), (((-1.9, 2.0), (lam[0], lam[0] + 0.5), (-6.0, -2.05)), F.AT_BOUND_LAMBDA),
                        (((-1.9, 2.0), lam, (-2.5, -2.05)), F.AT_BOUND_BETA)):
        got, want = both(eng, F.BAND, edges, count[4:6], w[4:6], bounds=bounds, grid=(4, 4, 4), n_rounds=8, shrink=0.6)
        same(got, want, "face %d" % bit)
        assert (got["status"] & bit).all(), (bit, got["status"])


def test_no_finite_candidate(eng):
    """weights that overflow: y^2 underflows to 0, g is +inf, every chi^2 is not a number and counts as +inf"""
    edges = P.edges_of(8)
    w = np.full((2, 8), 1e-200) * np.diff(edges)
    got, want = both(eng, F.COMP, edges, np.full((2, 8), 5, dtype=np.int64), w, **SMALL)
    same(got, want, "no finite candidate")
    assert (got["status"] == F.NO_FINITE_CANDIDATE).all() and np.isinf(got["chi2"]).all() and np.isnan(got["alpha"]).all()


@pytest.mark.parametrize("model", [F.BAND, F.COMP])
def test_noise_free_spectra_against_their_parameters(eng, model):
    """oracle-free: the device recovers alpha, beta and ln E_pk of the noise-free spectra to 1e-6, as the checker does on the host"""
    edges, count, w, truth = N.noise_free(model)
    got = eng.fit_spectra(count, w, edges, model=model)
    worst = N.recovery_errors(got, truth, model)
    print("noise-free recovery on the device, model %d: worst error %.3e" % (model, worst))
    assert worst <= 1e-6


def test_from_a_resampled_pool_observation_to_error_bars(eng, hip):
    _, ph, _ = synth.config2(n_photons=20000, nzc=4)
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    try:
        pool.pool_create(4, 5000)
        for r in range(4):
            pool.pool_rank(r, r).set_photons({k: v[5000 * r:5000 * (r + 1)] for k, v in ph.items()})
        G = 8
        edges = np.logspace(-1.0, np.log10(300.0), 17) * F.KEV
        n = np.array([[0.0, np.sin(0.05)], [0.0, 0.0], [1.0, np.cos(0.05)]])
        res = pool.pool_observe_sky_resampled(n, [-1.0, -1.0], [-1e30, 0.0, 1e30], edges, np.zeros(4), hip.RESAMPLE_JACKKNIFE, G, seed=5)
        count, w = hip.spectra_from(res, hip.RESAMPLE_JACKKNIFE, reduce="time")
        assert count.shape == (2, G + 1, 16) and count[:, 0].sum() == (res["n_accepted"] - res["n_outside"]).sum() > 30000
        assert np.array_equal(count[:, 0], res["count"].sum(axis=(1, 2))) and np.array_equal(count[:, 1:], count[:, :1] - res["count"].sum(axis=2))
        fit = pool.fit_spectra(count, w, edges, model=hip.FIT_COMP, min_count=5)
        want = F.fit(count.reshape(-1, 16), w.reshape(-1, 16), edges, F.log_e_of(edges), F.COMP, F.default_bounds(edges), min_count=5)
        same({k: v.ravel() for k, v in fit.items()}, want, "end to end")
        est = hip.fitted_estimates(fit, hip.RESAMPLE_JACKKNIFE)
        enough = (fit["n_used"] >= 3).all(axis=1)
        assert enough.all() and (fit["status"] & (F.TOO_FEW_BINS | F.NO_FINITE_CANDIDATE) == 0).all()
        for k in ("alpha", "e_peak", "ln_e_peak"):
            assert np.isfinite(est[k]["value"][enough]).all() and np.isfinite(est[k]["stderr"][enough]).all() and (est[k]["stderr"][enough] > 0).all(), k
        assert np.isnan(est["beta"]["value"]).all()
        print("E_pk = %s keV +- %s" % (est["e_peak"]["value"] / F.KEV, est["e_peak"]["stderr"] / F.KEV))
    finally:
        pool.close()


def test_refusals_reach_the_caller(eng, hip):
    lib = hip.load_library()
    keep = []

    def good():
        edges, log_e = np.array([1.0, 2.0, 4.0, 8.0]), np.array([0.25, 0.75, 1.25])
        count, w = np.arange(1, 7, dtype=np.int64), np.arange(1.0, 7.0)
        keep.extend([edges, log_e, count, w])
        dp, ll = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
        return hip.FitArgs(F.BAND, 2, 3, count.ctypes.data_as(ll), w.ctypes.data_as(dp), edges.ctypes.data_as(dp), log_e.ctypes.data_as(dp), 1.0, -1.9, 2.0, 0.0, 2.0,
                           -6.0, -2.05, 16, 16, 8, 10, 0.5, 1), edges, log_e

    def call(a):
        out = hip.FitResult()
        rc = lib.mcrat_hip_fit_spectra(eng.ctx, C.byref(a), C.byref(out))
        return rc, lib.mcrat_hip_last_error(eng.ctx).decode()

    def edge(i, v):
        def spoil(a, edges, log_e):
            edges[i] = v
        return spoil

    def field(**kw):
        def spoil(a, edges, log_e):
            for k, v in kw.items():
                setattr(a, k, v)
        return spoil

    def log_e_nan(a, edges, log_e):
        log_e[1] = np.nan

    cases = [(field(model=2), P.BAD_MODEL), (field(w=None), P.NULL_ARRAY), (field(count=None), P.NULL_ARRAY), (field(n_e=0), P.BAD_N_E), (field(n_e=513), P.BAD_N_E),
             (edge(1, np.nan), P.EDGES_NOT_FINITE), (edge(2, 1.5), P.EDGES_NOT_ASCENDING), (edge(0, 0.0), P.EDGES_NOT_POSITIVE), (log_e_nan, P.LOG_E_NOT_FINITE),
             (field(e_piv=0.0), P.BAD_PIVOT), (field(alpha_lo=np.nan), P.BOUNDS_NOT_FINITE), (field(beta_hi=-7.0), P.BOUNDS_EMPTY),
             (field(alpha_lo=-5.0, alpha_hi=-2.0), P.BOUNDS_NO_CANDIDATE), (field(g_beta=0), P.BAD_GRID), (field(g_alpha=2048, g_lambda=2048), P.GRID_TOO_LARGE),
             (field(n_rounds=-1), P.BAD_ROUNDS), (field(shrink=0.25), P.BAD_SHRINK), (field(shrink=1.0), P.BAD_SHRINK), (field(min_count=0), P.BAD_MIN_COUNT),
             (field(n_spec=2 ** 31), P.BAD_N_SPEC), (field(n_spec=-1), P.BAD_N_SPEC)]
    assert {why for _, why in cases} == set(P.TEXTS)
    for spoil, why in cases:
        a, edges, log_e = good()
        spoil(a, edges, log_e)
        assert call(a) == (-1, P.TEXTS[why]), why                          # MCRAT_HIP_EINVAL
    a, _, _ = good()
    assert call(a)[0] == 0
    assert lib.mcrat_hip_fit_spectra(eng.ctx, None, None) == -1 and lib.mcrat_hip_fit_spectra(None, C.byref(a), C.byref(hip.FitResult())) == -1
    a.n_spec = 0                                                           # no spectrum: nothing to do, nothing written
    assert call(a)[0] == 0
    with pytest.raises(hip.McratHipError, match="fit_spectra: shrink must lie in"):
        eng.fit_spectra(np.ones((2, 3), dtype=np.int64), np.ones((2, 3)), [1.0, 2.0, 4.0, 8.0], shrink=1.5)
