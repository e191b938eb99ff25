"""The spectral fit (mcrat_amd/csrc/fit_plan.hpp, mcrat_hip_fit_spectra) restated in NumPy, operation by operation: fit_exp and fit_log as the
header's sequences of IEEE operations, the used bins compacted in bin order, a candidate's chi^2 in two passes with an explicit loop over the bins
(vectorised over spectra and candidates), and the search round by round.  NumPy rounds every + - * / once and contracts nothing, np.rint, np.frexp
and np.ldexp are exact (ldexp is kept away from subnormal results as the header keeps it), so every output has the header's bits."""
import numpy as np

COMP, BAND = 0, 1
TOO_FEW_BINS, AT_BOUND_ALPHA, AT_BOUND_LAMBDA, AT_BOUND_BETA, NO_FINITE_CANDIDATE = 1, 2, 4, 8, 16
MAX_BINS, WAVE, WAVES, MAX_COARSE, MAX_ROUNDS = 512, 64, 4, 1 << 20, 4096
LN2_HI, LN2_LO, INV_LN2, SQRT_HALF = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00, 7.07106781186547524401e-01
NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]
INF = np.inf
KEV = 1.602176634e-9                             # erg
E_PIV = 100.0 * KEV
# the binding's defaults (mcrat_amd/engine.py): chosen so that the noise-free spectra of tests/test_fit_checker_cpu.py are recovered to 1e-6
DEFAULTS = dict(alpha=(-1.9, 2.0), beta=(-6.0, -2.05), grid=(16, 16, 8), n_rounds=320, shrink=0.95, min_count=1)
EXP_C = [1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0,
         1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]
LOG_C = [1.0 / 23.0, 1.0 / 21.0, 1.0 / 19.0, 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0, 1.0]


def fit_exp(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        inside = (x >= -746.0) & (x <= 709.78)
        xs = np.where(inside, x, 0.0)
        kd = np.rint(xs * INV_LN2)
        r = (xs - kd * LN2_HI) - kd * LN2_LO
        p = np.full(x.shape, EXP_C[0])
        for c in EXP_C[1:]:
            p = p * r + c
        k = kd.astype(np.int32)
        small = k < -1000
        out = np.where(small, np.ldexp(p, np.where(small, k + 1000, 0)) * 2.0 ** -1000, np.ldexp(p, np.where(small, 0, k)))
        out = np.where(x < -746.0, 0.0, out)
        out = np.where(x > 709.78, INF, out)
        return np.where(x != x, x, out)


def fit_log(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ok = (x > 0.0) & (x <= np.finfo(np.float64).max)
        m, e = np.frexp(np.where(ok, x, 1.0))
        low = m < SQRT_HALF
        m = np.where(low, m * 2.0, m)
        e = np.where(low, e - 1, e)
        s = (m - 1.0) / (m + 1.0)
        z = s * s
        p = np.full(x.shape, LOG_C[0])
        for c in LOG_C[1:]:
            p = p * z + c
        ed = e.astype(np.float64)
        return np.where(ok, ed * LN2_HI + ((2.0 * s) * p + ed * LN2_LO), NAN)


def log_e_of(e_edges, e_piv=E_PIV):
    """L_i = ln(E_i / E_piv) at the geometric centres, as the binding computes it (an input of the fit: any finite array is legal)"""
    e = np.asarray(e_edges, dtype=np.float64)
    return np.log(np.sqrt(e[:-1] * e[1:]) / e_piv)


def n_par(model):
    return 3 if model == BAND else 2


def compact(count, w, e_edges, log_e, min_count):
    """-> n_used (S,), L, y, g (S, n_e): the used bins of every spectrum first, in bin order; what lies behind n_used is never read"""
    count, w = np.asarray(count, dtype=np.int64), np.asarray(w, dtype=np.float64)
    e = np.asarray(e_edges, dtype=np.float64)
    with np.errstate(all="ignore"):
        used = (count >= min_count) & (w > 0.0) & (w <= np.finfo(np.float64).max)
        y = w / (e[1:] - e[:-1])[None, :]
        g = count.astype(np.float64) / (y * y)
    order = np.argsort(~used, axis=1, kind="stable")                   # used bins first, each part in bin order
    take = lambda a: np.take_along_axis(a, order, axis=1)
    return used.sum(axis=1), take(np.broadcast_to(np.asarray(log_e, dtype=np.float64)[None, :], w.shape)), take(y), take(g)


def candidate(model, alpha, lam, beta):
    a2, amb = 2.0 + alpha, alpha - beta
    valid = (a2 > 0.0) & ((amb > 0.0) if model == BAND else True)
    c0 = np.zeros_like(a2)
    if model == BAND:
        with np.errstate(all="ignore"):
            c0 = np.where(valid, amb * (((fit_log(amb) - fit_log(a2)) + lam) - 1.0), 0.0)
    return dict(alpha=alpha, lam=lam, beta=beta, a2=a2, amb=amb, c0=c0, valid=valid)


def model_value(model, c, L, wrong_break_side=False):
    """m of the candidates c at L (broadcast)"""
    with np.errstate(all="ignore"):
        x = c["a2"] * fit_exp(L - c["lam"])
        ln_m = c["alpha"] * L - x
        if model == BAND:
            power_law = (x < c["amb"]) if wrong_break_side else ~(x < c["amb"])
            ln_m = np.where(power_law, c["c0"] + c["beta"] * L, ln_m)
        return fit_exp(ln_m)


def chi2(model, n_used, L, y, g, c, wrong_break_side=False):
    """n_used (S,), L, y, g (S, n_e), the candidates' arrays (S, C) -> chi^2 and amplitude (S, C); the loop over the bins is explicit"""
    shape = c["alpha"].shape
    sym, smm = np.zeros(shape), np.zeros(shape)
    most = int(n_used.max()) if n_used.size else 0
    with np.errstate(all="ignore"):
        for i in range(most):
            on = (i < n_used)[:, None]
            m = model_value(model, c, L[:, i:i + 1], wrong_break_side)
            gm = g[:, i:i + 1] * m
            sym = np.where(on, sym + gm * y[:, i:i + 1], sym)
            smm = np.where(on, smm + gm * m, smm)
        ok = c["valid"] & (smm > 0.0) & (smm <= np.finfo(np.float64).max)
        amp = sym / np.where(ok, smm, 1.0)
        chi = np.zeros(shape)
        for i in range(most):
            on = (i < n_used)[:, None]
            m = model_value(model, c, L[:, i:i + 1], wrong_break_side)
            r = y[:, i:i + 1] - amp * m
            chi = np.where(on, chi + g[:, i:i + 1] * (r * r), chi)
        chi = np.where(ok & (chi <= np.finfo(np.float64).max), chi, INF)
    return chi, amp


def _axis_lo(c, side, lo, hi):
    at = c - 0.5 * side
    at = np.where(at < lo, lo, at)
    return np.where(at + side > hi, hi - side, at)


def fit(count, w, e_edges, log_e, model, bounds, grid=DEFAULTS["grid"], n_rounds=DEFAULTS["n_rounds"], shrink=DEFAULTS["shrink"], min_count=DEFAULTS["min_count"],
        e_piv=E_PIV, wrong_break_side=False):
    """count, w (..., n_e); bounds ((alpha_lo, alpha_hi), (lambda_lo, lambda_hi), (beta_lo, beta_hi)) -> dict of the eight output columns, (S,) each"""
    count, w = np.asarray(count, dtype=np.int64), np.asarray(w, dtype=np.float64)
    count, w = count.reshape(-1, count.shape[-1]), w.reshape(-1, count.shape[-1])   # any leading shape: the columns come back flat
    S = count.shape[0]
    band = model == BAND
    lo = [float(bounds[0][0]), float(bounds[1][0]), float(bounds[2][0]) if band else 0.0]
    hi = [float(bounds[0][1]), float(bounds[1][1]), float(bounds[2][1]) if band else 0.0]
    n_used, L, y, g = compact(count, w, e_edges, log_e, min_count)
    n = [int(grid[0]), int(grid[1]), int(grid[2]) if band else 1]
    side = [np.full(S, hi[k] - lo[k]) for k in range(3)]
    box_lo = [np.full(S, lo[k]) for k in range(3)]
    best = [np.full(S, lo[k] + 0.5 * (hi[k] - lo[k])) for k in range(3)]
    best_amp, best_chi = np.full(S, NAN), np.full(S, INF)
    cell = None
    for rnd in range(n_rounds + 1):
        if rnd > 0:
            n = [4, 4, 4] if band else [8, 8, 1]
            side = [s * shrink for s in side]
            box_lo = [_axis_lo(best[k], side[k], lo[k], hi[k]) for k in range(3)]
        cell = [side[k] / float(n[k]) for k in range(3)]
        idx = np.arange(n[0] * n[1] * n[2])
        i0, rest = idx % n[0], idx // n[0]
        ik = [i0, rest % n[1], rest // n[1]]
        u = [box_lo[k][:, None] + (ik[k].astype(np.float64)[None, :] + 0.5) * cell[k][:, None] for k in range(3)]
        chi, amp = chi2(model, n_used, L, y, g, candidate(model, u[0], u[1], u[2]), wrong_break_side)
        j = np.argmin(chi, axis=1)                                     # the first of equal minima: the lowest index
        rows = np.arange(S)
        better = chi[rows, j] < best_chi
        for k in range(3):
            best[k] = np.where(better, u[k][rows, j], best[k])
        best_amp = np.where(better, amp[rows, j], best_amp)
        best_chi = np.where(better, chi[rows, j], best_chi)
    few = n_used < n_par(model) + 1
    none = ~few & ~(best_chi <= np.finfo(np.float64).max)
    bad = few | none
    near = lambda k: (best[k] - lo[k] <= cell[k]) | (hi[k] - best[k] <= cell[k])
    status = np.where(near(0), AT_BOUND_ALPHA, 0) | np.where(near(1), AT_BOUND_LAMBDA, 0) | (np.where(near(2), AT_BOUND_BETA, 0) if band else 0)
    status = np.where(few, TOO_FEW_BINS, np.where(none, NO_FINITE_CANDIDATE, status)).astype(np.int32)
    with np.errstate(all="ignore"):
        e_peak = e_piv * fit_exp(best[1])
    return {"alpha": np.where(bad, NAN, best[0]), "beta": np.where(bad | (not band), NAN, best[2]), "e_peak": np.where(bad, NAN, e_peak),
            "amplitude": np.where(bad, NAN, best_amp), "chi2": np.where(few, NAN, best_chi), "n_used": n_used.astype(np.int32),
            "dof": (n_used - n_par(model)).astype(np.int32), "status": status}


def default_bounds(e_edges, e_piv=E_PIV):
    e = np.asarray(e_edges, dtype=np.float64)
    return (DEFAULTS["alpha"], (float(np.log(e[0] / e_piv)), float(np.log(e[-1] / e_piv))), DEFAULTS["beta"])


def band_shape(alpha, beta, e_peak, e, e_piv=E_PIV):
    """the Band function's shape in plain NumPy (np.exp, np.log), independent of fit_exp and fit_log: for synthetic spectra"""
    e = np.asarray(e, dtype=np.float64)
    L, lam = np.log(e / e_piv), np.log(e_peak / e_piv)
    x = (2.0 + alpha) * np.exp(L - lam)
    low = alpha * L - x
    if beta is None:
        return np.exp(low)
    amb = alpha - beta
    return np.exp(np.where(x < amb, low, amb * (np.log(amb) - np.log(2.0 + alpha) + lam - 1.0) + beta * L))
