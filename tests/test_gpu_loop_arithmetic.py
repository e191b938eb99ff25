"""Function-level tests of the loop kernel's OWN arithmetic forms.  tests/test_gpu_functions.py covers the functions of physics.hpp that
restate a reference function; the loop kernels do not call those any more -- they call cell_staged_operands, kf_of_gamma, boost_with with
zero_norm_lean, optical_depth_staged, the Newton reciprocal / reciprocal root (rcp_nr, rsqrt_nr, sqrt_nr), the azimuth selects, hydro_coords
and the table look-up.  Here each of them is evaluated on arrays through mcrat_hip_eval_function and compared with

  A  mpmath at 200 bits (60 digits) on the very doubles sent to the device, and
  B  where one exists, the oracle's reference-form function,

with bars derived from the conditioning of the operation, not from agreement with another double computation.  u = 2^-53 throughout;
"spacing" is np.spacing of the correctly rounded result.  Every test prints the figures it measured before it asserts (pytest -s)."""
import ctypes as C
import math
import threading
import time
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_functions import GOLD, _kn_tol

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
M_EL, C_LIGHT = synth.M_EL, synth.C_LIGHT
K_B, M_P, THOM = 1.380658e-16, 1.6726231e-24, 6.65246e-25      # device_types.hpp
GAMMAS = (1.0, 1.0 + 1e-12, 1.0 + 1e-7, 1.5, 10.0, 100.0, 1000.0)
TINY, HUGE = 2.0 ** -1022, np.finfo(float).max
EINVAL = -1                                  # MCRAT_HIP_EINVAL


@pytest.fixture(autouse=True)
def _mp_200_bits():
    """reference A works at 200 bits (60 digits) inside these tests only: mpmath's precision is global to the process"""
    with mp.workprec(200):
        yield


@pytest.fixture(scope="module")
def dev():
    from mcrat_amd import engine
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 0)
    yield e
    e.close()


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def M(x):
    return mp.mpf(float(x))


def spacings_from(got, exact, rounded):
    """|got - rounded| and |got - exact| in spacings of the correctly rounded result (exact: mpf, rounded: its double)"""
    sp = float(np.spacing(abs(rounded)))
    return abs(got - rounded) / sp, float(abs(M(got) - exact) / sp)


# ---------------------------------------------------------------------------------------------- the primitives
def _primitive_inputs(signed):
    rng = np.random.default_rng(41)
    x = [np.ldexp(rng.uniform(1.0, 2.0, 12000), rng.integers(-1022, 1024, 12000))]                  # log-uniform over the normal range
    p2 = np.ldexp(1.0, np.arange(-1022, 1024))
    x += [p2, np.nextafter(p2, np.inf), np.nextafter(p2[1:], 0.0)]                                    # powers of two and their neighbours
    k = np.arange(1, 200, 2, dtype=float)
    # near-ties: 1/(1 - k 2^-53) = 1 + k 2^-53 + ..; sqrt(1 + k 2^-52) = 1 + k 2^-53 - ..; 1/sqrt(1 - k 2^-52) = 1 + k 2^-53 + ..  (k odd: just
    # off the midpoint of two doubles), each in a few binades (even shifts, so that the roots stay near-ties)
    ties = np.concatenate([1.0 - k * 2.0 ** -53, 1.0 + k * 2.0 ** -52, 1.0 - k * 2.0 ** -52])
    x += [np.ldexp(ties, s) for s in (0, -2, 2, -600, 600, -1020, 1020)]
    n = rng.integers(1, 2 ** 26, 400).astype(float)
    x += [n * n, np.ldexp(n * n, -400), 1.0 / np.ldexp(1.0, rng.integers(0, 500, 50)) * 3.0]          # exact roots; exact-ish reciprocals
    x += [np.array([TINY, np.nextafter(TINY, 1.0), HUGE, np.nextafter(HUGE, 0.0), 1.0, 2.0, 3.0, 4.0, 0.25, 10.0, 1e-300, 1e300])]
    x = np.concatenate(x)
    if signed:
        x = x * np.where(rng.uniform(size=x.size) < 0.5, -1.0, 1.0)
    assert x.size >= 10000 and np.all(np.isfinite(x)) and np.all(np.abs(x) >= TINY)
    return x


def _exact_rcp(x):
    f = Fraction(1) / Fraction(float(x))
    try:
        cr = float(f)                                                     # (int / int is correctly rounded, subnormal results included)
    except OverflowError:
        cr = math.copysign(math.inf, x)
    return mp.mpf(f.numerator) / mp.mpf(f.denominator), cr


def _exact_rsqrt(x):
    a = 1 / mp.sqrt(M(x))
    return a, float(a)


def _exact_sqrt(x):
    a = mp.sqrt(M(x))
    return a, float(a)


_PRIMS = {"rcp_nr": (_exact_rcp, 1, True), "rsqrt_nr": (_exact_rsqrt, 2, False), "sqrt_nr": (_exact_sqrt, 2, False)}


@pytest.mark.parametrize("name", ["rcp_nr", "rsqrt_nr", "sqrt_nr"])
def test_newton_primitive_within_its_derived_bound_over_the_normal_range(dev, name):
    """rcp_nr: after two Newton steps the unrounded r + r e = (1/x)(1 - e^2) is 1/x to 2^-100; the last fma rounds it once, so the result is the
    correctly rounded 1/x or, within 2^-100 of a midpoint, its neighbour: 1 spacing.  rsqrt_nr: the product h*y is rounded before the last fma
    (relative u, on a term that is 1/2: an absolute u/2 on e, a relative u/2 <= half a spacing on y) and the fma rounds once more (half a
    spacing): 1 spacing from the exact value, so at most 2 from the correctly rounded one once that is itself half a spacing off.  sqrt_nr
    = x * rsqrt_nr(x): the factor's relative 1.5 u is up to 1.5 spacings of a root just below a power of two, the product rounds once more:
    2 spacings from the exact value, 2 from the correctly rounded one (an integer number of spacings <= 2.5).
    A subnormal result (1/x for |x| > 2^1022, the upper end of the normal range included) is held to the same bar, in ITS spacing, 2^-1074: the last
    fma still rounds the nearly exact r + r e once, now to the subnormal grid."""
    exact, bar, signed = _PRIMS[name]
    x = _primitive_inputs(signed)
    got = dev.eval_function(name, x)[:, 0]
    worst_r, worst_e, at = 0.0, 0.0, None
    n = 0
    for xi, gi in zip(x, got):
        a, cr = exact(xi)
        assert math.isfinite(gi), (name, xi, gi)
        dr, de = spacings_from(gi, a, cr)
        n += 1
        if dr > worst_r or (dr == worst_r and de > worst_e):
            worst_r, worst_e, at = dr, max(worst_e, de), xi
        worst_e = max(worst_e, de)
    print("%s: %d inputs, worst %.0f spacings from the correctly rounded result, %.3f from the exact one (x = %r)" % (name, n, worst_r, worst_e, at))
    assert n == len(x) >= 10000 and worst_r <= bar


def test_newton_primitives_specials_are_exact(dev):
    inf, nan = np.inf, np.nan
    x = np.array([0.0, -0.0, inf, -inf, nan, -1.0, -TINY, -HUGE])
    r, q, s = (dev.eval_function(f, x)[:, 0] for f in ("rcp_nr", "rsqrt_nr", "sqrt_nr"))
    assert r[0] == inf and r[1] == -inf and r[2] == 0 and not np.signbit(r[2]) and r[3] == 0 and np.signbit(r[3]) and np.isnan(r[4])
    assert r[5] == -1.0
    assert q[0] == inf and q[2] == 0 and not np.signbit(q[2])                       # x = 0 -> inf, x = inf -> 0
    assert np.isinf(q[1])                                                           # 1/sqrt(-0) = -inf in IEEE arithmetic, as the hardware's estimate
    assert np.isnan(q[3:]).all()                                                    # -inf, NaN, negative arguments
    assert s[0] == 0 and s[1] == 0 and np.isnan(s[3:]).all()                        # sqrt_nr(0) == 0; NaN for negative x, like sqrt
    # (sqrt_nr(inf) is outside the stated domain, physics.hpp: inf * rsqrt_nr(inf) = inf * 0 today, where sqrt gives inf; neither is asserted)


def test_newton_primitives_on_subnormals(dev):
    """Subnormal inputs and results stay finite wherever the IEEE result is finite -- but for a reciprocal within 2^-20 of the largest double, where
    the hardware's estimate overflows (measured: 2^-30) -- and rcp_nr keeps its 1 spacing on them.  rsqrt_nr and
    sqrt_nr are outside their stated domain on a subnormal x = m 2^-1074 (physics.hpp): h = 0.5 x is rounded to a multiple of 2^-1074, a relative
    error d with |d| <= 1/m, and two Newton steps towards 1/sqrt(2h) from an estimate of 1/sqrt(x) leave y (1 - d/2)(1 + 3d^2/8 - d^3/8), a relative
    error of at most 1.25/m (m = 1: h = 0, y = 2.25 y0) -- plus the 2 spacings (4u) of the normal range.  The iteration has not converged there, so
    the hardware estimate's own relative error eta (well under 2^-20) survives at first order in d, at most 4 eta/m.  That bound is asserted."""
    rng = np.random.default_rng(42)
    m = np.unique(np.concatenate([np.arange(1, 65), 2 ** np.arange(0, 52), 2 ** np.arange(1, 52) - 1, 2 ** np.arange(1, 52) + 1,
                                  rng.integers(1, 2 ** 52, 2000), (2 ** rng.uniform(0, 52, 2000)).astype(np.int64)]))
    m = np.unique(np.concatenate([m, 2 ** 50 + np.arange(1, 64), 2 ** 50 + 2 ** np.arange(6, 50)]))      # 1/x from the largest double down
    m = m[(m >= 1) & (m < 2 ** 52)]
    sub = m.astype(float) * 2.0 ** -1074
    # 1/x: subnormal x (IEEE: finite from 2^-1024 on, m >= 2^50; +-inf below) and x beyond 2^1022, whose reciprocal is subnormal
    big = np.concatenate([np.ldexp(rng.uniform(1.0, 2.0, 2000), rng.integers(1022, 1024, 2000)), [2.0 ** 1022, 2.0 ** 1023, HUGE]])
    for x in (np.concatenate([sub, -sub]), np.concatenate([big, -big])):
        got = dev.eval_function("rcp_nr", x)[:, 0]
        worst, lost = 0.0, []
        for xi, gi in zip(x, got):
            a, cr = _exact_rcp(xi)
            if math.isinf(cr):
                assert gi == cr, (xi, gi)
                continue
            if not math.isfinite(gi):
                assert gi == math.copysign(math.inf, xi), (xi, gi)
                lost.append(abs(cr) / HUGE)
                continue
            worst = max(worst, spacings_from(gi, a, cr)[0])
        print("rcp_nr, %s: worst %.3g spacings from the correctly rounded result; %d finite reciprocals returned as inf, the smallest at %s of the "
              "largest double" % ("subnormal x" if abs(x[0]) < TINY else "subnormal 1/x", worst, len(lost), "1 - %.3g" % (1 - min(lost)) if lost else "-"))
        # the estimate is the hardware's, good to eta < 2^-20 relative: where 1/x is within eta of the largest double the estimate may overflow, and
        # rcp_nr returns a non-finite estimate as it is (physics.hpp).  Everywhere else the result is finite, and within the 1 spacing of the
        # normal range: subnormal x with a finite reciprocal, and subnormal reciprocals in their own spacing.
        assert all(v > 1 - 2.0 ** -20 for v in lost), min(lost)
        assert worst <= 1, worst
    for name, exact in (("rsqrt_nr", _exact_rsqrt), ("sqrt_nr", _exact_sqrt)):
        got = dev.eval_function(name, sub)[:, 0]
        worst_sp, worst_ratio = 0.0, 0.0
        for mi, xi, gi in zip(m, sub, got):
            a, cr = exact(xi)
            assert math.isfinite(gi) and gi > 0, (name, xi, gi)
            rel = float(abs(M(gi) - a) / a)
            worst_sp = max(worst_sp, spacings_from(gi, a, cr)[0])
            bound = (1.25 + 2.0 ** -18) / float(mi) + 4 * U
            worst_ratio = max(worst_ratio, rel / bound)
            assert rel <= bound, (name, int(mi), rel)
        print("%s, subnormal x: worst %.3g spacings (%.3f of the 1.25/m bound)" % (name, worst_sp, worst_ratio))


# ---------------------------------------------------------------------------------------------- cell_staged_operands, kf_of_gamma
def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def test_cell_staged_operands(dev):
    """gam = 1/sqrt(1 - v^2): v^2 carries a relative rounding error of 2u, which 1 - v^2 amplifies by v^2/(1 - v^2) = Gamma^2 - 1, the root halves
    it, root and division add u each: 4u (1 + Gamma^2) has a factor 2 in hand.  kf = gam^2/(gam + 1) from the RETURNED gam: three roundings (IEEE
    form) or two and the Newton reciprocal's 1 spacing (kf_of_gamma): 4u.  nsig: two roundings, 2u.  w = beta_g / |v|: |v| as above without the
    amplification (3.5u); beta_g = sqrt(1 - 1/gamma_cell^2) is the reference's expression (optical_depth.c:52) and is ill-conditioned at
    the OTHER end: q = 1/gamma_cell^2 carries 2u, an absolute 2u q on 1 - q, relative 2u q/(1 - q) = 2u/(Gamma_cell^2 - 1), halved by the
    root.  The bar 4u (1 + Gamma_cell^2) covers every roundoff but that one, so the term u/(Gamma_cell^2 - 1) -- 2u with the same factor 2 in
    hand -- is added to it: at Gamma_cell = 1 + 1e-12 the reference's own beta is good to 3e-5 only, on the host as on the device."""
    rng = np.random.default_rng(43)
    rows = []
    for g in GAMMAS[1:]:
        for _ in range(40):
            rows.append([*(math.sqrt(1.0 - 1.0 / g ** 2) * _unit(rng)), g, 10 ** rng.uniform(-8, 3)])
    rows.append([0.0, 0.0, 0.0, 1.0, 1e-3])                                         # a cell at rest
    rows = np.array(rows)
    got = dev.eval_function("cell_operands", rows)
    worst = dict(gam=0.0, kf=0.0, kfg=0.0, nsig=0.0, w=0.0, kf_pair=0.0)
    for r, (w, nsig, gam, kf, kfg) in zip(rows[:-1], got[:-1]):
        a, b, c, gc, dens = (M(v) for v in r)
        v2 = a * a + b * b + c * c
        gam_a = 1 / mp.sqrt(1 - v2)
        G2 = float(gam_a) ** 2
        e = float(abs(M(gam) - gam_a) / gam_a) / (4 * U * (1 + G2))
        worst["gam"] = max(worst["gam"], e)
        kf_a = M(gam) ** 2 / (M(gam) + 1)
        worst["kf"] = max(worst["kf"], float(abs(M(kf) - kf_a) / kf_a) / (4 * U))
        worst["kfg"] = max(worst["kfg"], float(abs(M(kfg) - kf_a) / kf_a) / (4 * U))
        worst["kf_pair"] = max(worst["kf_pair"], abs(kf - kfg) / float(np.spacing(min(kf, kfg))) / 2)
        nsig_a = dens / M(M_P) * M(THOM)
        worst["nsig"] = max(worst["nsig"], float(abs(M(nsig) - nsig_a) / nsig_a) / (2 * U))
        w_a = mp.sqrt(1 - 1 / (gc * gc)) / mp.sqrt(v2)
        gc2 = float(gc) ** 2
        worst["w"] = max(worst["w"], float(abs(M(w) - w_a) / w_a) / (4 * U * (1 + gc2) + 2 * U / (gc2 - 1)))
    print("cell_staged_operands, worst fraction of each bar: " + ", ".join("%s %.3f" % kv for kv in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    w, nsig, gam, kf, kfg = got[-1]
    assert gam == 1.0 and kf == 0.5 and kfg == 0.5 and np.isnan(w) and nsig > 0       # at rest: 0/0, as the reference's cosine (optical_depth.c:46)


# ---------------------------------------------------------------------------------------------- boost_with
def _boost_cases(rng, reps):
    """Gamma x {head-on, tail-on, sideways, random, within 1/Gamma of the flow}; photon energies 1e-20 .. 1e-15, p0 = |p|.
    -> b[3], p[4], kind"""
    rows, kinds = [], []
    for g in GAMMAS:
        beta = math.sqrt(1.0 - 1.0 / g ** 2)
        for kind in range(5):
            for _ in range(reps):
                n = _unit(rng)
                t = np.cross(n, _unit(rng))
                t /= np.linalg.norm(t)
                if kind == 0:
                    d = -n
                elif kind == 1:
                    d = n.copy()
                elif kind == 2:
                    d = t
                elif kind == 3:
                    d = _unit(rng)
                else:
                    th = rng.uniform(0.0, 1.0) / g
                    d = math.cos(th) * n + math.sin(th) * t
                e = 10 ** rng.uniform(-20, -15)
                sp = e * d
                rows.append([*(beta * n), float(np.sqrt(sp @ sp)), *sp])
                kinds.append(kind)
    return np.array(rows), np.array(kinds)


def _kappa(b, p):
    """(1 + |c|)/(1 - c), c = b . p_hat: how much the cancellation in p0 - b.p amplifies the roundoff of its operands"""
    c = (b[0] * p[1] + b[1] * p[2] + b[2] * p[3]) / mp.sqrt(p[1] ** 2 + p[2] ** 2 + p[3] ** 2)
    return (1 + abs(c)) / (1 - c)


def _exact_boost(b, g, kf, p, photon):
    """p'_0 = g (p_0 - b.p), p'_i = p_i + (kf (b.p) - g p_0) b_i; 'photon': the spatial part rescaled to p'_0 (zeroNorm)"""
    bp = b[0] * p[1] + b[1] * p[2] + b[2] * p[3]
    f = kf * bp - g * p[0]
    out = [g * (p[0] - bp)] + [p[k + 1] + f * b[k] for k in range(3)]
    if photon:
        s = out[0] / mp.sqrt(out[1] ** 2 + out[2] ** 2 + out[3] ** 2)
        out = [out[0]] + [s * out[k] for k in (1, 2, 3)]
    return out


def _boost_error(got, want):
    """the largest component error relative to |p'_0|"""
    return float(max(abs(M(got[k]) - want[k]) for k in range(4)) / abs(want[0]))


@pytest.mark.parametrize("what", ["photon", "electron"])
def test_boost_with_given_gamma_and_kf(dev, what):
    """A evaluates the loop's formula exactly on the doubles sent (g and kf included): what remains is roundoff.  b.p carries 2.5u of |b.p|,
    p_0 - b.p one more rounding: relative (2.5 |c| + 1)u / (1 - c) <= 2.5 u kappa on p'_0; f = kf (b.p) - g p_0 cancels two terms of g p_0 to
    O(p_0), an absolute 3.5 u g p_0 that f b_i hands to the spatial part, against p'_0 = g p_0 (1 - c): 3.5 u /(1 - c) again.  The photon's
    rescaling adds the reciprocal root's 2 spacings and two roundings, not amplified.  8 u kappa: the emulation's worst case was 2.75 u kappa
    over 1400 cases."""
    rng = np.random.default_rng(44)
    bp_rows, _ = _boost_cases(rng, 40)
    assert len(bp_rows) == 1400
    b2 = (bp_rows[:, :3] ** 2).sum(axis=1)
    g = 1.0 / np.sqrt(1.0 - b2)
    kf = g * g / (g + 1.0)
    rows = np.concatenate([bp_rows[:, :3], g[:, None], kf[:, None], bp_rows[:, 3:]], axis=1)
    got = dev.eval_function("boost_with_" + what, rows)
    worst, worst_null = 0.0, 0.0
    for r, o in zip(rows, got):
        b, gg, kk, p = [M(v) for v in r[:3]], M(r[3]), M(r[4]), [M(v) for v in r[5:]]
        want = _exact_boost(b, gg, kk, p, what == "photon")
        worst = max(worst, _boost_error(o, want) / float(8 * U * _kappa(b, p)))
        if what == "photon":
            worst_null = max(worst_null, float(abs(mp.sqrt(M(o[1]) ** 2 + M(o[2]) ** 2 + M(o[3]) ** 2) - M(o[0])) / M(o[0])) / (4 * U))
    print("boost_with<%s>: worst %.3f of 8 u kappa (%.2f u kappa); null to %.3f of 4u" % (what, worst, 8 * worst, worst_null))
    assert worst <= 1.0 and worst_null <= 1.0
    rest = b2 == 0
    assert rest.sum() == 200
    if what == "electron":
        assert np.array_equal(got[rest], rows[rest, 5:])                            # b = 0 needs no special case: g = 1, kf = 1/2, the identity


def _staged_errors(rows, out):
    """per case: error against A computed from b alone, as a fraction of 4 u kappa (1 + Gamma^2), and in units of u"""
    frac, in_u = np.zeros(len(rows)), np.zeros(len(rows))
    for i, (r, o) in enumerate(zip(rows, out)):
        b, p = [M(v) for v in r[:3]], [M(v) for v in r[3:]]
        b2 = b[0] ** 2 + b[1] ** 2 + b[2] ** 2
        g = 1 / mp.sqrt(1 - b2)
        want = _exact_boost(b, g, g * g / (g + 1), p, True)
        err = _boost_error(o, want)
        frac[i] = err / float(4 * U * _kappa(b, p) * (1 + g * g))
        in_u[i] = err / U
    return frac, in_u


def _oracle_boost(oracle, rows):
    want = np.zeros((len(rows), 4))
    for i, r in enumerate(rows):
        b, p = np.ascontiguousarray(r[:3]), np.ascontiguousarray(r[3:])
        oracle.lib().orc_lorentzBoost(dp(b), dp(p), dp(want[i]), b"p")
    return want


def test_boost_staged_photon_against_exact_boost_from_beta_alone(dev, oracle):
    """What a re-location runs: gam from the staged record (cell_staged_operands), kf_of_gamma(gam), boost_with<true>.  Against the exact boost of
    b: gam carries 2u (Gamma^2 - 1) + 2u (test_cell_staged_operands) and the cancellation amplifies by kappa as above; the bar is their product,
    4 u kappa (1 + Gamma^2).  The reference form (orc_lorentzBoost, on the CPU) goes through the SAME assertion: the bar is not the code under
    test's own."""
    rng = np.random.default_rng(45)
    rows, _ = _boost_cases(rng, 40)
    frac_ref, _ = _staged_errors(rows, _oracle_boost(oracle, rows))
    print("orc_lorentzBoost (reference form, CPU): worst %.3f of 4 u kappa (1 + Gamma^2)" % frac_ref.max())
    assert frac_ref.max() <= 1.0
    got = dev.eval_function("boost_staged_photon", rows)
    frac, in_u = _staged_errors(rows, got)
    g_of = np.repeat(GAMMAS, 200)
    print("boost_staged_photon: worst %.3f of 4 u kappa (1 + Gamma^2); worst loss per Gamma in u: %s"
          % (frac.max(), ", ".join("%.13g: %.3g" % (g, in_u[g_of == g].max()) for g in GAMMAS)))
    assert frac.max() <= 1.0
    null = np.abs(np.linalg.norm(got[:, 1:], axis=1) - got[:, 0]) / got[:, 0]
    assert null.max() <= 4 * U


def test_gamma_1000_tail_on_boost_loses_more_than_1e5_u(dev, oracle):
    """A photon travelling along a Gamma = 1000 flow: kappa = 4 Gamma^2 and the 2u (Gamma^2 - 1) of gam together cost millions of u (3.5e6 u, 4e-10
    relative, in the emulation) -- inherent conditioning, the reference form loses as much, and it is within a factor 3 of the 1e-9 trajectory
    gate.  A 'simplification' that changes the conditioning changes this figure."""
    rng = np.random.default_rng(46)
    beta = math.sqrt(1.0 - 1.0 / 1000.0 ** 2)
    rows = []
    for _ in range(64):
        n, e = _unit(rng), 10 ** rng.uniform(-20, -15)
        sp = e * n
        rows.append([*(beta * n), float(np.sqrt(sp @ sp)), *sp])
    rows = np.array(rows)
    _, dev_u = _staged_errors(rows, dev.eval_function("boost_staged_photon", rows))
    _, ref_u = _staged_errors(rows, _oracle_boost(oracle, rows))
    print("Gamma = 1000 tail-on, loss against the exact boost: device %.3g u (%.2g relative), reference form %.3g u" % (dev_u.max(), dev_u.max() * U, ref_u.max()))
    assert dev_u.max() > 1e5 and ref_u.max() > 1e5
    assert dev_u.max() * U < 1e-9                                                    # ... and still inside the trajectory gate


# ---------------------------------------------------------------------------------------------- optical_depth_staged
def _tau_cases(rng, reps, norm_one):
    rows = []
    for g in GAMMAS[1:]:
        beta = math.sqrt(1.0 - 1.0 / g ** 2)
        for kind in range(5):
            for _ in range(reps):
                n = _unit(rng)
                t = np.cross(n, _unit(rng))
                t /= np.linalg.norm(t)
                th = rng.uniform(0.0, 1.0) / g
                d = (-n, n, t, _unit(rng), math.cos(th) * n + math.sin(th) * t)[kind]
                rows.append([*(beta * n), g, 10 ** rng.uniform(-8, 3), *(10 ** rng.uniform(-20, -15) * d), 1.0 if norm_one else rng.uniform(0.05, 1.0)])
    return np.array(rows)


def _tau_bar_and_exact(r):
    """tau = nsig norm (1 - beta_g cos), cos = (v.p)/(|v||p|), beta_g = sqrt(1 - 1/gamma_cell^2).  With x = w c' = beta_g cos: the operands of
    1 - x carry the roundoff of w (4u (1 + Gamma_cell^2) without its beta_g term, test_cell_staged_operands), of v.p (2.5u) and of 1/|p| (2
    spacings), which the subtraction amplifies by |x|/(1 - x); its own rounding and the products with nsig norm add 4u: 8u (1 + |x|)/(1 - x)
    (1 + Gamma_cell^2).  The reference's beta_g adds what its own conditioning costs at Gamma_cell -> 1: an absolute u/(Gamma_cell^2 beta_g) on
    beta_g (relative u/(Gamma_cell^2 - 1)), |cos| of it on x, over (1 - x) on tau -- taken twice, like the other terms."""
    v, gc, dens, p, norm = [M(t) for t in r[:3]], M(r[3]), M(r[4]), [M(t) for t in r[5:8]], M(r[8])
    beta_g = mp.sqrt(1 - 1 / (gc * gc))
    cos = (v[0] * p[0] + v[1] * p[1] + v[2] * p[2]) / (mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2) * mp.sqrt(p[0] ** 2 + p[1] ** 2 + p[2] ** 2))
    x = beta_g * cos
    tau = dens / M(M_P) * M(THOM) * norm * (1 - x)
    bar = (8 * U * (1 + abs(x)) * (1 + gc * gc) + 2 * U * abs(cos) / (gc * gc * beta_g)) / (1 - x)
    return tau, float(bar)


def _oracle_tau(oracle, rows):
    cfg = oracle.make_config(oracle.THREE, oracle.CARTESIAN, 0)
    out = np.zeros(len(rows))
    for i, r in enumerate(rows):
        frame = dict(num_elements=1, v0=[r[0]], v1=[r[1]], v2=[r[2]], gamma=[r[3]], dens_lab=[r[4]], temp=[1e6])
        H = oracle.OracleHydro(frame)
        ph = np.zeros(1, dtype=oracle.PHOTON_DTYPE)
        ph["p1"], ph["p2"], ph["p3"] = r[5], r[6], r[7]
        ph["p0"] = math.sqrt(r[5] ** 2 + r[6] ** 2 + r[7] ** 2)
        ph["r0"], ph["r1"], ph["r2"] = 1e10, 2e10, 3e10
        oracle.lib().orc_calculateOpticalDepth(C.byref(cfg), ph.ctypes.data, C.byref(H.c))
        out[i] = ph["total_optical_depth"][0]
    return out


def test_optical_depth_staged(dev, oracle):
    rng = np.random.default_rng(47)
    rows = np.concatenate([_tau_cases(rng, 20, True), _tau_cases(rng, 20, False)])
    n_b = len(rows) // 2                                                             # the first half has norm = 1: what the oracle computes in DIRECT
    got = dev.eval_function("optical_depth_staged", rows)
    ref = _oracle_tau(oracle, rows[:n_b])
    worst_a, worst_b, worst_ref, worst_n = 0.0, 0.0, 0.0, 0.0
    for i, (r, (tau, ntau)) in enumerate(zip(rows, got)):
        tau_a, bar = _tau_bar_and_exact(r)
        worst_a = max(worst_a, float(abs(M(tau) - tau_a) / tau_a) / bar)
        if i < n_b:
            worst_b = max(worst_b, abs(tau - ref[i]) / ref[i] / bar)
            worst_ref = max(worst_ref, float(abs(M(ref[i]) - tau_a) / tau_a) / bar)   # the reference form through the same assertion
        _, cr = _exact_rcp(-tau)
        worst_n = max(worst_n, abs(ntau - cr) / float(np.spacing(abs(cr))))
    print("optical_depth_staged: worst fraction of the bar against A %.3f, against the oracle %.3f (oracle against A %.3f); ntau %.0f spacings from -1/tau"
          % (worst_a, worst_b, worst_ref, worst_n))
    assert worst_ref <= 1.0 and worst_a <= 1.0 and worst_b <= 1.0 and worst_n <= 1.0
    # a fluid at rest: 0/0 on both sides, as the reference's cosine (optical_depth.c:46)
    rest = np.array([[0.0, 0.0, 0.0, 1.0, 1e-3, 1e-18, 2e-18, -1e-18, 1.0]])
    g = dev.eval_function("optical_depth_staged", rest)
    assert np.isnan(g).all() and np.isnan(_oracle_tau(oracle, rest)).all()


# ---------------------------------------------------------------------------------------------- the azimuth selects
def test_azimuth_selects(dev):
    """c = x/h, s = y/h with h^2 = x^2 + y^2 (relative 2u, halved by the root), the reciprocal root (1.5u) or root and reciprocal (1u + 1u), and the
    product's rounding: under 3u of a value that is at most 1.  The radii stay inside the range the functions' comments give (2^-484 .. 2^511).
    The two functions against each other: the factors 1/h differ by up to 1.5u + 2u (rsqrt_nr: 1 spacing from the exact value, at most 1.5u;
    IEEE root then rcp_nr: half a spacing each, at most u each), which is up to 3.5 spacings of a result whose spacing is u of it, and each product
    rounds once more (half a spacing each): an integer number of spacings <= 4.5, so 4 -- not the 2 a count of the roundings alone suggests."""
    rng = np.random.default_rng(48)
    pts = []
    for r in 10 ** np.linspace(-3, 17, 41):
        for k in range(8):                                                           # every octant
            phi = (k + rng.uniform(0.02, 0.98)) * math.pi / 4
            pts.append([r * math.cos(phi), r * math.sin(phi)])
        pts += [[r, 0.0], [-r, 0.0], [0.0, r], [0.0, -r], [r, -0.0], [-r, -0.0], [-0.0, r], [-0.0, -r]]      # on the axes, either zero
        pts += [[r, r * 1e-9], [-r * 1e-12, r], [r, -r * 2.0 ** -60]]                 # next to them
    pts = np.array(pts)
    got = dev.eval_function("azimuth", pts)
    worst, worst_pair = 0.0, 0.0
    for (x, y), o in zip(pts, got):
        h = mp.sqrt(M(x) ** 2 + M(y) ** 2)
        for k, want in ((0, M(x) / h), (1, M(y) / h)):
            worst = max(worst, float(abs(M(o[k]) - want)) / (3 * U), float(abs(M(o[k + 2]) - want)) / (3 * U))
            lo = min(abs(o[k]), abs(o[k + 2]))
            worst_pair = max(worst_pair, abs(o[k] - o[k + 2]) / float(np.spacing(lo)) / 4 if lo > 0 else (0.0 if o[k] == o[k + 2] else np.inf))
    print("azimuth: worst %.3f of 3u against A; cos_sin_of_atan2 and cos_sin_with_hypot differ by at most %.1f spacings (bar: 4)" % (worst, 4 * worst_pair))
    assert worst <= 1.0 and worst_pair <= 1.0
    # The four origins.  The cosine is cos(atan2(y, x)) exactly: +1 for x = +0, -1 for x = -0.  The sine is a zero, exactly; its SIGN is not
    # atan2's: sin(atan2(-0, +0)) = -0 and the sine of the angle -pi of (-0, -0) is -0, the device returns the literal +0 for all four (stated
    # in the functions' comment with the reason it is harmless, and in DESIGN.md section 5).  What the device produces is pinned, sign included.
    # (math.sin(math.atan2(0.0, -0.0)) is 1.2e-16: the sine of pi's double, not of the angle.)
    zeros = np.array([[0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]])           # (x, y)
    g = dev.eval_function("azimuth", zeros)
    for (x, y), o in zip(zeros, g):
        assert o[0] == o[2] == math.cos(math.atan2(y, x)) == (-1.0 if np.signbit(x) else 1.0), (x, y, o)
        assert o[1] == 0.0 and o[3] == 0.0 and not np.signbit(o[1]) and not np.signbit(o[3]), (x, y, o)
    # on the axes, off the origin: the vanishing component is a zero with the sign of its coordinate, as cos / sin of atan2 give it
    # (sin(atan2(-0, x)) = -0 for either sign of x; cos(atan2(y, -0)) = cos(+-pi/2) rounds to +6e-17 in libm but is a signed zero as a product)
    on_x, on_y = pts[:, 1] == 0, pts[:, 0] == 0
    assert on_x.sum() == on_y.sum() == 41 * 4
    for k in (1, 3):
        assert np.all(got[on_x, k] == 0.0) and np.array_equal(np.signbit(got[on_x, k]), np.signbit(pts[on_x, 1]))
    for k in (0, 2):
        assert np.all(got[on_y, k] == 0.0) and np.array_equal(np.signbit(got[on_y, k]), np.signbit(pts[on_y, 0]))


# ---------------------------------------------------------------------------------------------- hydro_coords
_PAIRS = [(d, g) for d in (synth.TWO, synth.TWO_POINT_FIVE) for g in (synth.CARTESIAN, synth.CYLINDRICAL, synth.SPHERICAL)] + \
         [(synth.THREE, g) for g in (synth.CARTESIAN, synth.SPHERICAL, synth.POLAR)]


def _coord_points():
    rng = np.random.default_rng(49)
    pts = []
    for r in 10 ** np.linspace(6, 17, 23):
        for _ in range(6):
            pts.append(r * _unit(rng))
        pts += [[0.0, 0.0, r], [0.0, 0.0, -r], [r, 0.0, 0.0], [-r, 0.0, 0.0], [0.0, r, 0.0], [0.0, -r, 0.0]]     # on the axes
        for th in (1e-3, 1e-5, 3e-7, 1e-8, 1e-10):                                                                # towards both poles
            phi = rng.uniform(0, 2 * math.pi)
            for s in (1.0, -1.0):
                pts.append([r * math.sin(th) * math.cos(phi), r * math.sin(th) * math.sin(phi), s * r * math.cos(th)])
        for eps in (1e-3, 1e-9, 1e-15, 1e-17, 1e-30):                                                             # phi just below 2 pi, just above 0
            pts += [[r, -eps * r, 0.3 * r], [r, eps * r, -0.3 * r], [r, -0.0, r]]
    pts.append([0.0, 0.0, 0.0])                                                                                   # the origin: acos(0/0)
    return np.array(pts)


@pytest.mark.parametrize("dims,geom", _PAIRS)
def test_hydro_coords(oracle, dims, geom):
    """Against the oracle's mcratCoordinateToHydroCoordinate, the no-random-numbers bar of tests/test_gpu_functions.py: 1e-13 relative (sums, IEEE
    roots and quotients are the same bits on both sides; acos, atan2 and fmod are the two libraries').  An azimuth is relative to the full turn it
    is wrapped into: the + 360 of the wrap fixes its absolute quantum at an ulp of 360 degrees.  The polar angle within 1e-6 of a pole is compared
    with A instead: the rounding of z/r, one u next to 1, moves acos by u/sin(theta) -- a bar that needs an argument of its own: see below."""
    from mcrat_amd import engine
    e = engine.Engine(dims, geom, 0)
    pts = _coord_points()
    got = e.eval_function("hydro_coords", pts)
    e.close()
    cfg = oracle.make_config(dims, geom, 0)
    want = np.zeros_like(pts)
    for i, p in enumerate(pts):
        oracle.lib().orc_mcratCoordinateToHydroCoordinate(C.byref(cfg), dp(want[i]), *map(float, p))
    spherical = geom == synth.SPHERICAL
    wrapped = {synth.SPHERICAL: 2, synth.POLAR: 1}.get(geom) if dims == synth.THREE else None      # the azimuth's column
    scale = np.maximum(np.abs(want), 1e-300)
    if wrapped is not None:
        scale[:, wrapped] = 2 * math.pi
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want[-1, 1]) == spherical and not np.isnan(want[:-1]).any()                     # only the origin's acos(0/0)
    ok = ~np.isnan(want)
    rel = np.abs(got - want)[ok] / scale[ok]
    print("hydro_coords(%d, %d): worst %.3g relative against the oracle" % (dims, geom, rel.max()))
    assert rel.max() <= 1e-13
    if wrapped is not None:
        assert np.all((got[:, wrapped] >= 0) & (got[:, wrapped] < 2 * math.pi * (1 + 2 * U)))       # the fmod wrap
    if spherical:
        # near the poles against A.  fl(z/r): r = sqrt(fl(x^2 + y^2 + z^2)) carries 1.5u (the sum's two roundings halved, the root's own), the
        # quotient one more rounding: up to 2.5 u relative on a cosine next to +-1, i.e. 2.5 u / sin(theta) on the angle; acos adds an ulp of its
        # result.  u / sin(theta) is the size of ONE of these roundings; the bar is 3 u / sin(theta) + 2 ulp(theta).
        # The oracle's own theta (the reference form, on the CPU) goes through the SAME assertion: the bar is not the code under test's own.
        for who, res in (("oracle", want), ("device", got)):
            worst, n = 0.0, 0
            for p, o in zip(pts, res):
                x, y, z = (M(v) for v in p)
                rho = mp.sqrt(x * x + y * y)
                if rho == 0 and z == 0:
                    continue                                                          # the origin: NaN, compared above
                theta = mp.atan2(rho, z)
                if not (theta < 1e-6 or mp.pi - theta < 1e-6):
                    continue                                                          # away from the poles: the 1e-13 comparison above
                n += 1
                if rho == 0:
                    assert o[1] == (0.0 if z > 0 else math.pi)                        # on the axis: acos(+-1)
                    continue
                bar = 3 * U / float(mp.sin(theta)) + 2 * float(np.spacing(float(theta)))
                worst = max(worst, float(abs(M(o[1]) - theta)) / bar)
            print("hydro_coords(%d, %d), %s: polar angle within 1e-6 of the poles, %d points, worst %.3f of 3u/sin(theta)" % (dims, geom, who, n, worst))
            assert n > 100 and worst <= 1.0, who


# ---------------------------------------------------------------------------------------------- the table look-up
GRID = (-6.0, 2.0, -3.0, 2.0)              # 8 x 5 cells of one decade: the grid lines are integers, x0 + i dx is exact
N_E, N_T = 8, 5
MC, MCC = M_EL * C_LIGHT, M_EL * C_LIGHT * C_LIGHT


def _arg_with_log(f, inv, x, side=0):
    """An argument a (photon energy, temperature) whose normalised value f(a) has log10(f(a)) == x in double arithmetic (side 0; where no
    double gives exactly x, the nearest logarithm above it), or the nearest logarithm that is reached below (side -1) or above (side +1) x.
    Of the run of neighbouring doubles that give that logarithm the middle one is taken, so that a logarithm a last bit off the correctly
    rounded one still gives it.  inv: the inverse of f, for the starting point.  -> (a, log10(f(a)))"""
    a = float(inv(10.0 ** x))
    for _ in range(60):
        a = float(np.nextafter(a, 0.0))
    near = []                                             # 121 neighbouring doubles around f(a) = 10^x with their logarithms
    for _ in range(121):
        near.append((a, math.log10(f(a))))
        a = float(np.nextafter(a, np.inf))
    logs = [l for _, l in near]
    if side == 0 and x in logs:
        target = x
    else:
        target = max(l for l in logs if l < x) if side < 0 else min(l for l in logs if l > x)
    run = [a for a, l in near if l == target]
    if target == round(target):                           # a grid line: the power of ten itself, where an argument gives it
        run = [a for a in run if f(a) == 10.0 ** target] or run
    return run[len(run) // 2], target


def _table_points(f, inv, lines):
    """arguments on every grid line and next to it on both sides, in the cell centres and somewhere inside, and off the table on both sides
    -> {logarithm: argument}"""
    req = []
    for v in lines:
        req += [(v, 0), (v, -1), (v, 1)]
    req += [(v + 0.5, 0) for v in lines[:-1]] + [(lines[0] + 0.123, 0), (lines[-1] - 0.377, 0)]
    req += [(lines[0] - 1e-9, 0), (lines[0] - 0.5, 0), (lines[0] - 3.0, 0), (lines[-1] + 1e-9, 0), (lines[-1] + 0.5, 0), (lines[-1] + 2.0, 0)]
    out = {}
    for x, side in req:
        a, l = _arg_with_log(f, inv, x, side)
        out[l] = a
    return out


def test_thermal_cross_section_lookup(dev, oracle):
    from mcrat_amd import engine
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 0, tau_calculation=engine.TAU_TABLE)
    assert np.array_equal(e.eval_function("thermal_cross_section", [[1e-18, 1e8]]), [[1.0, 0.0, 0.0, 0.0]])       # no table yet
    table = e.create_hot_cross_section(N_E, N_T, GRID, calls=1000, seed=5)
    e.set_hot_cross_section(table, GRID)
    en = _table_points(lambda a: a / MC, lambda v: v * MC, [GRID[0] + i for i in range(N_E + 1)])
    tm = _table_points(lambda a: K_B * a / MCC, lambda v: v * MCC / K_B, [GRID[2] + j for j in range(N_T + 1)])
    xs, ys = sorted(en), sorted(tm)
    assert all(float(i) in en for i in range(-6, 3)) and all(float(j) in tm for j in range(-3, 3))     # the grid lines themselves are reached
    pts = np.array([[x, y] for x in xs for y in ys])
    rows = np.array([[en[x], tm[y]] for x, y in pts])
    got = e.eval_function("thermal_cross_section", rows)
    kn_dev = e.eval_function("kn_cross_section_ieee", rows[:, 0] / MC)[:, 0]
    cfg = oracle.make_config(synth.TWO, synth.CYLINDRICAL, 0, hot_table=table, grid=GRID, fallback_calls=256)
    tab = [[M(v) for v in row] for row in table]
    n_node = n_in = n_flag = n_cold = 0
    worst_node = worst_in = worst_flag = 0.0
    for (x, y), (ev, tv), (norm, flag, eps, theta), kn in zip(pts, rows, got, kn_dev):
        miss = C.c_int(0)
        want = oracle.lib().orc_getThermalCrossSection(C.byref(cfg), float(ev), float(tv), C.byref(miss))
        assert int(flag) == miss.value, (x, y)                                        # the oracle's decision, for every point
        inside = GRID[0] <= x <= GRID[1] and GRID[2] <= y <= GRID[3]
        assert not (inside and miss.value)                                            # on the table: never integrated afresh
        if miss.value:
            # eps = 10^log10(e): the logarithm's last bit (a faithful one: up to an ulp of x) is worth ln(10) ulp(x) of eps, pow adds an ulp of
            # its own (2u).  4u covers that for |x| < 1 only; beyond, the bar follows ulp(x)
            n_flag += 1
            for val, arg, lg in ((eps, ev / MC, x), (theta, K_B * tv / MCC, y)):
                bar = 2 * U + math.log(10.0) * float(np.spacing(abs(lg)))
                worst_flag = max(worst_flag, abs(val - arg) / arg / bar)
            continue
        assert eps == 0 and theta == 0
        if not inside:                                                                # colder than the table: 1 below e_min, else Klein-Nishina
            assert y < GRID[2]
            n_cold += 1
            assert norm == (1.0 if ev / MC < 10.0 ** GRID[0] else kn), (x, y)
            assert abs(norm - want) <= float(_kn_tol(ev / MC)) * want
            continue
        xa, ya = mp.log10(M(ev) / M(MC)), mp.log10(M(K_B) * M(tv) / M(MCC))         # A: the bilinear interpolant at the exact logarithms
        i, j = min(int(mp.floor(xa - GRID[0] + mp.mpf(2) ** -60)), N_E - 1), min(int(mp.floor(ya - GRID[2] + mp.mpf(2) ** -60)), N_T - 1)
        t, u = xa - (GRID[0] + i), ya - (GRID[2] + j)
        z = (1 - t) * (1 - u) * tab[i][j] + t * (1 - u) * tab[i + 1][j] + (1 - t) * u * tab[i][j + 1] + t * u * tab[i + 1][j + 1]
        n_in += 1
        worst_in = max(worst_in, float(abs(M(norm) - mp.power(10, z)) / mp.power(10, z)) / 1e-13)
        assert abs(norm - want) <= 1e-13 * want
        if x == round(x) and y == round(y):                                           # a node: table_cell's settle loops and the closed last cell
            n_node += 1
            node = mp.power(10, tab[int(x - GRID[0])][int(y - GRID[2])])
            worst_node = max(worst_node, float(abs(M(norm) - node) / node) / (2 * U))
    print("thermal_cross_section_lookup: %d nodes, worst %.3f of 2u; %d interior points, worst %.3f of 1e-13; %d flagged, eps / theta worst %.3f of "
          "their bar; %d cold" % (n_node, worst_node, n_in, worst_in, n_flag, worst_flag, n_cold))
    assert n_node == (N_E + 1) * (N_T + 1) and worst_node <= 1.0 and worst_in <= 1.0 and worst_flag <= 1.0
    assert n_flag > 100 and n_cold > 50
    e.close()
    # DIRECT: no table, the cross section is 1
    assert np.array_equal(dev.eval_function("thermal_cross_section", rows[:50]), np.tile([1.0, 0.0, 0.0, 0.0], (50, 1)))


def test_eval_function_refuses_unknown_codes_and_a_table_in_the_making(dev):
    from mcrat_amd import engine
    one, out = np.ones(16), np.zeros(16)
    last = max(v[0] for v in engine.Engine.FN.values())
    assert sorted(v[0] for v in engine.Engine.FN.values()) == list(range(1, last + 1))
    for fn in (0, -1, last + 1, 1000):
        assert dev.lib.mcrat_hip_eval_function(dev.ctx, fn, 1, dp(one), dp(out), 0) == EINVAL
    assert dev.lib.mcrat_hip_eval_function(dev.ctx, last, 1, dp(one), dp(out), 0) == 0
    # THERMAL_CROSS_SECTION while another thread is inside mcrat_hip_create_hot_cross_section on the same context.  A context is one thread at a
    # time (include/mcrat_hip.h); this refusal is a courtesy beyond that contract and the one place the suite drives a context from two threads:
    # the probes take the refused path only, which touches nothing but the flag.  The table is the reference's grid with 40 times its samples,
    # seconds of kernel, and the probes start 0.3 s into it (ctypes releases the interpreter lock around the call).
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 0, tau_calculation=engine.TAU_TABLE)
    e.create_hot_cross_section(4, 4, calls=1000)                                     # (code object load)
    made = {}

    def create():
        t0 = time.perf_counter()
        try:
            made["table"] = e.create_hot_cross_section(calls=20000000)
        except Exception as err:                                                     # handed to the asserting thread below
            made["error"] = err
        made["seconds"] = time.perf_counter() - t0

    worker = threading.Thread(target=create)
    fn = engine.Engine.FN["thermal_cross_section"][0]
    codes = []
    worker.start()
    time.sleep(0.3)
    while worker.is_alive():
        codes.append(e.lib.mcrat_hip_eval_function(e.ctx, fn, 1, dp(one), dp(out), 0))
        time.sleep(0.01)
    worker.join()
    assert "error" not in made, made.get("error")
    assert made["table"].shape == (221, 81) and np.isfinite(made["table"]).all()     # the creation itself was not disturbed
    assert made["seconds"] > 1.0, "the creation took %.2f s: too short for probes that start 0.3 s into it" % made["seconds"]
    assert codes and codes[0] == EINVAL and set(codes) <= {0, EINVAL}, codes[:8]
    assert e.lib.mcrat_hip_eval_function(e.ctx, fn, 1, dp(one), dp(out), 0) == 0     # ... and not a moment longer
    e.close()


# ---------------------------------------------------------------------------------------------- kn_cross_section_ieee
def test_kn_cross_section_ieee(dev, oracle):
    g = np.load(GOLD)
    got = dev.eval_function("kn_cross_section_ieee", g["kn_eps"])[:, 0]
    assert np.all(np.abs(got - g["kn_sigma"]) <= _kn_tol(g["kn_eps"]) * np.abs(g["kn_sigma"]))
    seam = np.array([1e-3, np.nextafter(1e-3, 0), np.nextafter(1e-3, 1), 0.0, 1e-300, 1e-6, 1.0, 50.0, 1e3, 1e6])
    got = dev.eval_function("kn_cross_section_ieee", seam)[:, 0]
    want = np.array([oracle.lib().orc_kleinNishinaCrossSection(float(e)) for e in seam])
    assert np.all(np.abs(got - want) <= _kn_tol(seam) * np.abs(want))
    assert got[1] == 1.0 - 2.0 * seam[1] and got[3] == 1.0
    # On [1e-3, 1] terms of 2/eps^2 cancel to O(1).  Errors below are in units of u (1 + 2/eps^2), one rounding of the largest term.  BOTH forms take
    # log(fl(1 + 2 eps)) times a coefficient of 1/eps^3: the rounding of 1 + 2 eps alone is worth 1/(2 eps) units, 500 at the seam, and is the same
    # number in both.  What the reference's own divisions remove is private to the terms: 2/(e e) and (1 + e)/(e e e) carry 1 + 2.5 units, against
    # 5 + 8 through ie, ie ie, (ie ie) ie (rcp_nr: 1 spacing, up to 2u).  So "no further from the exact value than kn_cross_section" holds up to
    # those private roundings, which in the reciprocal form can cancel part of the shared error by luck: err_ieee <= err_lean + 3.5 + 13 units at
    # every point, and so for the maxima; a strict <= between the two maxima would be a coin flip decided by the shared term.
    eps = 10 ** np.random.default_rng(50).uniform(-3, 0, 4000)
    eps[0], eps[1] = 1e-3, 1.0
    ieee = dev.eval_function("kn_cross_section_ieee", eps)[:, 0]
    lean = dev.eval_function("kn_cross_section", eps)[:, 0]
    err = np.zeros((2, len(eps)))
    for i, e in enumerate(eps):
        x = M(e)
        a = mp.mpf(3) / 4 * (2 / x ** 2 + (1 / (2 * x) - (1 + x) / x ** 3) * mp.log(1 + 2 * x) + (1 + x) / (1 + 2 * x) ** 2)
        unit = U * (1 + 2 / e ** 2)
        err[0, i], err[1, i] = float(abs(M(ieee[i]) - a)) / unit, float(abs(M(lean[i]) - a)) / unit
    print("Klein-Nishina on [1e-3, 1], error in u (1 + 2/eps^2): ieee worst %.3f mean %.3f; reciprocal form worst %.3f mean %.3f"
          % (err[0].max(), err[0].mean(), err[1].max(), err[1].mean()))
    assert np.all(err[0] <= err[1] + 16.5) and err[0].max() <= err[1].max() + 16.5
    assert np.all(err[0] <= 1.0 / (2 * eps) * 2 + 16.5)                              # ... and the shared term is what the analysis says it is
