"""An independent reference for the per-frame reductions -- phMinMax, phScattStats and averagePhotonEnergy (Src/mclib.c:1358-1515) -- and the
synthetic photon lists the reduction tests run on.  Plain Python over a record array with the members r0, r1, r2, p0, weight and num_scatt of
struct photon; it imports neither the engine nor the oracle.  `cs_switch` is CYCLOSYNCHROTRON_SWITCH: on, phScattStats (:1401-1403) and
averagePhotonEnergy (:1373-1375) pass over every photon with weight == 0; phMinMax filters on weight != 0 under either setting (:1479).

What is exact and what is rounded:
  * every sum (num_scatt, r, p0 * weight, weight) is formed in integer arithmetic on the doubles' mantissas, so it has no summation error; the
    products p0 * weight are held exactly (106-bit integers).  An average is the exact sum divided by the exact count, rounded once.
  * the r that goes into the sum of r is the correctly rounded square root of the exact x^2 + y^2 + z^2: an integer square root with a sticky
    bit, rounded to nearest even (tests/test_reductions_checker_cpu.py holds it against mpmath at 200 bits, the arithmetic of
    tests/test_gpu_loop_arithmetic.py).
  * min_r and max_r are what the C returns: the extremes of the DOUBLE sqrt(x*x + y*y + z*z), products and sums rounded one by one in that
    order (numpy does not contract them), which is what a device built with -ffp-contract=off computes to the bit.  `min_r_cr` / `max_r_cr`
    are the correctly rounded r of the same two photons.
  * theta is acos(z / r) in mpmath at 200 bits on the exact r, rounded once; beside it `*_theta_dq`, the same acos of the double z / r that
    the C hands to its acos (what separates the error of an acos from that of its argument), and `*_theta_zr`, how far the rounding of z / r
    can move theta (theta_of_double_quotient).  The extremes are found among the photons whose double theta lies
    within 1e-7 rad of the double extreme (the double value is off by a few ulp of z / r times |cot theta|, and by 1.5e-8 at most where z / r
    rounds to 1), every one of them evaluated at 200 bits.
  * comparisons are the reference's > and <, so a NaN never wins, from the initial values DBL_MAX, 0, INT_MAX, 0; when nothing passes the filter
    the averages are 0/0 = NaN and min_scatt stays INT_MAX, as in the C.
  * a sum with a term that is not finite is not exact arithmetic's business: it is added up in slot order in doubles, which gives the C's inf or
    NaN (inf * 0 = NaN with the switch off).
"""
import math
import sys
from fractions import Fraction

import mpmath as mp
import numpy as np

DBL_MAX = sys.float_info.max
INT_MAX = 2 ** 31 - 1
C_LIGHT = 2.99792458e10          # Src/mcrat.h
U = 2.0 ** -53                   # unit roundoff of a double
RED_SLOTS = 512 * 256            # slots one trip of the context form's grid covers


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): the relative error bound of m roundings in a row"""
    return m * U / (1.0 - m * U)


# ---------------------------------------------------------------------------------------------- exact pieces
def _mant_exp(a):
    """finite doubles -> (python-int mantissas as an object array, exponents): a == m * 2**e exactly"""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return (m * 2.0 ** 53).astype(np.int64).astype(object), e.astype(np.int64) - 53


def _exact_sum(m, e):
    """sum of m[i] * 2**e[i] as a Fraction (m: object array of python ints)"""
    if len(m) == 0:
        return Fraction(0)
    lo = int(e.min())
    total = int(np.sum(m << (e - lo).astype(object)))
    return Fraction(total) * Fraction(2) ** lo


def _round_sqrt(M, half_exp):
    """the double nearest to sqrt(M) * 2**half_exp (M a python int >= 0), ties to even"""
    if M == 0:
        return 0.0
    s = max(0, 116 - M.bit_length())
    s += s & 1
    t = math.isqrt(M << s)
    sticky = (t * t) != (M << s)
    drop = t.bit_length() - 53              # >= 5: t has at least 58 bits
    head, low, half = t >> drop, t & ((1 << drop) - 1), 1 << (drop - 1)
    if low > half or (low == half and (sticky or (head & 1))):
        head += 1
    return math.ldexp(head, drop - s // 2 + half_exp)


def sqrt_cr(x, y, z):
    """the correctly rounded sqrt(x^2 + y^2 + z^2) of the EXACT sum of squares, element by element (not finite: the double evaluation)"""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    out = np.sqrt(x * x + y * y + z * z)
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return out
    parts = [_mant_exp(v[idx]) for v in (x, y, z)]
    lo = np.minimum(np.minimum(parts[0][1], parts[1][1]), parts[2][1])
    S = sum((m << (e - lo).astype(object)) ** 2 for m, e in parts)        # exact: (sum of squares) * 2**(-2 lo)
    for k, i in enumerate(idx):
        out[i] = _round_sqrt(int(S[k]), int(lo[k]))
    return out


def theta_hp(x, y, z):
    """acos(z / r) at 200 bits, rounded once to a double (r = 0: NaN, as 0/0 is)"""
    with mp.workprec(200):
        X, Y, Z = mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z))
        r = mp.sqrt(X * X + Y * Y + Z * Z)
        if r == 0 or not mp.isfinite(r):
            return float("nan")
        return float(mp.acos(Z / r))


def theta_of_double_quotient(x, y, z):
    """(acos at 200 bits of the DOUBLE q = z / sqrt(x*x + y*y + z*z) the C hands to acos, rounded once; how far the rounding of q can move
    theta).  q carries the three roundings under the root -- (1 + d)^(3/2) --, the root's and the division's: 3.5 u, taken as 4 u with the
    second-order terms, so theta lies within max |acos(q (1 +- 4u)) - acos(q)| of acos(q).  On the axis (x = y = 0) q is +-1 exactly: 0."""
    x, y, z = float(x), float(y), float(z)
    q = float(np.float64(z) / np.sqrt(np.float64(x * x + y * y) + np.float64(z * z)))
    with mp.workprec(200):
        Q = mp.mpf(q)
        t = mp.acos(Q)
        if x == 0 and y == 0:
            return float(t), 0.0
        clip = lambda v: max(mp.mpf(-1), min(mp.mpf(1), v))
        zr = max(abs(mp.acos(clip(Q * (1 + 4 * mp.mpf(U)))) - t), abs(mp.acos(clip(Q * (1 - 4 * mp.mpf(U)))) - t))
        return float(t), float(zr)


def _sum_or_ieee(terms_exact, terms_double):
    """(Fraction or None, double): the exact sum where every term is finite, the C's slot-order double sum otherwise"""
    if np.all(np.isfinite(terms_double)):
        return terms_exact(), None
    s = 0.0
    for t in terms_double:
        s += float(t)
    return None, s


def _ratio(num, den):
    """exact num / den rounded once; den == 0: the C's 0/0 or x/0"""
    if den == 0:
        return float("nan") if num == 0 else math.copysign(float("inf"), num)
    return float(Fraction(num) / Fraction(den))


# ---------------------------------------------------------------------------------------------- the three reductions
def reductions(rec, cs_switch, r_cr=None):
    """-> dict with min_r, max_r, min_theta, max_theta (phMinMax), max_scatt, min_scatt, avg_scatt, avg_r (phScattStats), avg_energy
    (averagePhotonEnergy), num_output (photons with weight != 0: printPhotons' count), list_capacity, count (phScattStats' count) and the exact
    sums.  r_cr: sqrt_cr of rec's positions if the caller has it already."""
    n = len(rec)
    x, y, z = (np.asarray(rec[k], dtype=np.float64) for k in ("r0", "r1", "r2"))
    w, p0, ns = (np.asarray(rec[k], dtype=np.float64) for k in ("weight", "p0", "num_scatt"))
    weighted = w != 0
    with np.errstate(all="ignore"):
        r_c = np.sqrt(x * x + y * y + z * z)                  # the C's double r: squares and sums rounded one by one, in this order
        th_d = np.arccos(z / r_c)
    if r_cr is None:
        r_cr = sqrt_cr(x, y, z)
    out = dict(list_capacity=n, num_output=int(np.count_nonzero(weighted)))

    # phMinMax (:1465-1515): weight != 0 under either switch
    rw = r_c[weighted]
    out["max_r"] = float(np.fmax.reduce(rw, initial=0.0))
    out["min_r"] = float(np.fmin.reduce(rw, initial=DBL_MAX))
    for name, pick in (("max_r", np.flatnonzero(weighted & (r_c == out["max_r"]))), ("min_r", np.flatnonzero(weighted & (r_c == out["min_r"])))):
        out[name + "_cr"] = float(r_cr[pick[0]]) if len(pick) else out[name]
    valid = np.flatnonzero(weighted & ~np.isnan(th_d))
    out.update(min_theta=DBL_MAX, max_theta=0.0, min_theta_dq=DBL_MAX, max_theta_dq=0.0, min_theta_zr=0.0, max_theta_zr=0.0)
    if len(valid):
        lo, hi = th_d[valid].min(), th_d[valid].max()
        for i in valid[th_d[valid] <= lo + 1e-7]:
            t = theta_hp(x[i], y[i], z[i])
            if t < out["min_theta"]:
                out["min_theta"], (out["min_theta_dq"], out["min_theta_zr"]) = t, theta_of_double_quotient(x[i], y[i], z[i])
        for i in valid[th_d[valid] >= hi - 1e-7]:
            t = theta_hp(x[i], y[i], z[i])
            if t > out["max_theta"]:
                out["max_theta"], (out["max_theta_dq"], out["max_theta_zr"]) = t, theta_of_double_quotient(x[i], y[i], z[i])

    # phScattStats (:1385-1462) and averagePhotonEnergy (:1358-1383): the switch's filter
    keep = weighted if cs_switch else np.ones(n, dtype=bool)
    k = np.flatnonzero(keep)
    count = len(k)
    out["count"] = count
    out["max_scatt"] = int(np.fmax.reduce(ns[k], initial=0.0))
    out["min_scatt"] = int(np.fmin.reduce(ns[k], initial=float(INT_MAX)))
    sum_scatt, ieee = _sum_or_ieee(lambda: _exact_sum(*_mant_exp(ns[k])), ns[k])
    out["sum_scatt"] = sum_scatt
    out["avg_scatt"] = _ratio(sum_scatt, count) if ieee is None else (ieee / count if count else float("nan"))
    sum_r, ieee = _sum_or_ieee(lambda: _exact_sum(*_mant_exp(r_cr[k])), r_cr[k])
    out["sum_r"] = sum_r
    out["avg_r"] = _ratio(sum_r, count) if ieee is None else (ieee / count if count else float("nan"))

    def e_exact():
        (mp_, ep), (mw, ew) = _mant_exp(p0[k]), _mant_exp(w[k])
        return _exact_sum(mp_ * mw, ep + ew)
    with np.errstate(all="ignore"):
        e_terms = p0[k] * w[k]
    e_sum, e_ieee = _sum_or_ieee(e_exact, e_terms)
    w_sum, w_ieee = _sum_or_ieee(lambda: _exact_sum(*_mant_exp(w[k])), w[k])
    out["e_sum"], out["w_sum"] = e_sum, w_sum
    if e_ieee is None and w_ieee is None:
        out["avg_energy"] = _ratio(e_sum * Fraction(C_LIGHT), w_sum)
    else:
        num = float(e_sum) if e_ieee is None else e_ieee
        den = float(w_sum) if w_ieee is None else w_ieee
        with np.errstate(all="ignore"):
            out["avg_energy"] = float(np.float64(num * C_LIGHT) / np.float64(den))
    return out


# ---------------------------------------------------------------------------------------------- error bars, derived
def additions_context(n):
    """additions on the longest path of the context form (reduce_kernel and the host's combine) for a list of n slots: a thread's trips of the
    grid-stride loop, six shuffle levels, two additions of the four wavefronts' sums in LDS, and the host's blocks - 1"""
    blocks = min(512, max(1, (n + 255) // 256))
    trips = -(-n // (blocks * 256))
    return trips + 6 + 2 + (blocks - 1)


def additions_pool(n):
    """the same for the pool form (rank_reduce_kernel, one workgroup per list): ceil(n / 256) per thread, six shuffle levels, two in LDS"""
    return -(-n // 256) + 6 + 2


def bars(m):
    """relative bars against the checker's once-rounded values for m additions on the longest path (all four sums are of non-negative terms, so
    a sum's relative error is at most gamma_m on top of its terms'):
      avg_scatt   terms exact; the division and the checker's own rounding:                                    gamma(m + 2)
      avg_r       a term is sqrt of three rounded squares and two rounded sums, (1 + d)^(5/2) and the sqrt's rounding, against the
                  correctly rounded r, one more: four roundings at most; then as avg_scatt:                     gamma(m + 6)
      avg_energy  numerator: one product per term, m additions, the product with C_LIGHT; denominator: m additions; the division and the
                  checker's rounding:                                                                           gamma(2 m + 4)"""
    return dict(avg_scatt=gamma(m + 2), avg_r=gamma(m + 6), avg_energy=gamma(2 * m + 4))


# ---------------------------------------------------------------------------------------------- input families
SPECIALS = ("r_min", "r_max", "theta_min", "theta_max", "scatt_min", "scatt_max")
N_ROTATIONS = len(SPECIALS)


def set_null(rec, i):
    """slot i as setNullPhoton leaves it (Src/photons.c:208-236)"""
    rec[i] = np.zeros(1, dtype=rec.dtype)[0]
    rec["type"][i] = b"N"
    rec["nearest_block_index"][i] = -1


def generic_list(dtype, n, seed):
    """n photons: positions log-uniform in magnitude over 1e9 .. 1e13 per component with random signs, weights log-uniform over 1e40 .. 1e52,
    num_scatt 1 .. 9999, energies 1e-9 .. 1e-6; every seventh slot (i % 7 == 3) a null slot"""
    g = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=dtype)
    rec["type"] = b"i"
    for k in ("r0", "r1", "r2"):
        rec[k] = 10 ** g.uniform(9, 13, n) * g.choice([-1.0, 1.0], n)
    rec["weight"] = 10 ** g.uniform(40, 52, n)
    rec["num_scatt"] = g.integers(1, 10000, n)
    rec["p0"] = 10 ** g.uniform(-9, -6, n)
    rec["p3"] = rec["p0"]
    rec["comv_p0"] = rec["p0"]
    rec["s0"] = 1.0
    for i in range(3, n, 7):
        set_null(rec, i)
    return rec


def special_slots(n, rotation):
    """{special: slot}: where the six extremes go in a list of n slots.  The classes of slots: the last slot; a lane of the last wavefront (the
    partial one when n % 64 != 0); wavefront 3 of a workgroup (slot % 256 >= 192); beyond one trip of the context form's grid (slot >= 131072).
    In a list longer than one trip every class is taken from the slots >= 131072.  SPECIALS[rotation] gets the last slot, the others go round
    the remaining classes (a class with no free slot hands over to the next), so over the six rotations every extreme sits in every class."""
    if n < 2:
        return {}
    floor = RED_SLOTS if n > RED_SLOTS else 0
    last_wave = range(max(floor, 64 * ((n - 1) // 64)), n - 1)
    wave3 = [i for b in range((n - 1) // 256, -1, -1) for i in range(256 * b + 192, min(256 * b + 256, n - 1)) if i >= floor][:8]
    classes = [[n - 1], list(last_wave)[-8:], wave3]
    if floor:
        classes.append(list(range(floor + 5, min(floor + 13, n - 1))))
    classes = [c for c in classes if c]
    rest = list(range(floor, n - 1))[-16:]              # when those classes are full (n = 65: they are the last slot alone): the slots before it
    used, out = set(), {}
    for k in range(len(SPECIALS)):
        name = SPECIALS[(rotation + k) % len(SPECIALS)]
        for step in range(len(classes) + 1):
            free = [i for i in (classes[(k + step) % len(classes)] if step < len(classes) else rest) if i not in used]
            if free:
                out[name] = free[-1]
                used.add(free[-1])
                break
    return out


def place_specials(rec, slots):
    """the six extremes, every one a weighted photon: r_min (1e9, 0, 0) below every generic r >= sqrt(3) 1e9, r_max (1e13, -1e13, 1e13) above
    every generic r < sqrt(3) 1e13, theta_min on +z (theta = 0), theta_max on -z (theta = pi), num_scatt 0 and 10000"""
    pos = dict(r_min=(1e9, 0.0, 0.0), r_max=(1e13, -1e13, 1e13), theta_min=(0.0, 0.0, 5e11), theta_max=(0.0, 0.0, -5e11))
    for name, i in slots.items():
        if rec["weight"][i] == 0:                       # a null slot becomes a photon again, with no extreme of its own
            rec["type"][i], rec["nearest_block_index"][i] = b"i", 0
            rec["r0"][i], rec["r1"][i], rec["r2"][i] = 2e10, -3e11, 4e10 * (1 + i % 5)
            rec["weight"][i], rec["num_scatt"][i], rec["p0"][i], rec["p3"][i], rec["s0"][i] = 1e45, 5000, 1e-7, 1e-7, 1.0
        if name in pos:
            rec["r0"][i], rec["r1"][i], rec["r2"][i] = pos[name]
        elif name == "scatt_min":
            rec["num_scatt"][i] = 0
        else:
            rec["num_scatt"][i] = 10000
    return rec


def family(dtype, n, rotation, seed=20261019):
    """the list of n slots of the reduction tests with its extremes placed by special_slots(n, rotation) -> (records, {special: slot})"""
    rec = generic_list(dtype, n, seed + n)
    if n == 1:
        return rec, {}
    slots = special_slots(n, rotation)
    return place_specials(rec, slots), slots


CONTEXT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, RED_SLOTS, RED_SLOTS + 65, 2 * RED_SLOTS + 1)
POOL_LENGTHS = (None, 1, 64, 255, 256, 257, 300)      # None: a list that is never created
POOL_SLOTS_PER_RANK = 300


def semantics_lists(dtype):
    """{name: records}: the small lists of the semantics cases"""
    out = {}
    a = generic_list(dtype, 40, 7)                      # null slots at 3, 10, 17, ...; every weighted photon has num_scatt >= 1
    out["null-slots"] = a
    b = generic_list(dtype, 9, 8)
    for i in range(len(b)):
        set_null(b, i)
    out["all-null"] = b
    c = generic_list(dtype, 12, 9)
    c["weight"][5] = 0.0                                # an absorbed photon whose energy is not finite
    c["p0"][5] = np.inf
    out["weightless-inf-p0"] = c
    d = generic_list(dtype, 12, 10)
    d["r0"][4] = d["r1"][4] = d["r2"][4] = 0.0          # a weighted photon at the origin: r = 0, theta = acos(0/0) = NaN
    assert d["weight"][4] != 0
    out["weighted-at-origin"] = d
    return out
