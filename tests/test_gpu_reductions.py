"""The per-frame reductions on the device -- reduce_kernel with the host's combine (mcrat_hip_ph_minmax, _scatt_stats, _avg_energy) and
rank_reduce_kernel (mcrat_hip_pool_summaries) -- against tests/reductions_checker.py, with CYCLOSYNCHROTRON_SWITCH off and on, on synthetic
lists at the sizes where a reduction goes wrong: shorter than a wavefront, ending inside a wavefront and inside a workgroup, longer than the
131072 slots one trip of the grid covers (the grid-stride loop, all 512 partials of the host's combine), with every extreme placed where a
dropped tail, a dropped second trip, a wrong wavefront combine or a wrong LDS combine loses it (reductions_checker.special_slots).

BARS
  sums       All four sums (num_scatt, r, p0 * weight, weight) are of non-negative terms, so the computed sum is within gamma_m = m u / (1 - m u)
             of the exact one, m the additions on the longest path, on top of the terms' own roundings.  Context form: a thread's trips
             ceil(n / (blocks * 256)), six shuffle levels, two additions for the four wavefronts in LDS, blocks - 1 on the host
             (reductions_checker.additions_context).  Pool form: ceil(len / 256) + 6 + 2 (additions_pool).  Terms: r is the root of three
             rounded squares and two rounded sums and is compared with the correctly rounded r (four roundings), p0 * weight is one product;
             then the division by the count (and, for the energy, the product with C_LIGHT) and the checker's own single rounding:
             avg_scatt gamma(m + 2), avg_r gamma(m + 6), avg_energy gamma(2 m + 4) (reductions_checker.bars).
  exact      max_scatt, min_scatt, num_output and list_capacity are integers.  r_min and r_max are equal to the bit to the checker's double
             evaluation of sqrt(x*x + y*y + z*z): the library is built with -ffp-contract=off, so the device does not contract the sum of
             squares into FMAs, and its double sqrt is correctly rounded.
  theta      The device's acos cannot be bounded from its source here, so it is MEASURED: against acos at 200 bits of the very double z / r the
             device hands to its acos (r is equal to the bit, the division is correctly rounded), on every list of this file, the worst
             relative difference seen was ACOS_SEEN; the bar ACOS_BAR is twice that and below the 1e-12 of tests/test_gpu_parity.py.  Against
             the checker's theta of the exact z / r the bar is that plus what the rounding of z / r can move theta by
             (reductions_checker.theta_of_double_quotient: 4 u on z / r, through acos; nothing on the axis).  theta = 0 must come out as 0.
No case is skipped and nothing is masked out of a comparison."""
import math

import numpy as np
import pytest

from mcrat_amd import synth
from tests import reductions_checker as K

pytestmark = pytest.mark.gpu

# measured on an MI355X: all 542 theta comparisons of this file (0 and pi on the axes, and the generic angles of the one-photon list, the
# semantics lists and the emission frame) against mpmath's acos at 200 bits of the same double argument, rounded once: every one equal to the
# bit.  Twice the worst seen is therefore 0: the device's acos has to return the correctly rounded value on these inputs.
ACOS_SEEN = 0.0
ACOS_BAR = 2 * ACOS_SEEN
assert ACOS_BAR <= 1e-12


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _say(line):
    print(line)                                         # every figure is printed before it is asserted on


def _rel(got, want):
    if want != want or got != got:
        return 0.0 if (want != want and got != got) else math.inf
    if want == got:
        return 0.0
    return abs(got - want) / abs(want) if want != 0 and math.isfinite(want) else math.inf


def _check(label, got, want, m):
    """got: dict with the checker's keys, from the device; want: reductions_checker.reductions; m: additions on the longest path.  Every
    figure is printed, every member is compared, and the members that miss are reported together."""
    bar, bad = K.bars(m), []
    for k in ("max_scatt", "min_scatt", "min_r", "max_r", "num_output", "list_capacity"):
        if k in got:
            _say("%s %s got %r want %r" % (label, k, got[k], want[k]))
            if not got[k] == want[k]:
                bad.append((k, got[k], want[k]))
    for k in ("min_theta", "max_theta"):
        e_acos = _rel(got[k], want[k + "_dq"])
        allow = want[k + "_zr"] + ACOS_BAR * abs(want[k])
        _say("%s %s got %r want %r: vs acos of the double z/r %.3e (bar %.3e); vs exact %.3e abs (bar %.3e)" %
             (label, k, got[k], want[k], e_acos, ACOS_BAR, abs(got[k] - want[k]), allow))
        if want[k] == 0.0 or want[k] == K.DBL_MAX:
            if not got[k] == want[k]:
                bad.append((k, got[k], want[k]))
        elif not (e_acos <= ACOS_BAR and abs(got[k] - want[k]) <= allow):
            bad.append((k, got[k], want[k + "_dq"], e_acos, want[k], allow))
    for k in ("avg_scatt", "avg_r", "avg_energy"):
        e = _rel(got[k], want[k])
        _say("%s %s got %r want %r: rel %.3e (bar %.3e, m = %d)" % (label, k, got[k], want[k], e, bar[k], m))
        if not e <= bar[k]:
            bad.append((k, got[k], want[k], "rel %.3e > bar %.3e" % (e, bar[k])))
    assert not bad, (label, bad)


def _context_values(e):
    mm, ss = e.ph_minmax(), e.scatt_stats()
    return dict(min_r=mm[0], max_r=mm[1], min_theta=mm[2], max_theta=mm[3], max_scatt=ss[0], min_scatt=ss[1], avg_scatt=ss[2], avg_r=ss[3],
                avg_energy=e.avg_energy())


def _summary_values(s):
    return {k: getattr(s, k) for k in ("min_r", "max_r", "min_theta", "max_theta", "max_scatt", "min_scatt", "avg_scatt", "avg_r", "avg_energy",
                                       "num_output", "list_capacity")}


_WANT = {}


def _family(hip, n, rot):
    """(records, {cs_switch: checker's values}) of reductions_checker.family(n, rot), computed once; the big lists share their generic
    photons' correctly rounded r between the rotations"""
    key = (n, rot)
    if key not in _WANT:
        rec, slots = K.family(hip.PHOTON_DTYPE, n, rot)
        if ("r", n) not in _WANT:
            base = K.generic_list(hip.PHOTON_DTYPE, n, 20261019 + n)
            _WANT[("r", n)] = K.sqrt_cr(base["r0"], base["r1"], base["r2"])
        r_cr = _WANT[("r", n)].copy()
        idx = np.array(sorted(slots.values()), dtype=int)
        if len(idx):
            r_cr[idx] = K.sqrt_cr(rec["r0"][idx], rec["r1"][idx], rec["r2"][idx])
        _WANT[key] = (rec, {cs: K.reductions(rec, cs, r_cr) for cs in (0, 1)})
    return _WANT[key]


def _rotations(n):
    """every rotation where it is cheap; two where a list is tens of megabytes -- in a list longer than one trip every placed extreme sits at a
    slot >= 131072 under any rotation"""
    return range(K.N_ROTATIONS) if n <= 1000 else (0, 3)


# ---------------------------------------------------------------------------------------------- context form
@pytest.mark.parametrize("cs", [0, 1], ids=["off", "on"])
@pytest.mark.parametrize("n", K.CONTEXT_SIZES)
def test_context_form(hip, n, cs):
    """reduce_kernel and the host's combine over min(512, ceil(n / 256)) partials"""
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, 0, cyclosynchrotron=cs)
    for rot in _rotations(n):
        rec, want = _family(hip, n, rot)
        e.set_photons_aos(rec)
        _check("context n=%d cs=%d rot=%d" % (n, cs, rot), _context_values(e), want[cs], K.additions_context(n))
        if n > 1:                                       # the placed extremes are the answers, wherever they were put
            w = want[cs]
            assert (w["min_r"], w["max_r"], w["min_theta"], w["max_theta"], w["max_scatt"]) == (1e9, math.sqrt(3e26), 0.0, math.pi, 10000)
            assert w["min_scatt"] == 0
    e.close()


# ---------------------------------------------------------------------------------------------- pool form
@pytest.mark.parametrize("cs", [0, 1], ids=["off", "on"])
def test_pool_form(hip, cs):
    """rank_reduce_kernel, one workgroup per list, lists of every length around a wavefront and a workgroup in windows of 300 slots (the pool
    rounds them up): every member of mcrat_hip_rank_summary against the checker on that list alone, and every view's three entry points against
    the same values.  Each window held a full-length list of large values first, so a kernel that reads past a list's length finds slots that
    were in use (setting the shorter list clears them: such a kernel then counts empty slots)."""
    frame, _, cfg = synth.config1(n_photons=16, n0=8, n1=8)
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 0, cyclosynchrotron=cs)
    pool.set_hydro(frame)
    R = len(K.POOL_LENGTHS)
    pool.pool_create(R, K.POOL_SLOTS_PER_RANK)
    long_list = K.generic_list(hip.PHOTON_DTYPE, K.POOL_SLOTS_PER_RANK, 99)
    long_list["num_scatt"] += 20000
    for k in ("r0", "r1", "r2"):
        long_list[k] *= 1e3
    for rot in range(K.N_ROTATIONS):
        for r, length in enumerate(K.POOL_LENGTHS):
            if length is None:
                continue                                # this list is never created
            v = pool.pool_rank(r, r)
            v.set_photons_aos(long_list)
            v.set_photons_aos(_family(hip, length, rot)[0])
        summ = pool.pool_summaries()
        for r, length in enumerate(K.POOL_LENGTHS):
            s = _summary_values(summ[r])
            if length is None:
                assert all(v == 0 for v in s.values()), s
                continue
            rec, want = _family(hip, length, rot)
            _check("pool len=%d cs=%d rot=%d" % (length, cs, rot), s, want[cs], K.additions_pool(length))
            _check("view len=%d cs=%d rot=%d" % (length, cs, rot), _context_values(pool.pool_rank(r, r)), want[cs], K.additions_context(length))
    pool.close()


# ---------------------------------------------------------------------------------------------- semantics
def _both_forms(hip, rec, cs):
    """the list in a context of its own and as the one list of a pool -> (context's values, summary's values)"""
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, 0, cyclosynchrotron=cs)
    e.set_photons_aos(rec)
    a = _context_values(e)
    e.close()
    frame, _, cfg = synth.config1(n_photons=16, n0=8, n1=8)
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 0, cyclosynchrotron=cs)
    pool.set_hydro(frame)
    pool.pool_create(1, K.POOL_SLOTS_PER_RANK)
    pool.pool_rank(0, 0).set_photons_aos(rec)
    b = _summary_values(pool.pool_summaries()[0])
    pool.close()
    return a, b


@pytest.mark.parametrize("cs", [0, 1], ids=["off", "on"])
@pytest.mark.parametrize("name", ["null-slots", "all-null", "weightless-inf-p0", "weighted-at-origin"])
def test_semantics(hip, name, cs):
    """switch on: min_scatt, avg_scatt, avg_r and the energy are over the weighted photons only (mclib.c:1373-1375, :1401-1403), off: over all
    slots; phMinMax is over the weighted photons under both"""
    rec = K.semantics_lists(hip.PHOTON_DTYPE)[name]
    want = K.reductions(rec, cs)
    for form, got in zip(("context", "pool"), _both_forms(hip, rec, cs)):
        _check("%s %s cs=%d" % (name, form, cs), got, want, K.additions_context(len(rec)) if form == "context" else K.additions_pool(len(rec)))
        if name == "null-slots":
            assert want["num_output"] == 34
            if cs:
                assert got["min_scatt"] >= 1 and want["count"] == 34
            else:
                assert got["min_scatt"] == 0 and want["count"] == 40
        elif name == "all-null":
            assert (got["min_r"], got["max_r"], got["min_theta"], got["max_theta"]) == (K.DBL_MAX, 0.0, K.DBL_MAX, 0.0)
            assert got["avg_energy"] != got["avg_energy"]
            if cs:
                assert (got["max_scatt"], got["min_scatt"]) == (0, K.INT_MAX) and got["avg_scatt"] != got["avg_scatt"] and got["avg_r"] != got["avg_r"]
            else:
                assert (got["max_scatt"], got["min_scatt"], got["avg_scatt"], got["avg_r"]) == (0, 0, 0.0, 0.0)
        elif name == "weightless-inf-p0":
            assert math.isfinite(got["avg_energy"]) if cs else got["avg_energy"] != got["avg_energy"]
        else:
            assert got["min_r"] == 0.0 and 0.0 < got["min_theta"] <= got["max_theta"] < math.pi     # r = 0 counts, its NaN theta wins nothing


def test_after_a_real_cyclosynchrotron_emission(hip, oracle):
    """the `null-slots` list of tests/test_gpu_cyclosynch.py: 600 slots, every other one a null slot, into which mcrat_hip_emit_cyclosynch_pool
    puts its pool photons; the rest stay null.  The reductions of the switch-on context, and of a switch-on pool holding the list read back,
    against the checker on the photons read back."""
    from tests.test_gpu_cyclosynch import _oracle_pool
    frame, ph, cfg = synth.config2(n_photons=600, nzc=8, stokes=1, lumi=1e53)
    dens = np.ascontiguousarray(frame["dens"])
    aos = synth.photons_to_aos(ph, hip.PHOTON_DTYPE)
    _, _, _, before, _ = _oracle_pool(oracle, frame, cfg, aos, range(1, 600, 2), dens, 1, 77, 1500)
    e = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], cyclosynchrotron=1)
    e.set_hydro(frame)
    e.set_hydro_extras(dens)
    e.set_photons_aos(before.astype(hip.PHOTON_DTYPE))
    n, _, bad = e.emit_cyclosynch_pool(1e12, 1e40, 1500, 0.0, 0.05, frame["fps"], 77, b_field_calc=1, scatt_frame_number=200, inj_frame_number=200)
    got = e.get_photons_aos()
    nulls = int(np.count_nonzero(got["weight"] == 0))
    assert bad == 0 and n >= 1 and nulls == 300 - n > 0 and len(got) == 600
    want = K.reductions(got, 1)
    assert want["count"] == 300 + n
    _check("cs-emission context", _context_values(e), want, K.additions_context(len(got)))
    e.close()
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], cyclosynchrotron=1)
    pool.set_hydro(frame)
    pool.pool_create(2, 600)
    v = pool.pool_rank(1, 5)
    v.set_photons_aos(got)
    summ = pool.pool_summaries()
    assert summ[0].list_capacity == 0
    _check("cs-emission pool", _summary_values(summ[1]), want, K.additions_pool(len(got)))
    _check("cs-emission view", _context_values(v), want, K.additions_context(len(got)))
    pool.close()
