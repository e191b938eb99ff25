"""tests/reductions_checker.py against hand-worked lists and against the oracle's restatement of phMinMax, phScattStats and averagePhotonEnergy
(oracle/mcrat_oracle.c) under both settings of CYCLOSYNCHROTRON_SWITCH, on every input family of tests/test_gpu_reductions.py.  No GPU.

The oracle adds up in slot order in doubles, so against the checker's exact sums its averages are held to reductions_checker.bars(n): n
additions on the one path there is.  min_r, max_r and the scattering extremes are equal to the bit (the oracle is built without contraction);
theta is the C library's acos of the double z / r, held to the 1e-12 relative of tests/test_gpu_parity.py, and to 0 exactly on the +z axis."""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

from tests import reductions_checker as K


def _oracle(oracle, rec, cs_switch):
    L = oracle.lib()
    P = oracle.OraclePhotons(rec)
    a, b, c_, d = (C.c_double() for _ in range(4))
    L.orc_phMinMax(C.byref(P.c), C.byref(a), C.byref(b), C.byref(c_), C.byref(d))
    mx, mn, avg, ravg = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    L.orc_phScattStats_cs(C.byref(P.c), int(cs_switch), C.byref(mx), C.byref(mn), C.byref(avg), C.byref(ravg))
    out = dict(min_r=a.value, max_r=b.value, min_theta=c_.value, max_theta=d.value, max_scatt=mx.value, min_scatt=mn.value, avg_scatt=avg.value,
               avg_r=ravg.value, avg_energy=L.orc_averagePhotonEnergy_cs(C.byref(P.c), int(cs_switch)))
    if not cs_switch:                                   # the entry points without the argument are the switch-off ones, unchanged
        L.orc_phScattStats(C.byref(P.c), C.byref(mx), C.byref(mn), C.byref(avg), C.byref(ravg))
        same = lambda p, q: p == q or (p != p and q != q)
        assert (mx.value, mn.value) == (out["max_scatt"], out["min_scatt"]) and same(avg.value, out["avg_scatt"]) and same(ravg.value, out["avg_r"])
        assert same(L.orc_averagePhotonEnergy(C.byref(P.c)), out["avg_energy"])
    return out


def _close(got, want, rel):
    if want != want:
        return got != got
    if math.isinf(want) or want == 0:
        return got == want
    return abs(got - want) <= rel * abs(want)


def _agree(oracle, rec, cs_switch, r_cr=None):
    want, got = K.reductions(rec, cs_switch, r_cr), _oracle(oracle, rec, cs_switch)
    bar = K.bars(max(len(rec), 1))
    for k in ("min_r", "max_r", "max_scatt", "min_scatt"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("min_theta", "max_theta"):
        assert _close(got[k], want[k], 1e-12), (k, got[k], want[k])
        if want[k] not in (0.0, K.DBL_MAX):             # the C library's acos of the same double z / r: an ulp; then the rounding of z / r
            assert _close(got[k], want[k + "_dq"], 2 * K.U), (k, got[k], want[k + "_dq"])
            assert abs(got[k] - want[k]) <= want[k + "_zr"] + 2 * K.U * want[k], (k, got[k], want[k], want[k + "_zr"])
    for k in ("avg_scatt", "avg_r", "avg_energy"):
        assert _close(got[k], want[k], bar[k]), (k, got[k], want[k], bar[k])
    # the double r of the extremes is the correctly rounded one to two roundings and a half: sqrt of (1 + d)^3, and the sqrt's own
    for k in ("min_r", "max_r"):
        assert _close(want[k], want[k + "_cr"], 4 * K.U), (k, want[k], want[k + "_cr"])
    return want


def _list(oracle, rows):
    """rows of (x, y, z, weight, num_scatt, p0)"""
    rec = np.zeros(len(rows), dtype=oracle.PHOTON_DTYPE)
    rec["type"] = b"i"
    for i, (x, y, z, w, ns, p0) in enumerate(rows):
        rec["r0"][i], rec["r1"][i], rec["r2"][i], rec["weight"][i], rec["num_scatt"][i], rec["p0"][i] = x, y, z, w, ns, p0
    return rec


def test_three_photons_one_of_them_absorbed(oracle):
    """(3, 4, 0)e10 with weight 2, 4 scatterings, p0 = 1: r = 5e10 exactly, theta = pi/2;  (0, 0, 2e10) absorbed (weight 0), 0 scatterings,
    p0 = 5: r = 2e10, theta = 0;  (0, 0, -1e10) with weight 6, 10 scatterings, p0 = 3: r = 1e10, theta = pi"""
    rec = _list(oracle, [(3e10, 4e10, 0, 2, 4, 1.0), (0, 0, 2e10, 0, 0, 5.0), (0, 0, -1e10, 6, 10, 3.0)])
    for cs in (0, 1):
        got = _agree(oracle, rec, cs)
        assert (got["min_r"], got["max_r"], got["min_theta"], got["max_theta"]) == (1e10, 5e10, math.pi / 2, math.pi)   # the absorbed one is not looked at
        assert (got["num_output"], got["list_capacity"]) == (2, 3)
        assert got["avg_energy"] == 2.5 * K.C_LIGHT                               # (1*2 + 5*0 + 3*6) c / (2 + 0 + 6)
    off, on = K.reductions(rec, 0), K.reductions(rec, 1)
    assert (off["max_scatt"], off["min_scatt"], off["avg_scatt"], off["avg_r"], off["count"]) == (10, 0, 14 / 3, 8e10 / 3, 3)
    assert (on["max_scatt"], on["min_scatt"], on["avg_scatt"], on["avg_r"], on["count"]) == (10, 4, 7.0, 3e10, 2)


def test_four_null_slots(oracle):
    rec = _list(oracle, [(0, 0, 0, 0, 0, 0)] * 4)
    for i in range(4):
        K.set_null(rec, i)
    off, on = _agree(oracle, rec, 0), _agree(oracle, rec, 1)
    for got in (off, on):
        assert (got["min_r"], got["max_r"], got["min_theta"], got["max_theta"]) == (K.DBL_MAX, 0.0, K.DBL_MAX, 0.0)
        assert got["avg_energy"] != got["avg_energy"] and got["num_output"] == 0
    assert (off["max_scatt"], off["min_scatt"], off["avg_scatt"], off["avg_r"]) == (0, 0, 0.0, 0.0)
    assert (on["max_scatt"], on["min_scatt"]) == (0, K.INT_MAX) and on["avg_scatt"] != on["avg_scatt"] and on["avg_r"] != on["avg_r"]


def test_three_photons_one_at_the_origin_one_weightless_with_infinite_energy(oracle):
    """a weighted photon at the origin has r = 0 (it is r_min) and theta = acos(0/0) = NaN, which wins no comparison; a weightless slot with
    p0 = inf adds inf * 0 = NaN to the energy with the switch off and is passed over with it on"""
    rec = _list(oracle, [(0, 0, 0, 1, 2, 1.0), (1e10, 0, 0, 1, 3, 2.0), (0, 0, 1e10, 0, 7, np.inf)])
    off, on = _agree(oracle, rec, 0), _agree(oracle, rec, 1)
    for got in (off, on):
        assert (got["min_r"], got["max_r"], got["min_theta"], got["max_theta"]) == (0.0, 1e10, math.pi / 2, math.pi / 2)
    assert off["avg_energy"] != off["avg_energy"] and (off["max_scatt"], off["min_scatt"], off["avg_scatt"]) == (7, 2, 4.0)
    assert on["avg_energy"] == 1.5 * K.C_LIGHT and (on["max_scatt"], on["min_scatt"], on["avg_scatt"], on["avg_r"]) == (3, 2, 2.5, 5e9)


def test_the_integer_square_root_is_mpmaths_at_200_bits(oracle):
    rec = K.generic_list(oracle.PHOTON_DTYPE, 3000, 5)
    x, y, z = rec["r0"].copy(), rec["r1"].copy(), rec["r2"].copy()
    x[:4], y[:4], z[:4] = [3e10, 1.0, 0.0, 2.0 ** -600], [4e10, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]        # exact roots, sqrt(3), 0, a tiny one
    got = K.sqrt_cr(x, y, z)
    assert got[0] == 5e10 and got[2] == 0.0 and got[3] == 2.0 ** -600
    with mp.workprec(200):
        for i in range(len(x)):
            X, Y, Z = mp.mpf(float(x[i])), mp.mpf(float(y[i])), mp.mpf(float(z[i]))
            assert got[i] == float(mp.sqrt(X * X + Y * Y + Z * Z)), i


def _classes(n):
    floor = K.RED_SLOTS if n > K.RED_SLOTS else 0
    return dict(last=lambda i: i == n - 1, last_wave=lambda i: i >= 64 * ((n - 1) // 64), wave3=lambda i: i % 256 >= 192, second_trip=lambda i: i >= K.RED_SLOTS), floor


def test_every_extreme_sits_in_every_class_of_slots():
    """over the six rotations: in the last slot, in a lane of the last (partial) wavefront, in wavefront 3 of a workgroup and -- the two
    largest sizes, where every placed extreme is one -- in a slot the grid reaches only on its second or third trip"""
    for n in K.CONTEXT_SIZES + tuple(m for m in K.POOL_LENGTHS if m):
        if n < 2:
            continue
        cls, floor = _classes(n)
        seen = {name: set() for name in K.SPECIALS}
        for rot in range(K.N_ROTATIONS):
            slots = K.special_slots(n, rot)
            assert len(set(slots.values())) == len(slots) == min(len(K.SPECIALS), n) and all(floor <= i < n for i in slots.values())
            assert slots[K.SPECIALS[rot]] == n - 1
            for name, i in slots.items():
                seen[name] |= {c for c, f in cls.items() if f(i)}
        need = {"last", "last_wave"} | ({"wave3"} if n >= 255 and n != K.RED_SLOTS + 65 else set()) | ({"second_trip"} if floor else set())
        for name in K.SPECIALS:
            assert need <= seen[name], (n, name, seen[name])


@pytest.mark.parametrize("n", K.CONTEXT_SIZES)
def test_checker_equals_the_oracle_on_the_context_family(oracle, n):
    base = K.generic_list(oracle.PHOTON_DTYPE, n, 20261019 + n)
    r_base = K.sqrt_cr(base["r0"], base["r1"], base["r2"])
    for rot in (range(K.N_ROTATIONS) if n <= 1000 else (0, 3)):
        rec, slots = K.family(oracle.PHOTON_DTYPE, n, rot)
        r_cr = r_base.copy()
        idx = np.array(sorted(slots.values()), dtype=int)
        if len(idx):
            r_cr[idx] = K.sqrt_cr(rec["r0"][idx], rec["r1"][idx], rec["r2"][idx])
        for cs in (0, 1):
            got = _agree(oracle, rec, cs, r_cr)
            if n > 1:                                   # the placed extremes are the extremes
                assert got["min_r"] == 1e9 and got["max_r"] == math.sqrt(3e26) and (got["min_theta"], got["max_theta"]) == (0.0, math.pi)
                assert got["max_scatt"] == 10000 and got["min_scatt"] == 0
        if n > 1:
            on = K.reductions(rec, 1, r_cr)
            assert on["count"] == on["num_output"] < n or n < 4


@pytest.mark.parametrize("length", [m for m in K.POOL_LENGTHS if m])
def test_checker_equals_the_oracle_on_the_pool_family(oracle, length):
    for rot in range(K.N_ROTATIONS):
        rec, _ = K.family(oracle.PHOTON_DTYPE, length, rot)
        for cs in (0, 1):
            _agree(oracle, rec, cs)


def test_checker_equals_the_oracle_on_the_semantics_lists(oracle):
    lists = K.semantics_lists(oracle.PHOTON_DTYPE)
    for name, rec in lists.items():
        off, on = _agree(oracle, rec, 0), _agree(oracle, rec, 1)
        if name == "null-slots":
            assert off["min_scatt"] == 0 and on["min_scatt"] >= 1 and on["avg_scatt"] > off["avg_scatt"] and on["avg_r"] > off["avg_r"]
            assert on["count"] == on["num_output"] == 40 - 6 and off["count"] == 40
        elif name == "all-null":
            assert (on["max_scatt"], on["min_scatt"]) == (0, K.INT_MAX) and on["avg_r"] != on["avg_r"] and on["avg_energy"] != on["avg_energy"]
            assert (on["min_r"], on["max_r"], on["min_theta"], on["max_theta"]) == (K.DBL_MAX, 0.0, K.DBL_MAX, 0.0)
        elif name == "weightless-inf-p0":
            assert math.isfinite(on["avg_energy"]) and off["avg_energy"] != off["avg_energy"]
        else:
            assert on["min_r"] == 0.0 and 0 < on["min_theta"] <= on["max_theta"] < math.pi
