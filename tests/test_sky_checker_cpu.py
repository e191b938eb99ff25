"""tests/sky_checker.py against photons built by hand, whose acceptance, time bin and pixel are known in closed form -- so that the checker the GPU
test trusts is itself checked against something that is not a restatement of the same expressions."""
import math
from fractions import Fraction

import numpy as np

from tests import sky_checker as S

C = S.C_LIGHT
TIME_NOW = 1000.0
# observers whose vectors are exact in double: on the axis, and in the equatorial plane at phi = 90 degrees (theta_hat = -z, phi_hat = -x there)
ON_AXIS = (np.array([[0.0], [0.0], [1.0]]), np.array([[1.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]]))
PHI_90 = (np.array([[0.0], [1.0], [0.0]]), np.array([[0.0], [0.0], [-1.0]]), np.array([[-1.0], [0.0], [0.0]]))
T_EDGES = np.array([0.0, 850.0, 900.0, 950.0, 1000.0])              # t_det = 1000 - R / c
E_EDGES = np.array([1e-12, 1e-9, 1e-6])
X_EDGES = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, 3.0]) * 1e10         # 5 columns
Y_EDGES = np.array([-1.5, -0.5, 0.5, 1.5]) * 1e10                   # 3 rows


def placed(n, ex, ey, R, a, b, direction=None, p0=1e-18):
    """photons at r = R n + a ex + b ey moving along `direction` (default: n)"""
    R, a, b = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (R, a, b)))
    r = n * R + ex * a + ey * b
    d = np.broadcast_to(n if direction is None else direction, r.shape)
    p0 = np.broadcast_to(np.asarray(p0, dtype=np.float64), R.shape)
    return S.photon_list(r, np.stack([p0, p0 * d[0], p0 * d[1], p0 * d[2]]), 5)


def test_observer_vectors():
    n, cos_acc, ex, ey = S.observers([0.0, 0.3, 1.2, math.pi / 2], [0.0, 1.1, 4.0, math.pi / 2], [0.1, 0.2, 0.3, 0.4])
    assert np.allclose(np.cross(ex.T, ey.T).T, n, atol=1e-15)                               # ex x ey = n
    for a, b in ((n, n), (ex, ex), (ey, ey)):
        assert np.abs((a * b).sum(axis=0) - 1.0).max() < 1e-15
    for a, b in ((n, ex), (n, ey), (ex, ey)):
        assert np.abs((a * b).sum(axis=0)).max() < 1e-15
    assert np.array_equal(n[:, 0], [0.0, 0.0, 1.0]) and np.array_equal(ex[:, 0], [1.0, 0.0, 0.0]) and np.array_equal(ey[:, 0], [0.0, 1.0, 0.0])
    assert np.allclose(n[:, 3], PHI_90[0][:, 0], atol=1e-15) and np.allclose(ex[:, 3], PHI_90[1][:, 0], atol=1e-15) and np.allclose(ey[:, 3], PHI_90[2][:, 0], atol=1e-15)
    assert np.allclose(cos_acc, np.cos([0.1, 0.2, 0.3, 0.4]))
    from mcrat_amd import engine
    for got, want in zip(engine.sky_observers([0.0, 0.3, 1.2], [0.0, 1.1, 4.0], 0.2), S.observers([0.0, 0.3, 1.2], [0.0, 1.1, 4.0], 0.2)):
        assert np.allclose(got, want, rtol=0, atol=1e-15)


def test_exact_observers_put_a_photon_where_it_was_placed():
    """r = R n + a ex + b ey lands at X = a, Y = b, t_det = time_now - R / c: exactly, for vectors of zeros and ones"""
    R = C * np.array([120.0, 75.0, 20.0, 180.0])                   # t_det = 880, 925, 980, 820: time bins 1, 2, 3, 0 (C_LIGHT * small integers is exact)
    a = np.array([-1.5, 0.5, 2.5, 0.0]) * 1e10                     # columns 0, 2, 4, 2
    b = np.array([1.0, 0.0, -1.0, 0.0]) * 1e10                     # rows 2, 1, 0, 1
    for n, ex, ey in (ON_AXIS, PHI_90):
        ph = placed(n, ex, ey, R, a, b)
        q = S.per_photon(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, ex, ey, X_EDGES, Y_EDGES)
        assert q["accepted"].all() and q["inside"].all()
        assert np.array_equal(q["X"][0], a) and np.array_equal(q["Y"][0], b) and np.array_equal(q["t"][0], TIME_NOW - R / C)
        assert q["t"][0].tolist() == [880.0, 925.0, 980.0, 820.0]
        assert q["it"][0].tolist() == [1, 2, 3, 0] and q["ix"][0].tolist() == [0, 2, 4, 2] and q["iy"][0].tolist() == [2, 1, 0, 1]
        assert np.array_equal(q["e"][0], ph["p0"] * C) and q["ie"][0].tolist() == [1, 1, 1, 1]          # 1e-18 * c = 3e-8 erg
        want = S.observation(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, ex, ey, X_EDGES, Y_EDGES)
        assert want["count"].shape == (1, 4, 2, 3, 5) and want["count"].sum() == 4
        for it, iy, ix, k in ((1, 2, 0, 0), (2, 1, 2, 1), (3, 0, 4, 2), (0, 1, 2, 3)):
            assert want["count"][0, it, 1, iy, ix] == 1
            assert want["w"][0, it, 1, iy, ix] == ph["weight"][k] and want["q"][0, it, 1, iy, ix] == ph["weight"][k] * ph["s1"][k]
        assert want["n_accepted"].tolist() == [4] and want["n_outside"].tolist() == [0]
    # the observer at phi = 90 degrees sees the on-axis observer's photons edge on: other pixels, other times
    ph = placed(*ON_AXIS, R, a, b, direction=np.array([[0.0], [0.6], [0.8]]))
    q0 = S.per_photon(ph, ON_AXIS[0], [0.5], T_EDGES, E_EDGES, TIME_NOW, ON_AXIS[1], ON_AXIS[2], X_EDGES, Y_EDGES)
    q1 = S.per_photon(ph, PHI_90[0], [0.5], T_EDGES, E_EDGES, TIME_NOW, PHI_90[1], PHI_90[2], X_EDGES, Y_EDGES)
    assert q0["accepted"].all() and q1["accepted"].all()             # cosines 0.8 and 0.6 to the two observers
    assert np.array_equal(q1["X"][0], -R) and np.array_equal(q1["Y"][0], -a) and np.array_equal(q1["t"][0], TIME_NOW - b / C)


def test_general_observer_in_closed_form():
    """an observer off every axis: the placed photon is in the pixel and the time bin that hold (a, b, R) -- chosen away from the edges, so that the
    rounding of the rotation cannot matter -- and X, Y, t_det are a, b, time_now - R / c to a few units in the last place of |r|"""
    n, cos_acc, ex, ey = S.observers([0.3, 0.3], [1.1, 1.1 + math.pi / 2], 0.2)
    g = np.random.default_rng(3)
    m = 400
    it, ix, iy = g.integers(0, 4, m), g.integers(0, 5, m), g.integers(0, 3, m)
    frac = lambda: g.uniform(0.1, 0.9, m)
    t = T_EDGES[it] + frac() * (T_EDGES[it + 1] - T_EDGES[it])
    a = X_EDGES[ix] + frac() * 1e10
    b = Y_EDGES[iy] + frac() * 1e10
    R = (TIME_NOW - t) * C
    for o in (0, 1):
        no, xo, yo = n[:, o:o + 1], ex[:, o:o + 1], ey[:, o:o + 1]
        ph = placed(no, xo, yo, R, a, b)
        q = S.per_photon(ph, no, cos_acc[o:o + 1], T_EDGES, E_EDGES, TIME_NOW, xo, yo, X_EDGES, Y_EDGES)
        assert q["accepted"].all()
        assert np.array_equal(q["it"][0], it) and np.array_equal(q["ix"][0], ix) and np.array_equal(q["iy"][0], iy)
        scale = np.abs(R) + np.abs(a) + np.abs(b)
        assert (np.abs(q["X"][0] - a) <= 16 * S.U * scale).all() and (np.abs(q["Y"][0] - b) <= 16 * S.U * scale).all()
        assert (np.abs(q["t"][0] - t) <= 16 * S.U * (scale / C + TIME_NOW)).all()
        want = S.observation(ph, no, cos_acc[o:o + 1], T_EDGES, E_EDGES, TIME_NOW, xo, yo, X_EDGES, Y_EDGES)
        ref = np.zeros((4, 3, 5), dtype=np.int64)
        np.add.at(ref, (it, iy, ix), 1)
        assert np.array_equal(want["count"][0, :, 1], ref) and want["count"][0, :, 0].sum() == 0
        assert np.array_equal(want["bin"][0], ((it * 2 + 1) * 3 + iy) * 5 + ix)
    # the second observer does not see the first one's photons where they were placed: the azimuth matters
    ph = placed(n[:, :1], ex[:, :1], ey[:, :1], R, a, b)
    q = S.per_photon(ph, n[:, 1:], [-1.0], T_EDGES, E_EDGES, TIME_NOW, ex[:, 1:], ey[:, 1:], X_EDGES, Y_EDGES)
    late = R * (1.0 - float(n[:, 0] @ n[:, 1])) / C                 # n.n' = cos^2 theta: the photon is R sin^2 theta further from the second observer
    assert (np.abs((q["t"][0] - t) - late) < 2.0).all() and (late > 2.0).mean() > 0.8 and (q["ix"][0] != ix).mean() > 0.5


def test_acceptance_is_a_cone_about_the_direction():
    n, cos_acc, ex, ey = S.observers([0.4, 0.4, 0.4], [0.0, 0.5, math.pi], [0.3, 0.3, 0.3])      # the first two cones overlap, the third is across the axis
    g = np.random.default_rng(9)
    m = 3000
    th, phi = g.uniform(0.0, 0.9, m), g.uniform(-math.pi, math.pi, m)
    d = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)])
    ph = placed(d, d, d, np.full(m, 100.0 * C), 0.0, 0.0, direction=d)
    q = S.per_photon(ph, n, cos_acc, T_EDGES, E_EDGES, TIME_NOW)
    angle = np.arccos(np.clip(n.T @ d, -1.0, 1.0))
    clear = np.abs(angle - 0.3) > 1e-9
    assert np.array_equal(q["accepted"][clear], (angle < 0.3)[clear])
    acc = q["accepted"]
    assert (acc[0] & acc[1]).sum() > 20 and (acc[0] & acc[2]).sum() == 0 and acc[2].sum() > 20
    want = S.observation(ph, n, cos_acc, T_EDGES, E_EDGES, TIME_NOW)
    assert want["count"].shape == (3, 4, 2) and want["n_accepted"].tolist() == acc.sum(axis=1).tolist()
    assert want["n_accepted"].sum() == acc.any(axis=0).sum() + (acc[0] & acc[1]).sum()       # the photons in the overlap count twice
    # a ring observer would put all three at one polar angle into one light curve; here the photons of the far side are the third observer's alone
    assert (acc[2] & (np.abs(phi) < 2.0)).sum() == 0


def test_ties_and_non_numbers():
    n, ex, ey = ON_AXIS
    a = np.array([X_EDGES[2], X_EDGES[5], np.nextafter(X_EDGES[5], 0.0), X_EDGES[0], np.nextafter(X_EDGES[0], -1e300), 0.0, 0.0])
    b = np.array([0.0, 0.0, 0.0, 0.0, 0.0, Y_EDGES[1], Y_EDGES[3]])
    ph = placed(n, ex, ey, 100.0 * C, a, b)
    q = S.per_photon(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, ex, ey, X_EDGES, Y_EDGES)
    assert q["ix"][0].tolist() == [2, -1, 4, 0, -1, 2, 2]            # on an edge: the bin it opens; on the last edge: outside
    assert q["iy"][0].tolist() == [1, 1, 1, 1, 1, 1, -1]
    assert q["it"][0].tolist() == [2] * 7                            # t_det == 900 == T_EDGES[2]: the bin that edge opens
    assert q["inside"][0].tolist() == [True, False, True, True, False, True, False]
    # acceptance at equality: p3 = 0.5 * p0 with p0 a power of two, cos_acc = 0.5
    p0 = 2.0 ** -60
    s = math.sqrt(0.75)
    ph = placed(n, ex, ey, 100.0 * C, [0.0, 0.0], [0.0, 0.0], p0=p0)
    ph["p1"][:] = p0 * s
    ph["p2"][:] = 0.0
    ph["p3"][:] = [0.5 * p0, np.nextafter(0.5 * p0, 0.0)]
    q = S.per_photon(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW)
    assert q["accepted"][0].tolist() == [True, False]
    # a NaN and an infinite position: accepted (the direction decides), in no bin
    ph = placed(n, ex, ey, 100.0 * C, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    ph["r0"][0] = np.nan
    ph["r1"][1] = np.inf
    for image in (True, False):
        kw = dict(ex=ex, ey=ey, x_edges=X_EDGES, y_edges=Y_EDGES) if image else {}
        want = S.observation(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, **kw)
        assert want["n_accepted"].tolist() == [3] and want["n_outside"].tolist() == [2] and want["count"].sum() == 1, image


def test_bystanders_and_stokes_off():
    n, ex, ey = ON_AXIS
    ph = placed(n, ex, ey, 100.0 * C, np.zeros(6), np.zeros(6))
    ph["weight"][1] = 0.0
    ph["type"][2] = b"p"
    ph["type"][3] = b"N"
    ph["type"][4] = b"c"
    want = S.observation(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, ex, ey, X_EDGES, Y_EDGES)
    assert want["n_accepted"].tolist() == [3] and want["count"][0, 2, 1, 1, 2] == 3 and want["count"].sum() == 3
    assert want["bin"][0].tolist()[1:4] == [-1, -1, -1]
    off = S.observation(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, ex, ey, X_EDGES, Y_EDGES, stokes=False)
    for k in ("i", "q", "u", "v"):
        assert not off[k].any() and not off["abs_" + k].any() and want[k].any()
    assert np.array_equal(off["count"], want["count"]) and np.array_equal(off["w"], want["w"])


def test_sums_are_exact_and_carry_their_bound():
    n, ex, ey = ON_AXIS
    w = np.array([2.0 ** 70, 1.0, 1.0, 2.0 ** -10, 2.0 ** 70, 3.0])
    ph = placed(n, ex, ey, 100.0 * C, np.zeros(6), np.zeros(6))
    ph["weight"][:] = w
    ph["s1"][:] = [1.0, -1.0, 0.5, 1.0, -1.0, 0.25]
    want = S.observation(ph, n, [0.5], T_EDGES, E_EDGES, TIME_NOW, ex, ey, X_EDGES, Y_EDGES)
    where = (0, 2, 1, 1, 2)
    assert want["count"][where] == 6
    assert want["w"][where] == float(sum(Fraction(x) for x in w))
    assert want["q"][where] == float(sum(Fraction(x) * Fraction(s) for x, s in zip(w, ph["s1"]))) == 0.25 + 2.0 ** -10      # the two 2^70 cancel: a plain sum would lose the rest
    assert want["abs_q"][where] == float(sum(Fraction(x) * abs(Fraction(s)) for x, s in zip(w, ph["s1"])))
    res = {k: v.copy() for k, v in want.items()}
    S.compare(res, want, "itself")
    res["q"][where] += 7.9 * S.U * want["abs_q"][where]              # (6 + 2) u sum|term| is the bound
    S.compare(res, want, "inside the bound")
    res["q"][where] = want["q"][where] + 8.5 * S.U * want["abs_q"][where]
    try:
        S.compare(res, want, "beyond the bound")
    except AssertionError:
        pass
    else:
        raise AssertionError("an error beyond the bound passed")
    res = {k: v.copy() for k, v in want.items()}
    res["count"][where] += 1
    try:
        S.compare(res, want, "one count off")
    except AssertionError:
        pass
    else:
        raise AssertionError("a wrong count passed")


def test_jet_sample_is_not_axisymmetric():
    """the GPU test's photons: observers at one polar angle and different azimuths see different things"""
    ph = S.jet_photons(11, 2000)
    n, cos_acc, ex, ey = S.observers([0.25, 0.25], [0.0, math.pi], 0.2)
    want = S.observation(ph, n, cos_acc, np.array([-1e6, 1e6]), np.array([1e-300, 1e300]), 400.0)
    assert want["n_accepted"][0] > 1.5 * want["n_accepted"][1] > 30
    both = S.add([want, want])
    assert np.array_equal(both["count"], 2 * want["count"]) and np.array_equal(both["abs_w"], 2 * want["abs_w"]) and "bin" not in both
