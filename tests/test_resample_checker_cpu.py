"""tests/resample_checker.py held to closed forms -- what the GPU test compares the device against must itself be right -- and
mcrat_amd.engine.resampled_estimates on synthetic cubes.  Every statistical condition runs on fixed seeds: nothing here is flaky, and a seed that
fails is a finding about the hash, not a reason to widen a bound.  (The pattern of tests/test_sky_checker_cpu.py.)"""
import math
import os
import re
from decimal import Decimal, getcontext, ROUND_FLOOR

import numpy as np
import pytest

from mcrat_amd import engine as E
from tests import resample_checker as R
from tests import sky_checker as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_AXIS = (np.array([[0.0], [0.0], [1.0]]), np.array([[1.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]]))      # n, ex = x_hat, ey = y_hat
T_EDGES, E_EDGES = np.array([-1e9, 1e9]), np.array([1e-300, 1e300])


# ---------------------------------------------------------------------------------------------- Philox and the thresholds
def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10(*ctr, *key)
        assert tuple(int(g) for g in got) == want
    # whole arrays give what scalars give
    slots = np.arange(5)
    many = R.block(0x1234567890ABCDEF, 3, slots, 7, R.BOOTSTRAP)
    for i in slots:
        one = R.philox4x32_10(i, 3, 7, 2 | (2 << 8), 0x90ABCDEF, 0x12345678)
        assert [int(w[i]) for w in many] == [int(w) for w in one]


def thresholds_50_digits():
    getcontext().prec = 50
    e1, total, fact, out = Decimal(-1).exp(), Decimal(0), Decimal(1), []
    for m in range(12):
        if m:
            fact *= m
        total += e1 / fact
        out.append(int((total * Decimal(2 ** 32)).to_integral_value(rounding=ROUND_FLOOR)))
    return out


def test_threshold_literals_equal_the_50_digit_recomputation():
    want = thresholds_50_digits()
    assert want[0] == 1580030168 and list(R.THRESHOLDS) == want
    header = open(os.path.join(ROOT, "mcrat_amd", "csrc", "resample_plan.hpp")).read()
    body = header[header.index("inline unsigned resample_poisson"):]
    body = body[:body.index("}")]
    assert [int(t) for t in re.findall(r"word >= (\d+)u", body)] == want
    # k <= 12, and the truncation bias: P(k = 12) stands for the whole tail beyond 11
    assert int(R.poisson(0xFFFFFFFF)) == 12 and int(R.poisson(0)) == 0 and int(R.poisson(want[0] - 1)) == 0 and int(R.poisson(want[0])) == 1
    mean = sum((2 ** 32 - t) for t in want) / 2.0 ** 32                      # E k = sum_m P(k > m)
    assert abs(mean - 1.0) < 2.0 ** -31 + 12 * 2.0 ** -32                     # the tail beyond 12, and twelve floors


# ---------------------------------------------------------------------------------------------- the rotation in closed form
def check_parallel_photon_keeps_its_pair(R):
    """v = n exactly, off the pole, with the observer's natural axes: the SKY_PLANE terms are the stored ones bit for bit"""
    for theta, n, ey in ((0.3, lambda t: [math.sin(t), 0.0, math.cos(t)], [0.0, 1.0, 0.0]), (1.1, lambda t: [0.0, math.sin(t), math.cos(t)], [-1.0, 0.0, 0.0])):
        nv = np.array(n(theta))
        g = np.random.default_rng(3)
        for p0 in (2.0 ** -60, 3.3e-17):
            Q, Uq = g.uniform(-1, 1, 6), g.uniform(-1, 1, 6)
            q, u, undefined = R.rotation(p0 * nv[0], p0 * nv[1], p0 * nv[2], *ey, Q, Uq)
            assert not undefined.any()
            assert q.tobytes() == Q.tobytes() and u.tobytes() == Uq.tobytes()


def ring_q_sum(alpha):
    """sum of Q' over eight photons at polar angle alpha and azimuths k * 45 deg with stored (1, 0), seen from the axis: the four on the axes give
    +1, +1, -1, -1, the four diagonal ones sin^2 alpha / (1 + cos^2 alpha) each"""
    return 4.0 * math.sin(alpha) ** 2 / (1.0 + math.cos(alpha) ** 2)


def check_ring_about_the_axis(R):
    """photons at polar angle 1e-4 and azimuths k * 45 deg with stored (1, 0), the on-axis observer with ex = x_hat, ey = y_hat: each rotated pair is
    (cos 2 phi_p, -sin 2 phi_p) to 1e-7 (the deviation is O(alpha^2)); the eight sum to ring_q_sum(alpha) in Q' and to 0 in U' within the rounding
    bound -- to 0 in both at alpha = 1e-9 --; AS_STORED sums to sum W"""
    n, ex, ey = ON_AXIS
    az = np.arange(8) * (math.pi / 4)
    ph = R.ring_photons(1e-4, az)
    q, u, undefined = R.rotation(ph["p1"], ph["p2"], ph["p3"], 0.0, 1.0, 0.0, ph["s1"], ph["s2"])
    assert not undefined.any()
    assert np.abs(q - np.cos(2 * az)).max() < 1e-7 and np.abs(u + np.sin(2 * az)).max() < 1e-7
    sky = R.observation(ph, n, [math.cos(0.1)], T_EDGES, E_EDGES, 0.0, R.NONE, 1, R.SKY_PLANE, ex=ex, ey=ey)
    assert sky["count"].tolist() == [[[[8]]]] and sky["n_frame_undefined"].tolist() == [0]
    # The rounding bound: 8 terms of size <= 1, each ~10 roundings from its closed form, and their sum.  At a finite alpha the frames' angle psi obeys
    # tan psi = cos(alpha) tan(phi_p), so the four diagonal photons have cos 2 psi = sin^2 alpha / (1 + cos^2 alpha), not 0, and the eight Q' sum to
    # RING_Q_SUM(alpha) = 4 sin^2 alpha / (1 + cos^2 alpha) = 2e-8 at alpha = 1e-4: Q' is held to that closed form, U' to 0, both within the
    # rounding bound; and at alpha = 1e-9, where the closed form is 2e-18, below the bound, the eight sum to 0 in Q' and U' as they stand.
    bound = 8 * 10 * 2.0 ** -53 + (8 + 2) * 2.0 ** -53 * 8
    assert abs(sky["q"].item() - ring_q_sum(1e-4)) <= bound and abs(sky["u"].item()) <= bound
    assert 1.9e-8 < ring_q_sum(1e-4) < 2.1e-8 and ring_q_sum(1e-9) < 0.01 * bound
    tiny = R.observation(R.ring_photons(1e-9, az), n, [math.cos(0.1)], T_EDGES, E_EDGES, 0.0, R.NONE, 1, R.SKY_PLANE, ex=ex, ey=ey)
    assert tiny["count"].item() == 8 and abs(tiny["q"].item()) <= bound and abs(tiny["u"].item()) <= bound
    stored = R.observation(ph, n, [math.cos(0.1)], T_EDGES, E_EDGES, 0.0, R.NONE, 1, R.AS_STORED)
    assert stored["q"].item() == 8.0 == stored["w"].item() and stored["u"].item() == 0.0
    assert sky["w"].item() == 8.0 and sky["i"].item() == 8.0 and sky["v"].item() == 0.0            # I and V are unchanged


def check_pole_is_undefined(R):
    """p parallel to z_hat: counted undefined, added as stored"""
    n, ex, ey = ON_AXIS
    ph = R.ring_photons(0.0, [0.0, 1.0], Q=0.25, Uq=-0.5)
    ph2 = R.ring_photons(0.2, [0.7], Q=0.25, Uq=-0.5)
    ph = S.concatenate([ph, ph2])
    want = R.observation(ph, n, [math.cos(0.3)], T_EDGES, E_EDGES, 0.0, R.NONE, 1, R.SKY_PLANE, ex=ex, ey=ey)
    assert want["n_frame_undefined"].tolist() == [2] and want["count"].item() == 3
    q, u, undefined = R.rotation(ph["p1"], ph["p2"], ph["p3"], 0.0, 1.0, 0.0, ph["s1"], ph["s2"])
    assert undefined.tolist() == [True, True, False] and q[:2].tolist() == [0.25, 0.25] and u[:2].tolist() == [-0.5, -0.5]
    assert abs(q[2] - (0.25 * math.cos(1.4) - 0.5 * math.sin(1.4))) < 0.05        # (the third is rotated, by about twice its azimuth)
    # a photon along ey is undefined too, one along ex is not
    _, _, und = R.rotation(np.array([0.0, 1.0]), np.array([1.0, 0.0]), np.array([0.0, 0.0]), 0.0, 1.0, 0.0, 1.0, 0.0)
    assert und.tolist() == [True, False]


def check_rotation_is_the_reference_rule(R):
    """against findXY, findPhi and mullerMatrixRotation written out as mcrat_scattering.c has them (acos and cos/sin of twice the angle), for
    directions all over the sphere and observers' axes anywhere: the same to 1e-12 away from d = +-1"""
    g = np.random.default_rng(12)
    for _ in range(200):
        v = g.standard_normal(3)
        v /= np.linalg.norm(v)
        nobs = v + 0.3 * g.standard_normal(3)
        nobs /= np.linalg.norm(nobs)
        ey = np.cross(nobs, g.standard_normal(3))
        ey /= np.linalg.norm(ey)
        y = np.cross(v, [0.0, 0.0, 1.0]); y /= np.linalg.norm(y)
        x = np.cross(y, v); x /= np.linalg.norm(x)
        y_new = ey - ey.dot(v) * v; y_new /= np.linalg.norm(y_new)
        d = min(1.0, max(-1.0, y.dot(y_new)))
        phi = -np.sign(x.dot(y_new)) * math.acos(d)
        Q, Uq = g.uniform(-1, 1, 2)
        want_q = Q * math.cos(2 * phi) - Uq * math.sin(2 * phi)                # mullerMatrixRotation: (Q, U) -> (Q cos 2 phi - U sin 2 phi, Q sin 2 phi + U cos 2 phi)
        want_u = Q * math.sin(2 * phi) + Uq * math.cos(2 * phi)
        q, u, undefined = R.rotation(*(1e-17 * v), *ey, Q, Uq)
        assert not undefined and abs(q - want_q) < 1e-12 and abs(u - want_u) < 1e-12


ROTATION_CHECKS = (check_parallel_photon_keeps_its_pair, check_ring_about_the_axis, check_pole_is_undefined, check_rotation_is_the_reference_rule)


@pytest.mark.parametrize("check", ROTATION_CHECKS)
def test_rotation(check):
    check(R)


# ---------------------------------------------------------------------------------------------- the statistics of the multiplicities
TRIALS, N_STAT, G_STAT, B_STAT = 64, 12800, 64, 64
BOUND = 5.0 * math.sqrt(2.0 / ((G_STAT - 1) * TRIALS))


def check_jackknife_statistics(R, estimates=E.resampled_estimates):
    """equal weights: the mean over seeds of var_jk(W) / sum w^2 is 1 within 5 sqrt(2 / ((G - 1) 64)) = 0.111; each seed's group occupancy has
    chi^2 <= (G - 1) + 5 sqrt(2 (G - 1))"""
    assert abs(BOUND - 0.111) < 5e-4
    ratios = []
    for seed in range(TRIALS):
        k = R.multiplicities(R.JACKKNIFE, seed, 0, np.arange(N_STAT), G_STAT)
        assert k.shape == (G_STAT, N_STAT) and (k.sum(axis=0) == 1).all()          # every photon in exactly one group
        occupancy = k.sum(axis=1)
        expect = N_STAT / G_STAT
        chi2 = ((occupancy - expect) ** 2 / expect).sum()
        assert chi2 <= (G_STAT - 1) + 5.0 * math.sqrt(2.0 * (G_STAT - 1)), (seed, chi2)
        cube = {name: occupancy.astype(np.float64).reshape(1, G_STAT, 1, 1) for name in ("w", "we", "i", "q", "u")}
        cube["count"] = occupancy.reshape(1, G_STAT, 1, 1)
        est = estimates(cube, E.RESAMPLE_JACKKNIFE)
        assert est["w"]["value"].item() == N_STAT
        ratios.append(est["w"]["stderr"].item() ** 2 / N_STAT)                      # sum w^2 = N
    mean = float(np.mean(ratios))
    print("jackknife: mean var_jk(W) / sum w^2 over %d seeds = %.4f (bound +-%.3f)" % (TRIALS, mean, BOUND))
    assert abs(mean - 1.0) <= BOUND


def check_bootstrap_statistics(R):
    """the mean over seeds of var(W over the replicas) / sum w^2 is 1 within the same bound"""
    ratios = []
    for seed in range(TRIALS):
        k = R.multiplicities(R.BOOTSTRAP, seed, 0, np.arange(N_STAT), B_STAT + 1)
        assert (k[0] == 1).all() and k.max() <= 12 and k.min() == 0
        ratios.append(k[1:].sum(axis=1).var(ddof=1) / N_STAT)
    mean = float(np.mean(ratios))
    print("bootstrap: mean var(W) / sum w^2 over %d seeds = %.4f (bound +-%.3f)" % (TRIALS, mean, BOUND))
    assert abs(mean - 1.0) <= BOUND


def test_jackknife_statistics():
    check_jackknife_statistics(R)


def test_bootstrap_statistics():
    check_bootstrap_statistics(R)


def test_identity_is_rank_and_slot():
    """another rank, another seed or another mode gives other draws; the same identity gives the same"""
    slots = np.arange(4000)
    a = R.group(7, 0, slots, 16)
    assert np.array_equal(a, R.group(7, 0, slots, 16))
    for other in (R.group(8, 0, slots, 16), R.group(7, 1, slots, 16), R.group(7 + (1 << 32), 0, slots, 16)):
        assert 0.85 < (a != other).mean() < 1.0                                     # 15 / 16 differ
    assert a.min() == 0 and a.max() == 15
    k = R.multiplicities(R.BOOTSTRAP, 7, 2, slots, 7)
    for rho in range(1, 7):
        j = rho - 1
        assert np.array_equal(k[rho], R.poisson(R.block(7, 2, slots, j >> 2, R.BOOTSTRAP)[j & 3]))
    assert not np.array_equal(k[1], k[5])                                            # word 0 of block 0 and of block 1


# ---------------------------------------------------------------------------------------------- a wrong checker fails
class Wrong:
    """the checker with one definition replaced"""
    def __init__(self, **replaced):
        self.replaced = replaced

    def __getattr__(self, name):
        return self.replaced[name] if name in self.replaced else getattr(R, name)


def test_a_wrong_checker_fails():
    def other_sense(p1, p2, p3, ey0, ey1, ey2, Q, Uq):
        q, u, undefined = R.rotation(p1, p2, p3, ey0, ey1, ey2, Q, -np.asarray(Uq, dtype=np.float64))
        return q, -u, undefined                                                      # rotates by -2 phi
    with pytest.raises(AssertionError):
        check_rotation_is_the_reference_rule(Wrong(rotation=other_sense))
    q, u, _ = other_sense(1e-4, 1e-4, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0)                  # azimuth 45 deg: the right answer is (0, -1)
    assert abs(u - 1.0) < 1e-7
    # a group taken from the low bits of the word fills the groups unevenly or not at all
    def low_bits(mode, seed, rank, slot, n_rep):
        if mode != R.JACKKNIFE:
            return R.multiplicities(mode, seed, rank, slot, n_rep)
        g = (R.block(seed, rank, slot, 0, R.JACKKNIFE)[0] >> np.uint64(32 - 5)).astype(np.int64)      # 32 groups where 64 were asked for
        return (g[None, :] == np.arange(n_rep)[:, None]).astype(np.int64)
    with pytest.raises(AssertionError):
        check_jackknife_statistics(Wrong(multiplicities=low_bits))
    # a dropped rescale: the replicate totals are T - x_g, and the variance of a total comes out (G - 1)^2 / G^2 too small -- within the bound for
    # G = 64, so the identity below is what catches it
    def no_rescale(res, mode, reduce=()):
        x = res["w"].sum(axis=tuple(range(2, res["w"].ndim)))
        total = x.sum(axis=1)
        reps = total[:, None] - x
        G = x.shape[1]
        var = (G - 1.0) / G * ((reps - reps.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
        return {"w": {"value": total, "stderr": np.sqrt(var)}}
    with pytest.raises(AssertionError):
        check_linear_identity(no_rescale)
    # bootstrap multiplicities that are not Poisson(1): the word compared against the first threshold alone (Bernoulli: variance 0.23)
    def bernoulli(mode, seed, rank, slot, n_rep):
        return np.minimum(R.multiplicities(mode, seed, rank, slot, n_rep), 1)
    with pytest.raises(AssertionError):
        check_bootstrap_statistics(Wrong(multiplicities=bernoulli))


# ---------------------------------------------------------------------------------------------- resampled_estimates on synthetic cubes
def synthetic(G, shape=(2, 3), seed=1):
    g = np.random.default_rng(seed)
    full = (1, G) + shape
    cube = {"count": g.integers(1, 9, full)}
    cube["w"] = g.uniform(1.0, 2.0, full) * cube["count"]
    cube["we"] = cube["w"] * g.uniform(0.5, 1.5, full)
    cube["i"] = cube["w"].copy()
    cube["q"] = cube["w"] * g.uniform(-0.3, 0.3, full)
    cube["u"] = cube["w"] * g.uniform(-0.3, 0.3, full)
    return cube


def check_linear_identity(estimates):
    """a linear statistic: var_jk = G / (G - 1) sum (x_g - mean x)^2, to 1e-12 relative"""
    for G in (2, 5, 32):
        cube = synthetic(G)
        est = estimates(cube, E.RESAMPLE_JACKKNIFE)
        x = cube["w"]
        want = G / (G - 1.0) * ((x - x.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
        assert np.allclose(est["w"]["stderr"] ** 2, want, rtol=1e-12, atol=0.0)
        assert np.allclose(est["w"]["value"], x.sum(axis=1), rtol=1e-15)


def test_linear_statistic_identity():
    check_linear_identity(E.resampled_estimates)
    # ... which is the familiar sum w^2 when every group holds one photon: the jackknife subsumes a sum-of-squares plane
    w = np.random.default_rng(4).uniform(1.0, 3.0, 50)
    cube = {k: w.reshape(1, 50, 1, 1).copy() for k in ("w", "we", "i", "q", "u")}
    cube["count"] = np.ones((1, 50, 1, 1), dtype=np.int64)
    var = E.resampled_estimates(cube, E.RESAMPLE_JACKKNIFE)["w"]["stderr"].item() ** 2
    assert math.isclose(var, 50 / 49.0 * ((w - w.mean()) ** 2).sum(), rel_tol=1e-12)


def test_a_ratio_is_unchanged_by_the_rescale():
    G = 8
    cube = synthetic(G)
    est = E.resampled_estimates(cube, E.RESAMPLE_JACKKNIFE)
    total_w, total_we = cube["w"].sum(axis=1), cube["we"].sum(axis=1)
    reps = (total_we[:, None] - cube["we"]) / (total_w[:, None] - cube["w"])          # no rescale at all
    dev = reps - (total_we / total_w)[:, None]
    want = (G - 1.0) / G * ((dev - dev.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    assert np.allclose(est["e_mean"]["stderr"] ** 2, want, rtol=1e-9)
    assert np.allclose(est["e_mean"]["value"], total_we / total_w, rtol=1e-15)
    pi = np.sqrt(cube["q"].sum(axis=1) ** 2 + cube["u"].sum(axis=1) ** 2) / cube["i"].sum(axis=1)
    assert np.allclose(est["pi"]["value"], pi, rtol=1e-14) and (est["pi"]["stderr"] > 0).all()


def test_reduce_sums_the_axes_first():
    cube = synthetic(6, shape=(2, 3, 2, 2))
    for reduce, axes in (("energy", (3,)), ("time", (2,)), ("pixels", (4, 5)), (("time", "energy", "pixels"), (2, 3, 4, 5))):
        est = E.resampled_estimates(cube, E.RESAMPLE_JACKKNIFE, reduce=reduce)
        summed = {k: v.sum(axis=axes) for k, v in cube.items()}
        # (a cube with the axes gone has fewer dimensions: the helper is given what is left as time and energy axes)
        while summed["w"].ndim < 4:
            summed = {k: v[..., None] for k, v in summed.items()}
        again = E.resampled_estimates(summed, E.RESAMPLE_JACKKNIFE)
        assert np.allclose(est["pi"]["stderr"].ravel(), again["pi"]["stderr"].ravel(), rtol=1e-12)
        assert est["w"]["value"].shape == tuple(m for k, m in enumerate(cube["w"].shape) if k != 1 and k not in axes)
    with pytest.raises(ValueError):
        E.resampled_estimates(cube, E.RESAMPLE_JACKKNIFE, reduce="colour")


def test_the_angle_wraps_across_half_pi():
    """replicates on both sides of +-pi/2 are next to each other, not pi apart"""
    angles = np.array([1.55, -1.56, 1.57, -1.55, 1.56])                                 # about pi/2 = 1.5708: a spread of ~0.03
    B = len(angles)
    full = (1, B + 1, 1, 1)
    cube = {"count": np.ones(full, dtype=np.int64), "w": np.ones(full), "we": np.ones(full), "i": np.ones(full)}
    all_angles = np.concatenate([[1.57], angles])
    cube["q"], cube["u"] = np.cos(2 * all_angles).reshape(full), np.sin(2 * all_angles).reshape(full)
    est = E.resampled_estimates(cube, E.RESAMPLE_BOOTSTRAP, percentiles=(16, 84))
    assert math.isclose(est["angle"]["value"].item(), 1.57, rel_tol=1e-12)
    dev = np.array([1.55 - 1.57, -1.56 + math.pi - 1.57, 0.0, -1.55 + math.pi - 1.57, 1.56 - 1.57])
    assert math.isclose(est["angle"]["stderr"].item(), dev.std(ddof=1), rel_tol=1e-9) and est["angle"]["stderr"].item() < 0.03
    assert est["angle"]["lo"].item() < 1.57 < est["angle"]["hi"].item() < 1.57 + 0.03
    assert E._wrap_half_pi(np.array([math.pi / 2, -math.pi / 2, 0.0, 2.0, -2.0])).tolist() == pytest.approx([math.pi / 2, math.pi / 2, 0.0, 2.0 - math.pi, math.pi - 2.0])
    # the same through the jackknife: groups whose leave-one-out angles straddle the branch
    G = 4
    cube = synthetic(G, shape=(1, 1))
    cube["q"] = -cube["i"] * 0.2
    cube["u"] = cube["i"] * np.array([1e-3, -2e-3, 1.5e-3, -1e-3]).reshape(1, G, 1, 1)      # angles about +-pi/2
    est = E.resampled_estimates(cube, E.RESAMPLE_JACKKNIFE)
    assert est["angle"]["stderr"].item() < 0.05


def test_empty_bins_give_nan():
    cube = synthetic(5)
    for k in cube:
        cube[k][:, :, 1, 2] = 0
    for mode in (E.RESAMPLE_JACKKNIFE, E.RESAMPLE_BOOTSTRAP):
        est = E.resampled_estimates(cube, mode)
        for name, e in est.items():
            assert np.isnan(e["value"][0, 1, 2]) and np.isnan(e["stderr"][0, 1, 2]), name
            assert np.isfinite(np.delete(e["value"].ravel(), 5)).all() and np.isfinite(np.delete(e["stderr"].ravel(), 5)).all(), name
    none = {k: v[:, :1] for k, v in cube.items()}
    est = E.resampled_estimates(none, E.RESAMPLE_NONE)
    assert np.isnan(est["w"]["value"][0, 1, 2]) and np.isnan(est["w"]["stderr"]).all() and est["w"]["value"][0, 0, 0] == none["w"][0, 0, 0, 0]


def test_bootstrap_estimates():
    B = 40
    g = np.random.default_rng(2)
    full = (1, B + 1, 1, 1)
    cube = {"count": np.full(full, 100), "w": 100.0 + g.standard_normal(full), "we": 50.0 + g.standard_normal(full), "i": np.full(full, 100.0),
            "q": 10.0 + g.standard_normal(full), "u": g.standard_normal(full)}
    est = E.resampled_estimates(cube, E.RESAMPLE_BOOTSTRAP)
    assert est["w"]["value"].item() == cube["w"][0, 0, 0, 0]
    assert math.isclose(est["w"]["stderr"].item(), cube["w"][0, 1:, 0, 0].std(ddof=1), rel_tol=1e-12)
    ratio = cube["we"][0, 1:, 0, 0] / cube["w"][0, 1:, 0, 0]
    assert math.isclose(est["e_mean"]["stderr"].item(), ratio.std(ddof=1), rel_tol=1e-9)
