"""Mock observations on the device (mcrat_hip_observe, mcrat_hip_pool_observe; mcrat_amd/csrc/observe.hip): the resident photons binned by observer,
detection time and energy, against a NumPy restatement of the definitions (include/mcrat_hip.h) that takes its per-bin sums
with math.fsum.

count, n_accepted and n_outside must be EXACTLY equal, every photon included: each expression that decides a bin is written in one fixed order and
evaluated without contraction, so it is bit-identical on the device and here.  Each of the six sums of a bin with m photons must be within
(m + 2) * 2**-53 * sum|term| of the fsum -- the worst case of any summation order (m - 1 roundings of partial sums no larger than sum|term|) plus
room for the term's own roundings; derived, not measured.  sum|term| is taken over the checker's terms."""
import math

import numpy as np
import pytest

from mcrat_amd import synth

pytestmark = pytest.mark.gpu

C_LIGHT = 2.99792458e10
PLANES = (("w", None), ("we", "e"), ("i", "s0"), ("q", "s1"), ("u", "s2"), ("v", "s3"))
PATHS = ("lds", "global")


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


# ---------------------------------------------------------------------------------------------- inputs
def make_photons(seed, n):
    """r ~ 1e12 .. 1e13 cm, positions and directions within ~0.3 rad of the axis, p0 log-uniform over 6 decades, weights over 3, Stokes of both signs"""
    g = np.random.default_rng(seed)
    r = 10.0 ** g.uniform(12.0, 13.0, n)
    th, phi = g.uniform(0.0, 0.3, n), g.uniform(0.0, 2 * np.pi, n)
    p0 = 10.0 ** g.uniform(-20.0, -14.0, n)
    thp, php = g.uniform(0.0, 0.3, n), g.uniform(0.0, 2 * np.pi, n)
    ph = {"r0": r * np.sin(th) * np.cos(phi), "r1": r * np.sin(th) * np.sin(phi), "r2": r * np.cos(th),
          "p0": p0, "p1": p0 * np.sin(thp) * np.cos(php), "p2": p0 * np.sin(thp) * np.sin(php), "p3": p0 * np.cos(thp),
          "s0": np.ones(n), "s1": g.uniform(-1.0, 1.0, n), "s2": g.uniform(-1.0, 1.0, n), "s3": g.uniform(-1.0, 1.0, n),
          "weight": 10.0 ** g.uniform(48.0, 51.0, n), "num_scatt": np.floor(g.uniform(0.0, 30.0, n)),
          "time_to_scatter": np.zeros(n), "total_optical_depth": np.ones(n),
          "type": np.full(n, b"i", dtype="S1"), "nearest_block_index": np.zeros(n, dtype=np.int32), "recalc_properties": np.ones(n, dtype=np.int32)}
    for k in ("comv_p0", "comv_p1", "comv_p2", "comv_p3"):
        ph[k] = ph[k[5:]].copy()
    return ph


def cones(theta_obs, half):
    theta_obs = np.asarray(theta_obs, dtype=np.float64)
    lo = np.where(theta_obs - half <= 0.0, 1.0, np.cos(np.maximum(theta_obs - half, 0.0)))
    return np.cos(theta_obs), np.sin(theta_obs), lo, np.cos(theta_obs + half)


TWO_OBSERVERS = cones([0.05, 0.2], 0.08)
T_EDGES = np.linspace(100.0, 360.0, 5)                 # t_det = 400 - r.n / c lies between ~65 and ~370 s: some photons fall outside
E_EDGES = 10.0 ** np.linspace(-9.0, -4.0, 9)           # e = p0 c lies between 3e-10 and 3e-4 erg: some fall outside
TIME_NOW = 400.0


def engine_with(hip, ph, stokes=1):
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, stokes)
    e.set_photons(ph)
    return e


# ---------------------------------------------------------------------------------------------- the checker
def find_bin(edges, x):
    """edges[k] <= x < edges[k + 1], else -1"""
    k = np.searchsorted(edges, x, side="right") - 1
    return np.where((k >= 0) & (k < len(edges) - 1), k, -1)


def per_photon(ph, obs, t_edges, e_edges, time_now):
    """(accepted, t_det, e, time bin, energy bin), each (n_obs, n): the definitions, every expression in the order they give"""
    co, so, cl, ch = (np.asarray(a, dtype=np.float64)[:, None] for a in obs)
    p0, p3, r0, r1, r2, w = (np.asarray(ph[k], dtype=np.float64)[None, :] for k in ("p0", "p3", "r0", "r1", "r2", "weight"))
    typ = np.asarray(ph["type"])[None, :]
    tn = np.broadcast_to(np.asarray(time_now, dtype=np.float64), p0.shape[1:])[None, :]
    observable = (w != 0) & (typ != b"p") & (typ != b"N")
    acc = observable & (p3 <= p0 * cl) & (p3 > p0 * ch)
    e = np.broadcast_to(p0 * C_LIGHT, acc.shape)
    t = tn - ((r2 * co + np.sqrt(r0 * r0 + r1 * r1) * so) / C_LIGHT)
    return acc, t, e, find_bin(t_edges, t), find_bin(e_edges, e)


def checker(ph, obs, t_edges, e_edges, time_now, stokes=True):
    acc, t, e, it, ie = per_photon(ph, obs, t_edges, e_edges, time_now)
    n_obs, n_t, n_e = acc.shape[0], len(t_edges) - 1, len(e_edges) - 1
    inside = acc & (it >= 0) & (ie >= 0)
    want = {"n_accepted": acc.sum(axis=1).astype(np.int64), "n_outside": (acc & ~inside).sum(axis=1).astype(np.int64),
            "count": np.zeros((n_obs, n_t, n_e), dtype=np.int64)}
    for k, _ in PLANES:
        want[k] = np.zeros((n_obs, n_t, n_e))
        want["abs_" + k] = np.zeros((n_obs, n_t, n_e))
    w = np.asarray(ph["weight"], dtype=np.float64)
    terms = {"w": w, "we": w * e[0]}
    for k, col in PLANES[2:]:
        terms[k] = w * np.asarray(ph[col], dtype=np.float64) if stokes else np.zeros_like(w)
    for o in range(n_obs):
        idx = np.nonzero(inside[o])[0]
        flat = it[o, idx] * n_e + ie[o, idx]
        order = np.argsort(flat, kind="stable")
        idx, flat = idx[order], flat[order]
        starts = np.nonzero(np.diff(flat, prepend=-1))[0]
        for a, b in zip(starts, list(starts[1:]) + [len(flat)]):
            members, where = idx[a:b], (o, flat[a] // n_e, flat[a] % n_e)
            want["count"][where] = b - a
            for k, _ in PLANES:
                want[k][where] = math.fsum(terms[k][members])
                want["abs_" + k][where] = math.fsum(np.abs(terms[k][members]))
    return want


def compare(res, want, label=""):
    for k in ("n_accepted", "n_outside", "count"):
        assert np.array_equal(res[k], want[k]), (label, k, res[k].sum(), want[k].sum())
    assert np.array_equal(want["count"].sum(axis=(1, 2)), want["n_accepted"] - want["n_outside"])
    m = want["count"].astype(np.float64)
    for k, _ in PLANES:
        bound = (m + 2.0) * 2.0 ** -53 * want["abs_" + k]
        err = np.abs(res[k] - want[k])
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        print("%s %s: largest error / bound = %.3g over %d bins in use" % (label, k, worst, int((m > 0).sum())))
        assert (err <= bound).all(), (label, k, worst)          # (an empty bin: bound 0, the device's plane must hold 0)


def observe(e, obs, t_edges, e_edges, time_now):
    return e.observe(obs[0], obs[1], obs[2], obs[3], t_edges, e_edges, time_now)


# ---------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [1, 3, 63, 65, 1000, 4099])
def test_ragged_sizes(hip, monkeypatch, n, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    ph = make_photons(100 + n, n)
    e = engine_with(hip, ph)
    res = observe(e, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)
    assert e.observe_path() == (hip.OBSERVE_PATH_LDS if path == "lds" else hip.OBSERVE_PATH_GLOBAL)
    assert res["count"].shape == (2, 4, 8) and res["w"].shape == (2, 4, 8) and res["n_accepted"].shape == (2,)
    want = checker(ph, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)
    compare(res, want, "n=%d %s" % (n, path))
    if n >= 1000:
        assert (want["n_accepted"] > n // 20).all() and (want["n_outside"] > 0).all() and (want["count"] > 0).sum() > 20
    e.close()


@pytest.mark.parametrize("path", PATHS)
def test_exclusions(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    n = 1000
    ph = make_photons(7, n)
    g = np.random.default_rng(8)
    kind = g.integers(0, 10, n)
    ph["weight"][kind == 0] = 0.0
    ph["type"][kind == 1] = b"p"
    ph["type"][kind == 2] = b"N"
    ph["type"][kind == 3] = b"c"                       # other types count
    e = engine_with(hip, ph)
    res = observe(e, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)
    want = checker(ph, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)
    compare(res, want, "exclusions " + path)
    assert np.array_equal(res["count"].sum(axis=(1, 2)), res["n_accepted"] - res["n_outside"])
    # what the sample holds: every kind of exclusion removes photons that would otherwise have counted, both axes lose some, some are in no cone
    all_in = dict(ph, weight=np.where(ph["weight"] == 0, 1.0, ph["weight"]), type=np.full(n, b"i", dtype="S1"))
    acc_all = per_photon(all_in, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)[0]
    acc, t, en, it, ie = per_photon(ph, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)
    for k in (0, 1, 2):
        assert (acc_all[:, kind == k].any(axis=0)).sum() > 10 and not acc[:, kind == k].any()
    assert acc[:, kind == 3].any()
    assert (acc & (it < 0)).any() and (acc & (ie < 0)).any() and (~acc_all.any(axis=0)).sum() > 10
    e.close()


@pytest.mark.parametrize("path", PATHS)
def test_edges_are_half_open_and_cones_closed_below(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    n = 600
    ph = make_photons(21, n)
    cos_lo, cos_hi = 127.0 / 128.0, 31.0 / 32.0                 # exact binary fractions: theta from 0.125 to 0.2506 rad
    obs = (np.array([math.cos(0.19)]), np.array([math.sin(0.19)]), np.array([cos_lo]), np.array([cos_hi]))
    on_lo, on_hi = 10, 11
    ph["p3"][on_lo] = ph["p0"][on_lo] * cos_lo                  # p3 == p0 * cos_lo: inside
    ph["p3"][on_hi] = ph["p0"][on_hi] * cos_hi                  # p3 == p0 * cos_hi: outside
    wide_t, wide_e = np.array([-1e6, 1e6]), np.array([1e-300, 1e300])
    acc, t, en, _, _ = per_photon(ph, obs, wide_t, wide_e, TIME_NOW)
    inside = np.nonzero(acc[0])[0]
    assert on_lo in inside and on_hi not in inside and len(inside) > 100
    # edges that ARE the t_det and e of accepted photons, the last edge of each axis among them
    by_t, by_e = inside[np.argsort(t[0, inside])], inside[np.argsort(en[0, inside])]
    t_pick, e_pick = by_t[[20, 60, 100, len(by_t) - 5]], by_e[[15, 50, 90, len(by_e) - 7]]
    t_edges, e_edges = t[0, t_pick].copy(), en[0, e_pick].copy()
    assert (np.diff(t_edges) > 0).all() and (np.diff(e_edges) > 0).all()
    e = engine_with(hip, ph)
    res = observe(e, obs, t_edges, e_edges, TIME_NOW)
    want = checker(ph, obs, t_edges, e_edges, TIME_NOW)
    compare(res, want, "edges " + path)
    _, _, _, it, ie = per_photon(ph, obs, t_edges, e_edges, TIME_NOW)
    assert it[0, t_pick].tolist() == [0, 1, 2, -1] and ie[0, e_pick].tolist() == [0, 1, 2, -1]      # on a left edge: in its bin; on the last edge: outside
    # ... and on the device photon by photon: a list of one chosen photon, the other axis wide open
    def alone(i, te, ee):
        one = {k: v[i:i + 1].copy() for k, v in ph.items()}
        e1 = engine_with(hip, one)
        r1 = observe(e1, obs, te, ee, TIME_NOW)
        compare(r1, checker(one, obs, te, ee, TIME_NOW), "edges, photon %d, %s" % (i, path))
        e1.close()
        return r1
    r1 = alone(int(t_pick[0]), t_edges, wide_e)
    assert r1["count"][0, :, 0].tolist() == [1, 0, 0]                        # t_det == t_edges[0]: the first bin
    r1 = alone(int(t_pick[3]), t_edges, wide_e)
    assert (r1["n_accepted"][0], r1["n_outside"][0], r1["count"].sum()) == (1, 1, 0)      # t_det == the last edge: outside
    r1 = alone(int(e_pick[1]), wide_t, e_edges)
    assert r1["count"][0, 0].tolist() == [0, 1, 0]
    r1 = alone(int(e_pick[3]), wide_t, e_edges)
    assert (r1["n_accepted"][0], r1["n_outside"][0], r1["count"].sum()) == (1, 1, 0)
    assert alone(on_lo, wide_t, wide_e)["count"].sum() == 1                  # p3 == p0 * cos_lo: accepted
    r1 = alone(on_hi, wide_t, wide_e)
    assert (r1["n_accepted"][0], r1["count"].sum()) == (0, 0)                # p3 == p0 * cos_hi: not
    e.close()


@pytest.mark.parametrize("path", PATHS)
def test_overlapping_cones(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    n = 1000
    ph = make_photons(33, n)
    obs = cones([0.08, 0.14, 0.2], 0.08)                        # [0, 0.16], [0.06, 0.22], [0.12, 0.28]: every pair overlaps
    e = engine_with(hip, ph)
    res = observe(e, obs, T_EDGES, E_EDGES, TIME_NOW)
    want = checker(ph, obs, T_EDGES, E_EDGES, TIME_NOW)
    compare(res, want, "overlap " + path)
    acc = per_photon(ph, obs, T_EDGES, E_EDGES, TIME_NOW)[0]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert (acc[a] & acc[b]).sum() > 20
    assert res["n_accepted"].sum() > acc.any(axis=0).sum() + 100      # the photons in the overlaps count once per observer
    e.close()


@pytest.mark.parametrize("path", PATHS)
def test_contention_in_one_bin(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    n = 4096
    ph = make_photons(44, n)
    obs = (np.array([1.0]), np.array([0.0]), np.array([1.0]), np.array([0.9]))      # on the axis, a cone of 0.45 rad: every photon
    t_edges, e_edges = np.array([0.0, 1.0, 50.0, 390.0, 1000.0]), np.array([1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-3, 1e-2, 1e-1, 1.0])
    e = engine_with(hip, ph)
    res = observe(e, obs, t_edges, e_edges, TIME_NOW)
    want = checker(ph, obs, t_edges, e_edges, TIME_NOW)
    assert want["count"][0, 2, 4] == n and want["n_outside"][0] == 0
    compare(res, want, "contention " + path)
    e.close()


def test_cube_beyond_lds_takes_the_global_path(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_OBSERVE_PATH", raising=False)
    n = 4099
    ph = make_photons(55, n)
    e = engine_with(hip, ph)
    assert e.observe_path() == 0
    # 4 x 512 x 64 bins of 56 bytes: 7 MB, far beyond the 80 KiB a workgroup may use
    obs = cones([0.04, 0.1, 0.16, 0.22], 0.05)
    t_edges, e_edges = np.linspace(60.0, 380.0, 513), 10.0 ** np.linspace(-9.6, -3.4, 65)
    res = observe(e, obs, t_edges, e_edges, TIME_NOW)
    assert e.observe_path() == hip.OBSERVE_PATH_GLOBAL
    want = checker(ph, obs, t_edges, e_edges, TIME_NOW)
    compare(res, want, "4x512x64")
    assert (want["count"] > 0).sum() > 2000
    # 1 x 1 x 8
    one = tuple(a[:1] for a in TWO_OBSERVERS)
    res = observe(e, one, np.array([0.0, 1000.0]), E_EDGES, TIME_NOW)
    assert e.observe_path() == hip.OBSERVE_PATH_LDS
    compare(res, checker(ph, one, np.array([0.0, 1000.0]), E_EDGES, TIME_NOW), "1x1x8")
    e.close()


@pytest.mark.parametrize("n_e, lds", [(682, True), (683, False)])
def test_path_changes_at_the_lds_budget(hip, monkeypatch, n_e, lds):
    """1 x 2 x 682 bins with their edges and counters are 80 KiB of LDS exactly -- the largest workgroup copy, more than the 64 KiB a kernel gets
    unasked; one energy bin more and the cube stays in HBM (tests/test_observe_plan_cpu.py has the rule)"""
    monkeypatch.delenv("MCRAT_HIP_OBSERVE_PATH", raising=False)
    ph = make_photons(66, 3000)
    e = engine_with(hip, ph)
    one = tuple(a[1:] for a in TWO_OBSERVERS)
    t_edges, e_edges = np.array([60.0, 250.0, 380.0]), 10.0 ** np.linspace(-9.6, -3.4, n_e + 1)
    res = observe(e, one, t_edges, e_edges, TIME_NOW)
    assert e.observe_path() == (hip.OBSERVE_PATH_LDS if lds else hip.OBSERVE_PATH_GLOBAL)
    want = checker(ph, one, t_edges, e_edges, TIME_NOW)
    compare(res, want, "1x2x%d" % n_e)
    assert (want["count"] > 0).sum() > 500 and want["count"][0, :, -20:].sum() > 0 and want["count"][0, :, :20].sum() > 0      # both ends of the planes are in use
    e.close()


@pytest.mark.parametrize("path", PATHS)
def test_pool_every_list_its_own_clock(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    lens, ranks = [137, 1000, 3, 512, 64], [0, 1, 2, 3, 5]      # rank 4 is never created
    clocks = np.array([400.0, 380.0, 410.0, 395.5, -1.0e9, 420.0])
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(6, 1100)
    lists = [make_photons(60 + r, m) for r, m in zip(ranks, lens)]
    for r, ph in zip(ranks, lists):
        pool.pool_rank(r, r).set_photons(ph)
    res = pool.pool_observe(*TWO_OBSERVERS, T_EDGES, E_EDGES, clocks)
    cat = {k: np.concatenate([ph[k] for ph in lists]) for k in lists[0]}
    tn = np.concatenate([np.full(m, clocks[r]) for r, m in zip(ranks, lens)])
    want = checker(cat, TWO_OBSERVERS, T_EDGES, E_EDGES, tn)
    compare(res, want, "pool " + path)
    assert want["count"].sum() > 500
    # the clocks matter: with one clock for all the cube is another one
    assert not np.array_equal(checker(cat, TWO_OBSERVERS, T_EDGES, E_EDGES, 400.0)["count"], want["count"])
    # the view of list 1 observes that list alone
    v = pool.pool_rank(1, 1)
    compare(observe(v, TWO_OBSERVERS, T_EDGES, E_EDGES, clocks[1]), checker(lists[1], TWO_OBSERVERS, T_EDGES, E_EDGES, clocks[1]), "view 1 " + path)
    with pytest.raises(hip.McratHipError):
        observe(pool, TWO_OBSERVERS, T_EDGES, E_EDGES, 400.0)    # the pool itself has no single clock
    pool.close()


@pytest.mark.parametrize("path", PATHS)
def test_stokes_off(hip, monkeypatch, path):
    monkeypatch.setenv("MCRAT_HIP_OBSERVE_PATH", path)
    ph = make_photons(77, 1000)
    on, off = engine_with(hip, ph, stokes=1), engine_with(hip, ph, stokes=0)
    r_on, r_off = observe(on, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW), observe(off, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW)
    compare(r_off, checker(ph, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW, stokes=False), "stokes off " + path)
    for k in ("i", "q", "u", "v"):
        assert not r_off[k].any() and r_on[k].any()
    for k in ("count", "n_accepted", "n_outside"):
        assert np.array_equal(r_on[k], r_off[k])
    compare(r_on, checker(ph, TWO_OBSERVERS, T_EDGES, E_EDGES, TIME_NOW), "stokes on " + path)
    on.close()
    off.close()


def test_refusals_reach_the_caller(hip):
    e = engine_with(hip, make_photons(1, 10))
    with pytest.raises(hip.McratHipError, match="cos_lo > cos_hi"):
        e.observe([1.0], [0.0], [0.5], [0.9], T_EDGES, E_EDGES, TIME_NOW)
    with pytest.raises(hip.McratHipError, match="t_edges is not strictly ascending"):
        e.observe([1.0], [0.0], [1.0], [0.9], [0.0, 2.0, 1.0], E_EDGES, TIME_NOW)
    with pytest.raises(hip.McratHipError, match="at least 1"):
        e.observe([1.0], [0.0], [1.0], [0.9], [0.0], E_EDGES, TIME_NOW)
    e.close()


def test_after_real_propagation(hip, monkeypatch):
    """the observer on the columns the loop actually leaves behind"""
    monkeypatch.delenv("MCRAT_HIP_OBSERVE_PATH", raising=False)
    frame, ph, cfg = synth.config2(n_photons=2000, nzc=8, stokes=1, lumi=1e54)
    e = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    e.set_hydro(frame)
    e.set_photons(ph)
    time_now, rem = 2.0, 0.1
    e.begin_frame(1234, time_now, rem)
    st = e.run(250)
    assert st.frame_scatt_cnt > 0
    # observers and edges from the initial photons' range, so that the cube is well filled whatever the frame did
    theta = np.arccos(ph["p3"] / ph["p0"])
    obs = cones(np.percentile(theta, [25, 50, 75]), 0.5 * (np.percentile(theta, 90) - np.percentile(theta, 10)))
    _, t0, e0, _, _ = per_photon(ph, obs, np.array([0.0, 1.0]), np.array([0.0, 1.0]), st.time_now)
    t_edges = np.linspace(np.percentile(t0, 2), np.percentile(t0, 98), 7)
    e_edges = 10.0 ** np.linspace(np.log10(np.percentile(e0, 2)), np.log10(np.percentile(e0, 98)), 9)
    res = observe(e, obs, t_edges, e_edges, st.time_now)
    after = e.get_photons()
    assert not np.array_equal(after["r2"], ph["r2"]) and not np.array_equal(after["p0"], ph["p0"])      # the frame moved and scattered them
    want = checker(after, obs, t_edges, e_edges, st.time_now)
    compare(res, want, "after a frame")
    assert want["count"].sum() > 1000 and (want["count"] > 0).sum() > 30 and np.abs(res["q"]).sum() > 0
    e.close()
