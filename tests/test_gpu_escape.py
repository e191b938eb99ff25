"""Escape-weighted sky observations on the device (mcrat_hip_observe_escaping, mcrat_hip_pool_observe_escaping; mcrat_amd/csrc/escape.hip) against
tests/escape_checker.py -- an independent NumPy restatement built on tests/sky_checker.py and tests/sightline_checker.py -- and against the products
that exist, without any checker: mcrat_hip_sightline_photons' device tau binned on the host, and mcrat_hip_observe_sky.

The cases are the sightline checker's (16 x 16 and 8 x 8 x 8 meshes), their rays placed as resident slots; three observers -- the polar axis and two
directions within 0.15 rad of it, cones of 0.15 to 0.5 rad; clock 40 s; log energy edges 1e-10 .. 1e-5 erg; tau edges (0, 0.1, 0.3, 1, 3, 10, 30).
Time bins: the photons sit at r.n / c = 33 .. 39 s and are detected between 1 and 7 s, so the 1-s bins that hold them run from 0 s (T_EDGES); 1-s bins
from 30 s hold none, and test_time_bins_from_30_s asserts just that: every accepted LEFT_MESH photon is then outside.

Exact: every counter and the count plane (tests/test_escape_checker_cpu.py holds the condition that no case has a fragile photon; one would be
tolerated as the issue says), and both identities.  Raw sums within (m + 2) 2^-53 sum|term|; WX and WEX within that plus
sum_k |term_k| (bound_k + 3 2^-53), bound_k the sightline checker's bound on tau_k -- derived, not measured; the largest error / bound is printed."""
import ctypes as C

import numpy as np
import pytest

from mcrat_amd import synth
from tests import escape_checker as ec
from tests import sightline_checker as sc
from tests import sky_checker as S
from tests import test_escape_plan_cpu as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in ("MCRAT_HIP_ESCAPE_PATH", "MCRAT_HIP_SKY_PATH", "MCRAT_HIP_SIGHTLINE_REFILL"):
        monkeypatch.delenv(k, raising=False)


def engine_for(hip, c, stokes=1, frame=None):
    frame = c["frame"] if frame is None else frame
    e = hip.Engine(frame["dimensions"], frame["geometry"], stokes, tau_calculation=hip.TAU_TABLE if c["table"] else hip.TAU_DIRECT)
    e.set_hydro(frame)
    if c["table"]:
        e.set_hot_cross_section(c["table"]["values"], c["table"]["grid"])
    return e


def observe(e, c, t_edges=ec.T_EDGES, e_edges=ec.E_EDGES, tau_edges=ec.TAU_EDGES, time_now=ec.TIME_NOW, image=False, pool=False, **kw):
    n, cos_acc, ex, ey = ec.observers()
    if image:
        kw.update(ex=ex, ey=ey, x_edges=ec.X_EDGES, y_edges=ec.Y_EDGES)
    call = e.pool_observe_escaping if pool else e.observe_escaping
    return call(n, cos_acc, t_edges, e_edges, tau_edges, time_now, **dict(ec.march_params(c["params"]), **kw))


def run_case(hip, name, exclusions=True, stokes=1):
    k = ec.case(name, exclusions)
    e = engine_for(hip, k["c"], stokes)
    e.set_photons(k["ph"])
    return k, e


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def from_device_tau(e, c, ph, t_edges=ec.T_EDGES, **kw):
    """no checker of the march involved: mcrat_hip_sightline_photons' tau and status, binned on the host with the same rules"""
    sl = e.sightline_photons(surface_level=-1.0, **ec.march_params(c["params"]))
    marched = dict(tau=sl["tau"], status=sl["status"], bound=np.zeros(len(sl["tau"])), fragile=np.zeros(len(sl["tau"]), dtype=bool))
    n, cos_acc, _, _ = ec.observers()
    return ec.observation(ph, marched, n, cos_acc, t_edges, ec.E_EDGES, ec.TAU_EDGES, ec.TIME_NOW, **kw)


def same_counts(res, want, label):
    for key in ("count",) + ec.COUNTERS + ("n_status",):
        assert np.array_equal(res[key], want[key]), (label, key)
    assert res["n_selected"] == want["n_selected"] and res["n_observable"] == want["n_observable"], label


# ---------------------------------------------------------------------------------------------- slot counts, no side effects
@pytest.mark.parametrize("name", ["uniform_n1", "uniform_n63", "uniform_n65", "pair_0_1", "uniform_n1000"])
def test_slot_counts(hip, name):
    k, e = run_case(hip, name, exclusions=name != "uniform_n1")
    before = e.get_photons()
    res = observe(e, k["c"])
    after = e.get_photons()
    for col in before:                                     # no photon column changes, bit for bit
        assert np.array_equal(bits(before[col]), bits(after[col])), col
    want = k["want"]
    assert res["count"].shape == (3, 6, 10, 5) and res["n_status"].shape == (5,) and res["n_accepted"].shape == (3,)
    ec.compare(res, want, name)
    live = ~np.isin(k["ph"]["type"], (b"p", b"N")) & (k["ph"]["weight"] != 0)
    assert res["n_observable"] == live.sum() and (name == "uniform_n1" or 0 < (~live).sum())
    frac = hip.escape_fraction(res)
    used = res["w"] != 0
    # x <= 1, so WX <= W up to the two sums' own orders: each within (m + 2) 2^-53 of its exact sum, m <= 1000
    assert np.isnan(frac[~used]).all() and (frac[used] > 0).all() and (frac[used] <= 1.0 + 2 * 1002 * ec.U).all()
    e.close()


# ---------------------------------------------------------------------------------------------- geometries; the shared march step
@pytest.mark.parametrize("dims, geom", sc.PAIRS)
def test_every_dimensions_geometry_pair(hip, dims, geom):
    name = "pair_%d_%d" % (dims, geom)
    k, e = run_case(hip, name)
    res = observe(e, k["c"])
    ec.compare(res, k["want"], name)
    # the cube's counts are those of the sightline kernel's own tau, photon for photon: both kernels call one step
    same_counts(res, from_device_tau(e, k["c"], k["ph"]), name)
    # n_selected is the number of slots the host rule accepts for any observer
    n, cos_acc, _, _ = ec.observers()
    accepted = S.per_photon(k["ph"], n, cos_acc, ec.T_EDGES, ec.E_EDGES, ec.TIME_NOW)["accepted"]
    assert res["n_selected"] == accepted.any(axis=0).sum() == res["n_status"].sum() and 20 < res["n_selected"] < res["n_observable"]
    assert (res["n_accepted"] == accepted.sum(axis=1)).all() and res["n_accepted"].sum() > res["n_selected"]        # cones overlap
    e.close()


# ---------------------------------------------------------------------------------------------- TABLE and how a march ends
@pytest.mark.parametrize("name", ["table_in", "table_off", "table_cold", "opaque", "cap_1", "cap_7", "gap"])
def test_table_and_march_endings(hip, name):
    k, e = run_case(hip, name)
    res = observe(e, k["c"])
    ec.compare(res, k["want"], name)
    same_counts(res, from_device_tau(e, k["c"], k["ph"]), name)
    if name == "table_off":
        assert res["n_unresolved"].sum() > 10 and res["n_status"][sc.OFF_TABLE] > 10
    if name in ("table_in", "table_cold", "gap"):
        assert not res["n_unresolved"].any() and not res["n_opaque"].any() and res["count"].sum() + res["n_outside"].sum() > 50
    if name == "table_cold":                               # its photons are softer than 1e-10 erg, all outside: once more with edges that hold them
        n, cos_acc, _, _ = ec.observers()
        soft = 10.0 ** np.linspace(-11.0, -5.0, 7)
        again = observe(e, k["c"], e_edges=soft)
        ec.compare(again, ec.observation(k["ph"], ec.marched_slice(k["c"]["want"]), n, cos_acc, ec.T_EDGES, soft, ec.TAU_EDGES, ec.TIME_NOW), name + ", softer edges")
        assert not res["count"].any() and again["count"].sum() > 50
    if name == "opaque":
        assert res["n_opaque"].sum() > 50 and res["n_status"][sc.OPAQUE] > 30 and not res["count"][:, 4:].any()      # nothing beyond tau = 3: tau_stop is 2
    if name.startswith("cap"):
        assert res["n_unresolved"].sum() > 50 and res["n_status"][sc.STEP_CAP] > 30
    zero = k["want"]["selected"] & (k["want"]["status"] == sc.LEFT_MESH) & (k["want"]["tau"] == 0)
    if zero.any():                                         # photons that start outside the frame: in the bin that holds 0, with x = 1 exactly
        assert res["count"][:, 0].sum() >= (k["want"]["bin"][:, zero] >= 0).sum()
    e.close()


# ---------------------------------------------------------------------------------------------- Stokes off, image axes, another context's frame
@pytest.mark.parametrize("stokes", [0, 1])
@pytest.mark.parametrize("image", [False, True])
def test_stokes_and_image_axes(hip, stokes, image):
    k, e = run_case(hip, "pair_0_2", stokes=stokes)
    n, cos_acc, ex, ey = ec.observers()
    kw = dict(ex=ex, ey=ey, x_edges=ec.X_EDGES, y_edges=ec.Y_EDGES) if image else {}
    want = ec.observation(k["ph"], ec.marched_slice(k["c"]["want"]), n, cos_acc, ec.T_EDGES, ec.E_EDGES, ec.TAU_EDGES, ec.TIME_NOW, stokes=bool(stokes), **kw)
    res = observe(e, k["c"], image=image)
    assert res["count"].shape == ((3, 6, 10, 5, 6, 8) if image else (3, 6, 10, 5))
    ec.compare(res, want, "Stokes %d, image %d" % (stokes, image))
    if not stokes:
        assert not any(res[p].any() for p in ("i", "q", "u", "v")) and res["wx"].any()
    if image:
        assert want["n_outside"].sum() > k["want"]["n_outside"].sum()          # some photons lie off the image
        assert np.array_equal(res["count"].sum(axis=(4, 5)) <= k["want"]["count"], np.ones((3, 6, 10, 5), dtype=bool))
    e.close()


def test_frame_of_another_context(hip):
    """the photons' own context holds only their slab, which they leave at once; a second context holds the whole frame"""
    k = ec.case("larger_frame")
    c = k["c"]
    whole = c["frame"]
    own = engine_for(hip, c, frame=synth.select_slab(whole, whole["r1"] < 1.04e12))
    own.set_photons(k["ph"])
    big = engine_for(hip, c)
    through_slab = observe(own, c)
    through_whole = observe(own, c, hydro=big)
    ec.compare(through_whole, k["want"], "another context's frame")
    ec.identities(through_slab)
    assert np.array_equal(through_slab["n_accepted"], through_whole["n_accepted"]) and through_slab["n_selected"] == through_whole["n_selected"]
    assert through_slab["count"][:, :2].sum() > through_whole["count"][:, :2].sum()          # less of the frame: shallower
    own.close()
    big.close()


# ---------------------------------------------------------------------------------------------- a pool of three lists with clocks of their own
def test_pool_of_three_ragged_lists(hip):
    c = sc.case("photons")
    lens, ranks, clocks = [137, 300, 3], [0, 1, 3], np.array([40.0, 41.0, 0.0, 42.0])          # rank 2 is never created
    pool = engine_for(hip, c)
    pool.pool_create(4, 320)
    n, cos_acc, _, _ = ec.observers()
    wants, first = [], 0
    for r, m in zip(ranks, lens):
        ph = ec.photons_of(c, 50 + r, first, m)
        pool.pool_rank(r, r).set_photons(ph)
        wants.append(ec.observation(ph, ec.marched_slice(c["want"], first, m), n, cos_acc, ec.T_EDGES, ec.E_EDGES, ec.TAU_EDGES, clocks[r]))
        first += m
    res = observe(pool, c, time_now=clocks, pool=True)
    ec.compare(res, ec.add(wants), "pool of three lists")
    assert res["n_opaque"].sum() > 10 and res["count"].sum() > 50                          # (the case stops at tau = 3)
    for r, want in zip(ranks, wants):
        ec.compare(observe(pool.pool_rank(r, r), c, time_now=clocks[r]), want, "view of list %d" % r)
    with pytest.raises(hip.McratHipError, match="observe_escaping: a rank pool's lists have clocks of their own"):
        observe(pool, c)                                   # the pool itself is not one list
    with pytest.raises(hip.McratHipError, match="pool_observe_escaping: the context is no rank pool"):
        view = pool.pool_rank(0, 0)
        view.n_pool_ranks = 4
        observe(view, c, time_now=clocks, pool=True)
    pool.close()


# ---------------------------------------------------------------------------------------------- both accumulation paths
@pytest.mark.parametrize("image", [False, True])
def test_both_paths_agree(hip, monkeypatch, image):
    k, e = run_case(hip, "uniform_n1000")
    n, cos_acc, ex, ey = ec.observers()
    kw = dict(ex=ex, ey=ey, x_edges=ec.X_EDGES, y_edges=ec.Y_EDGES) if image else {}
    want = ec.observation(k["ph"], ec.marched_slice(k["c"]["want"]), n, cos_acc, ec.T_EDGES, ec.E_EDGES, ec.TAU_EDGES, ec.TIME_NOW, **kw) if image else k["want"]
    assert e.observe_escaping_path() == 0
    got = {}
    for path, code in (("global", hip.ESCAPE_PATH_GLOBAL), ("lds", hip.ESCAPE_PATH_LDS)):
        if image and path == "lds":                        # 3 x 6 x 10 x 5 x 6 x 8 bins of 72 bytes do not fit: lds is refused, the rule takes global
            monkeypatch.setenv("MCRAT_HIP_ESCAPE_PATH", "lds")
            with pytest.raises(hip.McratHipError, match="MCRAT_HIP_ESCAPE_PATH=lds, but the cube does not fit"):
                observe(e, k["c"], image=True)
            assert e.observe_escaping_path() == 0
            monkeypatch.delenv("MCRAT_HIP_ESCAPE_PATH")
            code = hip.ESCAPE_PATH_GLOBAL
        else:
            monkeypatch.setenv("MCRAT_HIP_ESCAPE_PATH", path)
        got[path] = observe(e, k["c"], image=image)
        assert e.observe_escaping_path() == code
        ec.compare(got[path], want, "path %s, image %d" % (path, image))
    same_counts(got["global"], got["lds"], "both paths")
    m = want["count"].astype(np.float64)
    for p in ec.PLANES:                                    # each within its bound of the exact sum of the same terms: of each other within two
        assert (np.abs(got["global"][p] - got["lds"][p]) <= 2 * (m + 2.0) * ec.U * want["abs_" + p]).all(), p
    e.close()


def test_the_rule_changes_path_at_the_lds_budget(hip):
    """3 observers x 6 tau x 10 time bins of 72 bytes: with 6 energy bins 77 760 bytes of cube and 392 of staging fit the 81 920, with 7 they do not"""
    k, e = run_case(hip, "pair_0_1")
    n, cos_acc, _, _ = ec.observers()
    for n_e, code in ((6, hip.ESCAPE_PATH_LDS), (7, hip.ESCAPE_PATH_GLOBAL)):
        e_edges = 10.0 ** np.linspace(-10.0, -5.0, n_e + 1)
        res = observe(e, k["c"], e_edges=e_edges)
        assert e.observe_escaping_path() == code
        ec.compare(res, ec.observation(k["ph"], ec.marched_slice(k["c"]["want"]), n, cos_acc, ec.T_EDGES, e_edges, ec.TAU_EDGES, ec.TIME_NOW), "%d energy bins" % n_e)
    e.close()


# ---------------------------------------------------------------------------------------------- against observe_sky; the issue's time bins
def test_one_wide_tau_bin_is_observe_sky(hip):
    k, e = run_case(hip, "pair_0_1")
    n, cos_acc, ex, ey = ec.observers()
    for image in (False, True):
        kw = dict(ex=ex, ey=ey, x_edges=ec.X_EDGES, y_edges=ec.Y_EDGES) if image else {}
        sky = e.observe_sky(n, cos_acc, ec.T_EDGES, ec.E_EDGES, ec.TIME_NOW, **kw)
        res = observe(e, k["c"], tau_edges=[0.0, 1e300], image=image, max_steps=4000)
        assert not res["n_unresolved"].any() and not res["n_opaque"].any()
        assert np.array_equal(res["count"][:, 0], sky["count"]) and sky["count"].sum() > 50
        assert np.array_equal(res["n_accepted"], sky["n_accepted"]) and np.array_equal(res["n_outside"], sky["n_outside"])
        bound = (sky["count"] + 2.0) * 2 * ec.U * np.abs(sky["w"])
        assert (np.abs(res["w"][:, 0] - sky["w"]) <= bound).all() and (res["wx"][:, 0] <= res["w"][:, 0] * (1.0 + 2 * 259 * ec.U)).all()
    e.close()


def test_time_bins_from_30_s(hip):
    """1-s bins from 30 s with the clock at 40 s: the photons, 33 to 39 light-seconds out, are detected between 1 and 7 s -- all outside"""
    k, e = run_case(hip, "pair_0_1")
    res = observe(e, k["c"], t_edges=ec.T_EDGES_LATE)
    n, cos_acc, _, _ = ec.observers()
    want = ec.observation(k["ph"], ec.marched_slice(k["c"]["want"]), n, cos_acc, ec.T_EDGES_LATE, ec.E_EDGES, ec.TAU_EDGES, ec.TIME_NOW)
    ec.compare(res, want, "time bins from 30 s")
    assert not res["count"].any() and res["n_outside"].sum() > 50 and res["n_status"][sc.LEFT_MESH] > 50
    e.close()


# ---------------------------------------------------------------------------------------------- refusals and states
def test_refusals_through_the_python_interface(hip, monkeypatch):
    k, e = run_case(hip, "uniform_n63")
    c = k["c"]
    n, cos_acc, ex, ey = ec.observers()
    good = dict(n=n, cos_acc=cos_acc, t_edges=ec.T_EDGES, e_edges=ec.E_EDGES, tau_edges=ec.TAU_EDGES, time_now=40.0, step_frac=0.01, h_min=1e8, max_steps=16)
    img = dict(ex=ex, ey=ey, x_edges=ec.X_EDGES, y_edges=ec.Y_EDGES)
    nan0 = lambda a: np.concatenate([[np.nan], np.asarray(a, dtype=np.float64)[1:]])
    swap = lambda a: np.concatenate([np.asarray(a, dtype=np.float64)[1::-1], np.asarray(a, dtype=np.float64)[2:]])
    refused = [(dict(t_edges=[0.0]), "n_obs, n_t and n_e must each be at least 1"), (dict(n=n * np.array([[np.nan], [1.0], [1.0]])), "direction holds a value that is not finite"),
               (dict(n=1.001 * n), "direction is not a unit vector"), (dict(cos_acc=[0.5, 1.5, 0.5]), "cos_acc must be a number in"),
               (dict(img, ex=nan0(ex.ravel()).reshape(3, 3)), "sky-plane vector holds a value that is not finite"), (dict(img, ey=2.0 * ey), "sky-plane vector is not a unit vector"),
               (dict(img, ex=ey), "are not orthogonal"), (dict(t_edges=nan0(ec.T_EDGES)), "t_edges holds a value that is not finite"),
               (dict(t_edges=swap(ec.T_EDGES)), "t_edges is not strictly ascending"), (dict(e_edges=nan0(ec.E_EDGES)), "e_edges holds a value that is not finite"),
               (dict(e_edges=swap(ec.E_EDGES)), "e_edges is not strictly ascending"), (dict(img, x_edges=nan0(ec.X_EDGES)), "x_edges holds a value that is not finite"),
               (dict(img, x_edges=swap(ec.X_EDGES)), "x_edges is not strictly ascending"), (dict(img, y_edges=nan0(ec.Y_EDGES)), "y_edges holds a value that is not finite"),
               (dict(img, y_edges=swap(ec.Y_EDGES)), "y_edges is not strictly ascending"),
               (dict(tau_edges=[0.0]), "n_tau must be at least 1"), (dict(tau_edges=[0.0, np.inf]), "tau_edges holds a value that is not finite"),
               (dict(tau_edges=[0.0, 1.0, 1.0]), "tau_edges is not strictly ascending"),
               (dict(step_frac=-1.0), "step_frac must be finite and not negative"), (dict(h_min=0.0), "h_min must be finite and positive"),
               (dict(max_steps=0), "max_steps must lie between 1 and 1048576"), (dict(tau_stop=0.0), "tau_stop must be positive"),
               (dict(t_edges=np.arange(9300.0)), "do not fit the kernel's LDS budget"),
               # the first in the order decides
               (dict(t_edges=swap(ec.T_EDGES), tau_edges=[0.0]), "t_edges is not strictly ascending"), (dict(tau_edges=[0.0], step_frac=-1.0), "n_tau must be at least 1"),
               (dict(tau_edges=[1.0, 0.0], h_min=-1.0), "tau_edges is not strictly ascending"), (dict(step_frac=np.nan, max_steps=0), "step_frac must be finite")]
    for change, text in refused:
        with pytest.raises(hip.McratHipError, match="observe_escaping: .*" + text):
            e.observe_escaping(**dict(good, **change))
    monkeypatch.setenv("MCRAT_HIP_ESCAPE_PATH", "hbm")
    with pytest.raises(hip.McratHipError, match="observe_escaping: MCRAT_HIP_ESCAPE_PATH must be lds or global"):
        e.observe_escaping(**good)
    with pytest.raises(hip.McratHipError, match="observe_escaping: .*max_steps must lie between"):
        e.observe_escaping(**dict(good, max_steps=0))             # the arguments come before the switch
    monkeypatch.setenv("MCRAT_HIP_ESCAPE_PATH", "lds")
    with pytest.raises(hip.McratHipError, match="observe_escaping: MCRAT_HIP_ESCAPE_PATH=lds, but the cube does not fit"):
        e.observe_escaping(**dict(good, **img))
    monkeypatch.delenv("MCRAT_HIP_ESCAPE_PATH")
    # a frame on a context with other switches; the switches' refusals come before it, the frame's state after it
    other = hip.Engine(synth.TWO, synth.CARTESIAN, 1)
    other.set_hydro(dict(c["frame"], geometry=synth.CARTESIAN))
    tab = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1, tau_calculation=hip.TAU_TABLE)
    tab.set_hydro(c["frame"])
    for h in (other, tab):
        with pytest.raises(hip.McratHipError, match="observe_escaping: a frame staged on a context with other switches"):
            e.observe_escaping(hydro=h, **good)
    with pytest.raises(hip.McratHipError, match="tau_stop must be positive"):
        e.observe_escaping(hydro=other, **dict(good, tau_stop=-1.0))
    bare = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    with pytest.raises(hip.McratHipError, match="observe_escaping: no staged hydro frame"):
        e.observe_escaping(hydro=bare, **good)
    bare.set_photons(k["ph"])
    with pytest.raises(hip.McratHipError, match="observe_escaping: no staged hydro frame"):
        bare.observe_escaping(**good)
    tab.set_photons(k["ph"])
    with pytest.raises(hip.McratHipError, match="needs mcrat_hip_set_hot_cross_section first"):
        tab.observe_escaping(**good)                              # TABLE without a table
    empty = engine_for(hip, c)
    with pytest.raises(hip.McratHipError, match="call out of order"):
        empty.observe_escaping(**good)                            # no photons
    res = e.observe_escaping(**good)                              # ... and the context still works
    ec.identities(res)
    assert res["n_status"][sc.STEP_CAP] > 0
    for x in (other, tab, bare, empty, e):
        x.close()


# ---------------------------------------------------------------------------------------------- every refusal and state through the ABI itself
EINVAL, ESTATE = -1, -5


def _abi_observer(hip, c, keep):
    """a mcrat_hip_escape_observer from a case of tests/test_escape_plan_cpu.py (keep: the arrays it points to)"""
    dp = C.POINTER(C.c_double)

    def arr(v, n):
        v = [float(k) for k in range(n + 1)] if v == "ramp" else list(v)
        a = np.array(v + [0.0], dtype=np.float64)                 # (never empty: a pointer to something)
        keep.append(a)
        return a.ctypes.data_as(dp)

    def vec(rows):
        if rows is None:
            return [None, None, None]
        return [arr([r[k] for r in rows], 0) for k in range(3)]
    sky = hip.SkyObserver(c["n_obs"], *vec(c["n"]), arr(c["cos_acc"], 0), *vec(c["ex"]), *vec(c["ey"]), c["n_t"], arr(c["te"], c["n_t"]),
                          c["n_e"], arr(c["ee"], c["n_e"]), c["n_x"], arr(c["xe"], c["n_x"]), c["n_y"], arr(c["ye"], c["n_y"]))
    return hip.EscapeObserver(sky, c["n_tau"], arr(c["taue"], c["n_tau"]),
                              hip.SightlineParams(c["step_frac"], c["h_min"], c["max_steps"], c["tau_stop"], c["surface_level"]))


def test_every_refusal_reaches_the_caller_through_the_abi(hip, monkeypatch):
    """every case tests/test_escape_plan_cpu.py refuses, handed to mcrat_hip_observe_escaping as a raw struct: MCRAT_HIP_EINVAL, mcrat_hip_last_error
    equal to the header's text, the path query still 0; then the frame's context, NULL outputs, NULL arguments and the states"""
    k, e = run_case(hip, "uniform_n63")
    lib, last = e.lib, lambda x: e.lib.mcrat_hip_last_error(x.ctx).decode()
    for name, why in sorted(P.REFUSED.items()):
        c = P.PLANS[name]
        if c["env"] is None:
            monkeypatch.delenv("MCRAT_HIP_ESCAPE_PATH", raising=False)
        else:
            monkeypatch.setenv("MCRAT_HIP_ESCAPE_PATH", c["env"])
        keep = []
        obs, out = _abi_observer(hip, c, keep), hip.EscapeObservation()
        assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(obs), ec.TIME_NOW, C.byref(out)) == EINVAL, name
        assert last(e) == P.TEXTS[why], name
        assert e.observe_escaping_path() == 0, name
    monkeypatch.delenv("MCRAT_HIP_ESCAPE_PATH", raising=False)
    assert set(P.REFUSED.values()) | {P.HYDRO_MISMATCH} == set(P.TEXTS)
    for why in (P.TOO_MANY_BINS, P.SKY_TOO_MANY_BINS, P.SKY_AXES_MISMATCH, P.SKY_AXES_NULL):
        assert why in P.REFUSED.values()
    # the frame's context: other switches -> the last EINVAL of the order; then the states, MCRAT_HIP_ESTATE
    keep = []
    good, out = _abi_observer(hip, P.PLANS["curve"], keep), hip.EscapeObservation()
    frame = k["c"]["frame"]
    other = hip.Engine(synth.TWO, synth.CARTESIAN, 1)
    other.set_hydro(dict(frame, geometry=synth.CARTESIAN))
    tab = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1, tau_calculation=hip.TAU_TABLE)
    tab.set_hydro(frame)
    for h in (other, tab):
        assert lib.mcrat_hip_observe_escaping(e.ctx, h.ctx, C.byref(good), ec.TIME_NOW, C.byref(out)) == EINVAL
        assert last(e) == P.TEXTS[P.HYDRO_MISMATCH] and e.observe_escaping_path() == 0
    bad = _abi_observer(hip, P.PLANS["tau_stop_zero"], keep)
    assert lib.mcrat_hip_observe_escaping(e.ctx, other.ctx, C.byref(bad), ec.TIME_NOW, C.byref(out)) == EINVAL and last(e) == P.TEXTS[P.BAD_TAU_STOP]
    bare = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    assert lib.mcrat_hip_observe_escaping(e.ctx, bare.ctx, C.byref(good), ec.TIME_NOW, C.byref(out)) == ESTATE
    assert last(e) == "observe_escaping: no staged hydro frame"
    assert lib.mcrat_hip_observe_escaping(bare.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == ESTATE          # no photons
    bare.set_photons(k["ph"])
    assert lib.mcrat_hip_observe_escaping(bare.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == ESTATE
    assert last(bare) == "observe_escaping: no staged hydro frame"
    tab.set_photons(k["ph"])
    assert lib.mcrat_hip_observe_escaping(tab.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == ESTATE
    assert last(tab) == "TAU_CALCULATION == TABLE needs mcrat_hip_set_hot_cross_section first"
    # NULL output pointers: the call runs and writes nowhere; then only one counter, then one plane
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == 0 and e.observe_escaping_path() == hip.ESCAPE_PATH_LDS
    c = P.PLANS["curve"]
    n_obs1 = np.array([[0.0], [0.0], [1.0]])
    marched = sc.march(frame, *ec.rays_of(k["ph"]), c["step_frac"], c["h_min"], c["max_steps"])
    want = ec.observation(k["ph"], marched, n_obs1, [0.5], np.arange(5.0), np.arange(9.0), np.arange(7.0), ec.TIME_NOW)
    assert not want["fragile"].any() and want["n_accepted"][0] > 10 and want["count"].sum() > 5
    assert out.n_selected == want["n_selected"] and out.n_observable == want["n_observable"] and list(out.n_status) == list(want["n_status"])
    ll = C.POINTER(C.c_longlong)
    n_acc, count = np.full(1, -1, dtype=np.int64), np.full(want["count"].shape, -1, dtype=np.int64)
    out.n_accepted = n_acc.ctypes.data_as(ll)
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == 0 and n_acc[0] == want["n_accepted"][0]
    out.count = count.ctypes.data_as(ll)
    wx = np.full(want["count"].shape, -1.0)
    out.wx = wx.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == 0
    assert np.array_equal(count, want["count"])
    assert (np.abs(wx - want["wx"]) <= (want["count"] + 2.0) * ec.U * want["abs_wx"] + want["tol_wx"]).all()
    # ... and a block of megabytes, which is read back plane by plane: 6 x 10 x 10 x 10 x 10 bins, only the count and one counter asked for.  The
    # image's edges are 0 .. 10 cm, so every accepted photon (all leave the mesh) is outside
    big = _abi_observer(hip, P.plan(n_t=10, n_e=10, n_x=10, n_y=10), keep)
    few = hip.EscapeObservation()
    big_count, n_out = np.full(60000, -1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
    few.count, few.n_outside = big_count.ctypes.data_as(ll), n_out.ctypes.data_as(ll)
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(big), ec.TIME_NOW, C.byref(few)) == 0 and e.observe_escaping_path() == hip.ESCAPE_PATH_GLOBAL
    assert not big_count.any() and n_out[0] == want["n_accepted"][0] == few.n_status[sc.LEFT_MESH] and few.n_selected == want["n_selected"]
    # NULL arguments
    assert lib.mcrat_hip_observe_escaping(None, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == EINVAL
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, None, ec.TIME_NOW, C.byref(out)) == EINVAL
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(good), ec.TIME_NOW, None) == EINVAL and lib.mcrat_hip_observe_escaping_path(None) == 0
    for field in ("tau_edges", "t_edges", "n0", "cos_acc", "e_edges"):
        broken = _abi_observer(hip, P.PLANS["curve"], keep)
        setattr(broken if field == "tau_edges" else broken.sky, field, None)
        assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(broken), ec.TIME_NOW, C.byref(out)) == EINVAL, field
        assert last(e) == "observe_escaping: a null array in mcrat_hip_escape_observer" and e.observe_escaping_path() == 0, field
    broken = _abi_observer(hip, P.PLANS["image"], keep)
    broken.sky.x_edges = None
    assert lib.mcrat_hip_observe_escaping(e.ctx, None, C.byref(broken), ec.TIME_NOW, C.byref(out)) == EINVAL
    assert last(e) == "observe_escaping: a null array in mcrat_hip_escape_observer"
    # the wrong kind of context
    dp = C.POINTER(C.c_double)
    clocks = np.array([ec.TIME_NOW, ec.TIME_NOW])
    assert lib.mcrat_hip_pool_observe_escaping(e.ctx, None, C.byref(good), clocks.ctypes.data_as(dp), C.byref(out)) == ESTATE
    assert last(e) == "pool_observe_escaping: the context is no rank pool"
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.set_hydro(frame)
    pool.pool_create(2, 64)
    pool.pool_rank(0, 0).set_photons(k["ph"])
    assert lib.mcrat_hip_observe_escaping(pool.ctx, None, C.byref(good), ec.TIME_NOW, C.byref(out)) == ESTATE
    assert "mcrat_hip_pool_observe_escaping" in last(pool) and last(pool).startswith("observe_escaping: ")
    for args in ((None, C.byref(good), clocks.ctypes.data_as(dp), C.byref(out)), (pool.ctx, None, clocks.ctypes.data_as(dp), C.byref(out)),
                 (pool.ctx, C.byref(good), None, C.byref(out)), (pool.ctx, C.byref(good), clocks.ctypes.data_as(dp), None)):
        assert lib.mcrat_hip_pool_observe_escaping(args[0], None, *args[1:]) == EINVAL
    n_acc[0] = -1
    assert lib.mcrat_hip_pool_observe_escaping(pool.ctx, None, C.byref(good), clocks.ctypes.data_as(dp), C.byref(out)) == 0 and n_acc[0] == want["n_accepted"][0]
    with pytest.raises(ValueError):
        observe(pool, k["c"], time_now=[ec.TIME_NOW], pool=True)      # one clock per list
    for x in (other, tab, bare, pool, e):
        x.close()
