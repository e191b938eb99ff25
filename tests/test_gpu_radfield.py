"""The radiation field on the hydro mesh on the device (mcrat_hip_radiation_field, mcrat_hip_pool_radiation_field; mcrat_amd/csrc/radfield.hip)
against tests/radfield_checker.py, an independent NumPy restatement of the definitions (include/mcrat_hip.h) that finds the
cell by brute force, takes the cell's velocity from synth.hydro_vector_to_cartesian and the comoving energy from a textbook boost.

Exact: count per bin and n_observable, n_unlocated, n_outside -- what decides a cell or a shell is written in one fixed order and evaluated without
contraction, and no committed case holds a photon within 1e-9 of a cell's size of a face (tests/test_radfield_checker_cpu.py).  Sums, per bin with
m terms t_i of the checker, u = 2^-53:
    W, WE_lab, WNS, WT   |dev - chk| <= (m + 2) u sum|t_i|                      (the terms are the same bits on both sides; any summation order)
    WE_comv              |dev - chk| <= sum 2 bar_e,i |t_i| + (m + 2) u sum|t_i|,   bar_e = 8u (1 + |x_v|)(1 + Gamma_v^2) / (1 - x_v),  x_v = v.p / p0
-- the conditioning bar tests/sightline_checker.py derives for the same boost, taken twice because both sides round (at most 2.6e-11 for
gamma <= 10, 1.6e-8 for gamma <= 100 on these meshes).  Derived, not measured; a bin nobody is in has the bound 0: its planes must hold exactly 0.
The largest error / bound is printed per case."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import radfield_checker as rc
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

CYL = (synth.TWO, synth.CYLINDRICAL)


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(autouse=True)
def no_forced_path(monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_RADFIELD_PATH", raising=False)


def engine_for(hip, frame, ph=None):
    e = hip.Engine(frame["dimensions"], frame["geometry"], 0)
    e.set_hydro(frame)
    if ph is not None:
        e.set_photons(ph)
    return e


def compare(res, want, label, fragile_ok=False):
    assert fragile_ok or want["n_fragile"] == 0, label
    assert res["count"].shape == want["count"].shape and res["count"].dtype == np.int64, label
    for k in ("n_observable", "n_unlocated", "n_outside"):
        assert res[k] == want[k], (label, k, res[k], want[k])
    assert np.array_equal(res["count"], want["count"]), (label, np.nonzero(res["count"] != want["count"])[0][:8])
    assert int(res["count"].sum()) + res["n_unlocated"] + res["n_outside"] == res["n_observable"], label
    worst = {}
    for k in rc.SUMS:
        err, bound = np.abs(res[k] - want[k]), want["bound_" + k]
        worst[k] = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
    print("%s: %d counted, %d bins in use; largest error / bound: %s" % (label, int(want["count"].sum()), int((want["count"] > 0).sum()),
                                                                         ", ".join("%s %.3g" % (k, worst[k]) for k in rc.SUMS)))
    for k in rc.SUMS:
        assert (np.abs(res[k] - want[k]) <= want["bound_" + k]).all(), (label, k, worst[k])      # (an empty bin: bound 0, the device's plane must hold 0)
        assert not res[k][want["count"] == 0].any(), (label, k)


def run_case(hip, name, mode, **kw):
    c = rc.case(name)
    e = engine_for(hip, c["frame"], c["ph"])
    res = e.radiation_field(mode, rc.SHELL_R, rc.SHELL_MU, **kw) if mode == rc.SHELLS else e.radiation_field(mode, **kw)
    path = e.radiation_field_path()
    e.close()
    return c, res, path


# ---------------------------------------------------------------------------------------------- CELLS
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_cells_ragged_sizes(hip, n):
    c, res, path = run_case(hip, "cells_n%d" % n, rc.CELLS)
    assert res["w"].shape == (256,) and path == hip.RADFIELD_PATH_GLOBAL
    compare(res, rc.want("cells_n%d" % n, rc.CELLS), "CELLS, n = %d" % n)


@pytest.mark.parametrize("dims, geom", sc.PAIRS)
def test_every_dimensions_geometry_pair(hip, dims, geom):
    name = "pair_%d_%d" % (dims, geom)
    c, res, path = run_case(hip, name, rc.CELLS)
    assert path == hip.RADFIELD_PATH_GLOBAL and res["count"].shape == (c["frame"]["num_elements"],)
    compare(res, rc.want(name, rc.CELLS), "CELLS, DIMENSIONS %d, geometry %d" % (dims, geom))
    assert res["count"].sum() > 100 and (res["count"] > 0).sum() > 50
    c, res, path = run_case(hip, name, rc.SHELLS)
    assert path == hip.RADFIELD_PATH_LDS and res["count"].shape == (8, 4)
    compare(res, rc.want(name, rc.SHELLS), "SHELLS 8 x 4, DIMENSIONS %d, geometry %d" % (dims, geom))
    assert res["count"].sum() > 20


def test_lorentz_factors_up_to_100(hip):
    for mode in (rc.CELLS, rc.SHELLS):
        c, res, _ = run_case(hip, "gamma_100", mode)
        compare(res, rc.want("gamma_100", mode), "gamma_max 100, mode %d" % mode)
    assert c["frame"]["gamma"].max() > 80
    # the boost matters: the comoving sums are far from the lab sums
    w = rc.want("gamma_100", rc.CELLS)
    assert (np.abs(w["we_comv"] - w["we_lab"]) > 1e6 * w["bound_we_comv"])[w["count"] > 0].all()


@pytest.mark.parametrize("name", ["crowded_4", "crowded_1", "spread"])
def test_crowded_and_spread(hip, name):
    """1000 photons in four cells and in one (same-address adds, the in-wave grouping), and in 1000 different cells of a 32 x 32 mesh (every lane alone)"""
    c, res, path = run_case(hip, name, rc.CELLS)
    assert path == hip.RADFIELD_PATH_GLOBAL
    compare(res, rc.want(name, rc.CELLS), name)
    assert res["count"].sum() == 1000 and (res["count"] > 0).sum() == {"crowded_4": 4, "crowded_1": 1, "spread": 1000}[name]
    assert res["count"].max() >= {"crowded_4": 250, "crowded_1": 1000, "spread": 1}[name]
    if name == "spread":                                   # one term per bin: the four equal-bits sums are the terms themselves
        ph = c["ph"]
        for k, t in (("w", ph["weight"]), ("we_lab", ph["weight"] * (ph["p0"] * synth.C_LIGHT)), ("w_nscatt", ph["weight"] * ph["num_scatt"])):
            assert np.array_equal(res[k][c["cells"]], t), k


def test_gap_domain_and_slots_that_do_not_count(hip):
    """a slab with a gap and photons beyond the domain: n_unlocated; weight 0, 'p', 'N': not counted; 'c' counted"""
    c, res, _ = run_case(hip, "gap", rc.CELLS)
    want = rc.want("gap", rc.CELLS)
    compare(res, want, "gap")
    ph = c["ph"]
    n = len(ph["weight"])
    observable = (ph["weight"] != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")
    assert res["n_observable"] == observable.sum() < n - 200 and ((ph["type"] == b"c") & (want["bin"] >= 0)).sum() > 30
    for excluded in (ph["weight"] == 0, ph["type"] == b"p", ph["type"] == b"N"):
        assert excluded.sum() > 50 and (want["bin"][excluded] < 0).all()
    whole = rc.field(c["whole"], ph, rc.CELLS)
    assert res["n_unlocated"] > whole["n_unlocated"] + 20 > 30
    # SHELLS on the same slab: what is not located is in no shell either
    c, res, _ = run_case(hip, "gap", rc.SHELLS)
    compare(res, rc.want("gap", rc.SHELLS), "gap, SHELLS")
    assert res["n_unlocated"] == want["n_unlocated"] and res["n_outside"] > 0


def test_a_photon_on_a_shared_face_counts_in_the_lower_cell(hip):
    """2-D cylindrical, (x, 0, z) with x exactly on the face two cells share: sqrt(x * x) == x, so the tie is decided -- the closed extents of both
    hold the point and the lowest index wins -- not fragile"""
    frame = sc.random_fluid(sc.mesh(*CYL), 700)
    c0, s0, c1 = frame["r0"], frame["r0_size"], frame["r1"]
    faces = []
    for a in range(frame["num_elements"]):
        x = c0[a] + 0.5 * s0[a]
        both = np.nonzero((2 * np.abs(x - c0) - s0 <= 0) & (c1 == c1[a]))[0]
        if len(both) == 2 and np.sqrt(x * x + 0.0 * 0.0) == x:
            faces.append((x, c1[a], both))
    assert len(faces) >= 20
    pick = faces[:: len(faces) // 20][:20]
    r = np.array([[x for x, _, _ in pick], np.zeros(len(pick)), [z for _, z, _ in pick]])
    ph = rc.photon_list(r, rc.momenta(701, len(pick)), 702, exclusions=False)
    want = rc.field(frame, ph, rc.CELLS)
    assert want["n_fragile"] == len(pick)                    # the checker flags them, and this test is about exactly them
    assert np.array_equal(want["bin"], [both.min() for _, _, both in pick]) and len(set(want["bin"])) == len(pick)
    e = engine_for(hip, frame, ph)
    res = e.radiation_field(rc.CELLS)
    e.close()
    compare(res, want, "ties", fragile_ok=True)
    for _, _, both in pick:
        assert res["count"][both.min()] == 1 and res["count"][both.max()] == 0


# ---------------------------------------------------------------------------------------------- SHELLS
def axis_frame():
    """the 2-D cylindrical mesh with its domain opened below r0 = 0, so that a photon on the polar axis passes the strict domain test"""
    frame = sc.random_fluid(sc.mesh(*CYL), 710)
    frame["r0_domain"] = (-1.0, frame["r0_domain"][1])
    return frame


def test_shell_edges_are_half_open_and_the_axis_is_counted(hip):
    frame = axis_frame()
    r_edges = np.array([1.015e12, 1.035e12, 1.055e12, 1.075e12, 1.095e12])
    z = np.array([1.015e12, 1.035e12, 1.055e12, 1.075e12, 1.095e12, 1.0451e12, np.nextafter(1.035e12, 0.0)])      # on every edge, the last included
    r = np.array([np.zeros(len(z)), np.zeros(len(z)), z])
    ph = rc.photon_list(r, rc.momenta(711, len(z)), 712, exclusions=False)
    _, mu_axis = hip.shell_edges(r_edges, [0.0, 2.0, 5.0])
    assert mu_axis[-1] == np.nextafter(1.0, 2.0) and (np.diff(mu_axis) > 0).all()
    e = engine_for(hip, frame, ph)
    res = e.radiation_field(rc.SHELLS, r_edges, mu_axis)
    assert e.radiation_field_path() == hip.RADFIELD_PATH_LDS
    want = rc.field(frame, ph, rc.SHELLS, r_edges, mu_axis)
    compare(res, want, "on the edges, on the axis", fragile_ok=True)      # (a0 == 0 is the first cell's own face: decided, sqrt(0) == 0)
    assert want["q"]["r"].tolist() == z.tolist() and (want["q"]["mu"] == 1.0).all() and (want["q"]["cell"] >= 0).all()
    assert res["count"][:, 1].tolist() == [2, 2, 1, 1] and res["count"][:, 0].sum() == 0 and res["n_outside"] == 1      # r == an edge: the upper bin; the last edge: outside
    # a top edge of exactly 1: mu == 1 lies outside
    closed = e.radiation_field(rc.SHELLS, r_edges, [np.cos(np.radians(5.0)), np.cos(np.radians(2.0)), 1.0])
    compare(closed, rc.field(frame, ph, rc.SHELLS, r_edges, [np.cos(np.radians(5.0)), np.cos(np.radians(2.0)), 1.0]), "top edge 1", fragile_ok=True)
    assert closed["count"].sum() == 0 and closed["n_outside"] == len(z) == closed["n_observable"]
    e.close()


def test_lds_and_global_paths_agree(hip, monkeypatch):
    c = rc.case("shells")
    want = rc.want("shells", rc.SHELLS)
    e = engine_for(hip, c["frame"], c["ph"])
    got = {}
    for path, code in (("lds", hip.RADFIELD_PATH_LDS), ("global", hip.RADFIELD_PATH_GLOBAL)):
        monkeypatch.setenv("MCRAT_HIP_RADFIELD_PATH", path)
        got[path] = e.radiation_field(rc.SHELLS, rc.SHELL_R, rc.SHELL_MU)
        assert e.radiation_field_path() == code
        compare(got[path], want, "SHELLS 8 x 4, 1000 photons, " + path)
    assert np.array_equal(got["lds"]["count"], got["global"]["count"])
    assert want["n_outside"] > 20 and (want["count"] > 0).sum() > 12
    monkeypatch.setenv("MCRAT_HIP_RADFIELD_PATH", "lds")
    with pytest.raises(hip.McratHipError, match="CELLS always accumulates in global memory"):
        e.radiation_field(rc.CELLS)
    monkeypatch.setenv("MCRAT_HIP_RADFIELD_PATH", "global")
    compare(e.radiation_field(rc.CELLS), rc.want("shells", rc.CELLS), "CELLS, global asked for")
    e.close()


@pytest.mark.parametrize("n_r, lds", [(1462, True), (1463, False)])
def test_path_changes_at_the_lds_budget(hip, n_r, lds):
    """1462 x 1 shells with their edges and counters are 80 KiB of LDS exactly; one shell more and the planes stay in HBM
    (tests/test_radfield_plan_cpu.py has the rule)"""
    c = rc.case("shells")
    r_edges, mu_edges = np.linspace(1.0e12, 1.18e12, n_r + 1), np.array([0.9, np.nextafter(1.0, 2.0)])
    e = engine_for(hip, c["frame"], c["ph"])
    assert e.radiation_field_path() == 0
    res = e.radiation_field(rc.SHELLS, r_edges, mu_edges)
    assert e.radiation_field_path() == (hip.RADFIELD_PATH_LDS if lds else hip.RADFIELD_PATH_GLOBAL)
    want = rc.field(c["frame"], c["ph"], rc.SHELLS, r_edges, mu_edges)
    compare(res, want, "%d x 1" % n_r)
    assert res["count"].shape == (n_r, 1) and (want["count"] > 0).sum() > 300 and want["count"][-200:].sum() > 0 and want["count"][:200].sum() > 0
    e.close()


# ---------------------------------------------------------------------------------------------- another context's frame
def test_frame_of_another_context(hip):
    """the photons' own context holds a slab with a gap; a second context holds the whole frame, where the photons of the gap are located"""
    c = rc.case("gap")
    own = engine_for(hip, c["frame"], c["ph"])
    big = engine_for(hip, c["whole"])
    before = own.get_photons()
    through_slab = own.radiation_field(rc.CELLS)
    through_whole = own.radiation_field(rc.CELLS, hydro=big)
    after = own.get_photons()
    for k in before:                                       # no photon column changes, the cell index included
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    compare(through_slab, rc.want("gap", rc.CELLS), "own slab")
    want = rc.field(c["whole"], c["ph"], rc.CELLS)
    compare(through_whole, want, "the whole frame of another context")
    assert through_whole["count"].shape == (256,) and through_slab["count"].shape == (c["frame"]["num_elements"],) != (256,)
    assert through_whole["n_unlocated"] + 20 < through_slab["n_unlocated"] and through_whole["count"].sum() > through_slab["count"].sum() + 20
    shells = own.radiation_field(rc.SHELLS, rc.SHELL_R, rc.SHELL_MU, hydro=big)
    compare(shells, rc.field(c["whole"], c["ph"], rc.SHELLS, rc.SHELL_R, rc.SHELL_MU), "SHELLS in the whole frame")
    own.close()
    big.close()


# ---------------------------------------------------------------------------------------------- after a real frame
def test_after_a_real_frame(hip):
    """the columns the loop actually leaves behind: 1000 injected photons through one exact-mode frame on the 2-D cylindrical block mesh"""
    frame, ph, cfg = synth.config2(n_photons=1000, nzc=8, stokes=0, lumi=5e51)
    e = engine_for(hip, frame, ph)
    _, st = e.propagate_frame(0.0, 0.5 / frame["fps"], 4242)
    assert st.frame_scatt_cnt > 0
    after = e.get_photons()
    assert not np.array_equal(after["r2"], ph["r2"]) and after["num_scatt"].sum() > 0
    res = e.radiation_field(rc.CELLS)
    want = rc.field(frame, after, rc.CELLS)
    compare(res, want, "after a frame, CELLS")
    assert want["count"].sum() > 900 and (want["count"] > 0).sum() > 300 and res["w_nscatt"].sum() > 0
    r = want["q"]["r"]
    r_edges, mu_edges = hip.shell_edges(np.linspace(np.percentile(r, 2), np.percentile(r, 98), 7), [0.0, 0.5, 1.0, 1.5, 2.0, 2.5])
    shells = e.radiation_field(rc.SHELLS, r_edges, mu_edges)
    compare(shells, rc.field(frame, after, rc.SHELLS, r_edges, mu_edges), "after a frame, SHELLS 6 x 5")
    assert shells["count"].sum() > 600 and shells["n_outside"] > 10
    # photons hotter than the plasma they sit in or colder, but a finite temperature wherever there is weight
    t_ph = hip.photon_temperature(shells, "b")
    assert np.isfinite(t_ph[shells["w"] != 0]).all() and (t_ph[shells["w"] != 0] > 0).all() and np.isnan(t_ph[shells["w"] == 0]).all()
    e.close()


# ---------------------------------------------------------------------------------------------- rank pool
def test_pool_of_three_ragged_lists(hip):
    c = rc.case("shells")
    lens, ranks = [137, 300, 3], [0, 1, 3]                 # rank 2 is never created
    pool = engine_for(hip, c["frame"])
    pool.pool_create(4, 320)
    first, subs = 0, []
    for r, m in zip(ranks, lens):
        subs.append({k: v[first:first + m].copy() for k, v in c["ph"].items()})
        pool.pool_rank(r, r).set_photons(subs[-1])
        first += m
    for mode, args in ((rc.CELLS, ()), (rc.SHELLS, (rc.SHELL_R, rc.SHELL_MU))):
        res = pool.pool_radiation_field(mode, *args)
        views = [pool.pool_rank(r, r).radiation_field(mode, *args) for r in ranks]
        wants = [rc.field(c["frame"], sub, mode, *args) for sub in subs]
        for r, v, w in zip(ranks, views, wants):
            compare(v, w, "view %d, mode %d" % (r, mode))
        total = rc.add(wants)
        compare(res, total, "pool, mode %d" % mode)
        assert np.array_equal(res["count"], sum(v["count"] for v in views)) and res["n_observable"] == sum(v["n_observable"] for v in views)
        for k in rc.SUMS:                                   # the pool's call equals the per-view calls added up, within the summed bounds
            assert (np.abs(res[k] - sum(v[k] for v in views)) <= 2 * total["bound_" + k]).all(), k
        assert res["count"].sum() > 200
    with pytest.raises(hip.McratHipError, match="mcrat_hip_pool_radiation_field takes the pool"):
        pool.radiation_field(rc.CELLS)
    with pytest.raises(hip.McratHipError, match="no rank pool"):
        pool.pool_rank(0, 0).pool_radiation_field(rc.CELLS)
    pool.close()


def test_pool_reads_a_selected_captured_frame(hip):
    frame, ph, cfg = synth.config2(n_photons=900, nzc=8, stokes=0, lumi=5e51)
    lens = [300, 250, 350]
    offs = np.concatenate([[0], np.cumsum(lens)])
    R, F = len(lens), 2
    pool = engine_for(hip, frame)
    pool.pool_create(R, 512)
    stride = pool.n // R
    for r in range(R):
        pool.pool_rank(r, r).set_photons({k: v[offs[r]:offs[r + 1]].copy() for k, v in ph.items()})
    fps = frame["fps"]
    ends = np.array([[0.5 / fps] * R, [1.25 / fps] * R])
    seeds = np.array([[77 + r + 1000 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    got = pool.pool_run_frames(np.ones((F, R), dtype=np.int32), seeds, np.zeros((F, R)), ends.copy(), frame_end=ends, chain_clock=True, capture=True)
    assert sum(got[f][r].frame_scatt_cnt for f in range(F) for r in range(R)) > 0
    try:
        results = []
        for f in range(F):
            pool.pool_select_frame(f if f < F - 1 else -1)
            recs = [pool.get_photons_range(r * stride, lens[r]) for r in range(R)]
            cat = {k: np.concatenate([a[k] for a in recs]) for k in ("r0", "r1", "r2", "p0", "p1", "p2", "p3", "weight", "num_scatt", "type")}
            res = pool.pool_radiation_field(rc.CELLS)
            compare(res, rc.field(frame, cat, rc.CELLS), "pool, frame %d of a captured plan" % f)
            results.append((res, cat))
        assert not np.array_equal(results[0][1]["r2"], results[1][1]["r2"]) and not np.array_equal(results[0][0]["we_lab"], results[1][0]["we_lab"])
    finally:
        pool.pool_select_frame(-1)
        pool.close()


# ---------------------------------------------------------------------------------------------- refusals and helpers
def test_refusals_reach_the_caller(hip, monkeypatch):
    c = rc.case("cells_n63")
    e = engine_for(hip, c["frame"], c["ph"])
    r, mu = rc.SHELL_R, rc.SHELL_MU
    for args, text in (((7,), "mode must be MCRAT_HIP_RADFIELD_CELLS or MCRAT_HIP_RADFIELD_SHELLS"),
                       ((rc.SHELLS,), "SHELLS needs r_edges and mu_edges"),
                       ((rc.SHELLS, r[:1], mu), "n_r and n_mu must each be at least 1"),
                       ((rc.SHELLS, r, mu[:1]), "n_r and n_mu must each be at least 1"),
                       ((rc.SHELLS, [1e12, np.inf], mu), "r_edges holds a value that is not finite"),
                       ((rc.SHELLS, r, [0.5, np.nan, 1.0]), "mu_edges holds a value that is not finite"),
                       ((rc.SHELLS, r[::-1], mu), "r_edges is not strictly ascending"),
                       ((rc.SHELLS, r, [0.5, 0.5, 1.0]), "mu_edges is not strictly ascending"),
                       ((rc.SHELLS, [1.0, 1.0], [0.0, np.nan]), "mu_edges holds a value that is not finite"),      # the first in order decides
                       ((rc.SHELLS, np.arange(10236.0), [0.0, 1.0]), "the edges do not fit the kernel's LDS budget")):
        with pytest.raises(hip.McratHipError, match=text):
            e.radiation_field(*args)
    bins = hip.RadfieldBins(rc.SHELLS, 65536, None, 65536, None)          # n_r * n_mu = 2^32: refused before the arrays are looked at ...
    edge = np.zeros(1)
    bins.r_edges = bins.mu_edges = edge.ctypes.data_as(hip._dp)
    n_bins = hip.C.c_int(0)
    assert e.lib.mcrat_hip_radiation_field_bins(e.ctx, None, hip.C.byref(bins), hip.C.byref(n_bins)) == -1
    assert b"n_r * n_mu overflows an int" in e.lib.mcrat_hip_last_error(e.ctx)
    monkeypatch.setenv("MCRAT_HIP_RADFIELD_PATH", "hbm")
    with pytest.raises(hip.McratHipError, match="MCRAT_HIP_RADFIELD_PATH must be lds or global"):
        e.radiation_field(rc.CELLS)
    with pytest.raises(hip.McratHipError, match="r_edges is not strictly ascending"):      # the arguments come before the switch
        e.radiation_field(rc.SHELLS, r[::-1], mu)
    monkeypatch.setenv("MCRAT_HIP_RADFIELD_PATH", "lds")
    with pytest.raises(hip.McratHipError, match="the planes do not fit the kernel's LDS budget"):
        e.radiation_field(rc.SHELLS, np.linspace(1e12, 1.2e12, 1464), [0.0, 1.0])
    monkeypatch.delenv("MCRAT_HIP_RADFIELD_PATH")
    other = hip.Engine(synth.TWO, synth.CARTESIAN, 0)                    # a frame on a context with other switches
    other.set_hydro(dict(c["frame"], geometry=synth.CARTESIAN))
    with pytest.raises(hip.McratHipError, match="other switches"):
        e.radiation_field(rc.CELLS, hydro=other)
    with pytest.raises(hip.McratHipError, match="mode must be"):           # ... and the arguments come before the frame
        e.radiation_field(9, hydro=other)
    table = hip.Engine(*CYL, 0, tau_calculation=hip.TAU_TABLE)            # TAU_CALCULATION does not matter here
    table.set_hydro(c["frame"])
    compare(e.radiation_field(rc.CELLS, hydro=table), rc.want("cells_n63", rc.CELLS), "a TABLE context's frame")
    bare = hip.Engine(*CYL, 0)
    with pytest.raises(hip.McratHipError, match="no staged hydro frame"):
        e.radiation_field(rc.CELLS, hydro=bare)
    with pytest.raises(hip.McratHipError, match="no staged hydro frame"):
        bare.radiation_field(rc.CELLS)
    no_photons = engine_for(hip, c["frame"])
    with pytest.raises(hip.McratHipError, match="no photons"):
        no_photons.radiation_field(rc.CELLS)
    compare(e.radiation_field(rc.CELLS), rc.want("cells_n63", rc.CELLS), "the context still works")
    for x in (other, table, bare, no_photons, e):
        x.close()


def test_shell_edges_and_photon_temperature_follow_their_definitions(hip):
    r_edges, mu = hip.shell_edges([1e12, 2e12, 4e12], [0.0, 1.0, 3.0, 10.0])
    assert r_edges.tolist() == [1e12, 2e12, 4e12]
    assert mu.tolist() == [np.cos(np.radians(10.0)), np.cos(np.radians(3.0)), np.cos(np.radians(1.0)), np.nextafter(1.0, 2.0)]
    _, inner = hip.shell_edges([1.0, 2.0], [1.0, 3.0])                     # no edge on the axis: nothing is moved
    assert inner.tolist() == [np.cos(np.radians(3.0)), np.cos(np.radians(1.0))]
    res = {"w": np.array([[2.0e50, 0.0], [1.0e49, 3.0e51]]), "we_comv": np.array([[6.0e41, 0.0], [1.0e40, 4.5e43]])}
    for spect, xbar in (("b", 2.701), ("w", 3.0), (b"w", 3.0)):
        t = hip.photon_temperature(res, spect)
        assert np.isnan(t[0, 1]) and np.isnan(t).sum() == 1
        for i, j in ((0, 0), (1, 0), (1, 1)):
            assert t[i, j] == res["we_comv"][i, j] / (res["w"][i, j] * 1.380658e-16 * xbar)
